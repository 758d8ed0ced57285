"""The simulation report (include/reseq_amd.h rsq_sim_stats_*; reseq_amd/csrc/rsq_stats.h) without a GPU: the per-lane functions run on the CPU
(tests/hostemu/stats_trial.cpp, built here with g++).  The row accumulation -- stats_row_lane looped as k_stats_rows loops it -- runs over crafted word-major arrays
and must give, exactly, the histograms numpy counts from the same bytes; the mates' function stats_mate, both instantiations, runs over crafted pairs and must give
the tables tests/sim_stats.py reads off the pair's own SAM records (whose MD strings are checked against tests/truth_md.py md_nm here).  Every count is exact, so a
seam bug shows as a count off by one.  tests/test_sim_stats_gpu.py requires the same of the device."""
import ctypes as C

import numpy as np
import pytest

import sim_stats
from test_truth_md import LETTERS, MdIn, pair_over, read_of, var_pair
from test_truth_sam import CRAFTED, D, I, M, NAMES, build_trial, fill_trial, fragment, make_mate, template_bases
from test_truth_variants import build_allele, fragment_var
from truth_md import md_nm, parse_cigar

MARKER = 0xA7
# what the crafted cases below must have met, each at least once
CLASSES = ("I inside the template", "D inside the template", "I in the adapter part", "D in the adapter part", "0M", "0S", "H", "D at cycle L", "forward mismatch",
           "reverse mismatch", "reverse read_len mod 4 = 0", "reverse read_len mod 4 = 1", "reverse read_len mod 4 = 2", "reverse read_len mod 4 = 3",
           "mismatch at the first aligned base", "mismatch at the last aligned base", "read base N", "mate without an M column", "variants", "adapter-only pair")
met = set()


@pytest.fixture(scope="module")
def trial_lib(tmp_path_factory):
    L = build_trial(tmp_path_factory, "stats_trial")
    L.stats_trial_layout.restype = C.c_uint32
    L.stats_trial_layout.argtypes = [C.c_uint32] * 7 + [C.c_void_p] * 3
    L.stats_rows_trial.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_uint32] * 8 + [C.c_int32, C.c_void_p]
    L.stats_trial_geometry.restype = L.stats_trial_geometry_table.restype = None
    L.stats_trial_geometry.argtypes = [C.c_uint32] * 4 + [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64] + [C.c_int64] * 3 + [C.c_void_p]
    L.stats_trial_geometry_table.argtypes = [C.c_uint32] * 3 + [C.c_uint64, C.c_void_p]
    L.stats_mates_trial.argtypes = [C.POINTER(MdIn), C.c_int] + [C.c_uint32] * 4 + [C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p]
    return L


def tables_of(L, words, lengths, F, Q, T, phred=33, lds=48 * 1024):
    """the trial's flat array as named tables, by the layout the trial states"""
    off, dims, image = np.zeros(14, np.uint32), np.zeros(42, np.uint32), np.zeros(1, np.uint32)
    n = L.stats_trial_layout(lengths[0], lengths[1], F, Q, T, phred, lds, off.ctypes.data, dims.ctypes.data, image.ctypes.data)
    assert n == len(words)
    out = {}
    for t, name in enumerate(sim_stats.TABLES):
        segs, d0, d1 = (int(x) for x in dims[3 * t:3 * t + 3])
        shape = ([2] if segs == 2 else []) + [d0] + ([d1] if name in ("base_quality", "base_call") else [])
        out[name] = words[int(off[t]):int(off[t]) + segs * d0 * d1].reshape(shape)
    assert sum(v.size for v in out.values()) == n, "the tables tile the array"
    return out, int(image[0])


def layout_words(L, lengths, F, Q, T, lds=48 * 1024):
    off, dims, image = np.zeros(14, np.uint32), np.zeros(42, np.uint32), np.zeros(1, np.uint32)
    return L.stats_trial_layout(lengths[0], lengths[1], F, Q, T, 33, lds, off.ctypes.data, dims.ctypes.data, image.ctypes.data)


def same(got, want, names=sim_stats.TABLES):
    for name in names:
        assert got[name].shape == want[name].shape, name
        assert (got[name] == want[name]).all(), (name, np.argwhere(got[name] != want[name])[:8].tolist())


def test_layout_places_fragment_length_by_the_budget(trial_lib):
    words = np.zeros(layout_words(trial_lib, (151, 151), 900, 42, 3), np.uint64)
    t, image = tables_of(trial_lib, words, (151, 151), 900, 42, 3)
    assert t["base_quality"].shape == (2, 151, 42) and t["fragment_length"].shape == (901,) and t["tile"].shape == (3,) and t["read_length"].shape == (2, 152)
    small = image
    assert image * 4 <= 48 * 1024
    words = np.zeros(layout_words(trial_lib, (151, 151), 900, 42, 3, lds=8192), np.uint64)
    _, image = tables_of(trial_lib, words, (151, 151), 900, 42, 3, lds=8192)
    assert image == small - 901, "with a budget the table does not fit, its counters are outside the image"


# ------------------------------------------------------------------------------------------------ the rows
Q_ROWS, L_ROWS, PHRED = 42, 30, 33


def crafted_rows(rng, n, read_lens, bad_cells=()):
    """word-major seq and qual arrays of 2 n reads with pitch > 2 n: the marker in the rows beyond the reads and in every byte beyond a read's length"""
    reads, pitch, row_words = 2 * n, 2 * n + 7, (L_ROWS + 3) // 4 + 1
    seq = np.full((row_words * 4, pitch), MARKER, np.uint8)
    qual = np.full((row_words * 4, pitch), MARKER, np.uint8)
    lens = rng.choice(read_lens, reads).astype(np.uint16)
    lens[0], lens[-1] = read_lens[-1], read_lens[0]
    bases = rng.integers(0, 5, (L_ROWS, reads)).astype(np.uint8)
    quals = rng.choice([0, 2, 11, 25, 37, Q_ROWS - 1], (L_ROWS, reads)).astype(np.uint8)
    for p, r, what in bad_cells:
        if what == "quality":
            quals[p, r] = Q_ROWS
        else:
            bases[p, r] = 7
    inside = np.arange(L_ROWS)[:, None] < lens[None, :]
    seq[:L_ROWS, :reads][inside] = bases[inside]
    qual[:L_ROWS, :reads][inside] = quals[inside] + PHRED
    # the expected histograms, counted here
    want = sim_stats.empty((L_ROWS, L_ROWS), 10, Q_ROWS, 1)
    for seg in (0, 1):
        for r in range(seg * n, (seg + 1) * n):
            p = np.arange(lens[r])
            ok_q, ok_b = quals[p, r] < Q_ROWS, bases[p, r] < 5
            np.add.at(want["base_quality"], (seg, p[ok_q], quals[p, r][ok_q]), 1)
            np.add.at(want["base_call"], (seg, p[ok_b], bases[p, r][ok_b]), 1)
            want["bad"][0] += int((~ok_q).sum() + (~ok_b).sum())

    def words(a):                                              # [position][read] bytes -> [word][read] little-endian words
        return np.ascontiguousarray(a.reshape(row_words, 4, pitch).transpose(0, 2, 1)).view(np.uint32).reshape(row_words, pitch)
    return words(seq), words(qual), lens, pitch, row_words, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_accumulation(trial_lib, n):
    rng = np.random.default_rng(n)
    bad_cells = [(0, 0, "quality"), (L_ROWS - 1, 0, "base")] if n > 1 else [(0, 0, "quality"), (3, 0, "base")]
    seq, qual, lens, pitch, row_words, want = crafted_rows(rng, n, [1, 3, 4, 5, 29, 30], bad_cells)
    assert int(want["bad"][0]) == 2 and want["base_quality"][:, :, 0].any() and want["base_quality"][:, :, Q_ROWS - 1].any()
    for chunk in (4, 8, 32):
        for groups in (1, 3, 16, 40):
            for skew in (0, 1):
                got = np.zeros(layout_words(trial_lib, (L_ROWS, L_ROWS), 10, Q_ROWS, 1), np.uint64)
                outside = trial_lib.stats_rows_trial(seq.ctypes.data, qual.ctypes.data, lens.ctypes.data, pitch, n, row_words, L_ROWS, L_ROWS, Q_ROWS, PHRED, chunk, 64, groups,
                                                     skew, got.ctypes.data)
                assert outside == 0, "no addition falls outside a workgroup's image, none into a row's pad"
                t, _ = tables_of(trial_lib, got, (L_ROWS, L_ROWS), 10, Q_ROWS, 1)
                same(t, want)
    # the identity of the two tables, position by position
    assert (want["base_quality"].sum(axis=2) + 0 == want["base_call"].sum(axis=2)).sum() >= 2 * L_ROWS - 2


def test_segments_of_different_lengths_and_odd_slabs(trial_lib):
    """segment 1 shorter than segment 0: its last chunk ends earlier, and nothing is counted beyond its L"""
    rng = np.random.default_rng(5)
    n = 130
    seq, qual, lens, pitch, row_words, want = crafted_rows(rng, n, [1, 3, 4, 5, 29, 30])
    lens[n:] = np.minimum(lens[n:], 21)
    want = sim_stats.empty((30, 21), 10, Q_ROWS, 1)
    s8, q8 = seq.view(np.uint8).reshape(row_words, pitch, 4), qual.view(np.uint8).reshape(row_words, pitch, 4)
    for r in range(2 * n):
        p = np.arange(lens[r])
        np.add.at(want["base_quality"], (r // n, p, q8[p // 4, r, p % 4].astype(np.int64) - PHRED), 1)
        np.add.at(want["base_call"], (r // n, p, s8[p // 4, r, p % 4]), 1)
    for chunk, slab, groups in ((8, 64, 5), (12, 100, 2), (4, 7, 64)):
        got = np.zeros(layout_words(trial_lib, (30, 21), 10, Q_ROWS, 1), np.uint64)
        assert trial_lib.stats_rows_trial(seq.ctypes.data, qual.ctypes.data, lens.ctypes.data, pitch, n, row_words, 30, 21, Q_ROWS, PHRED, chunk, slab, groups, 1, got.ctypes.data) == 0
        t, _ = tables_of(trial_lib, got, (30, 21), 10, Q_ROWS, 1)
        same(t, want)


def test_the_librarys_geometry_of_the_rows_kernel(trial_lib):
    """stats_rows_geometry, what stats_take launches k_stats_rows by, for every Q in 1 .. 250, every longest read of 1 .. 400 and both forms: the chunk is a multiple
    of four between 4 and 64, the LDS at most 48 KiB, the units cover every position of either segment and none lies behind it, and no workgroup is without a slab"""
    q_hi, l_hi = 250, 400
    Q = np.arange(1, q_hi + 1)[:, None, None]
    lmax = np.arange(1, l_hi + 1)[None, :, None]
    skew = np.arange(2)[None, None, :]
    for n_cu, n_pairs in ((256, 1), (256, 1025), (256, 5000), (256, 10_000_000), (1, 5000), (8, 3)):
        out = np.zeros((q_hi, l_hi, 2, 6), np.uint32)
        trial_lib.stats_trial_geometry_table(q_hi, l_hi, n_cu, n_pairs, out.ctypes.data)
        chunk, slab, units0, units1, lds, groups = (out[..., k].astype(np.int64) for k in range(6))
        assert (chunk % 4 == 0).all() and (chunk >= 4).all() and (chunk <= 64).all()
        assert (lds <= 48 * 1024).all()
        stride = (Q + 5) | 1                                       # the image and, staged, per wave two words a lane for every four positions
        assert (lds == (chunk * stride + skew * 4 * 2 * (chunk // 4) * 64) * 4).all()
        for units, length in ((units0, lmax + 0 * Q + 0 * skew), (units1, lmax // 2 + 0 * Q + 0 * skew)):
            assert (units * chunk >= length).all() and ((units - 1) * chunk < length).all()
        assert (slab == 1024).all()
        slabs = max(-(-n_pairs // 1024), 1)
        assert (groups >= 1).all() and (groups <= (units0 + units1) * slabs).all()
    # the options replace the three choices
    one = np.zeros(6, np.uint32)
    trial_lib.stats_trial_geometry(151, 150, 151, 42, 1, 38, 256, 5000, 0, 0, 0, one.ctypes.data)
    assert one.tolist()[:4] == [52, 1024, 3, 3]                    # (three chunks of 52, not 64 + 64 + 22)
    trial_lib.stats_trial_geometry(151, 150, 151, 42, 1, 38, 256, 5000, 7, 100, 9, one.ctypes.data)
    assert one.tolist() == [8, 100, 19, 19, (8 * 47 + 4 * 2 * 2 * 64) * 4, 9]


# ------------------------------------------------------------------------------------------------ the mates
F_MATES, Q_MATES = 400, 42


def run_mates(L, mates, frag, ref, lengths, variants=None, xi=0, has_fv=False, num_alleles=1, allele_id=0, counts=None):
    """(the tables after the pair, the pair's SAM text with NM and MD) from the trial; variants None: the plain instantiation"""
    var = variants or {}
    t, keep = fill_trial(mates, frag, 33, 0, 1101, b"ReseqRead_", NAMES)
    pos = np.array(sorted(var), np.uint32)
    length = np.array([var[p] for p in sorted(var)], np.uint32)
    v = MdIn(pair=t, allele=allele_id, num_alleles=num_alleles, seq_len=len(ref), n_variants=len(pos), var_pos=pos.ctypes.data if len(pos) else None,
             var_len=length.ctypes.data if len(pos) else None, has_fv=1 if has_fv and frag is not None else 0, ref=ref.ctypes.data)
    if v.has_fv:
        fv = fragment_var(build_allele(len(ref), var), var, frag, xi)
        v.end, v.start_var, v.start_var_pos, v.end_var, v.end_var_pos = fv["end"], fv["start_var"], fv["start_var_pos"], fv["end_var"], fv["end_var_pos"]
    if counts is None:
        counts = np.zeros(layout_words(L, lengths, F_MATES, Q_MATES, 1), np.uint64)
    cap = 16384
    sam = C.create_string_buffer(cap)
    sizes = np.zeros(2, np.uint32)
    assert L.stats_mates_trial(C.byref(v), 0 if variants is None else 1, lengths[0], lengths[1], F_MATES, Q_MATES, counts.ctypes.data, sam, cap, sizes.ctypes.data) == 0
    return counts, sam.raw[:int(sizes.sum())]


MATE_TABLES = [n for n in sim_stats.TABLES if n not in ("base_quality", "base_call")]


def check_mates(L, mates, frag, ref, lengths, classes=(), **kw):
    """every table of the mates' kernel equals the statement applied to the pair's own records, whose MD is md_nm's"""
    counts, sam = run_mates(L, mates, frag, ref, lengths, **kw)
    got, _ = tables_of(L, counts, lengths, F_MATES, Q_MATES, 1)
    text = bytes(LETTERS[c] for c in ref)
    for line in sam.splitlines():
        f = line.split(b"\t")
        if not int(f[1]) & 0x4:
            assert (int(f[-2][5:]), f[-1][5:]) == md_nm(int(f[3]), parse_cigar(f[5]), f[9], text), line
    want = sim_stats.from_sam(sam, lengths, F_MATES, Q_MATES, 1, [1101])
    if frag and frag["len"]:                                    # (the one table the records do not give)
        want["fragment_length"][frag["len"]] += 1
        assert want["strand"].tolist() == [1 - frag["strand"], frag["strand"]] and want["pairs"].tolist() == [1, 0]
    want["base_quality"][:] = 0
    want["base_call"][:] = 0
    same(got, want, MATE_TABLES)
    assert not got["bad"][0]
    met.update(classes)
    return got, sam


@pytest.fixture(scope="module")
def ref():
    return np.random.default_rng(2024).integers(0, 4, 300).astype(np.uint8)


def classes_of_ops(name):
    return {"leading D (ReSeq prints 0M first)": ("0M", "D inside the template"), "adapter part begins with I (0S)": ("0S", "I in the adapter part"),
            "adapter part begins with D (0S)": ("0S", "D in the adapter part", "H"), "I and D inside the adapter part": ("I in the adapter part", "D in the adapter part"),
            "D at both ends": ("I inside the template", "D inside the template"), "trailing I": ("I inside the template", "H"),
            "a tail alone behind the template": ("H",), "neighbouring I and D": ("I inside the template", "D inside the template")}.get(name, ())


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_the_xc_walk_on_the_crafted_ops(trial_lib, ref, name):
    """the op lists the truth tests use, as either segment on either strand"""
    rng = np.random.default_rng(sorted(CRAFTED).index(name))
    template_ops, adapter_ops, tail = CRAFTED[name]
    for strand in (0, 1):
        for seg in (0, 1):
            crafted, plain = make_mate(rng, template_ops, adapter_ops, tail, 33, with_n=True), make_mate(rng, [M] * 21, [M] * 3, 1, 33)
            mates = [plain, crafted] if seg else [crafted, plain]
            got, sam = check_mates(trial_lib, mates, fragment(1, 100, max(21, template_bases(template_ops)) + 5, strand), ref, (130, 130), classes_of_ops(name))
            xc = sam.splitlines()[seg].split(b"\t")[11]
            if "0M" in name:
                assert b":0M" in xc
            if "0S" in name:
                assert b"0S" in xc
            if tail:
                assert int(got["tail"][seg].sum()) == tail


def test_a_deletion_at_cycle_l(trial_lib, ref):
    """a read of exactly L bases whose last op is a D: the D stands at q = L and is filed at cycle L - 1"""
    rng = np.random.default_rng(3)
    for L_seg in (12, 13):
        crafted = make_mate(rng, [M] * L_seg + [D, D], [], 0, 33)
        assert crafted["read_len"] == L_seg
        got, sam = check_mates(trial_lib, [crafted, make_mate(rng, [M] * 9, [], 0, 33)], fragment(0, 50, 40, 0), ref, (L_seg, 20), ("D at cycle L",))
        assert int(got["deletion"][0, L_seg - 1]) == 2 and int(got["deletion"].sum()) == 2 and int(got["read_length"][0, L_seg]) == 1
    # ... and D runs in the adapter part and at the very end behind a tail
    crafted = make_mate(rng, [M] * 5, [M, D, M, D], 0, 33)
    got, _ = check_mates(trial_lib, [crafted, crafted], fragment(0, 50, 40, 1), ref, (7, 7), ("D in the adapter part",))
    assert got["deletion"][0].tolist() == [0, 0, 0, 0, 0, 0, 2]


def test_mismatch_cycles_on_both_strands(trial_lib, ref):
    """the crafted mate as forward and as reverse mate: the same reference positions changed give mirrored cycles"""
    rng = np.random.default_rng(11)
    n, start = 20, 40
    for change, cls in (({40}, "mismatch at the first aligned base"), ({59}, "mismatch at the last aligned base"), ({47, 48, 55}, "forward mismatch")):
        for strand in (0, 1):
            for seg in (0, 1):
                reverse = seg != strand
                mates, frag = pair_over(rng, ref, start, [M] * n, strand, seg, change=change, adapter=3)
                got, _ = check_mates(trial_lib, mates, frag, ref, (40, 40), (cls, "reverse mismatch" if reverse else "forward mismatch"))
                want = sorted((start + n - 1 - p) if reverse else (p - start) for p in change)      # (a reverse mate's first cycle reads the fragment's last base)
                assert np.flatnonzero(got["mismatch"][seg]).tolist() == want and int(got["mismatch"].sum()) == len(change)
    mates, frag = pair_over(rng, ref, start, [M] * n, 0, 0, n_at={45})
    got, _ = check_mates(trial_lib, mates, frag, ref, (40, 40), ("read base N",))
    assert got["mismatch"][0].tolist() == [0] * 5 + [1] + [0] * 34


def test_every_read_length_modulo_four_on_a_reverse_mate(trial_lib, ref):
    rng = np.random.default_rng(12)
    for n in range(1, 14):
        for adapter in (0, 1, 2, 3):
            first, last = 40, 40 + n - 1
            mates, frag = pair_over(rng, ref, 40, [M] * n, 0, 1, change={first, last}, adapter=adapter)       # segment 1 of a forward fragment: the reverse mate
            got, _ = check_mates(trial_lib, mates, frag, ref, (20, 20), ("reverse read_len mod 4 = %d" % ((n + adapter) % 4),))
            assert np.flatnonzero(got["mismatch"][1]).tolist() == sorted({0, n - 1})


def test_mismatches_beside_indels_and_mates_without_an_m_column(trial_lib, ref):
    rng = np.random.default_rng(13)
    ops = [M] * 6 + [D, D] + [M] * 3 + [I] + [M] * 6
    for strand in (0, 1):
        for seg in (0, 1):
            reverse = seg != strand
            mates, frag = pair_over(rng, ref, 60, ops[::-1] if reverse else ops, strand, seg, change={62, 68, 75}, tail=2)
            check_mates(trial_lib, mates, frag, ref, (40, 40), ("I inside the template", "D inside the template"))
            for crafted_ops, kw in (([I, I, I], dict(adapter=4, flen=9)), ([D, D], dict(adapter=5))):
                mates, frag = pair_over(rng, ref, 40, crafted_ops, strand, seg, **kw)
                got, _ = check_mates(trial_lib, mates, frag, ref, (40, 40), ("mate without an M column",))
                assert not got["mismatch"][seg].any()


def test_random_pairs_accumulate(trial_lib, ref):
    """forty random pairs into one array: the statement applied to all their records together"""
    rng = np.random.default_rng(14)
    counts, text, lens, strands = None, b"", [], []
    for k in range(40):
        strand, ops = int(rng.integers(0, 2)), []
        while sum(o != D for o in ops) < int(rng.integers(1, 40)):
            r = rng.random()
            ops.append(D if r < 0.08 else I if r < 0.16 else M)
        t = template_bases(ops)
        start = int(rng.integers(0, len(ref) - t - 30))
        frag = fragment(int(rng.integers(0, 3)), start, t + int(rng.integers(0, 25)), strand)
        end = frag["start"] + frag["len"]
        mates = []
        for seg in (0, 1):
            reverse = seg != strand
            coords = range(end - 1, end - 1 - t, -1) if reverse else range(start, start + t)
            mates.append(read_of(rng, ref, end - 1 if reverse else start, ops, reverse, adapter=int(rng.integers(0, 4)), tail=int(rng.integers(0, 2)),
                                 change={c for c in coords if rng.random() < 0.1}, n_at={c for c in coords if rng.random() < 0.03}))
        counts, sam = run_mates(trial_lib, mates, frag, ref, (50, 50), counts=counts)
        text += sam
        lens.append(frag["len"])
        strands.append(strand)
    got, _ = tables_of(trial_lib, counts, (50, 50), F_MATES, Q_MATES, 1)
    want = sim_stats.from_sam(text, (50, 50), F_MATES, Q_MATES, 1, [1101])
    want["fragment_length"] += np.bincount(lens, minlength=F_MATES + 1).astype(np.uint64)
    same(got, want, MATE_TABLES)
    assert got["mismatch"].sum() > 20 and got["insertion"].sum() > 5 and got["deletion"].sum() > 5 and got["strand"].tolist() == [strands.count(0), strands.count(1)]


def test_an_adapter_only_pair(trial_lib, ref):
    rng = np.random.default_rng(15)
    mates = [make_mate(rng, [], [M] * 9 + [I, M, D, M], 5, 33), make_mate(rng, [], [M] * 12, 3, 33, with_n=True)]
    for frag in (None, fragment(2, 77, 0, 1)):
        got, sam = check_mates(trial_lib, mates, frag, ref, (40, 40), ("adapter-only pair",))
        assert got["pairs"].tolist() == [0, 1] and not got["strand"].any() and not got["tile"].any() and not got["fragment_length"].any() and not got["mismatch"].any()
        assert int(got["adapter"].sum()) == 9 + 1 + 1 + 12 and int(got["tail"].sum()) == 8 and int(got["insertion"].sum()) == 1


def test_out_of_range_values_are_counted_as_bad_and_nowhere_else(trial_lib, ref):
    """a read longer than its segment's L: no table takes it (its elements fall outside), bad counts"""
    rng = np.random.default_rng(16)
    mates = [make_mate(rng, [M] * 12, [M] * 3, 0, 33), make_mate(rng, [M] * 9, [], 0, 33)]
    counts, sam = run_mates(trial_lib, mates, fragment(0, 50, 500, 0), ref, (10, 20))
    got, _ = tables_of(trial_lib, counts, (10, 20), F_MATES, Q_MATES, 1)
    first = sam.splitlines()[0].split(b"\t")
    beyond = [c for c in sim_stats.mismatch_cycles(parse_cigar(first[5]), first[-1][5:], False, 15) if c >= 10]
    assert int(got["bad"][0]) == 3 + len(beyond)            # the read length, the adapter element, the fragment length beyond F, the mismatches at cycles beyond L_0
    assert not got["mismatch"][0, 10:].any() and not got["read_length"][0].any() and not got["adapter"].any() and not got["fragment_length"].any() and int(got["read_length"][1, 9]) == 1


def test_a_variant_case(trial_lib, ref):
    """the VARIANTS instantiation: an allele with a deletion, an insertion and a substitution inside the stretch; a reproduced substituted base is a mismatch"""
    rng = np.random.default_rng(17)
    variants = {105: 1, 108: 0, 112: 3}
    for strand in (0, 1):
        ops = [M] * 16
        by_seg = [ops, ops[::-1]] if strand == 0 else [ops[::-1], ops]
        mates, frag, _ = var_pair(rng, ref, variants, 100, 0, 16, by_seg, strand)
        got, sam = check_mates(trial_lib, mates, frag, ref, (40, 40), ("variants",), variants=variants, has_fv=True, num_alleles=2, allele_id=1)
        assert all(b"D" in line.split(b"\t")[5] and b"I" in line.split(b"\t")[5] for line in sam.splitlines())
        assert int(got["mismatch"].sum()) == 2 and int(got["mismatch"][strand, 5]) == 1       # the forward mate reads position 105 at cycle 5


def test_every_class_was_met():
    assert met >= set(CLASSES), sorted(set(CLASSES) - met)
