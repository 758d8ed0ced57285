"""Truth pileup (include/reseq_amd.h rsq_sim_pileup_*; reseq_amd/csrc/rsq_pileup.h) without a GPU: the per-lane function pileup_mate, both instantiations, runs on the
CPU (tests/hostemu/pileup_trial.cpp, built here with g++) over crafted rows, fragments, allele maps and a crafted packed reference.  For every crafted pair the
planes -- plane 0 prefix-summed, the reference letter's count filled in -- must be, exactly, the table that tests/truth_pileup.py reads off the pair's own SAM
records: the records sam_record / SamVarFormat::record write for the same rows, which tests/test_truth_sam.py and tests/test_truth_variants.py check against their
statements of the rules.  tests/test_truth_pileup_gpu.py requires the same of the device."""
import ctypes as C

import numpy as np
import pytest

from test_truth_md import LETTERS, MdIn, pair_over, read_of, var_pair
from test_truth_sam import D, I, M, NAMES, build_trial, fill_trial, fragment
from test_truth_variants import build_allele, fragment_var
from truth_pileup import DEL, DEPTH, INS, header_line, pileup_from_sam, pileup_text

SEQS = len(NAMES)
PLANES = 8
# what the crafted cases below must have met, each at least once (`met` collects them and the last test compares)
CLASSES = tuple("mismatch to %s %s" % (b, o) for b in "ACGTN" for o in ("forward", "reverse")) + (
    "no mismatch: two words", "D inside", "D leading dropped forward", "D leading dropped reverse", "D trailing dropped forward", "D trailing dropped reverse", "I inside",
    "I leading", "I clamped to position 0", "mate wholly inside an insertion", "variant deletion inside", "substitution-only set", "M run of 15", "M run of 16",
    "M run of 17", "M run of 32", "M run of 33", "mismatch on the last base", "mismatch on the first base", "overlapping mates add 2", "clip only", "strands add up",
    "line trial")
met = set()


@pytest.fixture(scope="module")
def trial_lib(tmp_path_factory):
    L = build_trial(tmp_path_factory, "pileup_trial")
    L.pileup_trial.argtypes = [C.POINTER(MdIn), C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_void_p]
    L.pileup_row_trial.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    L.pileup_line_trial.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32]
    return L


@pytest.fixture(scope="module")
def ref():
    return np.random.default_rng(2025).integers(0, 4, 300).astype(np.uint8)


def run_pair(L, mates, frag, ref, instantiation, strands, variants=None, xi=0, has_fv=False, num_alleles=1, allele_id=0, planes=None):
    """(the planes [S * 8, SEQS * (len + 1)], the pair's SAM text) from the trial; instantiation: 0 plain, 1 with variants"""
    variants = variants or {}
    t, keep = fill_trial(mates, frag, 33, 0, 1101, b"ReseqRead_", NAMES)
    pos = np.array(sorted(variants), np.uint32)
    length = np.array([variants[p] for p in sorted(variants)], np.uint32)
    v = MdIn(pair=t, allele=allele_id, num_alleles=num_alleles, seq_len=len(ref), n_variants=len(pos), var_pos=pos.ctypes.data if len(pos) else None,
             var_len=length.ctypes.data if len(pos) else None, has_fv=1 if has_fv else 0, ref=ref.ctypes.data)
    if v.has_fv:
        fv = fragment_var(build_allele(len(ref), variants), variants, frag, xi)
        v.end, v.start_var, v.start_var_pos, v.end_var, v.end_var_pos = fv["end"], fv["start_var"], fv["start_var_pos"], fv["end_var"], fv["end_var_pos"]
    words = SEQS * (len(ref) + 1)
    if planes is None:
        planes = np.zeros(((2 if strands else 1) * PLANES, words), np.uint32)
    cap = 16384
    sam = C.create_string_buffer(cap)
    sizes = np.zeros(2, np.uint32)
    assert L.pileup_trial(C.byref(v), instantiation, 1 if strands else 0, planes.ctypes.data, words, sam, cap, sizes.ctypes.data) == 0
    return planes, sam.raw[:int(sizes.sum())]


def tables_of(planes, ref):
    """the planes as full counts [len, S, 8] per sequence: plane 0's flat prefix sum modulo 2^32 (every sequence's extra word must end as 0, and nothing but
    plane 0 may touch it), the reference letter's count = depth - the five stored ones (its own plane must hold 0)"""
    n = len(ref)
    sets = planes.shape[0] // PLANES
    p = planes.reshape(sets, PLANES, SEQS, n + 1).copy()
    p[:, 0] = np.cumsum(planes.reshape(sets, PLANES, -1)[:, 0], axis=1, dtype=np.uint32).reshape(sets, SEQS, n + 1)
    assert not p[:, :, :, n].any(), "every sequence's differences sum to zero and no other plane touches the extra word"
    out = []
    for s in range(SEQS):
        t = p[:, :, s, :n].transpose(2, 0, 1).copy()                  # [pos, set, plane]
        own = 1 + ref.astype(np.int64)
        assert not t[np.arange(n), :, own].any(), "the reference letter's own count is never stored"
        t[np.arange(n), :, own] = t[:, :, 0] - t[:, :, 1:6].sum(axis=2, dtype=np.uint32)
        out.append(t)
    return out


def note_mismatch_classes(want, ref):
    own = 1 + ref.astype(np.int64)
    for s, orientation in ((0, "forward"), (1, "reverse")):
        for c, letter in enumerate("ACGTN", start=1):
            hit = want[:, s, c] > 0
            if (hit & (own != c)).any():
                met.add("mismatch to %s %s" % (letter, orientation))


def check_pair(L, mates, frag, ref, classes=(), variants=None, **kw):
    """planes == pileup_from_sam(the pair's own records), exactly, unstranded and per strand; forward + reverse == unstranded.  variants None: both instantiations
    (the one with variants over a reference without any).  Returns (the stranded tables, the records' fields)."""
    refs = {n: bytes(LETTERS[c] for c in ref) for n in NAMES}
    runs = [(0, {}), (1, dict(num_alleles=2, allele_id=1))] if variants is None else [(1, dict(dict(num_alleles=2, allele_id=1, has_fv=True), variants=variants, **kw))]
    out = None
    for instantiation, kv in runs:
        got = {}
        for strands in (False, True):
            planes, sam = run_pair(L, mates, frag, ref, instantiation, strands, **kv)
            got[strands], want = tables_of(planes, ref), pileup_from_sam(sam, refs, strands)
            for s in range(SEQS):
                assert got[strands][s].shape == want[s].shape
                assert (got[strands][s] == want[s]).all(), (instantiation, strands, s, np.argwhere(got[strands][s] != want[s])[:10], sam)
        for s in range(SEQS):
            assert (got[True][s].sum(axis=1, dtype=np.uint32) == got[False][s][:, 0]).all()
        met.add("strands add up")
        for s in range(SEQS):
            note_mismatch_classes(got[True][s], ref)
        if out is None:
            out = got[True], [line.split(b"\t") for line in sam.splitlines()]
    met.update(classes)
    return out


def crafted(L, ref, start, ops, classes=lambda reverse: (), seq_check=None, **kw):
    """the crafted mate as forward and as reverse mate, on either strand; ops, change and n_at in REFERENCE order (as tests/test_truth_md.py crafted).  Returns the
    stranded table of sequence 1 and the crafted record's fields of the last run."""
    rng = np.random.default_rng(len(ops) * 977 + start)
    for strand in (0, 1):
        for seg in (0, 1):
            reverse = seg != strand
            mates, frag = pair_over(rng, ref, start, ops[::-1] if reverse else ops, strand, seg, **kw)
            tables, fields = check_pair(L, mates, frag, ref, classes(reverse))
            if seq_check:
                seq_check(tables[1], fields[seg], reverse)
    return tables[1], fields[seg]


def test_mismatches_to_every_letter_on_both_strands(trial_lib, ref):
    for k, start in enumerate((20, 61, 97, 140)):
        crafted(trial_lib, ref, start, [M] * 40, change={start + 3, start + 4, start + 17, start + 31, start + 39}, n_at={start + 9 + k})
    # the letter a reverse mate's mismatch is filed under is SEQ's as written: the complement of the read's own base
    rng = np.random.default_rng(3)
    mates, frag = pair_over(rng, ref, 50, [M] * 10, 0, 1)
    mates[1]["seq"][:] = [3 - int(c) for c in ref[50:60][::-1]]
    mates[1]["seq"][0] = 3 - ((int(ref[59]) + 1) % 4)                 # the read's first base is the reference's last
    tables, _ = check_pair(trial_lib, mates, frag, ref)
    assert tables[1][59, 1, 1 + (int(ref[59]) + 1) % 4] == 1 and tables[1][59, 1, 1 + int(ref[59])] == 0


def test_a_read_without_a_mismatch_costs_two_additions(trial_lib, ref):
    rng = np.random.default_rng(4)
    for strand in (0, 1):
        for seg in (0, 1):
            mates, frag = pair_over(rng, ref, 70, [M] * 41, strand, seg)
            mates[1 - seg] = read_of(rng, ref, 0, [], False, adapter=9)    # a clip-only mate: nothing
            for instantiation, kv in ((0, {}), (1, dict(num_alleles=2, allele_id=1))):
                for strands in (False, True):
                    planes, _ = run_pair(trial_lib, mates, frag, ref, instantiation, strands, **kv)
                    assert np.count_nonzero(planes) == 2
            tables, fields = check_pair(trial_lib, mates, frag, ref, ("no mismatch: two words", "clip only"))
            assert b"M" not in fields[1 - seg][5] and int(tables[1][:, :, DEPTH].sum()) == 41


def test_deletions(trial_lib, ref):
    def inside(t, f, reverse):
        assert b"2D" in f[5] and (t[105:107, :, DEL].sum(axis=1) == 1).all() and int(t[:, :, DEL].sum()) == 2
    crafted(trial_lib, ref, 100, [M] * 5 + [D, D] + [M] * 9, lambda r: ("D inside",), inside)

    def dropped(t, f, reverse):
        assert b"D" not in f[5] and not t[:, :, DEL].any()
    crafted(trial_lib, ref, 100, [D, D, M, M, M, M, M], lambda r: ("D leading dropped reverse" if r else "D leading dropped forward",), dropped)
    crafted(trial_lib, ref, 100, [M, M, M, M, D, D, D], lambda r: ("D trailing dropped reverse" if r else "D trailing dropped forward",), dropped)
    crafted(trial_lib, ref, 100, [D, M, M, M, I, I, M, D, M, M, D], adapter=2, change={102})
    crafted(trial_lib, ref, 100, [D] + [M] * 16 + [D] + [M] * 16 + [D], change={117, 118})


def test_insertions(trial_lib, ref):
    def inside(t, f, reverse):
        assert b"2I" in f[5] and int(t[:, :, INS].sum()) == 1 and t[103, :, INS].sum() == 1          # ONE count per element, on the base in front
    crafted(trial_lib, ref, 100, [M] * 4 + [I, I] + [M] * 6, lambda r: ("I inside",), inside)

    def leading(t, f, reverse):
        cigar = f[5].replace(b"3S", b"")
        assert cigar == b"1I8M" and int(f[3]) == 101 and t[99, :, INS].sum() == 1 and not t[99, :, DEPTH].any()
    crafted(trial_lib, ref, 100, [I] + [M] * 8, lambda r: ("I leading",), leading, adapter=3)

    def clamped(t, f, reverse):
        assert int(f[3]) == 1 and t[0, :, INS].sum() == 1 and int(t[:, :, INS].sum()) == 1 and t[0, :, DEPTH].sum() >= 1
    crafted(trial_lib, ref, 0, [I, I] + [M] * 8, lambda r: ("I clamped to position 0",), clamped)
    # a dropped leading D in front of an I: the I stands at POS - 2, on the last deleted position
    def behind_d(t, f, reverse):
        assert f[5] == b"1I4M" and int(f[3]) == 103 and t[101, :, INS].sum() == 1
    crafted(trial_lib, ref, 100, [D, D, I, M, M, M, M], seq_check=behind_d)


@pytest.mark.parametrize("n", [15, 16, 17, 32, 33])
def test_the_seams_of_the_sixteen_column_and_the_32_base_steps(trial_lib, ref, n):
    for start in (37, 64, 95):
        crafted(trial_lib, ref, start, [M] * n, lambda r: ("M run of %d" % n,), change={start, start + n - 1, start + n // 2}, adapter=1)
        crafted(trial_lib, ref, start, [M] * n + [D] + [M] * n, change={start + n - 1, start + n + 1})
        crafted(trial_lib, ref, start, [M] * n + [I] + [M] * n, n_at={start + n})


def test_the_ends_of_the_sequence(trial_lib, ref):
    n = len(ref)

    def last(t, f, reverse):
        assert t[n - 1, :, 1:6].sum() - t[n - 1, :, 1 + int(ref[n - 1])].sum() == 1
    crafted(trial_lib, ref, n - 35, [M] * 35, lambda r: ("mismatch on the last base",), last, change={n - 1})

    def first(t, f, reverse):
        assert t[0, :, 1:6].sum() - t[0, :, 1 + int(ref[0])].sum() == 1
    crafted(trial_lib, ref, 0, [M] * 35, lambda r: ("mismatch on the first base",), first, change={0})
    # in every sequence: nothing leaves it
    rng = np.random.default_rng(6)
    for seq in range(SEQS):
        mates, frag = pair_over(rng, ref, n - 20, [M] * 20, 0, 0, change={n - 1, n - 20})
        frag = fragment(seq, n - 20, 20, 0)
        tables, _ = check_pair(trial_lib, mates, frag, ref)
        assert all(tables[s].any() == (s == seq) for s in range(SEQS))


def test_overlapping_mates_and_pairs_accumulate(trial_lib, ref):
    rng = np.random.default_rng(8)
    mates, frag = pair_over(rng, ref, 100, [M] * 30, 0, 0, other_len=30, change={110})
    tables, _ = check_pair(trial_lib, mates, frag, ref, ("overlapping mates add 2",))
    assert (tables[1][100:130, :, DEPTH].sum(axis=1) == 2).all() and tables[1][110, 0, 1:6].sum() == 1 and tables[1][110, 1, 1 + int(ref[110])] == 1
    # several pairs into the same planes: the table of their records together
    refs = {name: bytes(LETTERS[c] for c in ref) for name in NAMES}
    for strands in (False, True):
        planes, text = None, b""
        for k in range(40):
            ops = [[M, D, I][int(x)] for x in rng.choice(3, int(rng.integers(1, 60)), p=[0.9, 0.05, 0.05])] + [M]
            start = int(rng.integers(0, 200))
            strand, seg = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            mates, frag = pair_over(rng, ref, start, ops[::-1] if seg != strand else ops, strand, seg, change={start + int(x) for x in rng.integers(0, 40, 4)},
                                    adapter=int(rng.integers(0, 4)))
            planes, sam = run_pair(trial_lib, mates, frag, ref, 0, strands, planes=planes)
            text += sam
        got, want = tables_of(planes, ref), pileup_from_sam(text, refs, strands)
        assert all((g == w).all() for g, w in zip(got, want)) and int(got[1][:, :, DEPTH].max()) >= 3


def test_an_unmapped_pair_adds_nothing(trial_lib, ref):
    rng = np.random.default_rng(9)
    mates = [read_of(rng, ref, 0, [], False, adapter=9, tail=2), read_of(rng, ref, 0, [], False, adapter=12)]
    for instantiation, kv in ((0, {}), (1, dict(num_alleles=2, allele_id=1, variants={5: 3}))):
        planes, sam = run_pair(trial_lib, mates, fragment(2, 77, 0, 1), ref, instantiation, True, **kv)
        assert not planes.any() and [line.split(b"\t")[1] for line in sam.splitlines()] == [b"77", b"141"]


def var_both(L, ref, variants, start, length, ops, classes=(), xi=0, **kw):
    """the same template ops as forward and (reversed) as reverse mate over the allele, on either strand; returns sequence 1's stranded table and the records"""
    rng = np.random.default_rng(start * 31 + length)
    for strand in (0, 1):
        by_seg = [ops, ops[::-1]] if strand == 0 else [ops[::-1], ops]
        mates, frag, _ = var_pair(rng, ref, variants, start, xi, length, by_seg, strand, **kw)
        tables, fields = check_pair(L, mates, frag, ref, classes, variants=variants, xi=xi)
    return tables[1], fields


def test_variants_inside_the_stretch(trial_lib, ref):
    L = trial_lib
    t, fields = var_both(L, ref, {105: 0}, 100, 12, [M] * 12, ("variant deletion inside",))
    assert fields[0][5] == b"5M1D7M" and t[105, :, DEL].sum() == 2 and t[105, :, DEPTH].sum() == 0 and int(t[:, :, DEL].sum()) == 2
    t, fields = var_both(L, ref, {105: 3}, 100, 12, [M] * 12)                                  # 6M2I4M: the insertion stands on the base it follows
    assert fields[0][5] == b"6M2I4M" and t[105, :, INS].sum() == 2 and int(t[:, :, INS].sum()) == 2
    t, _ = var_both(L, ref, {105: 1}, 100, 12, [M] * 12)                                       # a substituted allele base the read reproduces
    assert t[105, :, 1:6].sum() == 2 and t[105, :, 1 + int(ref[105])].sum() == 0
    var_both(L, ref, {104: 0, 105: 4, 106: 0}, 100, 12, [M] * 12)
    var_both(L, ref, {103: 0}, 100, 5, [M, M, D, M, M])
    var_both(L, ref, {101: 0, 102: 0}, 100, 4, [D, M, M, M])
    var_both(L, ref, {115: 2}, 100, 48, [M] * 48, change={130})
    var_both(L, ref, {116: 0}, 100, 48, [M] * 40 + [I] + [M] * 8)
    var_both(L, ref, {40: 0, 41: 3, 250: 2}, 100, 12, [M] * 12)                                # no entry in reach: the plain walk
    var_both(L, ref, {len(ref) - 1: 3}, len(ref) - 4, 6, [M] * 6)
    var_both(L, ref, {0: 3}, 0, 6, [M] * 6)


def test_a_mate_wholly_inside_an_insertion(trial_lib, ref):
    """nI and the clip: one insertion on the base the variant's insertion follows, no depth from that mate"""
    rng = np.random.default_rng(77)
    variants = {150: 20}
    for strand in (0, 1):
        for forward in (True, False):
            frag = fragment(0, 150, 60, strand) if forward else fragment(0, 100, 50 + 12, strand)
            seg = strand if forward else 1 - strand
            inside = read_of(rng, ref, 10, [M, M, I, M, D, M, M], False, adapter=2)
            other = read_of(rng, ref, 10, [M] * 30, False)
            mates = [other, other]
            mates[seg] = inside
            tables, fields = check_pair(trial_lib, mates, frag, ref, ("mate wholly inside an insertion",), variants=variants, xi=3 if forward else 0)
            assert fields[seg][5] == (b"6I2S" if forward else b"2S6I") and int(fields[seg][3]) == 152
            assert tables[0][150, 1 if int(fields[seg][1]) & 0x10 else 0, INS] == 1
            assert int(tables[0][:, :, DEPTH].sum()) == 30                                          # the other mate's bases alone


def test_a_substitution_only_set(trial_lib, ref):
    """allele copies: no FragmentVar, the fragment's own coordinates; the comparison is against the reference as loaded"""
    rng = np.random.default_rng(32)
    variants = {105: 1}
    for strand in (0, 1):
        mates, frag, _ = var_pair(rng, ref, variants, 100, 0, 12, [[M] * 12, [M] * 12], strand)
        tables, fields = check_pair(trial_lib, mates, frag, ref, ("substitution-only set",), variants=variants, has_fv=False)
        assert tables[1][105, :, 1:6].sum() == 2 and tables[1][105, :, 1 + int(ref[105])].sum() == 0


def test_rows_and_lines(trial_lib):
    """pileup_row and pileup_keep; pileup_line through the image sink, at every phase, equals the plain sink's and its stated size"""
    rng = np.random.default_rng(12)
    for _ in range(200):
        sets, refc = int(rng.integers(1, 3)), int(rng.integers(0, 4))
        planes = rng.integers(0, 3, (sets, PLANES)).astype(np.uint32) * rng.integers(0, 2, (sets, PLANES)).astype(np.uint32)
        planes[:, 1 + refc] = 0
        planes[:, 0] = planes[:, 1:6].sum(axis=1) + rng.integers(0, 3, sets)
        v = np.zeros((sets, PLANES), np.uint32)
        keep = [trial_lib.pileup_row_trial(planes.ctypes.data, sets, refc, a, v.ctypes.data) for a in (0, 1)]
        want = planes.copy()
        want[:, 1 + refc] = planes[:, 0] - planes[:, 1:6].sum(axis=1)
        other = want.copy()
        other[:, [0, 1 + refc]] = 0
        assert (v == want).all() and keep == [int(other.any()), int(want.any())]
    names = list(NAMES) + [b"a_long_name_" + b"x" * 600]
    name_ptr = np.concatenate([[0], np.cumsum([len(n) for n in names])]).astype(np.uint32)
    out = C.create_string_buffer(2048)
    big = 4294967295
    rows = ([0] * 8, [1, 1, 0, 0, 0, 0, 0, 0], [12, 9, 1, 0, 2, 0, 3, 1], [big] * 8, [1234567890, 999999999, 1000000000, 10, 9, 99999, 100000, 4294967295])
    for sets in (1, 2):
        for seq, pos in ((0, 0), (1, 8), (2, 99998), (1, 4294967294), (3, 4095)):
            for k, row in enumerate(rows):
                v = np.array(row + rows[(k + 1) % len(rows)] if sets == 2 else row, np.uint32)
                for at in range(4):
                    n = trial_lib.pileup_line_trial(b"".join(names), name_ptr.ctypes.data, seq, pos, k % 4, v.ctypes.data, sets, at, out, 2048)
                    assert n > 0 and out.raw[:n] == b"%s\t%d\t%c\t%s\n" % (names[seq], pos + 1, LETTERS[k % 4], b"\t".join(b"%d" % x for x in v.tolist()))
    met.add("line trial")


def test_the_statement_reads_a_cigar_and_writes_the_text():
    sam = (b"@HD\tVN:1.6\nr\t99\tx\t3\t60\t2S2M1I1D2M\t=\t1\t0\tAAACNTG\tIIIIIII\nr\t77\t*\t0\t0\t*\t*\t0\t0\tA\tI\nq\t147\ty\t1\t60\t1I3M\t=\t1\t0\tGAAA\tIIII\n"
           b"p\t83\tx\t5\t60\t1I1M\t*\t0\t0\tTT\tII\n")
    refs = {b"x": b"ACGTACGT", b"y": b"AAA"}
    x, y = pileup_from_sam(sam, refs, False)
    assert x.dtype == np.uint32 and x.shape == (8, 1, 8) and y.shape == (3, 1, 8)
    assert x[:, 0, DEPTH].tolist() == [0, 0, 1, 1, 1, 1, 1, 0] and x[:, 0, DEL].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and x[:, 0, INS].tolist() == [0, 0, 0, 2, 0, 0, 0, 0]
    assert x[2, 0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and x[3, 0].tolist() == [1, 0, 1, 0, 0, 0, 0, 2] and x[5, 0, 4] == 1 and x[6, 0, 3] == 1
    assert y[:, 0, DEPTH].tolist() == [1, 1, 1] and y[0, 0, INS] == 1                              # the clamp
    xs, ys = pileup_from_sam(sam, refs, True)
    assert (xs.sum(axis=1) == x[:, 0]).all() and ys[:, 0].sum() == 0 and xs[3, 1, INS] == 1 and xs[4, 1].tolist() == [1, 0, 0, 0, 1, 0, 0, 0]
    sites = pileup_text([b"x", b"y"], [refs[b"x"], refs[b"y"]], [x, y], False)
    assert sites == (b"x\t3\tG\t1\t1\t0\t0\t0\t0\t0\t0\nx\t4\tT\t1\t0\t1\t0\t0\t0\t0\t2\nx\t5\tA\t1\t0\t0\t0\t1\t0\t1\t0\nx\t6\tC\t1\t0\t0\t0\t1\t0\t0\t0\n"
                     b"y\t1\tA\t1\t1\t0\t0\t0\t0\t0\t1\n")
    lines = sites.splitlines()
    assert [l.split(b"\t")[1] for l in lines] == [b"3", b"4", b"5", b"6", b"1"] and lines[1] == b"x\t4\tT\t1\t0\t1\t0\t0\t0\t0\t2" and lines[-1] == b"y\t1\tA\t1\t1\t0\t0\t0\t0\t0\t1"
    everything = pileup_text([b"x", b"y"], [refs[b"x"], refs[b"y"]], [x, y], True).splitlines()
    assert [l.split(b"\t")[:2] for l in everything] == [[b"x", b"%d" % p] for p in (3, 4, 5, 6, 7)] + [[b"y", b"%d" % p] for p in (1, 2, 3)]
    assert header_line(False) == b"#chrom\tpos\tref\tdepth\tA\tC\tG\tT\tN\tdel\tins\n" and header_line(True).count(b"+") == 8 and header_line(True).endswith(b"\tdel-\tins-\n")


def test_every_class_was_met():
    assert met >= set(CLASSES), sorted(set(CLASSES) - met)
