"""Truth depth (include/reseq_amd.h rsq_sim_depth_*; reseq_amd/csrc/rsq_depth.h) without a GPU: the per-lane function depth_mate, both instantiations, runs on the
CPU (tests/hostemu/depth_trial.cpp, built here with g++) over crafted rows, fragments and allele maps.  For every crafted pair the prefix sum of the array of
differences must be, exactly, the depth that tests/truth_depth.py reads off the pair's own SAM records -- the records sam_record / SamVarFormat::record write for
the same rows, which tests/test_truth_sam.py and tests/test_truth_variants.py check against their statements of the rules.  tests/test_truth_depth_gpu.py
requires the same of the device."""
import ctypes as C

import numpy as np
import pytest

from test_truth_sam import D, I, M, NAMES, build_trial, fill_trial, fragment, make_mate, template_bases
from test_truth_variants import VarIn, build_allele, fragment_var
from truth_depth import bedgraph_from_depth, depth_from_sam

SEQS = len(NAMES)
# what the crafted cases below must have met, each at least once (a case names its classes; `met` collects them and the last test compares)
CLASSES = ("plain forward", "plain reverse", "D inside", "I inside", "D leading forward", "D leading reverse", "D trailing forward", "D trailing reverse", "D alone",
           "n_iter_m 15", "n_iter_m 16", "n_iter_m 17", "n_iter_m 32", "last base of the sequence", "clip only", "variant insertion inside", "variant deletion inside",
           "mate wholly inside an insertion", "substitution-only set")
met = set()


@pytest.fixture(scope="module")
def trial_lib(tmp_path_factory):
    L = build_trial(tmp_path_factory, "depth_trial")
    L.depth_trial.argtypes = [C.POINTER(VarIn), C.c_int, C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p]
    L.depth_line_trial.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32]
    return L


def run_pair(L, mates, frag, seq_len, variants=None, xi=0, has_fv=True, diff=None, allele_id=1, num_alleles=2):
    """(the array of differences [SEQS * (seq_len + 1)], the pair's SAM text) from the trial; variants None: the plain instantiation"""
    t, keep = fill_trial(mates, frag, 33, 0, 1101, b"ReseqRead_", NAMES)
    var = variants or {}
    pos = np.array(sorted(var), np.uint32)
    length = np.array([var[p] for p in sorted(var)], np.uint32)
    v = VarIn(pair=t, allele=allele_id, num_alleles=num_alleles, seq_len=seq_len, n_variants=len(pos), var_pos=pos.ctypes.data if len(pos) else None,
              var_len=length.ctypes.data if len(pos) else None, has_fv=1 if variants is not None and has_fv else 0)
    if v.has_fv:
        fv = fragment_var(build_allele(seq_len, var), var, frag, xi)
        v.end, v.start_var, v.start_var_pos, v.end_var, v.end_var_pos = fv["end"], fv["start_var"], fv["start_var_pos"], fv["end_var"], fv["end_var_pos"]
    if diff is None:
        diff = np.zeros(SEQS * (seq_len + 1), np.uint32)
    cap = 16384
    sam = C.create_string_buffer(cap)
    sizes = np.zeros(2, np.uint32)
    assert L.depth_trial(C.byref(v), 0 if variants is None else 1, diff.ctypes.data, sam, cap, sizes.ctypes.data) == 0
    return diff, sam.raw[:int(sizes.sum())]


def depths_of(diff, seq_len):
    """the flat prefix sum modulo 2^32, cut into sequences: every sequence's extra word must end as 0"""
    flat = np.cumsum(diff, dtype=np.uint32).reshape(SEQS, seq_len + 1)
    assert (flat[:, -1] == 0).all(), "every sequence's differences sum to zero"
    return [flat[s, :-1] for s in range(SEQS)]


def check_pair(L, mates, frag, seq_len, classes=(), **kw):
    """cumsum(differences) == depth_from_sam(the pair's own records), exactly; returns (depths, the records' fields)"""
    diff, sam = run_pair(L, mates, frag, seq_len, **kw)
    got, want = depths_of(diff, seq_len), depth_from_sam(sam, [seq_len] * SEQS, NAMES)
    for s in range(SEQS):
        assert (got[s] == want[s]).all(), (s, np.flatnonzero(got[s] != want[s])[:10], sam)
    assert np.count_nonzero(diff) <= 2 * sum(line.split(b"\t")[5].count(b"M") for line in sam.splitlines()), "two additions per M element"
    met.update(classes)
    return got, [line.split(b"\t") for line in sam.splitlines()]


PLAIN = [M] * 21


@pytest.mark.parametrize("strand", [0, 1])
def test_plain_mates_of_both_strands(trial_lib, strand):
    rng = np.random.default_rng(1 + strand)
    mates = [make_mate(rng, [M] * 30, [M, M], 1, 33), make_mate(rng, [M] * 25, [], 0, 33)]
    got, fields = check_pair(trial_lib, mates, fragment(1, 100, 70, strand), 400, ("plain forward", "plain reverse"))
    fwd, rev = (0, 1) if strand == 0 else (1, 0)
    n = [30, 25]
    want = np.zeros(400, np.uint32)
    want[100:100 + n[fwd]] += 1
    want[170 - n[rev]:170] += 1
    assert (got[1] == want).all() and not got[0].any() and not got[2].any()
    # overlapping mates add
    got, _ = check_pair(trial_lib, mates, fragment(2, 10, 40, strand), 400)
    assert got[2].max() == 2 and int(got[2].sum()) == 55


CRAFTED = {
    # name: (template ops, adapter ops, classes as the forward mate, classes as the reverse mate)
    "D and I inside": ([M] * 5 + [D, D] + [M] * 4 + [I] + [M] * 6, [M, M], ("D inside", "I inside"), ("D inside", "I inside")),
    "leading D": ([D, D, M, M, M, I, M, M], [], ("D leading forward",), ("D leading reverse",)),
    "trailing D": ([M, M, M, M, D, M, M, D, D, D], [], ("D trailing forward",), ("D trailing reverse",)),
    "D at both ends": ([D, M, M, M, I, I, M, D, M, M, D], [M, M], ("D leading forward", "D trailing forward"), ("D leading reverse", "D trailing reverse")),
    "a template part of D alone": ([D, D, D], [M, M, M, M], ("D alone",), ("D alone",)),
    "sixteen plain ops between two D": ([D] + [M] * 16 + [D] + [M] * 16 + [D], [], (), ()),
    "a clip only": ([], [M] * 9, ("clip only",), ("clip only",)),
}


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_ops(trial_lib, name):
    rng = np.random.default_rng(sorted(CRAFTED).index(name))
    template_ops, adapter_ops, as_forward, as_reverse = CRAFTED[name]
    for strand in (0, 1):
        for seg in (0, 1):                                    # the crafted mate as either segment: forward and reverse
            crafted, plain = make_mate(rng, template_ops, adapter_ops, 0, 33), make_mate(rng, PLAIN, [M] * 3, 1, 33)
            mates = [plain, crafted] if seg else [crafted, plain]
            got, fields = check_pair(trial_lib, mates, fragment(1, 321, max(21, template_bases(template_ops)) + 5, strand), 700, as_forward if seg == strand else as_reverse)
            cigar = fields[seg][5]
            if "D" in name and "alone" not in name:
                assert b"D" in cigar or "leading" in name or "trailing" in name
            if name in ("a template part of D alone", "a clip only"):
                assert b"M" not in cigar and int(got[1].sum()) == 21     # the other mate's 21 bases and nothing else


@pytest.mark.parametrize("n_iter_m", [15, 16, 17, 32])
def test_the_seams_of_the_sixteen_op_path(trial_lib, n_iter_m):
    """template parts of 15, 16, 17 and 32 iterations, plain and with an indel in every position's word, in both orientations"""
    rng = np.random.default_rng(n_iter_m)
    for strand in (0, 1):
        for ops in ([M] * n_iter_m, [M] * (n_iter_m - 1) + [D], [D] + [M] * (n_iter_m - 1), [M] * (n_iter_m // 2) + [I] + [M] * (n_iter_m - n_iter_m // 2 - 1),
                    [M] * (n_iter_m - 2) + [D, M]):
            assert len(ops) == n_iter_m
            mates = [make_mate(rng, ops, [M], 0, 33), make_mate(rng, ops[::-1], [], 2, 33)]
            check_pair(trial_lib, mates, fragment(0, 50, 40, strand), 200, ("n_iter_m %d" % n_iter_m,))


def test_a_read_that_reaches_the_last_base_of_its_sequence(trial_lib):
    """the -1 behind it lands on the sequence's extra word, not on the next sequence's first base"""
    rng = np.random.default_rng(7)
    seq_len = 120
    for seq in (0, 1, 2):
        for strand in (0, 1):
            mates = [make_mate(rng, [M] * 30, [], 0, 33), make_mate(rng, [M] * 12 + [I] + [M] * 12, [M], 0, 33)]
            diff, _ = run_pair(trial_lib, mates, fragment(seq, seq_len - 50, 50, strand), seq_len)
            flat = diff.reshape(SEQS, seq_len + 1)
            assert flat[seq, seq_len] == 0xFFFFFFFF and not np.delete(flat, seq, axis=0).any()
            got, _ = check_pair(trial_lib, mates, fragment(seq, seq_len - 50, 50, strand), seq_len, ("last base of the sequence",))
            assert got[seq][-1] == 1 and got[seq][0] == 0
    # ... and one that begins at a sequence's first base
    got, _ = check_pair(trial_lib, mates, fragment(1, 0, 50, 0), seq_len)
    assert got[1][0] == 1


def test_pairs_accumulate_into_one_array(trial_lib):
    """several pairs into the same array: the depth of their records together"""
    rng = np.random.default_rng(8)
    seq_len, diff, text = 300, None, b""
    for k in range(40):
        ops = [[M, D, I][int(x)] for x in rng.choice(3, int(rng.integers(1, 60)), p=[0.9, 0.05, 0.05])] + [M]
        mates = [make_mate(rng, ops, [M] * int(rng.integers(0, 4)), 0, 33), make_mate(rng, [M] * int(rng.integers(1, 60)), [], 0, 33)]
        length = max(template_bases(m["ops"][:m["n_iter_m"]]) for m in mates) + int(rng.integers(0, 20))
        diff, sam = run_pair(trial_lib, mates, fragment(int(rng.integers(0, 3)), int(rng.integers(0, seq_len - length + 1)), length, int(rng.integers(0, 2))), seq_len, diff=diff)
        text += sam
    got, want = depths_of(diff, seq_len), depth_from_sam(text, [seq_len] * SEQS, NAMES)
    assert all((g == w).all() for g, w in zip(got, want)) and max(int(g.max()) for g in got) >= 3


def test_an_unmapped_pair_adds_nothing(trial_lib):
    rng = np.random.default_rng(9)
    mates = [make_mate(rng, [], [M] * 9, 2, 33), make_mate(rng, [], [M] * 12, 0, 33)]
    for variants in (None, {5: 3}):
        diff, sam = run_pair(trial_lib, mates, fragment(2, 77, 0, 1), 100, variants=variants, has_fv=False)
        assert not diff.any() and [line.split(b"\t")[1] for line in sam.splitlines()] == [b"77", b"141"]


def var_both_strands(L, ops, variants, seq_len, start, classes, xi=0, flen=None, **kw):
    """the fragment is exactly the template part of `ops`; the forward mate reads it in order, the reverse mate (ops reversed) from the other end, on either strand"""
    rng = np.random.default_rng(len(ops) + start)
    out = []
    for strand in (0, 1):
        fwd, rev = make_mate(rng, ops, [M, M], 0, 33), make_mate(rng, ops[::-1], [], 0, 33)
        frag = fragment(1, start, template_bases(ops) if flen is None else flen, strand)
        got, fields = check_pair(L, [fwd, rev] if strand == 0 else [rev, fwd], frag, seq_len, classes, variants=variants, xi=xi, **kw)
        out.append((got[1], fields))
    assert (out[0][0] == out[1][0]).all()
    return out[0]


def test_variants_inside_the_stretch(trial_lib):
    L = trial_lib
    d, fields = var_both_strands(L, [M] * 12, {105: 3}, 300, 100, ("variant insertion inside",))       # 6M2I4M: ten reference positions
    assert fields[0][5].replace(b"2S", b"") == b"6M2I4M" and (d[100:110] == 2).all() and d[110] == 0 and int(d.sum()) == 20
    d, fields = var_both_strands(L, [M] * 12, {105: 0}, 300, 100, ("variant deletion inside",))         # 5M1D7M: the deleted position is not covered
    assert fields[0][5].replace(b"2S", b"") == b"5M1D7M" and d[105] == 0 and (d[100:105] == 2).all() and (d[106:113] == 2).all()
    d, fields = var_both_strands(L, [M] * 12, {104: 0, 105: 4, 106: 0}, 300, 100, ())
    assert d[104] == 0 and d[105] == 2 and d[106] == 0
    # read indels beside allele events, and the sixteen-op path with an entry inside a word
    var_both_strands(L, [M, M, D, M, M], {103: 0}, 300, 100, ())
    var_both_strands(L, [D, M, M, M], {101: 0, 102: 0}, 300, 100, ())
    var_both_strands(L, [M] * 48, {115: 2}, 300, 100, ())
    var_both_strands(L, [M] * 40 + [I] + [M] * 8, {116: 0}, 300, 100, ())
    # a mate without an entry in reach: the plain walk, two additions
    d, fields = var_both_strands(L, [M] * 12, {40: 0, 41: 3, 250: 2}, 300, 100, ())
    assert (d[100:112] == 2).all() and int(d.sum()) == 24
    # variants at the ends of the sequence
    var_both_strands(L, [M] * 6, {49: 3}, 50, 46, ("last base of the sequence",))
    var_both_strands(L, [M] * 6, {0: 3}, 50, 0, ())


def test_a_mate_wholly_inside_an_insertion_adds_nothing(trial_lib):
    rng = np.random.default_rng(77)
    variants = {150: 20}
    for strand in (0, 1):
        inside, other = make_mate(rng, [M, M, I, M, D, M, M], [M, M], 0, 33), make_mate(rng, [M] * 30, [], 0, 33)
        for forward in (True, False):
            frag = fragment(0, 150, 60, strand) if forward else fragment(0, 100, 50 + 12, strand)
            seg = strand if forward else 1 - strand
            mates = [other, other]
            mates[seg] = inside
            got, fields = check_pair(trial_lib, mates, frag, 400, ("mate wholly inside an insertion",), variants=variants, xi=3 if forward else 0)
            assert b"M" not in fields[seg][5] and int(got[0].sum()) == 30       # the other mate's bases alone


def test_a_substitution_only_set(trial_lib):
    """allele copies: no FragmentVar, the fragment's own coordinates"""
    rng = np.random.default_rng(32)
    for strand in (0, 1):
        mates = [make_mate(rng, [M] * 20 + [D] + [M] * 9, [M, M], 1, 33), make_mate(rng, [D, D, M, M, M, D], [], 0, 33)]
        got, _ = check_pair(trial_lib, mates, fragment(0, 1000, 80, strand), 1200, ("substitution-only set",), variants={}, has_fv=False, allele_id=0)
        assert int(got[0].sum()) == 29 + 3


def test_bedgraph_lines(trial_lib):
    """depth_line through the image sink, at every phase, equals the plain sink's and its stated size; bedgraph_from_depth is what the tests' reader expects"""
    name_ptr = np.concatenate([[0], np.cumsum([len(n) for n in NAMES])]).astype(np.uint32)
    out = C.create_string_buffer(256)
    for seq, start, end, depth in ((0, 0, 1, 0), (1, 9, 10, 9), (2, 99999, 100000, 10), (1, 123456789, 4294967295, 4294967295), (0, 4095, 4096, 12345)):
        for at in range(4):
            n = trial_lib.depth_line_trial(b"".join(NAMES), name_ptr.ctypes.data, seq, start, end, depth, at, out, 256)
            assert n > 0 and out.raw[:n] == b"%s\t%d\t%d\t%d\n" % (NAMES[seq], start, end, depth)
    text = bedgraph_from_depth([b"a", b"bb", b"c"], [np.array([0, 0, 1, 1, 1, 0], np.uint32), np.zeros(0, np.uint32), np.array([5], np.uint32)])
    assert text == b"a\t0\t2\t0\na\t2\t5\t1\na\t5\t6\t0\nc\t0\t1\t5\n"


def test_depth_from_sam_reads_a_cigar():
    sam = b"@HD\tVN:1.6\nr\t99\tx\t3\t60\t2S2M1I1D2M\t=\t1\t0\tAAAAAAA\tIIIIIII\nr\t77\t*\t0\t0\t*\t*\t0\t0\tA\tI\nq\t147\ty\t1\t60\t3M\t=\t1\t0\tAAA\tIII\n"
    x, y = depth_from_sam(sam, {b"x": 8, b"y": 3})
    assert x.tolist() == [0, 0, 1, 1, 0, 1, 1, 0] and y.tolist() == [1, 1, 1] and x.dtype == np.uint32


def test_every_class_was_met():
    assert met >= set(CLASSES), sorted(set(CLASSES) - met)
