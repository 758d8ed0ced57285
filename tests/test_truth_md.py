"""NM:i and MD:Z of the truth alignments (rsq_sim_truth_md; reseq_amd/csrc/rsq_md.h) without a GPU: the per-lane functions of the four formats with the tags run
on the CPU (tests/hostemu/truth_md_trial.cpp, built here with g++) over crafted rows, fragments, alleles and a crafted packed reference.  Every record's tags are
compared with `md_nm` (tests/truth_md.py: the rule of include/reseq_amd.h) applied to the record's own POS, CIGAR and SEQ, and without the tags the records are,
byte for byte, what the formats without them write from the same rows.  Inside the trial the writer kernel's lane roles are replayed into a zeroed image and
compared with the record function's bytes.  tests/test_truth_md_gpu.py applies the same checks to the device's output."""
import ctypes as C

import numpy as np
import pytest

from test_truth_bam import MARKER
from test_truth_sam import D, I, M, NAMES, TrialPair, build_trial, fill_trial, fragment, template_bases
from test_truth_variants import build_allele, fragment_var, stretch_start
from truth_md import bam_fields, bam_records, check_bam, check_sam

LETTERS = b"ACGT"


class MdIn(C.Structure):
    _fields_ = [("pair", TrialPair), ("allele", C.c_uint32), ("num_alleles", C.c_uint32), ("seq_len", C.c_uint32), ("n_variants", C.c_uint32), ("var_pos", C.c_void_p),
                ("var_len", C.c_void_p), ("has_fv", C.c_int32), ("end", C.c_uint32), ("sub", C.c_uint32), ("start_var", C.c_int32), ("start_var_pos", C.c_uint32),
                ("end_var", C.c_int32), ("end_var_pos", C.c_uint32), ("ref", C.c_void_p)]


@pytest.fixture(scope="module")
def trial_lib(tmp_path_factory):
    L = build_trial(tmp_path_factory, "truth_md_trial")
    L.truth_md_trial.argtypes = [C.POINTER(MdIn), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
    return L


def run(L, fmt, mates, frag, ref, variants=None, xi=0, has_fv=False, num_alleles=1, allele_id=0, at=0, phred_offset=33):
    """the pair's two records in format `fmt` (bit 0 BAM, bit 1 the variant formats, bit 2 with the tags) and the two FASTQ records"""
    variants = variants or {}
    t, keep = fill_trial(mates, frag, phred_offset, 0, 1101, b"ReseqRead_", NAMES)
    pos = np.array(sorted(variants), np.uint32)
    length = np.array([variants[p] for p in sorted(variants)], np.uint32)
    v = MdIn(pair=t, allele=allele_id, num_alleles=num_alleles, seq_len=len(ref), n_variants=len(pos), var_pos=pos.ctypes.data if len(pos) else None,
             var_len=length.ctypes.data if len(pos) else None, has_fv=1 if has_fv and frag is not None else 0, ref=ref.ctypes.data)
    if v.has_fv:
        fv = fragment_var(build_allele(len(ref), variants), variants, frag, xi)
        v.end, v.start_var, v.start_var_pos, v.end_var, v.end_var_pos = fv["end"], fv["start_var"], fv["start_var_pos"], fv["end_var"], fv["end_var_pos"]
    cap = 8192
    f1, f2 = (C.create_string_buffer(cap) for _ in range(2))
    out = C.create_string_buffer(bytes([MARKER]) * cap, cap)
    sizes = np.zeros(6, np.uint32)
    assert L.truth_md_trial(C.byref(v), fmt, f1, f2, out, at, cap, sizes.ctypes.data) == 0, fmt
    assert sizes[2] == sizes[4] and sizes[3] == sizes[5], sizes          # the size the entry states is the record's length
    end = at + int(sizes[2]) + int(sizes[3])
    assert out.raw[:at] == bytes([MARKER]) * at and out.raw[end:] == bytes([MARKER]) * (cap - end)
    return out.raw[at:end], f1.raw[:sizes[0]], f2.raw[:sizes[1]]


def check(L, mates, frag, ref, var_formats=(False, True), **kw):
    """all formats: tags against md_nm, the rest against the format without the tags; returns the SAM lines' (CIGAR, NM, MD) of the format without variants (or
    of the variant format, if that alone is asked for)"""
    text = bytes(LETTERS[c] for c in ref)
    refs = {n: text for n in NAMES}
    out = None
    for var in var_formats:
        bits = 2 if var else 0
        kv = dict(kw)
        if var and "num_alleles" not in kv:
            kv.update(num_alleles=2, allele_id=1)
        tagged, f1, f2 = run(L, bits | 4, mates, frag, ref, **kv)
        plain, g1, g2 = run(L, bits, mates, frag, ref, **kv)
        assert (f1, f2) == (g1, g2)
        check_sam(tagged, plain, refs)
        for at in (0, 3):
            tagged_bam = run(L, bits | 5, mates, frag, ref, at=at, **kv)[0]
            check_bam(tagged_bam, run(L, bits | 1, mates, frag, ref, at=at, **kv)[0], [text] * 3)
        # both encodings carry the same tags
        lines = [l.split(b"\t") for l in tagged.splitlines()]
        for line, rec in zip(lines, bam_records(tagged_bam)):
            tags = bam_fields(rec)[5]
            if not int(line[1]) & 0x4:
                assert (b"NM:i:%d" % tags[-2][2], b"MD:Z:" + tags[-1][2]) == (line[-2], line[-1])
        if out is None:
            out = [(l[5], int(l[-2][5:]), l[-1][5:]) if not int(l[1]) & 0x4 else None for l in lines]
    return out


def read_of(rng, allele_seq, first, ops, reverse, adapter=0, tail=0, change=(), n_at=(), num_errors=3):
    """a mate whose template part reads allele_seq from coordinate `first` on -- `ops` in read order; a reverse mate reads the complement from `first` down.
    change / n_at: allele coordinates whose read base is another base / N.  Inserted and non-template bases are random."""
    seq, at = [], first
    for op in ops:
        if op == I:
            seq.append(int(rng.integers(0, 4)))
            continue
        base = int(allele_seq[at])
        if op == M:
            if at in change:
                base = (base + 1 + int(rng.integers(0, 3))) % 4
            base = 3 - base if reverse else base
            seq.append(4 if at in n_at else base)
        at += -1 if reverse else 1
    seq += [int(x) for x in rng.integers(0, 4, adapter + tail)]
    all_ops = np.array(list(ops) + [M] * adapter, np.uint8)
    return dict(read_len=len(seq), n_iter_m=len(ops), n_iter_s=adapter, hard_clip=tail, num_errors=num_errors, seq=np.array(seq, np.uint8),
                qual=(rng.integers(2, 41, len(seq)) + 33).astype(np.uint8), ops=all_ops)


def pair_over(rng, ref, start, ops, strand, seg, other_len=20, flen=None, **kw):
    """(mates, fragment): the mate of `ops` as segment `seg` of a fragment that is exactly its template part, the other mate a plain one of other_len bases
    (or the whole fragment, if shorter); the crafted mate is the reverse one where seg != strand"""
    t = template_bases(ops) if flen is None else flen
    frag = fragment(1, start, t, strand)
    mates = [None, None]
    for s in (0, 1):
        reverse = s != strand
        o = ops if s == seg else [M] * min(other_len, t)
        mates[s] = read_of(rng, ref, start + t - 1 if reverse else start, o, reverse, **(kw if s == seg else {}))
    return mates, frag


def crafted(L, ref, start, ops, want=None, var_formats=(False, True), **kw):
    """the crafted mate as forward and as reverse mate, on either strand.  `ops`, change and n_at are given in REFERENCE order (ascending), change / n_at as
    reference positions: a reverse mate reads the ops from the last one down, so all four records show the same columns and the same MD.  Returns (CIGAR without
    the clip, NM, MD), and asserts it equals `want` if given."""
    rng = np.random.default_rng(len(ops) * 977 + start)
    seen = set()
    for strand in (0, 1):
        for seg in (0, 1):
            reverse = seg != strand
            mates, frag = pair_over(rng, ref, start, ops[::-1] if reverse else ops, strand, seg, **kw)
            got = check(L, mates, frag, ref, var_formats)[seg]
            n_clip = kw.get("adapter", 0) + kw.get("tail", 0)
            clip = b"%dS" % n_clip if n_clip else b""
            assert got[0].startswith(clip) if reverse else got[0].endswith(clip)
            seen.add((got[0][len(clip):] if reverse else got[0][:len(got[0]) - len(clip)], got[1], got[2]))
    assert len(seen) == 1, seen
    got = seen.pop()
    if want is not None:
        assert got == want, (got, want)
    return got


@pytest.fixture(scope="module")
def ref():
    return np.random.default_rng(2024).integers(0, 4, 300).astype(np.uint8)


def letters(ref, lo, hi):
    return bytes(LETTERS[c] for c in ref[lo:hi])


def test_no_mismatch(trial_lib, ref):
    for n in (1, 5, 16, 31, 32, 33, 64, 70):
        crafted(trial_lib, ref, 40, [M] * n, (b"%dM" % n, 0, b"%d" % n), adapter=3)


def test_mismatch_at_the_first_and_at_the_last_aligned_base(trial_lib, ref):
    L = trial_lib
    crafted(L, ref, 40, [M] * 20, (b"20M", 1, b"0" + letters(ref, 40, 41) + b"19"), change={40})
    crafted(L, ref, 40, [M] * 20, (b"20M", 1, b"19" + letters(ref, 59, 60) + b"0"), change={59}, adapter=2)
    crafted(L, ref, 40, [M] * 20, (b"20M", 2, b"0" + letters(ref, 40, 41) + b"18" + letters(ref, 59, 60) + b"0"), change={40, 59})


def test_two_adjacent_mismatches_and_a_read_base_n(trial_lib, ref):
    L = trial_lib
    crafted(L, ref, 40, [M] * 20, (b"20M", 2, b"7" + letters(ref, 47, 48) + b"0" + letters(ref, 48, 49) + b"11"), change={47, 48})
    crafted(L, ref, 40, [M] * 20, (b"20M", 1, b"7" + letters(ref, 47, 48) + b"12"), n_at={47})                 # N is a mismatch, MD names the reference base
    crafted(L, ref, 40, [M] * 20, (b"20M", 3, b"7" + b"0".join(letters(ref, p, p + 1) for p in (47, 48, 49)) + b"10"), change={47, 49}, n_at={48})


def test_mismatches_beside_deletions(trial_lib, ref):
    L = trial_lib
    ops = [M] * 6 + [D, D] + [M] * 6                                     # reference 40 .. 45, 46 47 deleted, 48 .. 53
    crafted(L, ref, 40, ops, (b"6M2D6M", 2, b"6^" + letters(ref, 46, 48) + b"6"))
    crafted(L, ref, 40, ops, (b"6M2D6M", 3, b"6^" + letters(ref, 46, 48) + b"0" + letters(ref, 48, 49) + b"5"), change={48})      # a mismatch directly behind
    crafted(L, ref, 40, ops, (b"6M2D6M", 3, b"5" + letters(ref, 45, 46) + b"0^" + letters(ref, 46, 48) + b"6"), change={45})      # a deletion directly behind a mismatch


def test_dropped_d_runs_and_leading_i(trial_lib, ref):
    L = trial_lib
    # D at both ends: no part of the alignment, POS has moved past the leading run
    crafted(L, ref, 40, [D, D] + [M] * 8 + [D], (b"8M", 1, b"3" + letters(ref, 45, 46) + b"4"), change={45})
    # a leading I: in NM, not in MD
    crafted(L, ref, 40, [I, I] + [M] * 8, (b"2I8M", 2, b"8"))
    crafted(L, ref, 40, [I] + [M] * 8 + [I, I], (b"1I8M2I", 4, b"2" + letters(ref, 42, 43) + b"5"), change={42})
    # I between a dropped D and the alignment
    crafted(L, ref, 40, [D, I, M, M], (b"1I2M", 1, b"2"))


def test_mates_without_an_m_column(trial_lib, ref):
    L = trial_lib
    crafted(L, ref, 40, [I, I, I], (b"3I", 3, b"0"), adapter=4, flen=9)  # a template part of I only
    crafted(L, ref, 40, [D, D], (b"", 0, b"0"), adapter=5)               # ... of D only: a bare clip
    # no read bases at all: "*"
    rng = np.random.default_rng(8)
    for strand in (0, 1):
        empty = read_of(rng, ref, 40, [], False)
        other = read_of(rng, ref, 40 if strand == 0 else 59, [M] * 20, strand == 1)
        got = check(L, [other, empty], fragment(0, 40, 20, strand), ref)
        assert got[1] == (b"*", 0, b"0")


def test_every_read_length_modulo_four_on_a_reverse_mate(trial_lib, ref):
    for n in range(1, 14):
        for adapter in (0, 1, 2, 3):                                     # (the clip stands in front of a reverse mate's aligned bases: they begin at any byte of a row word)
            last = 40 + n - 1
            crafted(trial_lib, ref, 40, [M] * n, (b"%dM" % n, 1, b"%d" % (n - 1) + letters(ref, last, last + 1) + b"0"), change={last}, adapter=adapter)


def test_spans_at_the_ends_of_the_sequence(trial_lib, ref):
    L = trial_lib
    n = len(ref)
    crafted(L, ref, 0, [M] * 25, (b"25M", 1, b"0" + letters(ref, 0, 1) + b"24"), change={0})                    # begins at position 0
    crafted(L, ref, n - 25, [M] * 25, (b"25M", 1, b"24" + letters(ref, n - 1, n) + b"0"), change={n - 1})       # ends on the sequence's last base
    crafted(L, ref, n - 40, [M] * 37 + [D] * 3, (b"37M", 0, b"37"))
    whole = np.random.default_rng(3).integers(0, 4, 64).astype(np.uint8)                                        # a sequence of exactly two words, read whole
    crafted(L, whole, 0, [M] * 64, (b"64M", 2, b"31" + letters(whole, 31, 32) + b"0" + letters(whole, 32, 33) + b"31"), change={31, 32})


def test_reference_word_borders_and_partial_groups(trial_lib, ref):
    L = trial_lib
    # a run of 16 plain ops of a row with stored ops crosses the border between reference positions 63 and 64 (start 55: ops 0 .. 15 are 55 .. 70)
    ops = [M] * 32 + [I] + [M] * 9
    for p in (62, 63, 64, 65):
        crafted(L, ref, 55, ops, (b"32M1I9M", 2, b"%d" % (p - 55) + letters(ref, p, p + 1) + b"%d" % (55 + 41 - 1 - p)), change={p})
    crafted(L, ref, 55, ops, (b"32M1I9M", 3, b"8" + letters(ref, 63, 64) + b"0" + letters(ref, 64, 65) + b"31"), change={63, 64})
    # a mismatch in the last partial group of a 16-op step: 16 + 16 + 5 ops, the mismatch among the last five; plain rows and rows with stored ops
    for ops, cigar, first in (([M] * 37, b"37M", 0), ([D] + [M] * 37, b"37M", 1), ([M] * 3 + [D] + [M] * 34, b"3M1D34M", None)):
        for k in (32, 35, 36):
            if first is None:
                p = 91 + 1 + k
                want = (cigar, 2, b"3^" + letters(ref, 94, 95) + b"%d" % (k - 3) + letters(ref, p, p + 1) + b"%d" % (36 - k))
            else:
                p = 91 + first + k
                want = (cigar, 1, b"%d" % k + letters(ref, p, p + 1) + b"%d" % (36 - k))
            crafted(L, ref, 91, ops, want, change={p})
    # every start position modulo 32 with a long plain read, a mismatch at every sixth base
    for start in range(0, 64, 5):
        change = set(range(start + 2, start + 90, 6))
        got = crafted(L, ref, start, [M] * 90, change=change, tail=1)
        assert got[1] == len(change)


def test_random_rows(trial_lib, ref):
    """random ops, random errors and N, all read lengths 1 .. 45, every format: the tags against md_nm, the rest against the formats without them"""
    rng = np.random.default_rng(77)
    for read_len in range(1, 46):
        for strand in (0, 1):
            ops = []
            while sum(o != D for o in ops) < read_len:
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
            check(trial_lib, mates, frag, ref)


def test_unmapped_pairs_carry_no_tags(trial_lib, ref):
    rng = np.random.default_rng(5)
    mates = [read_of(rng, ref, 0, [], False, adapter=9, tail=2), read_of(rng, ref, 0, [], False, adapter=12)]
    assert check(trial_lib, mates, None, ref) == [None, None]
    assert check(trial_lib, mates, fragment(2, 77, 0, 1), ref) == [None, None]            # a fragment of length 0


# ------------------------------------------------------------------------------------------------ a reference with variants
def allele_bases(rng, ref, variants, allele):
    """the allele's bases by allele coordinate: a base standing at p is the reference's, or -- substituted -- another one; inserted bases are random"""
    out = []
    for cls, p, k in allele:
        if cls == "X":
            out.append(int(rng.integers(0, 4)))
        elif variants.get(p, -1) == 1:
            out.append((int(ref[p]) + 1 + int(rng.integers(0, 3))) % 4)
        else:
            out.append(int(ref[p]))
    return out


def var_pair(rng, ref, variants, start, xi, length, ops_by_seg, strand, **kw):
    """mates that read the allele without errors (but kw: change / n_at in allele coordinates, for both mates), the fragment, the allele's bases"""
    allele = build_allele(len(ref), variants)
    bases = allele_bases(np.random.default_rng(1), ref, variants, allele)
    hs = stretch_start(allele, start, xi)
    frag = fragment(1, start, length, strand)
    mates = []
    for seg in (0, 1):
        reverse = seg != strand
        mates.append(read_of(rng, bases, hs + length - 1 if reverse else hs, ops_by_seg[seg], reverse, **kw))
    return mates, frag, hs


def var_check(L, ref, variants, start, length, ops, xi=0, **kw):
    """the same template ops as forward and (reversed) as reverse mate over the allele, on either strand; returns {(CIGAR, NM, MD)} of the variant formats"""
    rng = np.random.default_rng(start * 31 + length)
    seen = set()
    for strand in (0, 1):
        by_seg = [ops, ops[::-1]] if strand == 0 else [ops[::-1], ops]
        mates, frag, _ = var_pair(rng, ref, variants, start, xi, length, by_seg, strand, **kw)
        got = check(L, mates, frag, ref, var_formats=(True,), variants=variants, xi=xi, has_fv=True)
        seen.update(got)
    return seen


def test_variant_columns_in_md(trial_lib, ref):
    L = trial_lib
    # an allele deletion inside the stretch: a D column from the map, MD prints the deleted reference base, NM counts it
    assert var_check(L, ref, {105: 0}, 100, 12, [M] * 12) == {(b"5M1D7M", 1, b"5^" + letters(ref, 105, 106) + b"7")}
    assert var_check(L, ref, {104: 0, 105: 0, 106: 0}, 100, 12, [M] * 12) == {(b"4M3D8M", 3, b"4^" + letters(ref, 104, 107) + b"8")}
    # an insertion: I columns count in NM only
    assert var_check(L, ref, {105: 3}, 100, 12, [M] * 12) == {(b"6M2I4M", 2, b"10")}
    # a substituted allele base the read reproduces is a mismatch against the reference ...
    assert var_check(L, ref, {105: 1}, 100, 12, [M] * 12) == {(b"12M", 1, b"5" + letters(ref, 105, 106) + b"6")}
    # ... beside an allele deletion as well
    assert var_check(L, ref, {105: 1, 106: 0}, 100, 12, [M] * 12) == {(b"6M1D6M", 2, b"5" + letters(ref, 105, 106) + b"0^" + letters(ref, 106, 107) + b"6")}
    # a deletion that touches only the outside of the stretch is no part of it
    assert var_check(L, ref, {99: 0, 112: 0}, 100, 12, [M] * 12) == {(b"12M", 0, b"12")}
    # a leading read-D in front of an allele deletion: all dropped
    assert var_check(L, ref, {101: 0, 102: 0}, 100, 4, [D, M, M, M]) == {(b"3M", 0, b"3")}


def test_a_substituted_base_turned_back_by_an_error_is_a_match(trial_lib, ref):
    """the read's base at the substituted position is set to the REFERENCE's base: no mismatch, whatever the allele holds"""
    L = trial_lib
    variants = {105: 1, 120: 0}
    rng = np.random.default_rng(4)
    for strand in (0, 1):
        mates, frag, hs = var_pair(rng, ref, variants, 100, 0, 12, [[M] * 12, [M] * 12], strand)
        for seg in (0, 1):
            reverse = seg != strand
            i = 12 - 1 - 5 if reverse else 5                         # the read base over position 105
            mates[seg]["seq"][i] = 3 - int(ref[105]) if reverse else int(ref[105])
        got = check(L, mates, frag, ref, var_formats=(True,), variants=variants, has_fv=True)
        assert got == [(b"12M", 0, b"12")] * 2
    # allele copies (substitutions only, no FragmentVar): the comparison is against the reference as well
    variants = {105: 1}
    for strand in (0, 1):
        mates, frag, _ = var_pair(rng, ref, variants, 100, 0, 12, [[M] * 12, [M] * 12], strand)
        got = check(L, mates, frag, ref, var_formats=(True,), variants=variants, has_fv=False)
        assert got == [(b"12M", 1, b"5" + letters(ref, 105, 106) + b"6")] * 2


def test_a_mate_wholly_inside_an_insertion(trial_lib, ref):
    """nI and the clip: MD:Z:0, NM = the inserted bases"""
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
            got = check(trial_lib, mates, frag, ref, var_formats=(True,), variants=variants, xi=3 if forward else 0, has_fv=True)
            assert got[seg] == (b"6I2S" if forward else b"2S6I", 6, b"0")


def test_random_rows_over_dense_alleles(trial_lib, ref):
    from test_truth_variants import random_variants
    rng = np.random.default_rng(4100)
    for read_len in range(1, 38, 2):
        for strand in (0, 1):
            variants = random_variants(rng, len(ref), int(rng.choice([3, 6, 18])))
            allele = build_allele(len(ref), variants)
            by_seg = []
            for seg in (0, 1):
                ops = []
                while sum(o != D for o in ops) < read_len:
                    r = rng.random()
                    ops.append(D if r < 0.1 else I if r < 0.2 else M)
                by_seg.append(ops)
            length = max(template_bases(o) for o in by_seg) + int(rng.integers(0, 30))
            hs = int(rng.integers(0, len(allele) - length - 40))
            while allele[hs + length - 1][1] == allele[hs][1]:
                length += 1
            _, start, xi = allele[hs]
            mates, frag, _ = var_pair(rng, ref, variants, start, xi, length, by_seg, strand, adapter=int(rng.integers(0, 3)),
                                      change={hs + int(k) for k in rng.integers(0, length, 3)})
            check(trial_lib, mates, frag, ref, var_formats=(True,), variants=variants, xi=xi, has_fv=True)
