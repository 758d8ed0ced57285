"""Truth alignments of a reference with variants, in reference coordinates (rsq_sim_truth_variants; reseq_amd/csrc/rsq_sam.h SamVarFormat, rsq_bam.h BamVarFormat)
without a GPU: the per-lane functions run on the CPU (tests/hostemu/truth_var_trial.cpp, built here with g++) over crafted alleles, fragments and rows, and both
formats' records are compared with `var_sam_pair`, this module's own statement of the rules.  The statement spells the allele out base by base -- one
(class, position, index in its replacement) per allele base -- and shares no arithmetic with the coordinate map the device walks.  It predicts the records from
the FASTQ records, the fragment, XI and the variant list alone; tests/test_truth_variants_gpu.py applies it to the device's output."""
import ctypes as C
import struct

import numpy as np
import pytest

from test_truth_bam import MARKER, decode_bam
from test_truth_sam import (D, I, M, NAMES, TrialPair, _COMPLEMENT, build_trial, fill_trial, fragment, make_mate, mate_alignment, parse_fastq, random_template,
                            template_bases, template_part)

# ------------------------------------------------------------------------------------------------ the statement
R, X = "R", "X"


def build_allele(seq_len, variants):
    """the allele base by base: [(class, p, k)] -- R: the base stands at reference position p (k = 0); X: base k >= 1 of the replacement at p.
    variants: {position: length of the replacement} of THIS allele"""
    bases = []
    for p in range(seq_len):
        n = variants.get(p, 1)
        bases += [(R if k == 0 else X, p, k) for k in range(n)]
    return bases


def stretch_start(allele, start, xi):
    """allele coordinate of (start position, XI bases of its replacement in front)"""
    return allele.index((R if xi == 0 else X, start, xi))


def columns(allele, first, ops):
    """the columns of a template part that begins at allele coordinate `first`, ops in ascending allele order: [(op, reference position or None)]"""
    cols, at, prev = [], first, None
    for op in ops:
        if op == b"I":
            cols.append((b"I", None))
            continue
        cls, p, _ = allele[at]
        at += 1
        if prev is not None and cls == R:
            cols += [(b"D", q) for q in range(prev + 1, p)]          # positions the allele deleted between two bases of the stretch
        prev = p
        if cls == R:
            cols.append((op, p))
        elif op == b"M":
            cols.append((b"I", None))                                # a read base over an inserted base; a read deletion of an inserted base is nothing
    return cols


def var_mate_alignment(allele, hs, frag, seg, record):
    """POS, last aligned position, CIGAR, reverse of one mate of a mapped pair"""
    part = template_part(record[0].split(b" ")[1])
    ops = [op for n, op in part for _ in range(n)]
    q, t = sum(op != b"D" for op in ops), sum(op != b"I" for op in ops)
    reverse = seg != int(frag["strand"])
    first = hs + int(frag["len"]) - t if reverse else hs
    cols = columns(allele, first, ops[::-1] if reverse else ops)
    # where the next reference-consuming column would stand, before any column
    if first < len(allele):
        cls, p, _ = allele[first]
        at = p + (cls == X)
    else:
        at = allele[-1][1] + 1
    # D runs at either end are dropped, the end the read begins at first (a template part of D alone is dropped there)
    left = right = 0
    for end in ((1, 0) if reverse else (0, 1)):
        while cols and cols[-end][0] == b"D":
            cols.pop(-end)
            left, right = left + (end == 0), right + (end == 1)
    ref = [p for op, p in cols if p is not None]
    pos = (ref[0] if ref else at + left) + 1
    assert ref == list(range(pos - 1, pos - 1 + len(ref))), "the reference-consuming columns are consecutive positions"
    last = pos + len(ref) - 1
    elements = []
    for op, _ in cols:
        if elements and elements[-1][1] == op:
            elements[-1][0] += 1
        else:
            elements.append([1, op])
    clip = len(record[1]) - q
    texts = [b"%d%s" % (n, op) for n, op in elements]
    clip_text = [b"%dS" % clip] if clip else []
    return pos, last, b"".join(clip_text + texts if reverse else texts + clip_text) or b"*", reverse


def var_sam_pair(frag, xi, allele, rec1, rec2, names, phred_offset):
    """the two records of a pair of a simulator with variants; frag None (or of length 0): unmapped; allele None: allele copies, the fragment's own coordinates"""
    out = []
    mapped = frag is not None and int(frag["len"]) > 0
    if mapped and allele is not None:
        hs = stretch_start(allele, int(frag["start"]), xi)
        al = [var_mate_alignment(allele, hs, frag, seg, rec) for seg, rec in enumerate((rec1, rec2))]
    elif mapped:
        al = [mate_alignment(frag, seg, rec) for seg, rec in enumerate((rec1, rec2))]
    for seg, (idline, seq, qual) in enumerate((rec1, rec2)):
        qname, cigar, errors = idline.split(b" ")
        qual33 = bytes(c - phred_offset + 33 for c in qual)
        if mapped:
            pos, last, sam_cigar, reverse = al[seg]
            other = al[seg ^ 1]
            span = max(last, other[1]) - min(pos, other[0]) + 1
            tlen = span if (pos < other[0] or (pos == other[0] and seg == 0)) else -span
            flag = 0x1 | 0x2 | (0x10 if reverse else 0x20) | (0x80 if seg else 0x40)
            if reverse:
                seq, qual33 = seq.translate(_COMPLEMENT)[::-1], qual33[::-1]
            fields = [qname, b"%d" % flag, names[int(frag["seq"])], b"%d" % pos, b"60", sam_cigar, b"=", b"%d" % other[0], b"%d" % tlen]
        else:
            fields = [qname, b"141" if seg else b"77", b"*", b"0", b"0", b"*", b"*", b"0", b"0"]
        out.append(b"\t".join(fields + [seq, qual33, b"XC:Z:" + cigar, b"XE:i:" + errors[1:], b"XI:i:%d" % xi]) + b"\n")
    return b"".join(out)


def var_sam_text(frags, xis, alleles, fastq1, fastq2, names, phred_offset):
    """the SAM text of a call; alleles: {(seq, allele): build_allele(...)} or None (allele copies)"""
    r1, r2 = parse_fastq(fastq1), parse_fastq(fastq2)
    assert len(r1) == len(r2) and (frags is None or len(frags) == len(r1))
    out = []
    for i in range(len(r1)):
        f = None if frags is None else frags[i]
        allele = None if f is None or alleles is None else alleles[int(f["seq"]), int(f["allele"])]
        out.append(var_sam_pair(f, 0 if f is None else int(xis[i]), allele, r1[i], r2[i], names, phred_offset))
    return b"".join(out)


def decode_var_bam(data, names):
    """decode_bam of tests/test_truth_bam.py for records that end with "XI" 'I' u32: the tag is taken off every record, the rest decoded, the tag added as text"""
    lines, records, at = [], [], 0
    while at < len(data):
        (block_size,) = struct.unpack_from("<i", data, at)
        rec = data[at + 4:at + 4 + block_size]
        assert len(rec) == block_size and rec[-7:-4] == b"XII", rec[-7:]
        (xi,) = struct.unpack_from("<I", rec, block_size - 4)
        text, recs = decode_bam(struct.pack("<i", block_size - 7) + rec[:-7], names)
        lines.append(text[:-1] + b"\tXI:i:%d\n" % xi)
        records.append(dict(recs[0], block_size=block_size))
        at += 4 + block_size
    return b"".join(lines), records


# ------------------------------------------------------------------------------------------------ the per-lane functions on the host
class VarIn(C.Structure):
    _fields_ = [("pair", TrialPair), ("allele", C.c_uint32), ("num_alleles", C.c_uint32), ("seq_len", C.c_uint32), ("n_variants", C.c_uint32), ("var_pos", C.c_void_p),
                ("var_len", C.c_void_p), ("has_fv", C.c_int32), ("end", C.c_uint32), ("sub", C.c_uint32), ("start_var", C.c_int32), ("start_var_pos", C.c_uint32),
                ("end_var", C.c_int32), ("end_var_pos", C.c_uint32)]


@pytest.fixture(scope="module")
def trial_lib(tmp_path_factory):
    L = build_trial(tmp_path_factory, "truth_var_trial")
    L.truth_var_trial.argtypes = [C.POINTER(VarIn), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def fragment_var(allele, variants, frag, xi):
    """what the sieve hands on beside the fragment (rsq_types.h FragmentVar), from the allele spelled out: the end position is the one behind the last base; a
    fragment that ends inside a replacement's bases names the variant and how many of its bases it uses, else the last variant in front of the end position"""
    positions = sorted(variants)
    hs = stretch_start(allele, int(frag["start"]), xi)
    cls, p, k = allele[hs + int(frag["len"]) - 1]
    end = p + 1
    if k + 1 < variants.get(p, 1):
        end_var, end_var_pos = positions.index(p), k + 1
    else:
        end_var, end_var_pos = sum(q < end for q in positions) - 1, 0
    start_var = positions.index(int(frag["start"])) if xi else sum(q < int(frag["start"]) for q in positions)
    return dict(end=end, start_var=start_var, start_var_pos=xi, end_var=end_var, end_var_pos=end_var_pos)


def run_var_pair(L, bam, mates, frag, phred_offset, variants, seq_len, xi=0, allele_id=1, num_alleles=2, has_fv=True, adapter_only_number=0, at=0):
    """(fastq record 1, fastq record 2, the pair's two records, placed) from the trial library: the format's size is what its record function wrote, nothing
    around the records is touched, and (inside the trial) the writer kernel's two sinks a mate give the same bytes"""
    t, keep = fill_trial(mates, frag, phred_offset, adapter_only_number, 1101, b"ReseqRead_", NAMES)
    pos = np.array(sorted(variants), np.uint32)
    length = np.array([variants[p] for p in sorted(variants)], np.uint32)
    v = VarIn(pair=t, allele=allele_id, num_alleles=num_alleles, seq_len=seq_len, n_variants=len(pos), var_pos=pos.ctypes.data if len(pos) else None,
              var_len=length.ctypes.data if len(pos) else None, has_fv=1 if has_fv and frag is not None else 0)
    if v.has_fv:
        fv = fragment_var(build_allele(seq_len, variants), variants, frag, xi)
        v.end, v.start_var, v.start_var_pos, v.end_var, v.end_var_pos = fv["end"], fv["start_var"], fv["start_var_pos"], fv["end_var"], fv["end_var_pos"]
    cap = 8192
    f1, f2 = (C.create_string_buffer(cap) for _ in range(2))
    out = C.create_string_buffer(bytes([MARKER]) * cap, cap)
    sizes, placed = np.zeros(6, np.uint32), np.zeros(10, np.uint32)
    assert L.truth_var_trial(C.byref(v), 1 if bam else 0, f1, f2, out, at, cap, sizes.ctypes.data, placed.ctypes.data) == 0
    assert sizes[2] == sizes[4] and sizes[3] == sizes[5], sizes
    end = at + int(sizes[2]) + int(sizes[3])
    assert out.raw[:at] == bytes([MARKER]) * at and out.raw[end:] == bytes([MARKER]) * (cap - end)
    return f1.raw[:sizes[0]], f2.raw[:sizes[1]], out.raw[at:end], placed.reshape(2, 5)


def check_var_pair(L, mates, frag, variants, seq_len, xi=0, phred_offset=33, **kw):
    """both formats against the statement; returns (the SAM lines' fields, placed)"""
    allele = build_allele(seq_len, variants) if kw.get("has_fv", True) else None
    f1, f2, sam, placed = run_var_pair(L, False, mates, frag, phred_offset, variants, seq_len, xi, **kw)
    want = var_sam_pair(frag, xi, allele, parse_fastq(f1)[0], parse_fastq(f2)[0], NAMES, phred_offset)
    assert sam == want, (sam, want)
    g1, g2, bam, placed_bam = run_var_pair(L, True, mates, frag, phred_offset, variants, seq_len, xi, at=3, **kw)
    assert (g1, g2) == (f1, f2) and (placed_bam == placed).all()
    got, records = decode_var_bam(bam, NAMES)
    assert got == want, (got, want)
    if frag is not None and frag["len"] and allele is not None:
        # the reverse mate's stretch, placed from the FragmentVar's end the way variant_template places it, ends where the forward mate's stretch plus the length does
        fwd, rev = (0, 1) if frag["strand"] == 0 else (1, 0)
        t_rev = template_bases(mates[rev]["ops"][:mates[rev]["n_iter_m"]])
        assert int(placed[rev][0]) + t_rev == int(placed[fwd][0]) + frag["len"] == stretch_start(allele, frag["start"], xi) + frag["len"]
    return [line.split(b"\t") for line in sam.splitlines()], placed


def mirrored(rng, ops, phred_offset=33, adapter=0, tail=0):
    """the same columns read from either end: (a mate with these template ops, a mate with them reversed)"""
    return make_mate(rng, ops, [M] * adapter, tail, phred_offset), make_mate(rng, ops[::-1], [M] * adapter, tail, phred_offset)


def both_orientations(L, ops, variants, seq_len, start, xi=0, adapter=0, flen=None):
    """a fragment that is exactly the template part of `ops`: the forward mate walks it in read order and the reverse mate (its ops reversed) from its last op
    down, on either strand -- four records that must show the same columns.  Returns (POS, CIGAR without the clip, placed flags) and asserts they agree."""
    rng = np.random.default_rng(len(ops) * 131 + start)
    seen = set()
    for strand in (0, 1):
        fwd, rev = mirrored(rng, ops, adapter=adapter)
        mates = [fwd, rev] if strand == 0 else [rev, fwd]
        frag = fragment(1, start, template_bases(ops) if flen is None else flen, strand)
        fields, placed = check_var_pair(L, mates, frag, variants, seq_len, xi)
        clip = b"%dS" % adapter if adapter else b""
        for seg in (0, 1):
            reverse = seg != strand
            cigar = fields[seg][5]
            assert cigar.startswith(clip) if reverse else cigar.endswith(clip)
            core = cigar[len(clip):] if reverse else cigar[:len(cigar) - len(clip)]
            seen.add((int(fields[seg][3]), core, int(placed[seg][2])))
    assert len(seen) == 1, seen
    return seen.pop()


def random_variants(rng, seq_len, every):
    variants = {}
    for p in range(seq_len):
        if rng.random() < 1.0 / every:
            variants[p] = int(rng.choice([0, 0, 1, 2, 2, 3, 5, 9]))
    return variants


@pytest.mark.parametrize("phred_offset", [33, 64])
def test_every_read_length_over_dense_alleles(trial_lib, phred_offset):
    """read lengths 1 .. 37 with random ops, as forward and reverse mates on either strand, over alleles with a variant every few bases; fragments start at
    plain bases, at replaced ones and inside inserted bases"""
    rng = np.random.default_rng(4000 + phred_offset)
    walked = 0
    for read_len in range(1, 38):
        for strand in (0, 1):
            for p_indel in (0.0, 0.12):
                seq_len = 400
                variants = random_variants(rng, seq_len, int(rng.choice([3, 6, 18])))
                allele = build_allele(seq_len, variants)
                mates = []
                for seg in (0, 1):
                    n_adapter = int(rng.integers(0, read_len)) if rng.random() < 0.4 else 0
                    mates.append(make_mate(rng, random_template(rng, read_len - n_adapter, p_indel), [M] * n_adapter, 0, phred_offset, with_n=read_len % 3 == 0))
                length = max(template_bases(m["ops"][:m["n_iter_m"]]) for m in mates) + int(rng.integers(0, 30))
                hs = int(rng.integers(0, len(allele) - length - 40))
                while allele[hs + length - 1][1] == allele[hs][1]:                   # (a fragment is no part of one replacement)
                    length += 1
                _, start, xi = allele[hs]
                _, placed = check_var_pair(trial_lib, mates, fragment(int(rng.integers(0, 3)), start, length, strand), variants, seq_len, xi, phred_offset)
                walked += int(placed[:, 2].sum())
    assert walked > 100


def test_variants_wholly_inside_a_mate(trial_lib):
    L = trial_lib
    assert both_orientations(L, [M] * 12, {105: 3}, 300, 100) == (101, b"6M2I4M", 1)          # an insertion: its first base stands at 105
    assert both_orientations(L, [M] * 12, {105: 0}, 300, 100) == (101, b"5M1D7M", 1)          # a deletion
    assert both_orientations(L, [M] * 12, {105: 1}, 300, 100) == (101, b"12M", 0)             # a substitution moves nothing: the plain walk
    assert both_orientations(L, [M] * 12, {104: 0, 105: 0, 106: 0}, 300, 100) == (101, b"4M3D8M", 1)
    assert both_orientations(L, [M] * 12, {104: 0, 105: 4, 106: 0}, 300, 100) == (101, b"4M1D1M3I1D4M", 1)      # deletion / insertion / deletion


def test_a_fragment_that_starts_or_ends_inside_an_insertion(trial_lib):
    L = trial_lib
    # the replacement at 100 has 5 bases: XI of them lie in front of the fragment
    assert both_orientations(L, [M] * 10, {100: 5}, 300, 100, xi=1) == (102, b"4I6M", 1)
    assert both_orientations(L, [M] * 10, {100: 5}, 300, 100, xi=4) == (102, b"1I9M", 1)
    assert both_orientations(L, [M] * 10, {100: 5}, 300, 100, xi=0) == (101, b"1M4I5M", 1)
    # ... and one that ends inside it
    assert both_orientations(L, [M] * 10, {107: 6}, 300, 100) == (101, b"8M2I", 1)
    assert both_orientations(L, [M] * 8, {107: 6}, 300, 100) == (101, b"8M", 1)               # its last base is the one standing at 107


def test_a_mate_wholly_inside_an_insertion(trial_lib):
    """nI and the clip, POS = p + 2, mapped, no reference bases"""
    rng = np.random.default_rng(77)
    variants = {150: 20}
    for strand in (0, 1):
        inside, other = make_mate(rng, [M, M, I, M, D, M, M], [M, M], 0, 33), make_mate(rng, [M] * 30, [], 0, 33)
        # forward: the fragment starts inside the insertion; reverse: it ends there
        for forward in (True, False):
            frag = fragment(0, 150, 60, strand) if forward else fragment(0, 100, 50 + 12, strand)
            seg = strand if forward else 1 - strand
            mates = [other, other]
            mates[seg] = inside
            fields, placed = check_var_pair(trial_lib, mates, frag, variants, 400, xi=3 if forward else 0)
            want = b"6I2S" if forward else b"2S6I"
            assert (fields[seg][3], fields[seg][5]) == (b"152", want) and not int(fields[seg][1]) & 0x4
            bam = decode_var_bam(run_var_pair(trial_lib, True, mates, frag, 33, variants, 400, 3 if forward else 0)[2], NAMES)[1]
            assert bam[seg]["pos"] == 151 and bam[seg]["n_cigar"] == 2


def test_deletions_outside_the_stretch_are_no_part_of_it(trial_lib):
    L = trial_lib
    plain = both_orientations(L, [M] * 12, {}, 300, 100)
    assert plain == (101, b"12M", 0)
    assert both_orientations(L, [M] * 12, {99: 0}, 300, 100) == plain                          # directly in front
    assert both_orientations(L, [M] * 12, {112: 0}, 300, 100) == plain                         # directly behind
    assert both_orientations(L, [M] * 12, {98: 0, 99: 0, 112: 0, 113: 0}, 300, 100) == plain


def test_read_indels_beside_allele_events(trial_lib):
    L = trial_lib
    # read-D on an inserted base vanishes (100: 3 bases; the D falls on the second)
    assert both_orientations(L, [M, D, M, M, M], {100: 3}, 300, 100) == (101, b"1M1I2M", 1)
    # read-D beside an allele deletion: one D
    assert both_orientations(L, [M, M, D, M, M], {103: 0}, 300, 100) == (101, b"2M2D2M", 1)
    assert both_orientations(L, [M, M, M, D, M], {103: 0}, 300, 100) == (101, b"3M2D1M", 1)
    # read-I beside an allele insertion: one I
    assert both_orientations(L, [M, M, I, M, M, M], {101: 3}, 300, 100) == (101, b"2M3I1M", 1)
    assert both_orientations(L, [M, M, M, M, I, M], {101: 3}, 300, 100) == (101, b"2M3I1M", 1)
    # a leading read-D followed by an allele deletion: all dropped, POS moves by both
    assert both_orientations(L, [D, M, M, M], {101: 0, 102: 0}, 300, 100) == (104, b"3M", 1)
    # ... and at the other end
    assert both_orientations(L, [M, M, M, D], {103: 0}, 300, 100) == (101, b"3M", 1)
    # I between a dropped D and the alignment: the CIGAR begins with I
    assert both_orientations(L, [D, I, M, M], {}, 300, 100) == (102, b"1I2M", 0)


def test_variants_at_the_ends_of_the_sequence(trial_lib):
    L = trial_lib
    assert both_orientations(L, [M] * 6, {0: 3}, 50, 0) == (1, b"1M2I3M", 1)
    assert both_orientations(L, [M] * 6, {0: 3}, 50, 0, xi=2) == (2, b"1I5M", 1)
    assert both_orientations(L, [M] * 6, {0: 0}, 50, 1) == (2, b"6M", 0)
    assert both_orientations(L, [M] * 6, {49: 3}, 50, 46) == (47, b"4M2I", 1)
    assert both_orientations(L, [M] * 4, {49: 0}, 50, 45) == (46, b"4M", 0)
    assert both_orientations(L, [M] * 3, {48: 0, 49: 1}, 50, 46) == (47, b"2M1D1M", 1)


def test_events_inside_a_word_of_plain_ops(trial_lib):
    """the 16-ops-at-once path is taken only where no entry stands among the 16 bases"""
    L = trial_lib
    plain, stored = [M] * 48, [M] * 40 + [I] + [M] * 8          # a plain row, and one whose ops are stored (the I lies in the third word)
    assert both_orientations(L, plain, {107: 0}, 300, 100)[1] == b"7M1D41M"
    assert both_orientations(L, plain, {115: 2}, 300, 100)[1] == b"16M1I31M"              # exactly at a word's 16th base
    assert both_orientations(L, stored, {115: 2}, 300, 100)[1] == b"16M1I23M1I8M"
    assert both_orientations(L, plain, {116: 0}, 300, 100)[1] == b"16M1D32M"              # at the next word's first base
    assert both_orientations(L, stored, {116: 0}, 300, 100)[1] == b"16M1D24M1I8M"
    assert both_orientations(L, plain, {123: 3}, 300, 100)[1] == b"24M2I22M"              # in the middle of the second word
    assert both_orientations(L, stored, {123: 3}, 300, 100)[1] == b"24M2I14M1I8M"
    # the reverse mate's words end at other bases: 40 ops over 37 bases of reference
    assert both_orientations(L, [M] * 40, {110: 4}, 300, 100)[1] == b"11M3I26M"


def test_a_mate_without_an_entry_in_reach_is_the_plain_record(trial_lib):
    """its record is the record of the same rows without variants (rsq_sam.h SamFormat), except for "_allele<a>" in the QNAME and XI:i:0"""
    from test_truth_sam import sam_pair
    rng = np.random.default_rng(31)
    variants = {40: 0, 41: 3, 300: 2, 420: 0}
    for strand in (0, 1):
        mates = [make_mate(rng, random_template(rng, 30, 0.1), [M, M], 1, 33), make_mate(rng, random_template(rng, 25, 0.1), [], 0, 33)]
        # 100 in the reference is 101 in the allele, and stays so up to 300
        frag = fragment(2, 100, 150, strand)
        fields, placed = check_var_pair(trial_lib, mates, frag, variants, 500)
        assert (placed[:, 2] == 0).all() and int(placed[strand][0]) == 101
        f1, f2, sam, _ = run_var_pair(trial_lib, False, mates, frag, 33, variants, 500)
        recs = [(r[0].replace(b"_allele1", b""), r[1], r[2]) for r in (parse_fastq(f1)[0], parse_fastq(f2)[0])]
        plain = sam_pair(frag, recs[0], recs[1], NAMES, 33)
        assert sam.replace(b"_allele1", b"").replace(b"\tXI:i:0\n", b"\n") == plain and b"_allele1:" in sam


def test_allele_copies_take_the_fragments_own_coordinates(trial_lib):
    """substitutions only: no FragmentVar, today's arithmetic with "_allele<a>" and XI:i:0"""
    rng = np.random.default_rng(32)
    for strand in (0, 1):
        mates = [make_mate(rng, random_template(rng, 30, 0.1), [M, M], 1, 64), make_mate(rng, [D, D, M, M, M, D], [], 0, 64)]
        fields, placed = check_var_pair(trial_lib, mates, fragment(0, 1000, 80, strand), {}, 5000, phred_offset=64, has_fv=False, allele_id=0)
        assert fields[0][0].startswith(b"ReseqRead_3_17_allele0:") and fields[0][-1] == b"XI:i:0" and (placed[:, 2] == 0).all()
    # one allele: the id names none
    fields, _ = check_var_pair(trial_lib, mates, fragment(0, 1000, 80, 0), {}, 5000, phred_offset=64, has_fv=False, allele_id=0, num_alleles=1)
    assert fields[0][0].startswith(b"ReseqRead_3_17:")


def test_unmapped_pairs_carry_the_tag(trial_lib):
    rng = np.random.default_rng(33)
    mates = [make_mate(rng, [], [M] * 9, 2, 33), make_mate(rng, [], [M] * 12, 0, 33)]
    fields, _ = check_var_pair(trial_lib, mates, None, {5: 3}, 100, adapter_only_number=77)
    assert [f[1] for f in fields] == [b"77", b"141"] and fields[1][-1] == b"XI:i:0"


def test_records_spelled_out(trial_lib):
    """a pair against literal expectations, independent of the statement: the allele of a 2000-base sequence has 1010 deleted, 4 bases at 1020 (3 inserted), and
    1030 and 1031 deleted; the fragment covers the reference positions 1000 .. 1059: 60 - 3 reference bases and 3 inserted ones, length 60"""
    rng = np.random.default_rng(34)
    variants = {1010: 0, 1020: 4, 1030: 0, 1031: 0}
    first = make_mate(rng, [M] * 8 + [I] + [M] * 6 + [D] + [M] * 10, [M, M, M], 0, 33)       # 25 template bases: 1000 .. 1009, 1011 .. 1020, 3 inserted, 1021, 1022
    second = make_mate(rng, [M] * 30, [], 1, 33)                                              # the last 30 allele bases: 1028, 1029, 1032 .. 1059
    fields, placed = check_var_pair(trial_lib, [first, second], fragment(0, 1000, 60, 0), variants, 2000)
    a, b = fields
    # 8M 1I 2M | 1D (1010) | 4M, the read's D falls on 1015, 5M (1016 .. 1020), 3 inserted, 2M: reference bases 1000 .. 1022
    assert (a[0], a[1], a[3], a[5], a[7], a[8]) == (b"ReseqRead_3_17_allele1:1001:chrA:1060:1101:1337:1337", b"99", b"1001", b"8M1I2M1D4M1D5M3I2M3S", b"1029", b"60")
    assert (b[1], b[3], b[5], b[7], b[8], b[-1]) == (b"147", b"1029", b"1S2M2D28M", b"1001", b"-60", b"XI:i:0")
    assert [int(p[3]) for p in placed] == [1000, 1028] and [int(p[4]) for p in placed] == [23, 32]
    # the same pair on the other strand: the first mate is the reverse one and covers the last 25 allele bases, 1035 .. 1059 (POS 1036)
    fields, _ = check_var_pair(trial_lib, [first, second], fragment(0, 1000, 60, 1), variants, 2000)
    a, b = fields
    assert (a[1], a[3], a[5], a[7]) == (b"83", b"1036", b"3S10M1D6M1I8M", b"1001")
    assert (b[1], b[3], b[5], b[8]) == (b"163", b"1001", b"10M1D10M3I7M1S", b"60")
