"""Truth alignments (reseq_amd/csrc/rsq_sam.h; include/reseq_amd.h rsq_sim_pairs_sam) without a GPU: the header, and the per-lane functions -- ops walk,
alignment, CIGAR writer, reversed data lines, record size, record -- run on the CPU (tests/hostemu/sam_trial.cpp over truth_trial.h, built here with g++) on crafted rows and
compared with `sam_pair`, this module's own statement of the record's rules, applied to the FASTQ records the same rows give.  The statement works from the
FASTQ text and the fragment alone (the SAM text is a pure function of the two); tests/test_truth_sam_gpu.py applies it to the device's output."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from reseq_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

# ------------------------------------------------------------------------------------------------ the statement
_ELEMENT = re.compile(rb"(\d+)([MIDSH])")
_COMPLEMENT = bytes.maketrans(b"ACGTN", b"TGCAN")


def parse_fastq(text):
    """[(id line without '@', SEQ, QUAL)]"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


def template_part(cigar):
    """the elements of ReSeq's CIGAR in front of its first S or H element"""
    elements = [(int(n), op) for n, op in _ELEMENT.findall(cigar)]
    assert b"".join(b"%d%s" % e for e in elements) == cigar
    part = []
    for n, op in elements:
        if op in (b"S", b"H"):
            break
        part.append((n, op))
    return part


def clean(part):
    """zero-length elements dropped, equal neighbours merged, D at either end dropped: (elements, D dropped at the first end, at the last end) in read order"""
    out = []
    for n, op in part:
        if n == 0:
            continue
        if out and out[-1][1] == op:
            out[-1] = (out[-1][0] + n, op)
        else:
            out.append((n, op))
    lead = out.pop(0)[0] if out and out[0][1] == b"D" else 0
    trail = out.pop()[0] if out and out[-1][1] == b"D" else 0
    return out, lead, trail


def mate_alignment(frag, seg, record):
    """POS, last aligned position, CIGAR, reverse of one mate of a mapped pair"""
    cigar = record[0].split(b" ")[1]
    part = template_part(cigar)
    q = sum(n for n, op in part if op in (b"M", b"I"))
    t = sum(n for n, op in part if op in (b"M", b"D"))
    elements, lead, trail = clean(part)
    reverse = seg != int(frag["strand"])
    d_left, d_right = (trail, lead) if reverse else (lead, trail)
    start, end = int(frag["start"]), int(frag["start"]) + int(frag["len"])
    pos = (end - t if reverse else start) + 1 + d_left
    last = pos + (t - d_left - d_right) - 1
    clip = len(record[1]) - q
    texts = [b"%d%s" % e for e in (elements[::-1] if reverse else elements)]
    clip_text = [b"%dS" % clip] if clip else []
    return pos, last, b"".join(clip_text + texts if reverse else texts + clip_text) or b"*", reverse


def sam_pair(frag, rec1, rec2, names, phred_offset):
    """the two SAM records of a pair; frag None (or of length 0): an adapter-only pair; names: the reference ids' first parts (bytes)"""
    out = []
    mapped = frag is not None and int(frag["len"]) > 0
    al = [mate_alignment(frag, seg, rec) for seg, rec in enumerate((rec1, rec2))] if mapped else None
    for seg, (idline, seq, qual) in enumerate((rec1, rec2)):
        qname, cigar, errors = idline.split(b" ")
        assert errors[:1] == b"E"
        qual33 = bytes(c - phred_offset + 33 for c in qual)
        if mapped:
            pos, last, sam_cigar, reverse = al[seg]
            other = al[seg ^ 1]
            span = max(last, other[1]) - min(pos, other[0]) + 1
            tlen = span if (pos < other[0] or (pos == other[0] and seg == 0)) else -span
            flag = 0x1 | 0x2 | (0x10 if reverse else 0) | (0x20 if other[3] else 0) | (0x80 if seg else 0x40)
            if reverse:
                seq, qual33 = seq.translate(_COMPLEMENT)[::-1], qual33[::-1]
            fields = [qname, b"%d" % flag, names[int(frag["seq"])], b"%d" % pos, b"60", sam_cigar, b"=", b"%d" % other[0], b"%d" % tlen]
        else:
            fields = [qname, b"141" if seg else b"77", b"*", b"0", b"0", b"*", b"*", b"0", b"0"]
        out.append(b"\t".join(fields + [seq, qual33, b"XC:Z:" + cigar, b"XE:i:" + errors[1:]]) + b"\n")
    return b"".join(out)


def sam_text(frags, fastq1, fastq2, names, phred_offset):
    """the SAM text of a call: frags None = adapter-only pairs"""
    r1, r2 = parse_fastq(fastq1), parse_fastq(fastq2)
    assert len(r1) == len(r2) and (frags is None or len(frags) == len(r1))
    return b"".join(sam_pair(None if frags is None else frags[i], r1[i], r2[i], names, phred_offset) for i in range(len(r1)))


# ------------------------------------------------------------------------------------------------ the header
def test_header_of_the_golden_reference():
    ref = api.Reference(os.path.join(GOLDEN, "reference-test.fa"))
    try:
        text = ref.sam_header()
        assert text == (b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@SQ\tSN:NC_000913.3_1-500\tLN:500\n@SQ\tSN:NC_000913.3_10000-10500\tLN:501\n"
                        b"@PG\tID:reseq_amd\tPN:reseq_amd\n")
        need = C.c_size_t(0)
        small = C.create_string_buffer(b"#" * 16, 16)
        assert api.lib().rsq_ref_sam_header(ref.h, small, 16, C.byref(need)) == api.RSQ_ENOSPC
        assert need.value == len(text) and small.raw == b"#" * 16
        exact = C.create_string_buffer(len(text))
        assert api.lib().rsq_ref_sam_header(ref.h, exact, len(text), C.byref(need)) == api.RSQ_OK and exact.raw == text
    finally:
        ref.close()


# ------------------------------------------------------------------------------------------------ the per-lane functions on the host
class TrialMate(C.Structure):
    _fields_ = [("read_len", C.c_uint32), ("n_iter_m", C.c_uint32), ("n_iter_s", C.c_uint32), ("hard_clip", C.c_uint32), ("num_errors", C.c_uint32),
                ("seq", C.c_void_p), ("qual", C.c_void_p), ("ops", C.c_void_p)]


class TrialPair(C.Structure):
    _fields_ = [("has_fragment", C.c_int32), ("seq", C.c_uint32), ("start", C.c_uint32), ("len", C.c_uint32), ("strand", C.c_uint32), ("block", C.c_uint32),
                ("number", C.c_uint32), ("adapter_only_number", C.c_uint64), ("phred_offset", C.c_uint32), ("tile", C.c_uint32), ("base_identifier", C.c_char_p),
                ("names", C.c_char_p), ("name_ptr", C.c_void_p), ("mate", TrialMate * 2)]


NAMES = [b"chrA", b"NC_000913.3_1-500", b"s"]
M, D, I = 0, 1, 2          # the 2-bit ops: the part's own op (M in the template part, S in the adapter part), D, I


def build_trial(tmp_path_factory, name):
    """tests/hostemu/<name>.cpp as a shared library (both formats' trials are tests/hostemu/truth_trial.h; tests/test_truth_bam.py builds bam_trial)"""
    out = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-shared", "-o", out,
                    os.path.join(HERE, "hostemu", name + ".cpp")], check=True)
    return C.CDLL(out)


@pytest.fixture(scope="module")
def trial_lib(tmp_path_factory):
    L = build_trial(tmp_path_factory, "sam_trial")
    L.sam_trial.argtypes = [C.POINTER(TrialPair), C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_void_p]
    return L


def make_mate(rng, template_ops, adapter_ops, hard_clip, phred_offset, with_n=False):
    """a mate from its ops: the read has a base for every M / I of the template part, every S / I of the adapter part and every base of the tail"""
    ops = np.array(list(template_ops) + list(adapter_ops), np.uint8)
    read_len = int(sum(o != D for o in ops)) + hard_clip
    seq = rng.integers(0, 4, read_len).astype(np.uint8)
    if with_n and read_len:
        seq[rng.integers(0, read_len, max(1, read_len // 5))] = 4
    qual = (rng.integers(2, 41, read_len) + phred_offset).astype(np.uint8)
    return dict(read_len=read_len, n_iter_m=len(template_ops), n_iter_s=len(adapter_ops), hard_clip=hard_clip, num_errors=int(rng.integers(0, 12)), seq=seq, qual=qual, ops=ops)


def fill_trial(mates, frag, phred_offset, adapter_only_number, tile, base, names):
    """(the trial's input, the arrays it points to: to be kept alive over the call)"""
    name_ptr = np.concatenate([[0], np.cumsum([len(n) for n in names])]).astype(np.uint32)
    t = TrialPair(has_fragment=0 if frag is None else 1, adapter_only_number=adapter_only_number, phred_offset=phred_offset, tile=tile, base_identifier=base,
                  names=b"".join(names), name_ptr=name_ptr.ctypes.data)
    if frag is not None:
        t.seq, t.start, t.len, t.strand, t.block, t.number = (int(frag[k]) for k in ("seq", "start", "len", "strand", "block", "number"))
    keep = [name_ptr]
    for seg, m in enumerate(mates):
        arrays = [np.ascontiguousarray(m[k]) if len(m[k]) else np.zeros(1, np.uint8) for k in ("seq", "qual", "ops")]
        keep.append(arrays)
        t.mate[seg] = TrialMate(m["read_len"], m["n_iter_m"], m["n_iter_s"], m["hard_clip"], m["num_errors"], *(a.ctypes.data for a in arrays))
    return t, keep


def run_pair(L, mates, frag, phred_offset, adapter_only_number=0, tile=1101, base=b"ReseqRead_"):
    """(fastq record 1, fastq record 2, SAM text of the pair) from the trial library; checks sam_record_size against what the record function wrote, and (inside
    the trial) that the writer kernel's two sinks a mate give the same bytes"""
    t, keep = fill_trial(mates, frag, phred_offset, adapter_only_number, tile, base, NAMES)
    cap = 8192
    f1, f2, sam = (C.create_string_buffer(cap) for _ in range(3))
    sizes = np.zeros(6, np.uint32)
    assert L.sam_trial(C.byref(t), f1, f2, sam, cap, sizes.ctypes.data) == 0
    assert sizes[2] == sizes[4] and sizes[3] == sizes[5], sizes          # sam_record_size is the record's length
    return f1.raw[:sizes[0]], f2.raw[:sizes[1]], sam.raw[:int(sizes[2]) + int(sizes[3])]


def check_pair(L, mates, frag, phred_offset, **kw):
    f1, f2, sam = run_pair(L, mates, frag, phred_offset, **kw)
    want = sam_text(None if frag is None else [frag], f1, f2, NAMES, phred_offset)
    assert sam == want, (sam, want, f1, f2)
    return sam


def fragment(seq, start, length, strand, block=3, number=17):
    return dict(seq=seq, start=start, len=length, strand=strand, block=block, number=number)


def template_bases(ops):
    return sum(o != I for o in ops)


def random_template(rng, read_bases, p_indel):
    """template-part ops with `read_bases` M / I among them"""
    ops = []
    while sum(o != D for o in ops) < read_bases:
        r = rng.random()
        ops.append(D if r < p_indel else I if r < 2 * p_indel else M)
    return ops


@pytest.mark.parametrize("phred_offset", [33, 64])
def test_every_read_length_in_both_orientations(trial_lib, phred_offset):
    """read lengths 1 .. 37: all residues modulo 4 and one to ten words per row, each as the forward and as the reverse mate, with and without indels"""
    rng = np.random.default_rng(1000 + phred_offset)
    for read_len in range(1, 38):
        for strand in (0, 1):
            for p_indel in (0.0, 0.12):
                mates = []
                for seg in (0, 1):
                    n_adapter = int(rng.integers(0, read_len)) if rng.random() < 0.4 else 0
                    mates.append(make_mate(rng, random_template(rng, read_len - n_adapter, p_indel), [M] * n_adapter, 0, phred_offset, with_n=read_len % 3 == 0))
                    assert mates[-1]["read_len"] == read_len
                length = max(template_bases(m["ops"][:m["n_iter_m"]]) for m in mates) + int(rng.integers(0, 30))
                sam = check_pair(trial_lib, mates, fragment(int(rng.integers(0, 3)), int(rng.integers(0, 100000)), length, strand), phred_offset)
                flags = [int(line.split(b"\t")[1]) for line in sam.splitlines()]
                assert flags == ([99, 147] if strand == 0 else [83, 163])


CRAFTED = {
    # name: (template ops, adapter ops, tail)
    "leading D (ReSeq prints 0M first)": ([D, D, M, M, M, I, M, M], [], 0),
    "trailing D": ([M, M, M, M, D, M, M, D, D, D], [], 0),
    "D at both ends": ([D, M, M, M, I, I, M, D, M, M, D], [M, M], 0),
    "leading I": ([I, I, M, M, M, M, D, M], [], 0),
    "trailing I": ([M, M, M, M, I], [M, M, M], 2),
    "adapter part begins with I (0S)": ([M] * 9, [I, M, M, D, M], 0),
    "adapter part begins with D (0S)": ([M] * 7, [D, D, M, I, I, M], 3),
    "I and D inside the adapter part": ([M, M, D, M, M], [M, I, M, D, D, M, I], 0),
    "a tail alone behind the template": ([M] * 11, [], 4),
    "long plain stretches around an indel": ([M] * 35 + [D] + [M] * 40 + [I] + [M] * 33, [M] * 5, 1),
    "sixteen plain ops between two D": ([D] + [M] * 16 + [D] + [M] * 16 + [D], [], 0),
    "neighbouring I and D": ([M, M, I, D, I, D, D, M, M], [], 0),
    "one base": ([M], [], 0),
    "a template part of D alone": ([D, D, D], [M, M, M, M], 0),
}


@pytest.mark.parametrize("phred_offset", [33, 64])
@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_ops(trial_lib, name, phred_offset):
    rng = np.random.default_rng(sorted(CRAFTED).index(name) * 2 + phred_offset)
    template_ops, adapter_ops, tail = CRAFTED[name]
    plain = make_mate(rng, [M] * 21, [M] * 3, 1, phred_offset)
    for strand in (0, 1):
        for seg in (0, 1):                                    # the crafted mate as either segment: forward and reverse
            crafted = make_mate(rng, template_ops, adapter_ops, tail, phred_offset, with_n=True)
            mates = [plain, crafted] if seg else [crafted, plain]
            length = max(21, template_bases(template_ops)) + 5
            sam = check_pair(trial_lib, mates, fragment(1, 4321, length, strand), phred_offset)
            fields = sam.splitlines()[seg].split(b"\t")
            assert not re.search(rb"(^|[A-Z])0[A-Z]", fields[5]) and b"H" not in fields[5] and not re.match(rb"\d+D", fields[5]) and not fields[5].endswith(b"D")
            if "0M" in name or "0S" in name:                  # ... which the id's own CIGAR does hold, and the tag keeps
                assert re.search(rb"(^|[A-Z])0[MS]", fields[11][5:])


def test_crafted_cigars_spelled_out(trial_lib):
    """a few records against literal expectations, independent of the statement above"""
    rng = np.random.default_rng(5)
    plain = make_mate(rng, [M] * 10, [], 0, 33)
    crafted = make_mate(rng, [D, D, M, M, M, I, M, M, D], [I, M, M], 2, 33)      # id: 0M2D3M1I2M1D0S1I2S2H; 6 template read bases, 8 template bases, read length 11
    frag = fragment(0, 1000, 40, 0)
    fwd = run_pair(trial_lib, [crafted, plain], frag, 33)[2].splitlines()
    f = fwd[0].split(b"\t")
    assert (f[1], f[3], f[5], f[11]) == (b"99", b"1003", b"3M1I2M5S", b"XC:Z:0M2D3M1I2M1D0S1I2S2H")
    assert fwd[1].split(b"\t")[3] == b"1031" and f[7] == b"1031" and f[8] == b"38" and fwd[1].split(b"\t")[8] == b"-38"      # [1002, 1007) and [1030, 1040)
    rev = run_pair(trial_lib, [plain, crafted], frag, 33)[2].splitlines()
    r = rev[1].split(b"\t")
    assert (r[1], r[3], r[5]) == (b"147", b"1034", b"5S2M1I3M")               # covers [1040 - 8, 1040): the trailing D (read order) is at the left end: POS 1033 + 1


def test_adapter_only_pair(trial_lib):
    rng = np.random.default_rng(9)
    for phred_offset in (33, 64):
        mates = [make_mate(rng, [], [M] * 9 + [I, M, D, M], 5, phred_offset), make_mate(rng, [], [M] * 12, 3, phred_offset, with_n=True)]
        sam = check_pair(trial_lib, mates, None, phred_offset, adapter_only_number=4_300_000_123)
        first, second = (line.split(b"\t") for line in sam.splitlines())
        assert first[:9] == [b"ReseqRead_0_4300000123:0:Adapter:0:1101:1337:1337", b"77", b"*", b"0", b"0", b"*", b"*", b"0", b"0"]
        assert second[1] == b"141" and second[0] == first[0]
    # a fragment of length 0 inside rsq_sim_pairs is unmapped as well
    sam = check_pair(trial_lib, mates, fragment(2, 77, 0, 1), 64)
    assert [line.split(b"\t")[1] for line in sam.splitlines()] == [b"77", b"141"]


def test_equal_pos_mates(trial_lib):
    """both mates over the whole fragment: equal POS, TLEN positive for segment 0"""
    rng = np.random.default_rng(11)
    for strand in (0, 1):
        mates = [make_mate(rng, [M] * 20, [M] * 4, 0, 33), make_mate(rng, [M] * 20, [], 2, 33)]
        sam = check_pair(trial_lib, mates, fragment(0, 500, 20, strand), 33)
        first, second = (line.split(b"\t") for line in sam.splitlines())
        assert first[3] == second[3] == b"501" and first[8] == b"20" and second[8] == b"-20"
