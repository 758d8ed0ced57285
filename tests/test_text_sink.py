"""The writers of the text kernels' image (reseq_amd/csrc/rsq_format.h: ImageSink, image_header, image_line_part, image_record_part) without a GPU: they are
host/device functions, and tests/hostemu/text_trial.cpp (built here with g++) runs them on a byte buffer beside format_record (rsq_text.h), the writer of the
host emulation and of the kernels' fallback.  A record's four parts are written as the kernel's four lanes write them, between two neighbours, in ascending and in
descending order, into a zeroed range with guard bytes around it; the number writer alone is compared with snprintf."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
M, D, I = 0, 1, 2          # the 2-bit ops: the part's own op (M in the template part, S in the adapter part), D, I


class TrialRecord(C.Structure):
    _fields_ = [("has_fragment", C.c_int32), ("seq", C.c_uint32), ("start", C.c_uint32), ("len", C.c_uint32), ("strand", C.c_uint32), ("block", C.c_uint32),
                ("number", C.c_uint32), ("allele", C.c_uint32), ("num_alleles", C.c_uint32), ("has_end", C.c_int32), ("end", C.c_uint32),
                ("adapter_only_number", C.c_uint64), ("tile", C.c_uint32), ("read_len", C.c_uint32), ("n_iter_m", C.c_uint32), ("n_iter_s", C.c_uint32),
                ("hard_clip", C.c_uint32), ("num_errors", C.c_uint32), ("base_identifier", C.c_char_p), ("names", C.c_void_p), ("name_ptr", C.c_void_p),
                ("bases", C.c_void_p), ("quals", C.c_void_p), ("ops", C.c_void_p)]


@pytest.fixture(scope="module")
def trial(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("text_trial") / "libtext_trial.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-shared", "-o", out,
                    os.path.join(HERE, "hostemu", "text_trial.cpp")], check=True)
    L = C.CDLL(out)
    L.text_trial_fastq.argtypes = [C.POINTER(TrialRecord), C.c_uint32, C.c_int, C.c_char_p, C.c_uint32]
    L.text_trial_numbers.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    L.text_trial_numbers.restype = C.c_int64
    L.text_trial_strings.argtypes = [C.c_void_p, C.c_uint32]
    return L


NAMES = [b"s", b"chrA", b"chr12", b"NC_000913.3_an_id_of_37_characters__x"]
assert [len(n) for n in NAMES] == [1, 4, 5, 37]


def name_table():
    """the names one after the other in a buffer that begins and ends on a word boundary (the writer reads the words a name lies in)"""
    text = b"".join(NAMES)
    buf = np.zeros((len(text) + 8) // 4, np.uint32)
    buf.view(np.uint8)[:len(text)] = np.frombuffer(text, np.uint8)
    ptr = np.concatenate([[0], np.cumsum([len(n) for n in NAMES])]).astype(np.uint32)
    return buf, ptr


def expected_record(rec, bases, quals, ops, base):
    """the record by this module's own statement of Simulator.cpp:596-632 (format_record is the reference the issue names; this pins format_record too)"""
    def cigar():
        out, it = [], 0
        for part, n in ((b"M", rec["n_iter_m"]), (b"S", rec["n_iter_s"])):
            element, length = part, 0
            for _ in range(n):
                want = (part, b"D", b"I")[ops[it]]
                it += 1
                if want == element:
                    length += 1
                else:
                    out.append(b"%d%s" % (length, element))
                    element, length = want, 1
            if length:
                out.append(b"%d%s" % (length, element))
        if rec["hard_clip"]:
            out.append(b"%dH" % rec["hard_clip"])
        return b"".join(out)
    if rec["has_fragment"]:
        end = rec["end"] if rec["has_end"] else rec["start"] + rec["len"]
        first, second = (end, rec["start"] + 1) if rec["strand"] else (rec["start"] + 1, end)
        allele = b"_allele%d" % rec["allele"] if rec["num_alleles"] > 1 else b""
        ident = b"%d_%d%s:%d:%s:%d" % (rec["block"], rec["number"], allele, first, NAMES[rec["seq"]], second)
    else:
        ident = b"0_%d:0:Adapter:0" % rec["adapter_only_number"]
    plain = all(o == M for o in ops)
    text = cigar()
    if plain:                                                       # the writers' short cut for reads without indels: the same text
        assert text == b"".join(b"%d%s" % (n, c) for n, c in ((rec["n_iter_m"], b"M"), (rec["n_iter_s"], b"S"), (rec["hard_clip"], b"H")) if n)
    return (b"@" + base + ident + b":%d:1337:1337 " % rec["tile"] + text + b" E%d\n" % rec["num_errors"] + bytes(b"ACGTN"[c] for c in bases) + b"\n+\n" +
            bytes(quals) + b"\n")


def default_record(**kw):
    rec = dict(has_fragment=1, seq=1, start=4321, len=300, strand=0, block=3, number=17, allele=0, num_alleles=1, has_end=0, end=0, adapter_only_number=0, tile=1101,
               hard_clip=0, num_errors=2)
    rec.update(kw)
    return rec


def run_record(L, rec, template_ops, adapter_ops, rng, phred_offset=33, base=b"ReseqRead_", aligns=range(16), with_n=True):
    """one record at every alignment in both orders; returns its text"""
    ops = np.array(list(template_ops) + list(adapter_ops) + [0], np.uint8)[:len(template_ops) + len(adapter_ops)]
    read_len = int(np.sum(ops != D)) + rec["hard_clip"]
    bases = rng.integers(0, 4, read_len).astype(np.uint8)
    if with_n and read_len > 2:
        bases[rng.integers(0, read_len, max(1, read_len // 5))] = 4
    quals = (rng.integers(2, 42, read_len) + phred_offset).astype(np.uint8)
    names, name_ptr = name_table()
    arrays = [a if len(a) else np.zeros(1, np.uint8) for a in (bases, quals, ops)]
    t = TrialRecord(base_identifier=base, names=names.ctypes.data, name_ptr=name_ptr.ctypes.data, read_len=read_len, n_iter_m=len(template_ops), n_iter_s=len(adapter_ops),
                    bases=arrays[0].ctypes.data, quals=arrays[1].ctypes.data, ops=arrays[2].ctypes.data, **rec)
    want = expected_record(dict(rec, n_iter_m=len(template_ops), n_iter_s=len(adapter_ops)), bases, quals, ops, base)
    cap = 4096
    for align in aligns:
        for order in (0, 1):
            got = C.create_string_buffer(cap)
            rc = L.text_trial_fastq(C.byref(t), align, order, got, cap)
            assert rc == len(want), (rc, align, order, got.raw[:len(want)], want)      # -2: the image differs (got: what it holds), -3: a guard byte changed
            assert got.raw[:rc] == want, (align, order)
    return want


@pytest.mark.parametrize("phred_offset", [33, 64])
def test_read_lengths_at_every_alignment(trial, phred_offset):
    """1 .. 13 and 147 .. 152: every residue modulo four at one to four words a line and at the flagship's 38, every split of the words over a line's two lanes"""
    rng = np.random.default_rng(100 + phred_offset)
    for read_len in list(range(1, 14)) + list(range(147, 153)):
        run_record(trial, default_record(seq=int(rng.integers(0, 4)), strand=read_len & 1), [M] * read_len, [], rng, phred_offset)
        if read_len > 4:                                              # an adapter part and a tail in the CIGAR
            run_record(trial, default_record(hard_clip=2), [M] * (read_len - 4), [M] * 2, rng, phred_offset, aligns=(0, 5, 10, 15))


BORDERS = [10 ** k - d for k in range(1, 10) for d in (1, 0)] + [10 ** 9, 2 ** 32 - 1, 0, 1, 4294, 42949, 99999999, 100000000]
assert 9 in BORDERS and 10 in BORDERS and 999_999_999 in BORDERS and 1_000_000_000 in BORDERS


def test_id_variants(trial):
    rng = np.random.default_rng(7)
    some = (0, 1, 2, 3, 7, 13)
    for seq in range(4):                                              # names of 1, 4, 5 and 37 characters
        for strand in (0, 1):
            run_record(trial, default_record(seq=seq, strand=strand), [M] * 30, [], rng)
    run_record(trial, default_record(num_alleles=2, allele=1), [M] * 30, [], rng)                     # "_allele1"
    run_record(trial, default_record(num_alleles=2, allele=0, number=123456), [M] * 29, [], rng)
    run_record(trial, default_record(has_end=1, end=4700), [M] * 30, [], rng)                         # a variant end
    run_record(trial, default_record(has_end=1, end=4700, strand=1, num_alleles=2, allele=1), [M] * 31, [], rng)
    run_record(trial, default_record(has_fragment=0, adapter_only_number=12), [], [M] * 30, rng)      # an adapter-only pair
    for base in (b"R", b"ab_", b"Read", b"ReseqRead_", b"x" * 63, b"y" * 64):                          # the base identifier: every residue of its length, the longest
        run_record(trial, default_record(), [M] * 30, [], rng, base=base, aligns=some)
    for v in BORDERS:                                                 # every number of the id line at every border
        if v:
            run_record(trial, default_record(block=v, number=BORDERS[(BORDERS.index(v) + 3) % len(BORDERS)] or 1), [M] * 10, [], rng, aligns=some)
            run_record(trial, default_record(has_fragment=0, adapter_only_number=v), [], [M] * 10, rng, aligns=some)
        if v + 300 < 2 ** 32:
            run_record(trial, default_record(start=v, len=300), [M] * 10, [], rng, aligns=some)
            run_record(trial, default_record(start=v, len=300, strand=1), [M] * 10, [], rng, aligns=some)
        if v < 2 ** 16:
            run_record(trial, default_record(tile=v, num_errors=v), [M] * 10, [], rng, aligns=some)
    for v in (2 ** 32, 2 ** 32 + 1, 10 ** 10 - 1, 10 ** 10, 4_300_000_123, 10 ** 18 - 1, 10 ** 18, 10 ** 18 + 7, 2 ** 63, 2 ** 64 - 1, 12_000_000_000_000_000_345):
        run_record(trial, default_record(has_fragment=0, adapter_only_number=v), [], [M] * 9, rng, aligns=some)


CIGARS = {
    "plain with an adapter part and a tail": ([M] * 21, [M] * 3, 1),
    "a tail alone": ([M] * 11, [], 4),
    "leading D (0M first)": ([D, D, M, M, M, I, M, M], [], 0),
    "trailing D": ([M, M, M, M, D, M, M, D, D, D], [], 0),
    "I and D in both parts, H behind": ([D, M, M, M, I, I, M, D, M, M, D], [M, I, M, D, D, M, I], 3),
    "adapter part begins with I (0S)": ([M] * 9, [I, M, M, D, M], 0),
    "long plain stretches around indels": ([M] * 35 + [D] + [M] * 40 + [I] + [M] * 33, [M] * 5, 1),
    "sixteen plain ops between two D": ([D] + [M] * 16 + [D] + [M] * 16 + [D], [], 0),
    "counts of one to three digits": ([M] * 100 + [I] + [M] * 9 + [D] * 12 + [M] * 7, [M] * 20, 3),
}


@pytest.mark.parametrize("name", sorted(CIGARS))
def test_cigars(trial, name):
    rng = np.random.default_rng(sorted(CIGARS).index(name))
    template_ops, adapter_ops, tail = CIGARS[name]
    for phred_offset in (33, 64):
        text = run_record(trial, default_record(hard_clip=tail, num_errors=11), template_ops, adapter_ops, rng, phred_offset)
    if "I and D in both" in name:
        assert b" 0M1D3M2I1M1D2M1D1S1I1S2D1S1I3H E11\n" in text


def test_numbers_equal_snprintf(trial):
    rng = np.random.default_rng(11)
    narrow = np.array(BORDERS + [int(v) for v in rng.integers(0, 2 ** 32, 3000)] + [int(v) for v in 10 ** rng.uniform(0, 9.6, 3000)], np.uint64)
    assert trial.text_trial_numbers(narrow.ctypes.data, len(narrow), 0) == -1
    assert trial.text_trial_numbers(narrow.ctypes.data, len(narrow), 1) == -1
    wide = np.array([2 ** 32, 2 ** 32 + 1, 10 ** 10 - 1, 10 ** 10, 10 ** 18 - 1, 10 ** 18, 10 ** 18 + 1, 10 ** 19, 2 ** 64 - 1, 10 ** 9 * (2 ** 32), 5_000_000_000_000_000_000] +
                    [10 ** k - d for k in range(10, 20) for d in (1, 0)] + [int(v) for v in rng.integers(2 ** 32, 2 ** 63, 2000)], np.uint64)
    assert trial.text_trial_numbers(wide.ctypes.data, len(wide), 1) == -1


def test_strings_from_every_alignment(trial):
    """ImageSink::str reads the aligned words its characters lie in: lengths 0 .. 41 from every alignment of the source, with and without '@' in front and ' ' behind"""
    rng = np.random.default_rng(13)
    for length in range(0, 42):
        source = np.zeros(16, np.uint32)
        source.view(np.uint8)[:] = rng.integers(33, 127, 64)
        assert trial.text_trial_strings(source.ctypes.data, length) == 0, length
