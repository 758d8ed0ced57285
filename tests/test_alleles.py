"""The alleles of a reference with variants as FASTA text (reseq_amd/csrc/rsq_alleles.h; rsq_sim_alleles_fasta, `reseq illuminaPE -V ... --writeAlleles`) without a
GPU: the kernel's two per-lane steps run as loops on the CPU (tests/hostemu/alleles_trial.cpp, built here with g++) over crafted references, and every piece is
compared with this module's text of the alleles spelled out base by base (build_allele of tests/test_truth_variants.py: no coordinate map, no arithmetic on
lines); and the host calls of the C ABI (lengths, the text's size, its .fai, the headers that list the alleles) on the golden variant file and on synthetic sets.
tests/test_alleles_gpu.py applies the same text to the device's output."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from reseq_amd import api, synth
from test_truth_bam import decode_bam_header
from test_truth_sam import build_trial
from test_truth_variants import build_allele

LINE = 70


# ------------------------------------------------------------------------------------------------ the statement
def spell(codes, mine):
    """the letters of an allele: codes = the sequence's base codes, mine = {position: the replacement's letters} of THIS allele"""
    allele = build_allele(len(codes), {p: len(b) for p, b in mine.items()})
    return b"".join((mine[p][k] if p in mine else "ACGT"[codes[p]]).encode() for _, p, k in allele)


def all_letters(seqs, variants, num_alleles):
    """{(sequence, allele): letters}; seqs: [(name, codes)], variants: {sequence: [(position, letters, allele bits)]}"""
    return {(s, a): spell(codes, {p: b for p, b, bits in variants.get(s, []) if bits >> a & 1}) for s, (_, codes) in enumerate(seqs) for a in range(num_alleles)}


def record_text(name, allele, letters):
    return b">" + name + b"_allele%d\n" % allele + b"".join(letters[i:i + LINE] + b"\n" for i in range(0, len(letters), LINE))


def fasta_text(names, letters, num_alleles):
    return b"".join(record_text(name, a, letters[s, a]) for s, name in enumerate(names) for a in range(num_alleles))


def fai_text(names, letters, num_alleles):
    """the index of fasta_text, offsets counted off the records' own texts"""
    out, at = [], 0
    for s, name in enumerate(names):
        for a in range(num_alleles):
            out.append(b"%s_allele%d\t%d\t%d\t%d\t%d\n" % (name, a, len(letters[s, a]), at + len(name) + 9 + len(str(a)), LINE, LINE + 1))
            at += len(record_text(name, a, letters[s, a]))
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ the kernel's lanes on the host
class TrialIn(C.Structure):
    _fields_ = [("n_seqs", C.c_uint32), ("num_alleles", C.c_uint32), ("seq_len", C.c_void_p), ("codes", C.c_void_p), ("names", C.c_char_p), ("name_ptr", C.c_void_p),
                ("var_ptr", C.c_void_p), ("var_pos", C.c_void_p), ("var_len", C.c_void_p), ("var_off", C.c_void_p), ("var_bases", C.c_void_p), ("var_allele", C.c_void_p),
                ("copies", C.c_int32)]


@pytest.fixture(scope="module")
def trial_lib(tmp_path_factory):
    L = build_trial(tmp_path_factory, "alleles_trial")
    L.alleles_trial.argtypes = [C.POINTER(TrialIn), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]
    return L


def run_trial(L, seqs, variants, num_alleles, pieces, copies=False):
    """pieces: [(at, bytes, lead)] -> ([their bytes], bytes of the whole text); None instead of the list when a piece reaches beyond the text"""
    u32 = lambda v: np.ascontiguousarray(v, np.uint32)
    names = [n.encode() for n, _ in seqs]
    listed = [(s, p, b, bits) for s in range(len(seqs)) for p, b, bits in variants.get(s, [])]
    var_ptr = u32(np.cumsum([0] + [len(variants.get(s, [])) for s in range(len(seqs))]))
    bases = np.array(["ACGT".index(c) for _, _, b, _ in listed for c in b] + [0], np.uint8)
    var_len = u32([len(b) for _, _, b, _ in listed] + [0])
    var_off = u32(np.cumsum([0] + [len(b) for _, _, b, _ in listed]))
    var_pos = u32([p for _, p, _, _ in listed] + [0])
    var_allele = np.array([w for _, _, _, bits in listed for w in (bits & (2 ** 64 - 1), bits >> 64)] + [0], np.uint64)
    seq_len, codes = u32([len(c) for _, c in seqs]), np.ascontiguousarray(np.concatenate([c for _, c in seqs] + [np.zeros(1, np.uint8)]), np.uint8)
    name_ptr = u32(np.cumsum([0] + [len(n) for n in names]))
    t = TrialIn(len(seqs), num_alleles, seq_len.ctypes.data, codes.ctypes.data, b"".join(names), name_ptr.ctypes.data, var_ptr.ctypes.data, var_pos.ctypes.data,
                var_len.ctypes.data, var_off.ctypes.data, bases.ctypes.data, var_allele.ctypes.data, 1 if copies else 0)
    at, size, lead = (np.ascontiguousarray([p[k] for p in pieces], d) for k, d in ((0, np.uint64), (1, np.uint64), (2, np.uint32)))
    out = C.create_string_buffer(int(size.sum()) + 1)
    total = C.c_uint64()
    rc = L.alleles_trial(C.byref(t), len(pieces), at.ctypes.data, size.ctypes.data, lead.ctypes.data, out, C.byref(total))
    if rc == -1:
        return None, total.value
    assert rc == 0, rc
    ends = np.cumsum([0] + [p[1] for p in pieces])
    return [out.raw[ends[i]:ends[i + 1]] for i in range(len(pieces))], total.value


def check_text(L, seqs, variants, num_alleles, rng, copies=False, n_random=12):
    """the whole text in one piece and in random pieces at random alignments; returns the text"""
    want = fasta_text([n.encode() for n, _ in seqs], all_letters(seqs, variants, num_alleles), num_alleles)
    pieces = [(0, len(want), 0)]
    for _ in range(n_random):
        at = int(rng.integers(0, len(want)))
        pieces.append((at, int(rng.integers(0, min(len(want) - at, 400) + 1)), int(rng.integers(0, 16))))
    got, total = run_trial(L, seqs, variants, num_alleles, pieces, copies)
    assert total == len(want)
    for (at, size, lead), text in zip(pieces, got):
        assert text == want[at:at + size], (at, size, lead)
    return want


def random_codes(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def letters_of(rng, n):
    return "".join("ACGT"[b] for b in rng.integers(0, 4, n))


def dense_variants(rng, length, num_alleles, every=3, longest=5):
    """a variant every few bases, replacements of 0 .. longest bases, each in a random set of alleles"""
    return [(p, letters_of(rng, int(rng.integers(0, longest + 1))), int(rng.integers(1, 2 ** num_alleles))) for p in range(length) if rng.random() < 1.0 / every]


def test_every_allele_length(trial_lib):
    """alleles of 0 .. 300 bases beside the plain sequence: the last line empty, one base, full, and one base more; a sequence that loses every base"""
    rng = np.random.default_rng(1)
    for n in range(0, 301):
        length = int(rng.integers(max(1, n - 5), n + 6))
        if n < length:                                             # n bases stay
            gone = sorted(int(p) for p in rng.choice(length, length - n, replace=False))
            variants = [(p, "", 2) for p in gone]
        elif n > length:                                           # one replacement brings the bases that are missing
            variants = [(int(rng.integers(0, length)), letters_of(rng, n - length + 1), 2)]
        else:
            variants = []
        seqs = [("s%d" % n, random_codes(rng, length))]
        text = check_text(trial_lib, seqs, {0: variants}, 2, rng, n_random=4)
        lines = text.split(b"\n")
        assert lines[0] == b">s%d_allele0" % n and sum(len(l) for l in text.split(b">s%d_allele1\n" % n)[1].split(b"\n")) == n


def test_dense_random_maps(trial_lib):
    rng = np.random.default_rng(2)
    for trial in range(40):
        num_alleles = int(rng.integers(1, 5))
        seqs = [("chr%d" % s, random_codes(rng, int(rng.integers(1, 700)))) for s in range(int(rng.integers(1, 4)))]
        variants = {s: dense_variants(rng, len(c), num_alleles) for s, (_, c) in enumerate(seqs)}
        check_text(trial_lib, seqs, variants, num_alleles, rng)


def test_events_at_line_ends_and_sequence_ends(trial_lib):
    rng = np.random.default_rng(3)
    codes = random_codes(rng, 211)
    for variants in ([(68, "ACGTA", 1)],                          # inserted bases on both sides of a line end
                     [(69, "TT", 1)], [(69, "TTT", 3)], [(70, "GG", 1)],
                     [(0, "", 1)], [(210, "", 1)], [(0, "", 1), (210, "", 2)],       # the first and the last base deleted
                     [(210, "ACGTACGT", 1)],                      # an insertion at the last base
                     [(0, "CCCC", 1), (1, "", 1), (209, "", 1), (210, "GA", 1)],
                     [(p, "", 1) for p in range(60, 80)],          # a line end inside a run of deletions
                     [(10, letters_of(rng, 200), 2)]):             # one insertion of several lines
        seqs = [("chrA", codes), ("b", random_codes(rng, 5))]
        text = check_text(trial_lib, seqs, {0: variants}, 2, rng)
        assert all(len(l) <= LINE for l in text.split(b"\n"))


def test_a_substitution_only_set(trial_lib):
    """allele copies of the packed reference (DevSim::hap_stride), and the same set over the maps: the same text, the alleles as long as the sequences"""
    rng = np.random.default_rng(4)
    seqs = [("chr1", random_codes(rng, 1000)), ("chr2", random_codes(rng, 64)), ("chr3", random_codes(rng, 333))]
    variants = {s: [(p, letters_of(rng, 1), int(rng.integers(1, 4))) for p in range(len(c)) if rng.random() < 0.1 or p in (0, 31, 32, len(c) - 1)] for s, (_, c) in enumerate(seqs)}
    copies = check_text(trial_lib, seqs, variants, 2, rng, copies=True)
    assert copies == check_text(trial_lib, seqs, variants, 2, rng, copies=False)
    assert [len(r.split(b"\n", 1)[1].replace(b"\n", b"")) for r in copies.split(b">")[1:]] == [1000, 1000, 64, 64, 333, 333]


@pytest.mark.parametrize("size", [1, 15, 16, 17, 4097])
def test_the_text_does_not_depend_on_how_it_is_cut(trial_lib, size):
    """a three-sequence, two-allele reference whose text spans several tiles, whole, in pieces of one size: the pieces begin at every offset modulo 16 of the text
    (the cuts are shifted by a first piece of 0 .. 15 bytes for that) and their destinations take every alignment in turn"""
    rng = np.random.default_rng(5)
    seqs = [("chrA", random_codes(rng, 9000)), ("NC_000913.3_1-500", random_codes(rng, 80)), ("s", random_codes(rng, 3210))]
    variants = {s: dense_variants(rng, len(c), 2, every=18, longest=7) for s, (_, c) in enumerate(seqs)}
    want = fasta_text([n.encode() for n, _ in seqs], all_letters(seqs, variants, 2), 2)
    assert len(want) > 16384 + 4097
    starts = set()
    for first in ([0] if size == 1 else range(16)):
        cuts = sorted({0, len(want)} | set(range(first, len(want), size)))
        pieces = [(a, b - a, (5 * i + first) % 16) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
        got, total = run_trial(trial_lib, seqs, variants, 2, pieces)
        assert total == len(want) and b"".join(got) == want, first
        starts |= {a % 16 for a, _, _ in pieces}
    assert starts == set(range(16))
    # a piece that reaches beyond the text is refused
    assert run_trial(trial_lib, seqs, variants, 2, [(len(want) - 3, 4, 0)])[0] is None
    assert run_trial(trial_lib, seqs, variants, 2, [(len(want), 0, 0)])[0] == [b""]


def test_an_allele_in_the_second_word_of_the_bits(trial_lib):
    rng = np.random.default_rng(6)
    seqs = [("chrA", random_codes(rng, 150))]
    variants = {0: [(5, "", 1 << 65), (40, "ACGT", (1 << 65) | (1 << 3)), (69, "", 1 << 64), (100, "T", 1 << 69)]}
    text = check_text(trial_lib, seqs, variants, 70, rng)
    records = text.split(b">")[1:]
    assert len(records) == 70 and records[65].startswith(b"chrA_allele65\n")
    lengths = [len(r.split(b"\n", 1)[1].replace(b"\n", b"")) for r in records]
    assert lengths[65] == 152 and lengths[64] == 149 and lengths[3] == 153 and lengths[69] == 150 and lengths[0] == 150


# ------------------------------------------------------------------------------------------------ the host calls
def reference_letters(ref):
    """(names, {(sequence, allele): letters}, number of alleles) of an api.Reference with variants, from its own variant list and codes"""
    num_alleles = api.lib().rsq_ref_num_alleles
    n = C.c_uint32()
    num_alleles(ref.h, C.byref(n))
    names = [ref.sequence_name(s).encode() for s in range(ref.num_sequences())]
    seqs = [(names[s].decode(), ref.codes(s)) for s in range(len(names))]
    return names, all_letters(seqs, {s: ref.variants(s) for s in range(len(names))}, n.value), n.value


def check_host_calls(ref):
    names, letters, na = reference_letters(ref)
    text = fasta_text(names, letters, na)
    for (s, a), l in letters.items():
        assert ref.allele_length(s, a) == len(l)
    assert ref.alleles_fasta_size() == len(text)
    fai = ref.alleles_fai()
    assert fai == fai_text(names, letters, na)
    for line in fai.splitlines():                                  # the index finds every allele's bases in the text
        name, length, offset, bases, width = line.split(b"\t")
        s, a = names.index(name.rsplit(b"_allele", 1)[0]), int(name.rsplit(b"_allele", 1)[1])
        assert (int(bases), int(width)) == (70, 71) and text[int(offset) - len(name) - 2:int(offset)] == b">" + name + b"\n"
        assert text[int(offset):int(offset) + int(length) + (int(length) + 69) // 70].replace(b"\n", b"") == letters[s, a]
    listed = [(name + b"_allele%d" % a, len(letters[s, a])) for s, name in enumerate(names) for a in range(na)]
    sam = ref.sam_header_alleles()
    assert sam == b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % e for e in listed) + b"@PG\tID:reseq_amd\tPN:reseq_amd\n"
    bam = ref.bam_header_alleles()
    header_text, refs, end = decode_bam_header(bam)
    assert header_text == sam and refs == listed and end == len(bam)
    return text, letters


def test_host_calls_on_the_golden_variant_file(workdir):
    """tests/golden/test-var.vcf (substitutions, insertions, deletions on two alleles, the first at the contig's first base) over a stand-in for its contig that
    carries the file's REF alleles, as tests/test_truth_md_gpu.py reads it"""
    g = json.load(open(os.path.join(GOLDEN, "reference_known_answers.json")))["variation_loading"]
    codes = np.random.default_rng(5).integers(0, 4, 12000).astype(np.uint8)
    for pos, bases in g["ref_alleles"]:
        if pos + len(bases) <= len(codes):
            codes[pos:pos + len(bases)] = ["ACGT".index(b) for b in bases]
    vcf = workdir / "alleles_golden.vcf"
    with open(os.path.join(GOLDEN, "test-var.vcf")) as f, open(vcf, "w") as out:
        for line in f:
            if line.startswith("#") or int(line.split("\t")[1]) <= len(codes):
                out.write(line)
    fa = workdir / "alleles_golden.fa"
    synth.write_fasta(fa, [(g["contig"] + " stand-in", codes)])
    ref = api.Reference(str(fa), 0)
    try:
        assert ref.read_variants(str(vcf)) == 2
        text, letters = check_host_calls(ref)
        assert len(letters[0, 0]) != len(codes) or len(letters[0, 1]) != len(codes)
        assert text.startswith(b">NC_000913.3_allele0\n")
    finally:
        ref.close()


def test_host_calls_on_the_reference_test_fasta(workdir):
    """tests/golden/reference-test.fa with the variants of the reference's own template test (a deletion, two insertions, a substitution on two alleles)"""
    from test_abi import write_known_answer_vcf
    ka = json.load(open(os.path.join(GOLDEN, "reference_known_answers.json")))["reference_sequence_with_variants"]
    vcf = workdir / "alleles_known_answers.vcf"
    write_known_answer_vcf(vcf, ka)
    ref = api.Reference(os.path.join(GOLDEN, "reference-test.fa"))
    try:
        assert ref.read_variants(vcf) == 2
        text, letters = check_host_calls(ref)
        assert len(letters[1, 0]) == len(letters[1, 1]) == 501 and text.count(b">") == 4
        # the size calls' contract: the bytes needed are reported, a short buffer is left alone
        need = C.c_size_t()
        short = C.create_string_buffer(b"\xee" * 8, 8)
        assert api.lib().rsq_ref_alleles_fai(ref.h, short, 8, C.byref(need)) == api.RSQ_ENOSPC and need.value == len(ref.alleles_fai()) and short.raw == b"\xee" * 8
        with pytest.raises(api.RsqError):
            ref.allele_length(0, 2)
        with pytest.raises(api.RsqError):
            ref.allele_length(2, 0)
    finally:
        ref.close()


def test_host_calls_on_synthetic_sets(workdir):
    import parity_cases as P
    rng = np.random.default_rng(8)
    seqs = [("chrA some text", random_codes(rng, 5000)), ("tiny", random_codes(rng, 80)), ("third", random_codes(rng, 3210))]
    for kind, samples in (("mixed", 1), ("subs", 1), ("mixed", 3)):
        vs = P._mixed_variant_set(seqs, rng, 18, [0, 3, 999, 1000, 1001], ends=40) if kind == "mixed" else P._substitution_set(seqs, rng, 25, [0, 999, 1000])
        if samples > 1:
            vs = [(si, p0, rl, alt, "\t".join(["0|1", "1|0", "1|1", "0|0"][int(rng.integers(0, 4))] for _ in range(samples - 1)) + "\t" + gt) for si, p0, rl, alt, gt in vs]
        vcf, fa = workdir / f"alleles_host_{kind}{samples}.vcf", workdir / f"alleles_host_{kind}{samples}.fa"
        P.write_vcf(vcf, seqs, vs, samples=samples)
        synth.write_fasta(fa, seqs)
        ref = api.Reference(str(fa))
        try:
            assert ref.read_variants(vcf) == 2 * samples
            text, letters = check_host_calls(ref)
            assert text.count(b">") == 6 * samples and len(letters[1, 0]) == 80
            if kind == "subs":
                assert all(len(l) == len(seqs[s][1]) for (s, a), l in letters.items())
        finally:
            ref.close()


def test_host_calls_refuse_a_reference_without_variants():
    ref = api.Reference(os.path.join(GOLDEN, "reference-test.fa"))
    try:
        for call in (lambda: ref.allele_length(0, 0), ref.alleles_fasta_size, ref.alleles_fai, ref.sam_header_alleles, ref.bam_header_alleles):
            with pytest.raises(api.RsqError) as e:
                call()
            assert e.value.code == api.RSQ_EINVAL and "no variants" in str(e.value)
    finally:
        ref.close()


# ------------------------------------------------------------------------------------------------ truth records in allele coordinates
from test_truth_sam import D, I, M, NAMES, fragment, make_mate, parse_fastq, random_template, sam_pair, template_bases
from test_truth_variants import decode_var_bam, mirrored, random_variants, run_var_pair, stretch_start


def allele_names(names, num_alleles):
    return [n + b"_allele%d" % a for n in names for a in range(num_alleles)]


def allele_sam_pair(frag, xi, allele, allele_id, num_alleles, rec1, rec2, names, phred_offset):
    """the statement: the PLAIN record of tests/test_truth_sam.py (sam_pair) of the same FASTQ records with the fragment where it lies in its allele -- start :=
    stretch_start(allele, start, XI), the sequence := the allele's record --, and the reference-coordinate record's QNAME (the id's own) and tags (XI behind XE).
    allele None: allele copies, the fragment's own start."""
    moved = None
    if frag is not None and int(frag["len"]) > 0:
        hs = int(frag["start"]) if allele is None else stretch_start(allele, int(frag["start"]), xi)
        moved = dict(seq=int(frag["seq"]) * num_alleles + allele_id, start=hs, len=int(frag["len"]), strand=int(frag["strand"]))
    text = sam_pair(moved, rec1, rec2, allele_names(names, num_alleles), phred_offset)
    return b"".join(line + b"\tXI:i:%d\n" % xi for line in text.splitlines())


def allele_sam_text(frags, xis, alleles, num_alleles, fastq1, fastq2, names, phred_offset):
    """the text of a call; alleles: {(sequence, allele): build_allele(...)} or None (allele copies); frags None: adapter-only pairs"""
    r1, r2 = parse_fastq(fastq1), parse_fastq(fastq2)
    assert len(r1) == len(r2) and (frags is None or len(frags) == len(r1))
    out = []
    for i in range(len(r1)):
        f = None if frags is None else frags[i]
        allele = None if f is None or alleles is None else alleles[int(f["seq"]), int(f["allele"])]
        out.append(allele_sam_pair(f, 0 if f is None else int(xis[i]), allele, 0 if f is None else int(f["allele"]), num_alleles, r1[i], r2[i], names, phred_offset))
    return b"".join(out)


@pytest.fixture(scope="module")
def record_lib(tmp_path_factory):
    from test_truth_variants import VarIn
    L = build_trial(tmp_path_factory, "truth_allele_trial")
    L.truth_var_trial.argtypes = [C.POINTER(VarIn), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def check_allele_pair(L, mates, frag, variants, seq_len, xi=0, phred_offset=33, allele_id=1, num_alleles=2, has_fv=True, **kw):
    """both formats against the statement; returns the SAM lines' fields"""
    allele = build_allele(seq_len, variants) if has_fv else None
    f1, f2, sam, placed = run_var_pair(L, False, mates, frag, phred_offset, variants, seq_len, xi, allele_id=allele_id, num_alleles=num_alleles, has_fv=has_fv, **kw)
    want = allele_sam_pair(frag, xi, allele, allele_id, num_alleles, parse_fastq(f1)[0], parse_fastq(f2)[0], NAMES, phred_offset)
    assert sam == want, (sam, want)
    g1, g2, bam, placed_bam = run_var_pair(L, True, mates, frag, phred_offset, variants, seq_len, xi, allele_id=allele_id, num_alleles=num_alleles, has_fv=has_fv, at=3, **kw)
    assert (g1, g2) == (f1, f2) and (placed_bam == placed).all()
    got, records = decode_var_bam(bam, allele_names(NAMES, num_alleles))
    assert got == want, (got, want)
    if frag is not None and frag["len"]:
        hs = stretch_start(allele, frag["start"], xi) if has_fv else frag["start"]
        assert [int(x) for x in placed[0][:3]] == [hs, hs + frag["len"], 0], placed        # one placement per pair; no columns walked
        assert all(r["ref_id"] == frag["seq"] * num_alleles + allele_id for r in records)
    return [line.split(b"\t") for line in sam.splitlines()]


@pytest.mark.parametrize("phred_offset", [33, 64])
def test_allele_records_of_every_read_length(record_lib, phred_offset):
    """read lengths 1 .. 151 with random ops as forward and reverse mates on either strand over dense alleles; fragments start at plain bases, at replaced ones
    and inside inserted bases, and end likewise"""
    rng = np.random.default_rng(5000 + phred_offset)
    inside = 0
    for read_len in range(1, 152):
        for strand in (0, 1):
            seq_len = 900
            variants = random_variants(rng, seq_len, int(rng.choice([3, 6, 18])))
            allele = build_allele(seq_len, variants)
            p_indel = (0.0, 0.12)[(read_len + strand) & 1]
            mates = []
            for seg in (0, 1):
                n_adapter = int(rng.integers(0, read_len)) if rng.random() < 0.4 else 0
                mates.append(make_mate(rng, random_template(rng, read_len - n_adapter, p_indel), [M] * n_adapter, 0, phred_offset, with_n=read_len % 3 == 0))
            length = max(template_bases(m["ops"][:m["n_iter_m"]]) for m in mates) + int(rng.integers(0, 30))
            hs = int(rng.integers(0, len(allele) - length - 40))
            while allele[hs + length - 1][1] == allele[hs][1]:                       # (a fragment is no part of one replacement)
                length += 1
            _, start, xi = allele[hs]
            inside += xi > 0
            fields = check_allele_pair(record_lib, mates, fragment(int(rng.integers(0, 3)), start, length, strand), variants, seq_len, xi, phred_offset)
            assert all(f[2].endswith(b"_allele1") and f[-1] == b"XI:i:%d" % xi for f in fields)
    assert inside > 10


def allele_orientations(L, ops, variants, seq_len, start, xi=0, flen=None):
    """a fragment that is exactly the template part of `ops`, on either strand (as both_orientations of tests/test_truth_variants.py): (POS, CIGAR) of its four
    records, which must agree"""
    rng = np.random.default_rng(len(ops) * 131 + start)
    seen = set()
    for strand in (0, 1):
        fwd, rev = mirrored(rng, ops)
        frag = fragment(1, start, template_bases(ops) if flen is None else flen, strand)
        fields = check_allele_pair(L, [fwd, rev] if strand == 0 else [rev, fwd], frag, variants, seq_len, xi)
        seen |= {(int(f[3]), f[5]) for f in fields}
    assert len(seen) == 1, seen
    return seen.pop()


def test_allele_records_around_insertions_and_deletions(record_lib):
    L = record_lib
    # no element comes from a variant; POS counts the allele's bases in front: 100 reference bases, plus or minus what the variants in front did
    assert allele_orientations(L, [M] * 12, {105: 3}, 300, 100) == (101, b"12M")
    assert allele_orientations(L, [M] * 12, {50: 3, 105: 0}, 300, 100) == (103, b"12M")
    assert allele_orientations(L, [M] * 12, {50: 0, 51: 0, 104: 0, 105: 4, 106: 0}, 300, 100) == (99, b"12M")
    # a fragment that starts inside an insertion (the replacement at 100 has 5 bases, XI of them in front) ...
    assert allele_orientations(L, [M] * 10, {100: 5}, 300, 100, xi=1) == (102, b"10M")
    assert allele_orientations(L, [M] * 10, {100: 5}, 300, 100, xi=4) == (105, b"10M")
    assert allele_orientations(L, [M] * 10, {100: 5}, 300, 100, xi=0) == (101, b"10M")
    # ... and one that ends inside it, or with the base standing at its position
    assert allele_orientations(L, [M] * 10, {107: 6}, 300, 100) == (101, b"10M")
    assert allele_orientations(L, [M] * 8, {107: 6}, 300, 100) == (101, b"8M")
    # deletions directly in front of the stretch, directly behind it, and at the sequence's ends
    assert allele_orientations(L, [M] * 12, {99: 0}, 300, 100) == (100, b"12M")
    assert allele_orientations(L, [M] * 12, {112: 0, 113: 0}, 300, 100) == (101, b"12M")
    assert allele_orientations(L, [M] * 6, {0: 0}, 50, 1) == (1, b"6M")
    assert allele_orientations(L, [M] * 4, {49: 0}, 50, 45) == (46, b"4M")
    assert allele_orientations(L, [M] * 6, {49: 3}, 50, 46) == (47, b"6M")
    # the read's own indels stay, D at the ends is dropped and moves POS
    assert allele_orientations(L, [M, M, D, M, I, M], {103: 0, 101: 3}, 300, 100) == (101, b"2M1D1M1I1M")
    assert allele_orientations(L, [D, M, M, M], {101: 0, 102: 0}, 300, 100) == (102, b"3M")


def test_a_mate_wholly_inside_an_insertion_in_allele_coordinates(record_lib):
    """in reference coordinates such a mate is nI and a clip; in its allele it is an alignment like any other"""
    rng = np.random.default_rng(77)
    variants = {150: 20}
    for strand in (0, 1):
        inside, other = make_mate(rng, [M, M, I, M, D, M, M], [M, M], 0, 33), make_mate(rng, [M] * 30, [], 0, 33)
        for forward in (True, False):
            frag = fragment(0, 150, 60, strand) if forward else fragment(0, 100, 50 + 12, strand)
            seg = strand if forward else 1 - strand
            mates = [other, other]
            mates[seg] = inside
            fields = check_allele_pair(record_lib, mates, frag, variants, 400, xi=3 if forward else 0)
            assert (fields[seg][3], fields[seg][5]) == ((b"154", b"2M1I1M1D2M2S") if forward else (b"157", b"2S2M1D1M1I2M"))


def test_allele_records_of_allele_copies_and_unmapped_pairs(record_lib):
    rng = np.random.default_rng(32)
    for strand in (0, 1):
        mates = [make_mate(rng, random_template(rng, 30, 0.1), [M, M], 1, 64), make_mate(rng, [D, D, M, M, M, D], [], 0, 64)]
        fields = check_allele_pair(record_lib, mates, fragment(2, 1000, 80, strand), {}, 5000, phred_offset=64, has_fv=False, allele_id=0)
        assert fields[0][2] == b"s_allele0" and fields[0][0].startswith(b"ReseqRead_3_17_allele0:")
    # one allele: the id names none, the sequence still does
    fields = check_allele_pair(record_lib, mates, fragment(0, 1000, 80, 0), {}, 5000, phred_offset=64, has_fv=False, allele_id=0, num_alleles=1)
    assert fields[0][0].startswith(b"ReseqRead_3_17:") and fields[0][2] == b"chrA_allele0"
    mates = [make_mate(rng, [], [M] * 9, 2, 33), make_mate(rng, [], [M] * 12, 0, 33)]
    fields = check_allele_pair(record_lib, mates, None, {5: 3}, 100, adapter_only_number=77)
    assert [f[1] for f in fields] == [b"77", b"141"] and fields[1][2] == b"*" and fields[1][-1] == b"XI:i:0"
