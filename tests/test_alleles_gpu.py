"""The alleles of a reference with variants as FASTA text on the device (rsq_sim_alleles_fasta, Simulator.alleles_fasta; `reseq illuminaPE -V ... --writeAlleles`):
the text against tests/test_alleles.py's text of the alleles spelled out base by base (VarCase.letters), whole and in pieces at odd offsets, sizes and
alignments; and -- tying the text to the simulation without the Python allele -- every aligned read base of a run without substitution errors against the
device-made text at the place the read's own id and tags name."""
import os
import subprocess

import numpy as np
import pytest

from reseq_amd import api, synth
from test_alleles import fai_text, fasta_text
from test_truth_sam import parse_fastq, template_part
from test_truth_sam_gpu import MARKER, inflate_members
from test_truth_variants import stretch_start
from test_truth_variants_gpu import VarCase

pytestmark = pytest.mark.gpu


def case_text(c):
    return fasta_text(c.names, c.letters, 2)


@pytest.fixture(scope="module")
def var(workdir):
    c = VarCase(workdir, "alleles", 7, 31)
    yield c
    c.close()


def test_the_text_of_a_mixed_set(var):
    want = case_text(var)
    assert var.ref.alleles_fasta_size() == len(want)
    assert var.sim.alleles_fasta() == want
    assert var.sim.last_kernel_launches("alleles_fasta") == 1 and var.sim.last_kernel_ms("alleles_fasta") > 0
    lengths = {key: len(l) for key, l in var.letters.items()}
    assert lengths[1, 0] == lengths[1, 1] == 80 and lengths[0, 0] != 5000 and lengths[0, 1] != 5000 and lengths[0, 0] != lengths[0, 1]
    # no other call launches the kernel, and the call leaves the simulation alone
    before = var.sim.pairs(1, 3)
    assert var.sim.last_kernel_launches("alleles_fasta") == 0
    var.sim.alleles_fasta(5, 77)
    after = var.sim.pairs(1, 3)
    assert before[1:] == after[1:] and before[0].tobytes() == after[0].tobytes()


def test_pieces_at_odd_offsets_sizes_and_alignments(var):
    """the same text fetched in pieces: cuts at odd offsets and sizes (one byte, sizes around 16 and around the kernel's 64-byte runs, several tiles), into a
    destination 1 .. 15 bytes off a 16-byte boundary; the bytes around a piece are left alone, and every call is one launch"""
    want = case_text(var)
    dev, room = var.sim.device, len(want) + 64
    marker = np.full(room, MARKER, np.uint8)
    dst = api.DeviceArray.from_numpy(dev, marker)
    try:
        def piece(at, size, shift):
            api._check(api.lib().rsq_dev_upload(dev, dst.ptr, marker.ctypes.data, room))
            assert var.sim.alleles_fasta_device(at, size, dst.ptr.value + shift) == api.RSQ_OK
            assert var.sim.last_kernel_launches("alleles_fasta") == 1
            got = dst.to_numpy(np.uint8, room)
            assert got[shift:shift + size].tobytes() == want[at:at + size], (at, size, shift)
            assert np.all(got[:shift] == MARKER) and np.all(got[shift + size:] == MARKER), (at, size, shift)
        sizes = [1, 15, 16, 17, 63, 64, 65, 127, 300, 4097]
        at, shifts = 0, set()
        for i in range(1000):
            size, shift = min(sizes[i % len(sizes)], len(want) - at), i % 15 + 1
            piece(at, size, shift)
            shifts.add(shift)
            at += size
            if at == len(want):
                break
        assert at == len(want) and shifts == set(range(1, 16))
        assert len(want) > 16384 + 16                                # more than one tile of the kernel
        piece(0, len(want), 5)
        piece(3, 16385, 13)
        piece(len(want) - 16400, 16400, 0)
    finally:
        dst.free()


def test_the_end_of_the_text_and_what_lies_behind_it(var):
    want = case_text(var)
    assert var.sim.alleles_fasta(len(want) - 5) == want[-5:] and var.sim.alleles_fasta(len(want), 0) == b""
    dst = api.DeviceArray(var.sim.device, 64)
    try:
        for at, size in ((len(want) - 3, 4), (len(want) + 1, 0), (0, len(want) + 1)):
            assert var.sim.alleles_fasta_device(at, size, dst) == api.RSQ_EINVAL and "the text has" in api.lib().rsq_last_error().decode()
    finally:
        dst.free()


def test_variants_that_crowd_the_ends_of_the_sequences(workdir):
    c = VarCase(workdir, "alleles_ends", 11, 43, ends=40)
    try:
        assert c.sim.alleles_fasta() == case_text(c)
        assert c.ref.alleles_fai() == fai_text(c.names, c.letters, 2)
    finally:
        c.close()


def test_a_substitution_only_set(workdir):
    """allele copies of the packed reference, no coordinate maps to walk"""
    c = VarCase(workdir, "alleles_subs", 7, 17, kind="subs")
    try:
        want = case_text(c)
        assert c.sim.alleles_fasta() == want and [len(c.letters[s, a]) for s in range(3) for a in range(2)] == [5000, 5000, 80, 80, 3210, 3210]
        assert c.letters[0, 0] != c.letters[0, 1]
        assert c.sim.alleles_fasta(4999, 300) == want[4999:5299]
    finally:
        c.close()


def test_methylation_beside_the_variants(workdir):
    """bisulfite conversion changes the reads, not the alleles; a substitution-only set then simulates over the maps and still writes its copies"""
    for kind in ("mixed", "subs"):
        c = VarCase(workdir, "alleles_meth_" + kind, 7, 61, kind=kind, methylation=True)
        try:
            assert c.sim.alleles_fasta() == case_text(c)
        finally:
            c.close()


def test_128_alleles(workdir):
    """samples=64: alleles in both words of the variants' allele bits, two and three digits in the names"""
    import parity_cases as P
    seqs = P.make_inputs(workdir, "alleles_128", synth.TINY, [3100])[2]
    rng = np.random.default_rng(5)
    vs = P._mixed_variant_set(seqs, rng, 18, [0, 3, 999, 1000, 1001])
    vs = [(si, p0, rl, alt, "\t".join(["0|1", "1|0", "1|1", "0|0"][int(rng.integers(0, 4))] for _ in range(63)) + "\t" + gt) for si, p0, rl, alt, gt in vs]
    vcf = workdir / "alleles_128.vcf"
    P.write_vcf(vcf, seqs, vs, samples=64)
    ppath, fpath, _ = P.make_inputs(workdir, "alleles_128", synth.TINY, [3100])
    prof, ref = api.Profile(ppath), api.Reference(fpath, 0)
    try:
        assert ref.read_variants(vcf) == 128
        sim = api.Simulator(prof, ref, 0)
        try:
            from test_alleles import reference_letters
            names, letters, na = reference_letters(ref)
            want = fasta_text(names, letters, na)
            assert na == 128 and len({letters[0, a] for a in range(128)}) > 100
            assert sim.alleles_fasta() == want                         # (valid after rsq_sim_create: nothing of the pre-pass is needed)
            assert sim.alleles_fasta(70000, 4097) == want[70000:74097]
        finally:
            sim.close()
    finally:
        ref.close()
        prof.close()


def test_a_reference_without_variants_is_refused(workdir):
    from test_truth_sam_gpu import tiny_case
    c = tiny_case(workdir)
    dst = api.DeviceArray(c.sim.device, 64)
    try:
        assert c.sim.alleles_fasta_device(0, 1, dst) == api.RSQ_EINVAL and "variants" in api.lib().rsq_last_error().decode()
    finally:
        dst.free()
        c.close()


def test_every_aligned_base_is_the_device_made_texts(workdir):
    """without substitution errors: every read base over an M op of the template part is the base of the DEVICE-MADE FASTA text at the allele coordinate the
    record names -- the record's allele from its QNAME, the fragment's first base from its start position and XI tag through the text's own .fai arithmetic
    (offset + h + h // 70).  Only where (start position, XI) lies in the allele comes from the variant list; no base of the Python allele is consulted."""
    c = VarCase(workdir, "alleles_nosub", 7, 31, no_substitutions=True)
    try:
        text = c.sim.alleles_fasta()
        offsets = {}
        for line in c.ref.alleles_fai().splitlines():
            name, length, offset = line.split(b"\t")[:3]
            offsets[name] = (int(offset), int(length))
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        xis, lines = c.xis(sam), sam.splitlines()
        checked = 0
        for i, f in enumerate(frags):
            offset, length = offsets[c.names[int(f["seq"])] + b"_allele%d" % int(f["allele"])]
            hs = stretch_start(c.alleles[int(f["seq"]), int(f["allele"])], int(f["start"]), xis[i])
            assert hs + int(f["len"]) <= length
            for seg in (0, 1):
                fields = lines[2 * i + seg].split(b"\t")
                ops = [op for n, op in template_part(fields[11][5:]) for _ in range(n)]
                q, t = sum(op != b"D" for op in ops), sum(op != b"I" for op in ops)
                reverse = seg != int(f["strand"])
                seq = fields[9]
                read = seq[len(seq) - q:] if reverse else seq[:q]
                at, r = (hs + int(f["len"]) - t if reverse else hs), 0
                for op in (ops[::-1] if reverse else ops):
                    if op == b"M":
                        assert read[r] == text[offset + at + at // 70], (f, seg, at)
                    r += op != b"D"
                    at += op != b"I"
                checked += 1
        assert checked >= 4000
    finally:
        c.close()


def test_command_line(workdir):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    c = VarCase(workdir, "alleles_cli", 7, 31, replace_n_seed=7, base_identifier="ReseqRead")
    try:
        want, fai = c.sim.alleles_fasta(), c.ref.alleles_fai()
        assert want == case_text(c)
        fpath, ppath, vcf = c.fpath, c.ppath, c.vcf
    finally:
        c.close()
    out = {k: str(workdir / f"alleles_cli_{k}") for k in ("1", "2", "g1", "g2", "w1", "w2", "x1", "x2")}
    fa, gz, fa2 = str(workdir / "alleles_cli.fa"), str(workdir / "alleles_cli.fa.gz"), str(workdir / "alleles_cli_two.fa")
    common = [exe, "illuminaPE", "-R", fpath, "-s", ppath, "--numReads", "3000", "--seed", "7"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True)
    read = lambda path: open(path, "rb").read()
    r = run(["-V", vcf, "-1", out["1"], "-2", out["2"], "--writeAlleles", fa])
    assert r.returncode == 0, r.stderr
    assert read(fa) == want and read(fa + ".fai") == fai
    r = run(["-V", vcf, "-1", out["g1"], "-2", out["g2"], "--writeAlleles", gz])
    assert r.returncode == 0, r.stderr
    packed = read(gz)
    assert packed[3] == 4 and packed.endswith(api.gzip_eof_member()) and inflate_members(packed) == want and not os.path.exists(gz + ".fai")
    assert read(out["g1"]) == read(out["1"]) and read(out["g2"]) == read(out["2"])
    # two workers: the first one's simulator writes the alleles; the FASTQ files are one worker's
    r = run(["-V", vcf, "-1", out["w1"], "-2", out["w2"], "--writeAlleles", fa2, "--gpus", "2"])
    assert r.returncode == 0, r.stderr
    assert read(fa2) == want and read(fa2 + ".fai") == fai and read(out["w1"]) == read(out["1"]) and read(out["w2"]) == read(out["2"])
    # without a variant file there are no alleles: nothing is simulated, no file is left
    for extra, message in ((["--writeAlleles", fa + ".x"], "-V"), (["-V", vcf, "--writeAlleles", fa + ".x.bz2"], "bzip2")):
        r = run(["-1", out["x1"], "-2", out["x2"]] + extra)
        assert r.returncode != 0 and message in r.stderr, r.stderr
        assert not any(os.path.exists(p) for p in (out["x1"], out["x2"], fa + ".x", fa + ".x.bz2", fa + ".x.fai"))


# ------------------------------------------------------------------------------------------------ truth records in allele coordinates
import re
import types

from test_alleles import allele_names, allele_sam_text
from test_truth_bam import decode_bam_header
from test_truth_sam import clean
from test_truth_sam_gpu import check_against_the_reference
from test_truth_variants import decode_var_bam


class AlleleCase(VarCase):
    """a VarCase whose truth calls write allele coordinates"""

    def __init__(self, *args, **kw):
        VarCase.__init__(self, *args, **kw)
        self.sim.truth_variants(False)
        self.sim.truth_alleles(True)

    def statement(self, frags, f1, f2, sam):
        return allele_sam_text(frags, None if frags is None else self.xis(sam), self.alleles if self.maps else None, 2, f1, f2, self.names, self.phred_offset)


@pytest.fixture(scope="module")
def al(workdir):
    c = AlleleCase(workdir, "main", 7, 31)
    c.whole = c.sim.pairs_sam(1, c.tb + 1)
    c.bam = c.sim.pairs_bam(1, c.tb + 1)
    yield c
    c.close()


def test_sam_text_in_allele_coordinates(al):
    frags, f1, f2, sam = al.whole
    pf, p1, p2 = al.sim.pairs(1, al.tb + 1)
    assert 2000 < len(frags) < 4000 and set(np.unique(frags["allele"])) == {0, 1}
    assert pf.tobytes() == frags.tobytes() and p1 == f1 and p2 == f2
    assert sam == al.statement(frags, f1, f2, sam)
    assert (np.array(al.xis(sam)) > 0).sum() > 3, "fragments that start inside inserted bases"
    lines = [line.split(b"\t") for line in sam.splitlines()]
    assert {f[2].rsplit(b"_allele", 1)[1] for f in lines} == {b"0", b"1"} and b"_allele0:" in sam and b"_allele1:" in sam
    for f in lines:                                                # no CIGAR gained an op: its elements are the id's template part, cleaned
        elements = clean(template_part(f[11][5:]))[0]
        texts = [b"%d%s" % e for e in (elements[::-1] if int(f[1]) & 0x10 else elements)]
        assert re.sub(rb"\d+S", b"", f[5]) == b"".join(texts), f
    # the reference-coordinate records of the same pairs do gain ops: the case has teeth
    al.sim.truth_alleles(False)
    al.sim.truth_variants(True)
    try:
        other = al.sim.pairs_sam(1, al.tb + 1)[3]
    finally:
        al.sim.truth_variants(False)
        al.sim.truth_alleles(True)
    assert sum(a.split(b"\t")[5] != b.split(b"\t")[5] for a, b in zip(sam.splitlines(), other.splitlines())) > 100
    al.sim.pairs_sam(1, 3)
    assert al.sim.last_kernel_launches("sam_write") == 1 and al.sim.last_kernel_launches("sam_sizes") == 1


def test_every_aligned_base_is_the_alleles_in_the_device_made_text(workdir):
    """check_against_the_reference of tests/test_truth_sam_gpu.py with the DEVICE-MADE FASTA text as the reference: every M base of every record is the base of
    the record's RNAME at POS.  Neither the Python allele nor the variant list takes part: the two halves check each other."""
    c = AlleleCase(workdir, "nosub", 7, 31, no_substitutions=True)
    try:
        records = [r.split(b"\n", 1) for r in c.sim.alleles_fasta().split(b">")[1:]]
        device_made = types.SimpleNamespace(names=[name for name, _ in records],
                                            seqs=[(name, np.frombuffer(body.replace(b"\n", b"").translate(bytes.maketrans(b"ACGT", bytes(range(4)))), np.uint8)) for name, body in records])
        assert device_made.names == allele_names(c.names, 2)
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        seen, residues, n = check_against_the_reference(device_made, sam)
        assert n == 2 * len(frags) > 4000 and seen["forward"] == seen["reverse"] == len(frags) and seen["without_m"] == 0
        for name in ("leading_d", "trailing_d", "leading_i", "adapter_part"):
            assert seen[name] > 0, (name, seen)
    finally:
        c.close()


def test_bam_in_allele_coordinates(al):
    frags, f1, f2, bam = al.bam
    assert (f1, f2) == al.whole[1:3] and frags.tobytes() == al.whole[0].tobytes()
    text, records = decode_var_bam(bam, allele_names(al.names, 2))
    assert text == al.whole[3] and len(records) == 2 * len(frags)
    assert [r["ref_id"] for r in records[0::2]] == [int(f["seq"]) * 2 + int(f["allele"]) for f in frags]
    header = al.ref.bam_header_alleles()
    header_text, refs, end = decode_bam_header(header)
    fai = [line.split(b"\t") for line in al.ref.alleles_fai().splitlines()]
    assert refs == [(f[0], int(f[1])) for f in fai] and end == len(header) and header_text == al.ref.sam_header_alleles()


@pytest.mark.parametrize("cuts", ["one block per call", "three uneven calls"])
def test_batching_in_allele_coordinates(al, cuts):
    bounds = list(range(1, al.tb + 2)) if cuts == "one block per call" else [1, 2, 7, al.tb + 1]
    for whole, call in ((al.whole, al.sim.pairs_sam), (al.bam, al.sim.pairs_bam)):
        parts = [call(lo, hi) for lo, hi in zip(bounds, bounds[1:])]
        assert b"".join(p[3] for p in parts) == whole[3] and b"".join(p[1] for p in parts) == whole[1] and b"".join(p[2] for p in parts) == whole[2]


def test_enospc_in_allele_coordinates(al):
    frags, f1, f2, sam = al.whole
    dev = al.sim.device
    r1, r2 = api.DeviceArray(dev, len(f1)), api.DeviceArray(dev, len(f2))
    short = api.DeviceArray.from_numpy(dev, np.full(len(sam) - 1, MARKER, np.uint8))
    full = api.DeviceArray.from_numpy(dev, np.full(len(sam), MARKER, np.uint8))
    try:
        n, l1, l2, ls, rc = al.sim.pairs_sam_device(1, al.tb + 1, r1, r2, short)
        assert rc == api.RSQ_ENOSPC and (n, l1, l2, ls) == (len(frags), len(f1), len(f2), len(sam))
        assert np.all(short.to_numpy(np.uint8, len(sam) - 1) == MARKER)
        n, l1, l2, ls, rc = al.sim.pairs_sam_device(1, al.tb + 1, r1, r2, full)
        assert rc == api.RSQ_OK and full.to_numpy(np.uint8, ls).tobytes() == sam
    finally:
        for d in (r1, r2, short, full):
            d.free()


def test_switching_the_coordinates(al, workdir):
    """reference-coordinate and allele-coordinate calls alternate on one simulator, each with its own bytes; with the new switch off again the calls are those of
    a simulator that never saw it, bytes and launches"""
    never = VarCase(workdir, "main", 7, 31)
    try:
        want = never.sim.pairs_sam(1, never.tb + 1)
        launches = {k: never.sim.last_kernel_launches(k) for k in ("sam_sizes", "sam_write", "bam_sizes", "bam_write", "alleles_fasta")}
        want_bam = never.sim.pairs_bam(1, never.tb + 1)
        for turn in range(2):
            al.sim.truth_alleles(False)
            al.sim.truth_variants(True)
            got = al.sim.pairs_sam(1, al.tb + 1)
            assert got[3] == want[3] != al.whole[3] and got[1:3] == want[1:3] and got[0].tobytes() == want[0].tobytes()
            assert {k: al.sim.last_kernel_launches(k) for k in launches} == launches
            assert al.sim.pairs_bam(1, al.tb + 1)[3] == want_bam[3]
            al.sim.truth_variants(False)
            al.sim.truth_alleles(True)
            assert al.sim.pairs_sam(1, al.tb + 1)[3] == al.whole[3] and al.sim.pairs_bam(1, al.tb + 1)[3] == al.bam[3]
    finally:
        al.sim.truth_variants(False)
        al.sim.truth_alleles(True)
        never.close()


@pytest.mark.parametrize("option,value", [("overlap", 3), ("image_tiles", 1)])
def test_options_in_allele_coordinates(al, workdir, rsq_options, option, value):
    rsq_options(option, value)
    c = AlleleCase(workdir, "main", 7, 31)
    try:
        if option == "image_tiles":
            assert c.sim.fill_plan()["image_tiles"] == 1
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        assert frags.tobytes() == al.whole[0].tobytes() and (f1, f2) == al.whole[1:3] and sam == al.whole[3]
        if option == "overlap":
            assert c.sim.last_kernel_launches("sam_write") == 3
        assert c.sim.pairs_bam(1, c.tb + 1)[3] == al.bam[3]
        a1, a2, asam = c.sim.adapter_only_pairs_sam(0, 150)
        assert asam == c.statement(None, a1, a2, asam) and asam.count(b"\tXI:i:0\n") == 300
    finally:
        c.close()


def test_other_variant_sets_in_allele_coordinates(workdir):
    """variants that crowd the sequences' ends; a substitution-only set (allele copies: the fragment's own coordinates); methylation beside the variants"""
    for tag, seed, variants_seed, kw in (("ends", 11, 43, dict(ends=40)), ("subs", 7, 17, dict(kind="subs")), ("meth", 7, 61, dict(methylation=True))):
        c = AlleleCase(workdir, tag, seed, variants_seed, **kw)
        try:
            frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
            assert len(frags) > 2000 and sam == c.statement(frags, f1, f2, sam)
            assert decode_var_bam(c.sim.pairs_bam(1, c.tb + 1)[3], allele_names(c.names, 2))[0] == sam
            if tag == "subs":
                assert set(c.xis(sam)) == {0} and all(int(l.split(b"\t")[3]) >= 1 for l in sam.splitlines())
            if tag == "meth":
                assert (f1, f2) == c.sim.pairs(1, c.tb + 1)[1:]
        finally:
            c.close()


def test_refusals_in_allele_coordinates(al, workdir):
    error = lambda: api.lib().rsq_last_error().decode()
    # a sorted run
    assert api.lib().rsq_sim_bam_sorted_begin(al.sim.h, 100) == api.RSQ_EINVAL and "rsq_sim_truth_alleles" in error() and "sorted" in error()
    # NM / MD
    al.sim.truth_md(True)
    try:
        for call in (al.sim.pairs_sam_device, al.sim.pairs_bam_device):
            assert call(1, 2, None, None, None)[4] == api.RSQ_EINVAL and "rsq_sim_truth_md" in error()
    finally:
        al.sim.truth_md(False)
    # both switches, whichever comes second
    assert api.lib().rsq_sim_truth_variants(al.sim.h, 1) == api.RSQ_EINVAL and "rsq_sim_truth_alleles" in error()
    al.sim.truth_alleles(False)
    al.sim.truth_variants(True)
    try:
        assert api.lib().rsq_sim_truth_alleles(al.sim.h, 1) == api.RSQ_EINVAL and "rsq_sim_truth_variants" in error()
    finally:
        al.sim.truth_variants(False)
        al.sim.truth_alleles(True)
    assert al.sim.pairs_sam(1, 2)[3] == al.sim.pairs_sam(1, 3)[3][:len(al.sim.pairs_sam(1, 2)[3])]
    # no variants
    from test_truth_sam_gpu import tiny_case
    c = tiny_case(workdir)
    try:
        assert api.lib().rsq_sim_truth_alleles(c.sim.h, 1) == api.RSQ_EINVAL and "variants" in error()
        assert len(c.sim.pairs_sam(1, 2)[3]) > 0                   # the plain call serves it as ever
    finally:
        c.close()


def test_command_line_in_allele_coordinates(workdir):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    c = AlleleCase(workdir, "cli", 7, 31, replace_n_seed=7, base_identifier="ReseqRead")
    try:
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        bam = c.sim.pairs_bam(1, c.tb + 1)[3]
        a1, a2, asam = c.sim.adapter_only_pairs_sam(0, c.info.adapter_only_pairs)
        abam = c.sim.adapter_only_pairs_bam(0, c.info.adapter_only_pairs)[2]
        bam_header, sam_header, fpath, ppath, vcf = c.ref.bam_header_alleles(), c.ref.sam_header_alleles(), c.fpath, c.ppath, c.vcf
    finally:
        c.close()
    out = {k: str(workdir / f"alleles_truth_cli_{k}") for k in ("1", "2", "x1", "x2", "xsam")}
    samgz, bamfile = str(workdir / "alleles_truth_cli.sam.gz"), str(workdir / "alleles_truth_cli.bam")
    common = [exe, "illuminaPE", "-R", fpath, "-s", ppath, "--numReads", "3000", "--seed", "7"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True)
    read = lambda path: open(path, "rb").read()
    r = run(["-V", vcf, "-1", out["1"], "-2", out["2"], "--truthSam", samgz, "--truthBam", bamfile, "--truthAlleles"])
    assert r.returncode == 0, r.stderr
    assert read(out["1"]) == f1 + a1 and read(out["2"]) == f2 + a2
    assert inflate_members(read(samgz)) == sam_header + sam + asam and read(samgz).endswith(api.gzip_eof_member())
    assert inflate_members(read(bamfile)) == bam_header + bam + abam
    # the new messages; the refusal of truth outputs with -V and neither switch stands; nothing is simulated, no file is left
    for extra, message in ((["-V", vcf, "--truthAlleles"], "--truthSam"),
                           (["--truthSam", out["xsam"], "--truthAlleles"], "-V"),
                           (["-V", vcf, "--truthSam", out["xsam"], "--truthAlleles", "--truthVariants"], "one coordinate system"),
                           (["-V", vcf, "--truthSam", out["xsam"], "--truthAlleles", "--truthMD"], "--truthMD"),
                           (["-V", vcf, "--truthBam", out["xsam"], "--truthAlleles", "--truthBamSort"], "--truthBamSort"),
                           (["-V", vcf, "--truthSam", out["xsam"]], "unless --truthVariants chooses reference coordinates"),
                           (["-V", vcf, "--truthSam", out["xsam"], "--truthAlleles", "--gpus", "2"], "one worker only")):
        r = run(["-1", out["x1"], "-2", out["x2"]] + extra)
        assert r.returncode != 0 and message in r.stderr, (extra, r.stderr)
        assert not any(os.path.exists(p) for p in (out["x1"], out["x2"], out["xsam"]))
