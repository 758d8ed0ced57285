"""Truth alignments of a reference with variants on the device (rsq_sim_truth_variants; `reseq illuminaPE -V ... --truthVariants`): SAM text, BAM records, the
sorted run and its index against the statement of tests/test_truth_variants.py applied to the call's own FASTQ texts, fragments and the reference's variant
list, and -- independent of that statement -- against the alleles themselves: with a profile without substitution errors every read base over a template base is
the allele's base there, inserted bases included, which shows that the stretch is placed right."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from reseq_amd import api, synth
from test_truth_bam import decode_bam_header
from test_truth_bam_sorted import block_table, build_bai, sorted_stream
from test_truth_sam import parse_fastq, template_part
from test_truth_sam_gpu import MARKER, Case
from test_truth_variants import X, build_allele, decode_var_bam, stretch_start, var_sam_text

pytestmark = pytest.mark.gpu

LENGTHS = [5000, 80, 3210]


def split_var_records(data, names):
    """split_records of tests/test_truth_bam_sorted.py for records that carry the XI tag"""
    _, fields = decode_var_bam(data, names)
    out, at = [], 0
    for f in fields:
        size = 4 + f["block_size"]
        raw = data[at:at + size]
        cigar = np.frombuffer(raw, "<u4", f["n_cigar"], 36 + f["l_read_name"])
        span = int(sum(int(c) >> 4 for c in cigar if (int(c) & 15) in (0, 2)))
        mapped = not f["flag"] & 0x4
        out.append(dict(raw=raw, ref_id=f["ref_id"], pos=f["pos"], span=max(span, 1) if mapped else 0, bin=f["bin"], mapped=mapped))
        at += size
    assert at == len(data)
    return out


class VarCase(Case):
    """a Case with a variant file and the opt-in set; alleles: {(sequence, allele): the allele base by base}, letters: the same bases as letters"""

    def __init__(self, workdir, tag, seed, variants_seed, kind="mixed", ends=0, methylation=False, **kw):
        import parity_cases as P
        seqs = P.make_inputs(workdir, "tiny_e2e", synth.TINY, LENGTHS)[2]
        rng = np.random.default_rng(variants_seed)
        vs = P._mixed_variant_set(seqs, rng, 18, [0, 3, 999, 1000, 1001], ends=ends) if kind == "mixed" else P._substitution_set(seqs, rng, 25, [0, 999, 1000])
        vcf = workdir / ("truth_variants_%s.vcf" % tag)
        P.write_vcf(vcf, seqs, vs)
        self.vcf = str(vcf)
        Case.__init__(self, workdir, "tiny_e2e", synth.TINY, LENGTHS, seed, 3000, vcf=self.vcf, **kw)
        if methylation:
            names = [n.split(" ")[0] for n, _ in seqs]
            bed = workdir / ("truth_variants_%s.bed" % tag)
            bed.write_text(f"{names[0]}\t0\t400\t0.0\t0.5\n{names[0]}\t900\t4500\t0.25\t0.75\n{names[2]}\t100\t3000\t0.3\n")
            self.sim.read_methylation(bed)
        self.sim.truth_variants(True)
        self.maps = kind == "mixed"
        self.alleles, self.letters = {}, {}
        for s, (_, codes) in enumerate(self.seqs):
            listed = self.ref.variants(s)
            for a in (0, 1):
                mine = {pos: bases for pos, bases, bits in listed if bits >> a & 1}
                assert len(mine) == sum(1 for pos, bases, bits in listed if bits >> a & 1), "one variant per position and allele"
                self.alleles[s, a] = build_allele(len(codes), {pos: len(bases) for pos, bases in mine.items()})
                self.letters[s, a] = b"".join((mine[p][k] if p in mine else "ACGT"[codes[p]]).encode() for _, p, k in self.alleles[s, a])

    def xis(self, sam):
        """the XI tag of every pair's first record; both mates carry the same"""
        tags = [int(line.rsplit(b"\tXI:i:", 1)[1]) for line in sam.splitlines()]
        assert tags[0::2] == tags[1::2]
        return tags[0::2]

    def statement(self, frags, f1, f2, sam):
        return var_sam_text(frags, self.xis(sam), self.alleles if self.maps else None, f1, f2, self.names, self.phred_offset)


@pytest.fixture(scope="module")
def var(workdir):
    c = VarCase(workdir, "main", 7, 31)
    c.whole = c.sim.pairs_sam(1, c.tb + 1)
    c.bam = c.sim.pairs_bam(1, c.tb + 1)
    yield c
    c.close()


def test_sam_text_equals_the_statement_and_the_plain_call(var):
    frags, f1, f2, sam = var.whole
    pf, p1, p2 = var.sim.pairs(1, var.tb + 1)
    assert 2000 < len(frags) < 4000 and set(np.unique(frags["allele"])) == {0, 1}
    assert pf.tobytes() == frags.tobytes() and p1 == f1 and p2 == f2
    assert sam == var.statement(frags, f1, f2, sam)
    xis = np.array(var.xis(sam))
    assert (xis > 0).sum() > 3, "fragments that start inside inserted bases"
    assert b"_allele0:" in sam and b"_allele1:" in sam
    cigars = [line.split(b"\t")[5] for line in sam.splitlines()]
    assert sum(b"D" in c for c in cigars) > 100 and sum(b"I" in c for c in cigars) > 100
    var.sim.pairs_sam(1, 3)
    assert var.sim.last_kernel_launches("sam_write") == 1 and var.sim.last_kernel_launches("sam_sizes") == 1


def test_the_fragments_end_where_the_ids_say(var):
    """the stretch [hs, hs + len) of the allele spelled out ends at the base in front of the id's end position: the reverse mate's stretch, which the device
    places from that end, ends at hs + len"""
    frags, f1, f2, sam = var.whole
    xis = var.xis(sam)
    for f, xi, rec in zip(frags, xis, parse_fastq(f1)):
        allele = var.alleles[int(f["seq"]), int(f["allele"])]
        hs = stretch_start(allele, int(f["start"]), xi)
        fields = rec[0].split(b" ")[0].split(b":")
        end = int(fields[1] if f["strand"] else fields[3])
        assert allele[hs + int(f["len"]) - 1][1] + 1 == end, (f, xi)


def test_bam_records_decode_to_the_sam_lines(var):
    frags, f1, f2, bam = var.bam
    assert (f1, f2) == var.whole[1:3] and frags.tobytes() == var.whole[0].tobytes()
    text, records = decode_var_bam(bam, var.names)
    assert text == var.whole[3] and len(records) == 2 * len(frags)


@pytest.mark.parametrize("cuts", ["one call", "three uneven calls"])
def test_sorted_run(var, cuts):
    from test_truth_bam_sorted_gpu import run_sorted
    records = sorted_stream(split_var_records(var.bam[3], var.names))
    expected = b"".join(r["raw"] for r in records)
    assert expected != var.bam[3]
    bounds = [1, var.tb + 1] if cuts == "one call" else [1, 2, 7, var.tb + 1]
    stream, calls, f1, f2, frags, flush = run_sorted(var.sim, bounds, first_record_offset=100)
    assert stream == expected and (f1, f2) == var.whole[1:3] and frags == var.whole[0].tobytes()
    # the index of the run: the file's blocks are the stream in pieces of 60000 bytes behind a header of 100 bytes
    size = 100 + len(stream)
    block_u = list(range(0, size, 60000)) + [size]
    block_c = [37 * u // 100 for u in block_u]
    n_no_coor = sum(not r["mapped"] for r in records)
    assert var.sim.bam_sorted_index(block_u, block_c, n_no_coor) == build_bai(records, 100, len(var.names), block_u, block_c, n_no_coor)


def test_enospc_with_a_short_truth_buffer(var):
    frags, f1, f2, sam = var.whole
    dev = var.sim.device
    r1, r2 = api.DeviceArray(dev, len(f1)), api.DeviceArray(dev, len(f2))
    short = api.DeviceArray.from_numpy(dev, np.full(len(sam) - 1, MARKER, np.uint8))
    full = api.DeviceArray.from_numpy(dev, np.full(len(sam), MARKER, np.uint8))
    try:
        n, l1, l2, ls, rc = var.sim.pairs_sam_device(1, var.tb + 1, r1, r2, short)
        assert rc == api.RSQ_ENOSPC and (n, l1, l2, ls) == (len(frags), len(f1), len(f2), len(sam))
        assert np.all(short.to_numpy(np.uint8, len(sam) - 1) == MARKER)
        n, l1, l2, ls, rc = var.sim.pairs_sam_device(1, var.tb + 1, r1, r2, full)
        assert rc == api.RSQ_OK and full.to_numpy(np.uint8, ls).tobytes() == sam
    finally:
        for d in (r1, r2, short, full):
            d.free()


def test_the_opt_in_can_be_taken_back(var):
    var.sim.truth_variants(False)
    try:
        assert var.sim.pairs_sam_device(1, 2, None, None, None)[4] == api.RSQ_EINVAL and "variants" in api.lib().rsq_last_error().decode()
    finally:
        var.sim.truth_variants(True)
    assert var.sim.pairs_sam(1, 3)[3] == var.sim.pairs_sam(1, 2)[3] + var.sim.pairs_sam(2, 3)[3]


def test_variants_that_crowd_the_ends_of_the_sequences(workdir):
    c = VarCase(workdir, "ends", 11, 43, ends=40)
    try:
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        assert len(frags) > 2000 and sam == c.statement(frags, f1, f2, sam)
        assert decode_var_bam(c.sim.pairs_bam(1, c.tb + 1)[3], c.names)[0] == sam
    finally:
        c.close()


def test_a_substitution_only_set(workdir):
    """allele copies, no coordinate maps: today's arithmetic with "_allele<a>" in the QNAME and XI:i:0"""
    c = VarCase(workdir, "subs", 7, 17, kind="subs")
    try:
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        assert len(frags) > 2000 and sam == c.statement(frags, f1, f2, sam) and set(c.xis(sam)) == {0} and b"_allele1:" in sam
        assert decode_var_bam(c.sim.pairs_bam(1, c.tb + 1)[3], c.names)[0] == sam
        a1, a2, asam = c.sim.adapter_only_pairs_sam(0, 50)
        assert asam == c.statement(None, a1, a2, asam) and asam.count(b"\tXI:i:0\n") == 100
    finally:
        c.close()


def test_methylation_beside_the_variants(workdir):
    c = VarCase(workdir, "meth", 7, 61, methylation=True)
    try:
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        pf, p1, p2 = c.sim.pairs(1, c.tb + 1)
        assert len(frags) > 2000 and (p1, p2) == (f1, f2)
        assert sam == c.statement(frags, f1, f2, sam)
        assert decode_var_bam(c.sim.pairs_bam(1, c.tb + 1)[3], c.names)[0] == sam
    finally:
        c.close()


def test_every_read_base_over_a_template_base_is_the_alleles(workdir):
    """without substitution errors: the read bases of every M op are the bases of the stretch the statement places, whether they stand at a reference position
    (M columns) or are inserted (I columns that come from the allele)"""
    c = VarCase(workdir, "nosub", 7, 31, no_substitutions=True)
    try:
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        assert sam == c.statement(frags, f1, f2, sam)
        xis, lines = c.xis(sam), sam.splitlines()
        checked = inserted = 0
        for i, f in enumerate(frags):
            key = int(f["seq"]), int(f["allele"])
            allele, letters = c.alleles[key], c.letters[key]
            hs = stretch_start(allele, int(f["start"]), xis[i])
            for seg in (0, 1):
                fields = lines[2 * i + seg].split(b"\t")
                assert not int(fields[1]) & 0x4
                ops = [op for n, op in template_part(fields[11][5:]) for _ in range(n)]
                q, t = sum(op != b"D" for op in ops), sum(op != b"I" for op in ops)
                reverse = seg != int(f["strand"])
                seq = fields[9]
                read = seq[len(seq) - q:] if reverse else seq[:q]           # SEQ is in reference orientation: a reverse mate's clip stands in front
                at, r = (hs + int(f["len"]) - t if reverse else hs), 0
                for op in (ops[::-1] if reverse else ops):
                    if op == b"M":
                        assert read[r] == letters[at], (f, seg, at)
                        inserted += allele[at][0] == X
                    r += op != b"D"
                    at += op != b"I"
                checked += 1
        assert checked >= 1000 and inserted > 100, (checked, inserted)
    finally:
        c.close()


def test_command_line(workdir):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    c = VarCase(workdir, "cli", 7, 31, replace_n_seed=7, base_identifier="ReseqRead")
    try:
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        bam = c.sim.pairs_bam(1, c.tb + 1)[3]
        a1, a2, asam = c.sim.adapter_only_pairs_sam(0, c.info.adapter_only_pairs)
        abam = c.sim.adapter_only_pairs_bam(0, c.info.adapter_only_pairs)[2]
        header, sam_header, names, fpath, ppath, vcf = c.ref.bam_header_so(1), c.ref.sam_header(), c.names, c.fpath, c.ppath, c.vcf
    finally:
        c.close()
    out = {k: str(workdir / f"truth_variants_cli_{k}") for k in ("1", "2", "sam", "x1", "x2")}
    out["bam"] = str(workdir / "truth_variants_cli.bam")
    common = [exe, "illuminaPE", "-R", fpath, "-s", ppath, "--numReads", "3000", "--seed", "7", "-V", vcf]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True)
    read = lambda path: open(path, "rb").read()
    r = run(["-1", out["1"], "-2", out["2"], "--truthSam", out["sam"], "--truthBam", out["bam"], "--truthBamSort", "--truthVariants"])
    assert r.returncode == 0, r.stderr
    assert read(out["1"]) == f1 + a1 and read(out["2"]) == f2 + a2 and read(out["sam"]) == sam_header + sam + asam
    packed = read(out["bam"])
    block_u, block_c = block_table(packed)
    content = b"".join(zlib.decompress(packed[c0:c1], 31) for c0, c1 in zip(block_c, block_c[1:] + [len(packed)]))
    records = sorted_stream(split_var_records(bam, names))
    assert content == header + b"".join(r["raw"] for r in records) + abam and decode_bam_header(content)[2] == len(header)
    in_file = records + split_var_records(abam, names)
    n_no_coor = sum(not r["mapped"] for r in in_file)
    assert read(out["bam"] + ".bai") == build_bai(in_file, len(header), len(names), block_u, block_c, n_no_coor)
    # without a truth output the flag is an error, and without the flag the refusal stands: nothing is simulated, no file is left
    for extra, message in ((["--truthVariants"], "--truthSam"), (["--truthSam", out["sam"] + ".x"], "variants")):
        r = run(["-1", out["x1"], "-2", out["x2"]] + extra)
        assert r.returncode != 0 and message in r.stderr, r.stderr
        assert not any(os.path.exists(p) for p in (out["x1"], out["x2"], out["sam"] + ".x"))
