"""NM:i and MD:Z on the device (rsq_sim_truth_md, `reseq illuminaPE --truthMD`): every mapped record's tags against `md_nm` (tests/truth_md.py: the rule of
include/reseq_amd.h) applied to the record's own POS, CIGAR and SEQ and the reference as loaded; without the tags every text is, byte for byte, what the same
simulator writes with the switch off; unmapped records carry no tags.  SAM and BAM, with and without variants, the sorted run, the calls cut in pieces, both
writer instantiations, the straight-to-HBM route and the command line."""
import os
import struct
import subprocess

import numpy as np
import pytest

from reseq_amd import api, synth
from test_truth_bam import decode_bam_header
from test_truth_bam_sorted import block_table, build_bai, sorted_stream
from test_truth_bam_sorted_gpu import run_sorted
from test_truth_sam_gpu import MARKER, inflate_members, long_name_case, tiny_case
from test_truth_variants_gpu import VarCase
from truth_md import bam_fields, bam_records, check_bam, check_sam

pytestmark = pytest.mark.gpu

# what the tests below want to have met; TINY's seed yields no record without a mismatch (the CPU oracle says so: 5834 of 5834 mapped records have one), that
# class is met by test_without_substitution_errors and by tests/test_truth_md.py
CLASSES = ("mismatch", "deletion", "insertion", "forward", "reverse", "0 separator")


def letters_of(case):
    """the reference as loaded, by sequence"""
    return [np.frombuffer(b"ACGTN", np.uint8)[case.ref.codes(i)].tobytes() for i in range(case.ref.num_sequences())]


def both(case, call, *args):
    """a call with the switch off and on: (off, on)"""
    case.sim.truth_md(False)
    off = call(*args)
    case.sim.truth_md(True)
    try:
        return off, call(*args)
    finally:
        case.sim.truth_md(False)


def check_case(case, wanted=CLASSES):
    """SAM and BAM over all blocks; returns the classes met"""
    letters = letters_of(case)
    refs = dict(zip(case.names, letters))
    off, on = both(case, case.sim.pairs_sam, 1, case.tb + 1)
    pf, p1, p2 = case.sim.pairs(1, case.tb + 1)
    assert len(pf) > 1000
    for frags, f1, f2, _ in (off, on):
        assert frags.tobytes() == pf.tobytes() and (f1, f2) == (p1, p2)
    seen = check_sam(on[3], off[3], refs)
    boff, bon = both(case, case.sim.pairs_bam, 1, case.tb + 1)
    assert bon[0].tobytes() == pf.tobytes() and bon[1:3] == (p1, p2)
    assert check_bam(bon[3], boff[3], letters) == seen
    # both encodings carry the same tags
    lines = [l for l in on[3].splitlines()]
    for line, rec in zip(lines, bam_records(bon[3])):
        tags = bam_fields(rec)[5]
        if tags[-1][0] == b"MD":
            assert line.endswith(b"\tNM:i:%d\tMD:Z:%s" % (tags[-2][2], tags[-1][2]))
    print(len(pf), "pairs;", seen)
    for c in wanted:
        assert seen.get(c, 0) > 0, (c, seen)                 # a change of TINY must not quietly weaken the test
    return seen, on, bon


@pytest.fixture(scope="module")
def tiny(workdir):
    c = tiny_case(workdir)
    c.seen, c.sam_on, c.bam_on = check_case(c)
    yield c
    c.close()


def test_sam_and_bam_over_all_blocks(tiny):
    assert tiny.seen["forward"] == tiny.seen["reverse"] == len(tiny.sam_on[0])
    # kernel-time names and launches are those of a call without the tags
    tiny.sim.truth_md(True)
    try:
        tiny.sim.pairs_sam(1, 3)
        assert tiny.sim.last_kernel_launches("sam_write") == 1 and tiny.sim.last_kernel_launches("sam_sizes") == 1 and tiny.sim.last_kernel_launches("bam_write") == 0
        tiny.sim.pairs_bam(1, 3)
        assert tiny.sim.last_kernel_launches("bam_write") == 1 and tiny.sim.last_kernel_launches("bam_sizes") == 1 and tiny.sim.last_kernel_launches("sam_write") == 0
    finally:
        tiny.sim.truth_md(False)


def test_without_substitution_errors(workdir):
    """every MD then has no letter outside its ^ runs, and records without a mismatch are met"""
    import re
    c = tiny_case(workdir, no_substitutions=True)
    try:
        seen, on, _ = check_case(c, ("deletion", "insertion", "forward", "reverse", "no mismatch"))
        assert seen.get("mismatch", 0) == 0
        for line in on[3].splitlines():
            md = line.rsplit(b"\tMD:Z:", 1)[1]
            assert re.fullmatch(rb"\d+(\^[ACGT]+\d+)*", md), line
    finally:
        c.close()


def test_with_a_methylation_file(workdir):
    """converted bases are mismatches: with a profile without substitution errors every mismatch is a conversion (reference C read as T on the forward strand of
    the conversion, G read as A on the other)"""
    c = tiny_case(workdir, no_substitutions=True)
    try:
        bed = workdir / "truth_md_meth.bed"
        bed.write_text(f"{c.names[0].decode()}\t0\t4500\t0.0\n{c.names[2].decode()}\t100\t3000\t0.1\n")
        c.sim.read_methylation(bed)
        seen, on, _ = check_case(c, ("mismatch", "deletion", "insertion", "forward", "reverse"))
        import re
        named = set()
        for line in on[3].splitlines():
            named.update(re.findall(rb"\d([ACGT])", re.sub(rb"\^[ACGT]+", b"", line.rsplit(b"\tMD:Z:", 1)[1])))
        assert named and named <= {b"C", b"G"}, named
    finally:
        c.close()


def test_two_uneven_calls(tiny):
    tiny.sim.truth_md(True)
    try:
        a, b = tiny.sim.pairs_sam(1, 4), tiny.sim.pairs_sam(4, tiny.tb + 1)
        assert a[3] + b[3] == tiny.sam_on[3] and len(a[0]) and len(b[0])
        a, b = tiny.sim.pairs_bam(1, 4), tiny.sim.pairs_bam(4, tiny.tb + 1)
        assert a[3] + b[3] == tiny.bam_on[3]
    finally:
        tiny.sim.truth_md(False)


@pytest.mark.parametrize("option,value", [("overlap", 3), ("image_tiles", 1)])
def test_pipelined_sub_ranges_and_binned_rows(tiny, workdir, rsq_options, option, value):
    rsq_options(option, value)
    c = tiny_case(workdir)
    try:
        if option == "image_tiles":
            assert c.sim.fill_plan()["image_tiles"] == 1
        c.sim.truth_md(True)
        assert c.sim.pairs_sam(1, c.tb + 1)[3] == tiny.sam_on[3]
        if option == "overlap":
            assert c.sim.last_kernel_launches("sam_write") == 3
        assert c.sim.pairs_bam(1, c.tb + 1)[3] == tiny.bam_on[3]
    finally:
        c.close()


@pytest.mark.parametrize("kind", ["sam", "bam"])
def test_records_larger_than_the_image(workdir, kind):
    """a fresh simulator's first writing call meets records its image cannot hold: every wave writes a lane a record (Format::record) -- with the tags; the second
    call has the image sized and writes the same bytes through it"""
    c = long_name_case(workdir)
    try:
        letters = letters_of(c)
        off, on = both(c, getattr(c.sim, "pairs_" + kind), 1, c.tb + 1)      # (sized by a first call that writes nothing but sizes the image: through the image)
    finally:
        c.close()
    c = long_name_case(workdir)                                             # a fresh simulator: its first writing call has the image of one that knows no record yet
    try:
        c.sim.truth_md(True)
        n, l1, l2, ls = len(on[0]), len(on[1]), len(on[2]), len(on[3])
        arrays = [api.DeviceArray(c.sim.device, x) for x in (l1, l2, ls, (n + 1) * api.FRAGMENT_DTYPE.itemsize)]
        try:
            texts = []
            for route in ("fallback", "image"):
                n2, _, _, ls2, rc = getattr(c.sim, "pairs_%s_device" % kind)(1, c.tb + 1, *arrays)
                assert rc == api.RSQ_OK and (n2, ls2) == (n, ls), route
                assert c.sim.last_kernel_launches(kind + "_write") == 1
                texts.append(arrays[2].to_numpy(np.uint8, ls).tobytes())
            assert texts[0] == texts[1] == on[3]
            assert ls / n > (1100 + 64 if kind == "sam" else 700 + 48) + 16          # the first of the two calls could not use its image
            if kind == "sam":
                check_sam(texts[0], off[3], dict(zip(c.names, letters)))
            else:
                check_bam(texts[0], off[3], letters)
        finally:
            for d in arrays:
                d.free()
    finally:
        c.close()


def test_adapter_only_calls_write_no_tags(tiny):
    off, on = both(tiny, tiny.sim.adapter_only_pairs_sam, 0, 150)
    assert on == off and len(on[2].splitlines()) == 300 and b"MD:Z" not in on[2]
    off, on = both(tiny, tiny.sim.adapter_only_pairs_bam, 0, 150)
    assert on == off


def test_enospc_with_a_truth_buffer_one_byte_short(tiny):
    frags, f1, f2, sam = tiny.sam_on
    dev = tiny.sim.device
    r1, r2 = api.DeviceArray(dev, len(f1)), api.DeviceArray(dev, len(f2))
    short = api.DeviceArray.from_numpy(dev, np.full(len(sam) - 1, MARKER, np.uint8))
    full = api.DeviceArray.from_numpy(dev, np.full(len(sam), MARKER, np.uint8))
    tiny.sim.truth_md(True)
    try:
        n, l1, l2, ls, rc = tiny.sim.pairs_sam_device(1, tiny.tb + 1, r1, r2, short)
        assert rc == api.RSQ_ENOSPC and (n, l1, l2, ls) == (len(frags), len(f1), len(f2), len(sam))          # the size includes the tags
        assert np.all(short.to_numpy(np.uint8, len(sam) - 1) == MARKER)
        n, l1, l2, ls, rc = tiny.sim.pairs_sam_device(1, tiny.tb + 1, r1, r2, full)
        assert rc == api.RSQ_OK and full.to_numpy(np.uint8, ls).tobytes() == sam
    finally:
        tiny.sim.truth_md(False)
        for d in (r1, r2, short, full):
            d.free()


# ------------------------------------------------------------------------------------------------ a reference with variants
def check_var_case(c, wanted=("mismatch", "deletion", "insertion", "forward", "reverse")):
    seen, on, bon = check_case(c, wanted)
    assert on[3].count(b"\tXI:i:") == 2 * len(on[0])
    for line in on[3].splitlines()[:50]:
        f = line.split(b"\t")
        assert [t[:5] for t in f[11:]] == [b"XC:Z:", b"XE:i:", b"XI:i:", b"NM:i:", b"MD:Z:"]
    return seen, on, bon


def test_variants_of_the_golden_file(workdir):
    """tests/golden/test-var.vcf: its 13 variants (substitutions, insertions, deletions on two alleles) lie in the first 21 bases and at 11368 of a contig of
    4.6 M bases; the stretch of the contig that holds them stands in for it (the VCF's REF alleles are checked when it is read)"""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    c = GoldenCase(workdir, golden)
    try:
        seen, on, _ = check_var_case(c, ("mismatch", "forward", "reverse"))
        low = [l for l in on[3].splitlines() if int(l.split(b"\t")[3]) <= 21 and b"_allele1:" in l]
        assert low, "records over the variants at the contig's beginning"
    finally:
        c.close()


class GoldenCase:
    """TINY's profile over a stand-in for the contig of tests/golden/test-var.vcf: 12000 random bases that carry the VCF's REF alleles in reach"""

    def __init__(self, workdir, golden):
        import json
        import parity_cases as P
        self.ppath = P.make_inputs(workdir, "tiny_e2e", synth.TINY, [5000, 80, 3210])[0]
        g = json.load(open(os.path.join(golden, "reference_known_answers.json")))["variation_loading"]
        codes = np.random.default_rng(5).integers(0, 4, 12000).astype(np.uint8)
        for pos, bases in g["ref_alleles"]:
            if pos + len(bases) <= len(codes):
                codes[pos:pos + len(bases)] = ["ACGT".index(b) for b in bases]
        vcf = workdir / "truth_md_golden.vcf"          # the golden file's records within the stand-in, its header with the stand-in's length
        with open(os.path.join(golden, "test-var.vcf")) as f, open(vcf, "w") as out:
            for line in f:
                if line.startswith("#") or int(line.split("\t")[1]) <= len(codes):
                    out.write(line)
        self.fpath = str(workdir / "truth_md_golden.fa")
        synth.write_fasta(self.fpath, [(g["contig"] + " stand-in", codes)])
        self.prof = api.Profile(self.ppath)
        self.ref = api.Reference(self.fpath, 0)
        self.ref.read_variants(str(vcf))
        self.names = [self.ref.sequence_name(i).encode() for i in range(self.ref.num_sequences())]
        self.sim = api.Simulator(self.prof, self.ref, 0)
        self.info = self.sim.prepare(7, 3000)
        self.tb = self.info.total_blocks
        self.sim.truth_variants(True)

    def close(self):
        self.sim.close()
        self.ref.close()
        self.prof.close()


@pytest.fixture(scope="module")
def var(workdir):
    c = VarCase(workdir, "md_main", 7, 31)
    c.seen, c.sam_on, c.bam_on = check_var_case(c)
    yield c
    c.close()


def test_mixed_variants(var):
    """I and D columns that come from the allele map are met: more records with ^ and with I than the read errors alone give"""
    cigars = [line.split(b"\t")[5] for line in var.sam_on[3].splitlines()]
    assert sum(b"D" in c for c in cigars) > 100 and sum(b"I" in c for c in cigars) > 100
    assert var.seen["deletion"] > 100 and var.seen["0 separator"] > 0


def test_variants_that_crowd_the_ends_of_the_sequences(workdir):
    c = VarCase(workdir, "md_ends", 11, 43, ends=40)
    try:
        check_var_case(c)
    finally:
        c.close()


def test_a_substitution_only_set(workdir):
    """allele copies: the comparison is against the reference, so the alleles' substitutions are mismatches even without substitution errors"""
    c = VarCase(workdir, "md_subs", 7, 17, kind="subs", no_substitutions=True)
    try:
        seen, on, _ = check_var_case(c, ("mismatch", "deletion", "insertion", "forward", "reverse", "no mismatch"))
    finally:
        c.close()


def split_tagged(data):
    """split_records of tests/test_truth_bam_sorted.py for records with any tags"""
    out = []
    for raw in bam_records(data):
        ref_id, pos, flag, cigar, _, _ = bam_fields(raw)
        span = sum(n for n, op in cigar if op in (b"M", b"D"))
        mapped = not flag & 0x4
        out.append(dict(raw=raw, ref_id=ref_id, pos=pos - 1, span=max(span, 1) if mapped else 0, bin=struct.unpack_from("<H", raw, 14)[0], mapped=mapped))
    return out


@pytest.mark.parametrize("which", ["plain", "variants"])
@pytest.mark.parametrize("cuts", ["one call", "three uneven calls"])
def test_sorted_run(tiny, var, which, cuts):
    c = tiny if which == "plain" else var
    records = sorted_stream(split_tagged(c.bam_on[3]))
    expected = b"".join(r["raw"] for r in records)
    assert expected != c.bam_on[3]
    bounds = [1, c.tb + 1] if cuts == "one call" else [1, 2, 7, c.tb + 1]
    c.sim.truth_md(True)
    try:
        c.sim.bam_sorted_begin(100)
        with pytest.raises(api.RsqError) as e:                      # the switch cannot change inside a run
            c.sim.truth_md(False)
        assert e.value.code == api.RSQ_ESTATE
        c.sim.truth_md(True)                                        # (setting it to what it is changes nothing)
        stream, calls, f1, f2, frags, flush = run_sorted(c.sim, bounds, first_record_offset=100)
        assert stream == expected and (f1, f2) == c.bam_on[1:3] and frags == c.bam_on[0].tobytes()
        size = 100 + len(stream)
        block_u = list(range(0, size, 60000)) + [size]
        block_c = [37 * u // 100 for u in block_u]
        n_no_coor = sum(not r["mapped"] for r in records)
        assert c.sim.bam_sorted_index(block_u, block_c, n_no_coor) == build_bai(records, 100, len(c.names), block_u, block_c, n_no_coor)
    finally:
        c.sim.truth_md(False)                                       # the run was flushed: the switch is free again


def test_command_line(tiny, workdir):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    out = {k: str(workdir / f"truth_md_cli_{k}") for k in ("1", "2", "sam", "bam", "o1", "o2", "osam", "obam", "x1", "x2")}
    common = [exe, "illuminaPE", "-R", tiny.fpath, "-s", tiny.ppath, "--numReads", "3000", "--seed", "7"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True)
    r = run(["-1", out["1"], "-2", out["2"], "--truthSam", out["sam"], "--truthBam", out["bam"], "--truthBamSort", "--truthMD"])
    assert r.returncode == 0, r.stderr
    r = run(["-1", out["o1"], "-2", out["o2"], "--truthSam", out["osam"], "--truthBam", out["obam"], "--truthBamSort"])
    assert r.returncode == 0, r.stderr
    read = lambda path: open(path, "rb").read()
    assert read(out["1"]) == read(out["o1"]) and read(out["2"]) == read(out["o2"])
    c = tiny_case(workdir, replace_n_seed=7)
    try:
        letters = letters_of(c)
        names = c.names
    finally:
        c.close()
    on, off = read(out["sam"]), read(out["osam"])
    header = b"".join(l + b"\n" for l in off.split(b"\n") if l.startswith(b"@"))
    assert on.startswith(header) and len(header) > 0
    seen = check_sam(on[len(header):], off[len(header):], dict(zip(names, letters)))
    assert seen["mismatch"] > 0 and seen["deletion"] > 0
    streams = []
    for key in ("bam", "obam"):
        data = inflate_members(read(out[key]))
        at = decode_bam_header(data)[2]
        streams.append(data[at:])
        assert os.path.exists(out[key] + ".bai")
    check_bam(streams[0], streams[1], letters)
    positions = [(r["ref_id"], r["pos"]) for r in split_tagged(streams[0]) if r["mapped"]]
    assert positions == sorted(positions) and len(positions) > 4000
    # --truthMD alone
    r = run(["-1", out["x1"], "-2", out["x2"], "--truthMD"])
    assert r.returncode != 0 and "--truthMD adds the tags" in r.stderr and "--truthSam / --truthBam" in r.stderr
    assert not os.path.exists(out["x1"])
