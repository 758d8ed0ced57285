"""Truth alignments on the device (rsq_sim_pairs_sam, rsq_sim_adapter_only_pairs_sam, `reseq illuminaPE --truthSam`): the SAM text against the statement of
tests/test_truth_sam.py applied to the call's own fragments and FASTQ text, and -- independent of that statement -- against the reference itself: with a profile
without substitution errors every M base of every mapped record is the reference base its POS and CIGAR point at."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from reseq_amd import api, synth
from test_truth_sam import sam_text

pytestmark = pytest.mark.gpu

MARKER = 0xA7


class Case:
    """profile + reference + a prepared simulator (made after the options a test sets)"""

    def __init__(self, workdir, tag, cfg, ref_lengths, seed, num_pairs, no_substitutions=False, vcf=None, replace_n_seed=0, base_identifier="", **kw):
        import parity_cases as P
        self.ppath, self.fpath, self.seqs = P.make_inputs(workdir, tag, cfg, ref_lengths, **kw)
        self.phred_offset = cfg["phred_offset"]
        self.prof = api.Profile(self.ppath)
        if no_substitutions:
            self.prof.remove_substitution_errors()
        self.ref = api.Reference(self.fpath, replace_n_seed)
        if vcf:
            self.ref.read_variants(vcf)
        self.names = [self.ref.sequence_name(i).encode() for i in range(self.ref.num_sequences())]
        self.sim = api.Simulator(self.prof, self.ref, 0)
        self.info = self.sim.prepare(seed, num_pairs, record_base_identifier=base_identifier)
        self.tb = self.info.total_blocks

    def statement(self, frags, f1, f2):
        return sam_text(frags, f1, f2, self.names, self.phred_offset)

    def close(self):
        self.sim.close()
        self.ref.close()
        self.prof.close()


def tiny_case(workdir, **kw):
    return Case(workdir, "tiny_e2e", synth.TINY, [5000, 80, 3210], 7, 3000, **kw)


@pytest.fixture(scope="module")
def tiny(workdir):
    c = tiny_case(workdir)
    c.whole = c.sim.pairs_sam(1, c.tb + 1)
    yield c
    c.close()


def test_equals_pairs_and_the_statement(tiny):
    frags, f1, f2, sam = tiny.whole
    pf, p1, p2 = tiny.sim.pairs(1, tiny.tb + 1)
    assert 2000 < len(frags) < 4000
    assert pf.tobytes() == frags.tobytes() and p1 == f1 and p2 == f2
    assert sam == tiny.statement(frags, f1, f2)
    assert tiny.sim.last_kernel_launches("sam_write") == 0 and tiny.sim.last_kernel_launches("sam_sizes") == 0      # the last call was a plain one
    tiny.sim.pairs_sam(1, 3)
    assert tiny.sim.last_kernel_launches("sam_write") == 1 and tiny.sim.last_kernel_launches("sam_sizes") == 1


_SAM_ELEMENT = re.compile(rb"(\d+)([MIDS])")


def check_against_the_reference(case, sam):
    """walks every mapped record's CIGAR from POS: every M base of SEQ is the reference's.  Returns the classes of reads met."""
    letters = [np.frombuffer(b"ACGTN", np.uint8)[codes].tobytes() for _, codes in case.seqs]
    index = {n: i for i, n in enumerate(case.names)}
    seen = dict(forward=0, reverse=0, leading_d=0, trailing_d=0, leading_i=0, zero_length=0, adapter_part=0, tail=0, without_m=0)
    residues = set()
    records = sam.splitlines()
    for line in records:
        f = line.split(b"\t")
        flag, pos, cigar, seq, xc = int(f[1]), int(f[3]), f[5], f[9], f[11][5:]
        assert not flag & 0x4 and f[4] == b"60" and f[6] == b"=", line
        ref = letters[index[f[2]]]
        elements = [(int(n), op) for n, op in _SAM_ELEMENT.findall(cigar)]
        assert b"".join(b"%d%s" % e for e in elements) == cigar and all(n > 0 for n, _ in elements), line
        assert sum(n for n, op in elements if op in b"MIS") == len(seq) == len(f[10]), line
        at_ref, at_read, matched = pos - 1, 0, 0
        for n, op in elements:
            if op == b"M":
                assert 0 <= at_ref and at_ref + n <= len(ref), line
                assert seq[at_read:at_read + n] == ref[at_ref:at_ref + n], line
                matched += n
            if op in b"MD":
                at_ref += n
            if op in b"MIS":
                at_read += n
        # the classes, from the id's own CIGAR (the XC tag)
        template = re.match(rb"(?:\d+[MDI])*", xc).group(0)
        seen["reverse" if flag & 0x10 else "forward"] += 1
        seen["leading_d"] += bool(re.match(rb"0M\d+D", template))
        seen["trailing_d"] += template.endswith(b"D")
        seen["leading_i"] += bool(re.match(rb"0M\d+I", template))
        seen["zero_length"] += bool(re.search(rb"(^|[A-Z])0[A-Z]", xc))
        seen["adapter_part"] += b"S" in xc
        seen["tail"] += b"H" in xc
        seen["without_m"] += matched == 0
        residues.add(len(seq) % 4)
    return seen, residues, len(records)


def test_every_aligned_base_is_the_reference_base(workdir):
    """no record is left out: every record of every pair is walked"""
    c = tiny_case(workdir, no_substitutions=True)
    try:
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        assert np.all(frags["len"] > 0)
        seen, residues, n = check_against_the_reference(c, sam)
        print(len(frags), "pairs;", seen, sorted(residues))
        assert n == 2 * len(frags) and seen["forward"] == seen["reverse"] == len(frags)
        for name in ("leading_d", "trailing_d", "leading_i", "zero_length", "adapter_part", "tail"):      # a change of TINY must not quietly weaken this test
            assert seen[name] > 0, (name, seen)
        assert residues == {0, 1, 2, 3} and seen["without_m"] == 0
        assert sam == c.statement(frags, f1, f2)
    finally:
        c.close()


def test_batching(tiny):
    frags, f1, f2, sam = tiny.whole
    a, b = tiny.sim.pairs_sam(1, 4), tiny.sim.pairs_sam(4, tiny.tb + 1)
    assert a[3] + b[3] == sam and a[1] + b[1] == f1 and a[2] + b[2] == f2
    assert len(a[0]) and len(b[0])
    empty = tiny.sim.pairs_sam(3, 3)
    assert (len(empty[0]), empty[1], empty[2], empty[3]) == (0, b"", b"", b"")


@pytest.mark.parametrize("option,value", [("overlap", 3), ("image_tiles", 1)])
def test_pipelined_sub_ranges_and_binned_rows(tiny, workdir, rsq_options, option, value):
    rsq_options(option, value)
    c = tiny_case(workdir)
    try:
        if option == "image_tiles":
            assert c.sim.fill_plan()["image_tiles"] == 1
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        assert frags.tobytes() == tiny.whole[0].tobytes()
        assert (f1, f2) == tiny.whole[1:3]
        assert sam == tiny.whole[3]
        if option == "overlap":
            assert c.sim.last_kernel_launches("sam_write") == 3
        a1, a2, asam = c.sim.adapter_only_pairs_sam(0, 150)
        assert (a1, a2) == tiny.sim.adapter_only_pairs(0, 150) and asam == c.statement(None, a1, a2)
    finally:
        c.close()


def test_adapter_only_pairs(tiny):
    f1, f2, sam = tiny.sim.adapter_only_pairs_sam(0, 150)
    assert (f1, f2) == tiny.sim.adapter_only_pairs(0, 150)
    assert tiny.sim.last_kernel_launches("sam_write") == 0
    lines = sam.splitlines()
    fastq = [x.split(b"\n") for x in (f1, f2)]
    assert len(lines) == 300
    for i, line in enumerate(lines):
        f = line.split(b"\t")
        pair, seg = divmod(i, 2)
        assert f[1:9] == [b"141" if seg else b"77", b"*", b"0", b"0", b"*", b"*", b"0", b"0"]
        assert f[0] == fastq[seg][4 * pair][1:].split(b" ")[0] and b":0:Adapter:0:" in f[0]
        assert f[9] == fastq[seg][4 * pair + 1] and f[10] == fastq[seg][4 * pair + 3]          # TINY's offset is 33
    assert sam == tiny.statement(None, f1, f2)
    assert tiny.sim.adapter_only_pairs_sam(10, 0) == (b"", b"", b"")


def test_calls_of_two_kinds_take_turns_on_one_simulator(tiny, workdir):
    """the pinned words a call's sizes arrive in belong to one kind of call each: an adapter-only call between two calls over the reference changes neither, and
    is itself the call of a simulator that has made no other"""
    first = tiny.sim.pairs_sam(1, tiny.tb + 1)
    between = tiny.sim.adapter_only_pairs_sam(0, 150)
    third = tiny.sim.pairs_sam(1, tiny.tb + 1)
    assert first[0].tobytes() == third[0].tobytes() == tiny.whole[0].tobytes() and first[1:] == third[1:] == tiny.whole[1:]
    fresh = tiny_case(workdir)
    try:
        assert fresh.sim.adapter_only_pairs_sam(0, 150) == between and len(between[2]) > 0
    finally:
        fresh.close()


def test_enospc_leaves_the_buffer_alone(tiny):
    frags, f1, f2, sam = tiny.whole
    dev = tiny.sim.device
    r1, r2 = api.DeviceArray(dev, len(f1)), api.DeviceArray(dev, len(f2))
    short = api.DeviceArray.from_numpy(dev, np.full(len(sam) - 1, MARKER, np.uint8))
    try:
        n, l1, l2, ls, rc = tiny.sim.pairs_sam_device(1, tiny.tb + 1, r1, r2, short)
        assert rc == api.RSQ_ENOSPC and (n, l1, l2, ls) == (len(frags), len(f1), len(f2), len(sam))
        assert np.all(short.to_numpy(np.uint8, len(sam) - 1) == MARKER)
        # a FASTQ buffer one byte short: the SAM text is not written either
        full = api.DeviceArray.from_numpy(dev, np.full(len(sam), MARKER, np.uint8))
        r1s = api.DeviceArray(dev, len(f1) - 1)
        n, l1, l2, ls, rc = tiny.sim.pairs_sam_device(1, tiny.tb + 1, r1s, r2, full)
        assert rc == api.RSQ_ENOSPC and (l1, l2, ls) == (len(f1), len(f2), len(sam))
        assert np.all(full.to_numpy(np.uint8, len(sam)) == MARKER)
        # buffers of exactly the needed sizes
        n, l1, l2, ls, rc = tiny.sim.pairs_sam_device(1, tiny.tb + 1, r1, r2, full)
        assert rc == api.RSQ_OK and full.to_numpy(np.uint8, ls).tobytes() == sam
        r1s.free()
        full.free()
    finally:
        for d in (r1, r2, short):
            d.free()


def test_a_reference_with_variants_is_refused(workdir):
    import parity_cases as P
    ppath, fpath, seqs = P.make_inputs(workdir, "tiny_e2e", synth.TINY, [5000, 80, 3210])
    vcf = workdir / "sam_refused.vcf"
    P.write_vcf(vcf, seqs, [(0, 99, 1, "ACGT"[(int(seqs[0][1][99]) + 1) % 4], "0|1"), (2, 1500, 1, "ACGT"[(int(seqs[2][1][1500]) + 2) % 4], "1|1")])
    c = Case(workdir, "tiny_e2e", synth.TINY, [5000, 80, 3210], 7, 3000, vcf=str(vcf))
    try:
        n, l1, l2, ls, rc = c.sim.pairs_sam_device(1, 2, None, None, None)
        assert rc == api.RSQ_EINVAL and "variants" in api.lib().rsq_last_error().decode()
        l = C.c_size_t()
        assert api.lib().rsq_sim_adapter_only_pairs_sam(c.sim.h, 0, 10, None, 0, C.byref(l), None, 0, C.byref(l), None, 0, C.byref(l), None) == api.RSQ_EINVAL
        assert len(c.sim.pairs(1, 2)[0]) > 0                      # the plain call serves it
    finally:
        c.close()


def inflate_members(data):
    out = []
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        assert d.eof
        data = d.unused_data
    return b"".join(out)


def test_command_line(tiny, workdir):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    out = {k: str(workdir / f"truth_cli_{k}") for k in ("p1", "p2", "s1", "s2", "sam", "g1", "g2", "samgz", "h1", "h2", "hostgz", "x1", "x2", "xsam")}
    common = [exe, "illuminaPE", "-R", tiny.fpath, "-s", tiny.ppath, "--numReads", "3000", "--seed", "7"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True)
    assert run(["-1", out["p1"], "-2", out["p2"]]).returncode == 0
    assert run(["-1", out["s1"], "-2", out["s2"], "--truthSam", out["sam"]]).returncode == 0
    assert run(["-1", out["g1"], "-2", out["g2"], "--truthSam", out["samgz"] + ".sam.gz"]).returncode == 0
    assert run(["-1", out["h1"], "-2", out["h2"], "--truthSam", out["hostgz"] + ".sam.gz", "--hostGzip"]).returncode == 0
    read = lambda path: open(path, "rb").read()
    for m in "12":
        assert read(out["p" + m]) == read(out["s" + m]) == read(out["g" + m]) == read(out["h" + m])
    # the API's texts of the same run: the command's seed (also ReplaceN's), pair count and base identifier
    c = tiny_case(workdir, replace_n_seed=7, base_identifier="ReseqRead")
    try:
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        a1, a2, asam = c.sim.adapter_only_pairs_sam(0, c.info.adapter_only_pairs)
        header = c.ref.sam_header()
    finally:
        c.close()
    assert len(frags) > 2000 and len(a1) > 0
    assert read(out["p1"]) == f1 + a1 and read(out["p2"]) == f2 + a2
    text = read(out["sam"])
    assert text == header + sam + asam
    packed = read(out["samgz"] + ".sam.gz")
    assert packed[3] == 4 and packed.endswith(api.gzip_eof_member()) and inflate_members(packed) == text      # BGZF members made on the device
    assert read(out["hostgz"] + ".sam.gz")[3] == 0 and inflate_members(read(out["hostgz"] + ".sam.gz")) == text
    # refusals: nothing is simulated, no file is left
    for extra, message in ((["--gpus", "2"], "one worker only"), (["-V", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test-var.vcf")], "variants"),
                           (["--truthSam", out["xsam"] + ".bz2"], "bzip2")):
        r = run(["-1", out["x1"], "-2", out["x2"], "--truthSam", out["xsam"]] + extra)
        assert r.returncode != 0 and message in r.stderr, r.stderr
        assert not any(os.path.exists(p) for p in (out["x1"], out["x2"], out["xsam"], out["xsam"] + ".bz2"))
    r = run(["-1", out["x1"], "-2", out["x2"], "--truthSam", out["xsam"], "-j", "1"])
    assert r.returncode == 0 and read(out["xsam"]) == text


def test_read_length_150(workdir):
    """P0: 38-word rows (150 is no multiple of four: every reversed word comes from two neighbours) and the writer's image at real record sizes"""
    c = Case(workdir, "sam_p0", synth.P0, [20000], 11, 1500, no_substitutions=True, prof_seed=103741084, ref_seed=2)
    try:
        frags, f1, f2, sam = c.sim.pairs_sam(1, c.tb + 1)
        pf, p1, p2 = c.sim.pairs(1, c.tb + 1)
        assert 1000 < len(frags) < 2000 and pf.tobytes() == frags.tobytes() and (p1, p2) == (f1, f2)
        assert sam == c.statement(frags, f1, f2)
        seen, residues, n = check_against_the_reference(c, sam)
        print(len(frags), "pairs;", seen)
        assert n == 2 * len(frags) and seen["without_m"] == 0 and residues == {150 % 4}
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ the writers' straight-to-HBM fallback
# The image a FRESH simulator gives its first writing call holds pairs of this many bytes: the initial values of rsq_sim::sam_pair_bytes and bam_pair_bytes in
# reseq_amd/csrc/rsq_sim.hip.  The test below takes the fallback only while its pairs are larger: whoever raises those two values raises these, and the test then
# says whether its records still are.
FRESH_IMAGE_PAIR_BYTES = {"sam": 1100, "bam": 700}


def long_name_case(workdir):
    """test_read_length_150's inputs with a reference name of 150 characters: a pair is about 1.45 KB of SAM and 1.0 KB of BAM, more than the image of a fresh
    simulator holds (pairs of 1100 and 700 bytes); the QNAME stays below BAM's 254"""
    return Case(workdir, "truth_long_name", synth.P0, [20000], 11, 1500, no_substitutions=True, prof_seed=103741084, ref_seed=2, names=["n" * 150 + " rest of the id"])


@pytest.fixture(scope="module")
def long_name_expected(workdir):
    """pairs_sam / pairs_bam size with a first call that writes nothing but already sizes the image for the second: these bytes went through the image"""
    c = long_name_case(workdir)
    try:
        return dict(sam=c.sim.pairs_sam(1, c.tb + 1), bam=c.sim.pairs_bam(1, c.tb + 1))
    finally:
        c.close()


@pytest.mark.parametrize("kind", ["sam", "bam"])
def test_records_larger_than_the_image_go_straight_to_the_output(workdir, long_name_expected, kind):
    """a fresh simulator's first writing call meets records its image cannot hold (every wave writes a lane a record, no LDS); its second call has the image sized"""
    from test_truth_bam import decode_bam
    frags, f1, f2, want = long_name_expected[kind]
    assert 1000 < len(frags) < 2000 and len(want) / len(frags) > FRESH_IMAGE_PAIR_BYTES[kind] + 16      # (16: the skew of a wave's text against its image)
    c = long_name_case(workdir)
    arrays = [api.DeviceArray(c.sim.device, n) for n in (len(f1), len(f2), len(want), (len(frags) + 1) * api.FRAGMENT_DTYPE.itemsize)]
    r1, r2, out, fr = arrays
    try:
        for route in ("fallback", "image"):
            n, l1, l2, ls, rc = getattr(c.sim, "pairs_%s_device" % kind)(1, c.tb + 1, r1, r2, out, fr)
            assert rc == api.RSQ_OK and (n, l1, l2, ls) == (len(frags), len(f1), len(f2), len(want)), route
            assert c.sim.last_kernel_launches(kind + "_write") == 1
            assert out.to_numpy(np.uint8, ls).tobytes() == want, route
            assert r1.to_numpy(np.uint8, l1).tobytes() == f1 and r2.to_numpy(np.uint8, l2).tobytes() == f2 and fr.to_numpy(api.FRAGMENT_DTYPE, n).tobytes() == frags.tobytes()
        text = want if kind == "sam" else decode_bam(want, c.names)[0]
        assert text == c.statement(frags, f1, f2) and text == long_name_expected["sam"][3]
        assert max(len(line.split(b"\t")[0]) for line in text.splitlines()) < 254
    finally:
        for d in arrays:
            d.free()
        c.close()
