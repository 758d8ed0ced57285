"""Truth alignments as BAM on the device (rsq_sim_pairs_bam, rsq_sim_adapter_only_pairs_bam, `reseq illuminaPE --truthBam`).  The oracle is the SAM text of the
same pairs (rsq_sim_pairs_sam, which tests/test_truth_sam_gpu.py pins to its statement): a BAM record is a pure re-encoding of its SAM line, so the records,
decoded by tests/test_truth_bam.py's pure-Python decoder (which also asserts block_size, l_read_name and bin == reg2bin), must give that text byte for byte."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from reseq_amd import api, synth
from test_truth_bam import UNMAPPED_BIN, decode_bam, decode_bam_header
from test_truth_sam_gpu import MARKER, Case, tiny_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny(workdir):
    c = tiny_case(workdir)
    c.sam = c.sim.pairs_sam(1, c.tb + 1)
    c.whole = c.sim.pairs_bam(1, c.tb + 1)
    yield c
    c.close()


def launches(sim):
    return {k: sim.last_kernel_launches(k) for k in ("bam_sizes", "bam_write", "sam_sizes", "sam_write")}


def test_decodes_to_the_sam_text(tiny):
    frags, f1, f2, bam = tiny.whole
    assert 2000 < len(frags) < 4000
    assert frags.tobytes() == tiny.sam[0].tobytes() and (f1, f2) == tiny.sam[1:3]
    text, records = decode_bam(bam, tiny.names)
    assert text == tiny.sam[3] and len(records) == 2 * len(frags)
    pf, p1, p2 = tiny.sim.pairs(1, tiny.tb + 1)
    assert pf.tobytes() == frags.tobytes() and (p1, p2) == (f1, f2)
    assert launches(tiny.sim) == dict(bam_sizes=0, bam_write=0, sam_sizes=0, sam_write=0)          # the last call was a plain one
    tiny.sim.pairs_bam(1, 3)
    assert launches(tiny.sim) == dict(bam_sizes=1, bam_write=1, sam_sizes=0, sam_write=0)
    tiny.sim.pairs_sam(1, 3)
    assert launches(tiny.sim) == dict(bam_sizes=0, bam_write=0, sam_sizes=1, sam_write=1)


def test_batching(tiny):
    frags, f1, f2, bam = tiny.whole
    a, b = tiny.sim.pairs_bam(1, 4), tiny.sim.pairs_bam(4, tiny.tb + 1)
    assert a[3] + b[3] == bam and a[1] + b[1] == f1 and a[2] + b[2] == f2
    assert len(a[0]) and len(b[0])
    empty = tiny.sim.pairs_bam(3, 3)
    assert (len(empty[0]), empty[1], empty[2], empty[3]) == (0, b"", b"", b"")


@pytest.mark.parametrize("option,value", [("overlap", 3), ("image_tiles", 1)])
def test_pipelined_sub_ranges_and_binned_rows(tiny, workdir, rsq_options, option, value):
    rsq_options(option, value)
    c = tiny_case(workdir)
    try:
        if option == "image_tiles":
            assert c.sim.fill_plan()["image_tiles"] == 1
        frags, f1, f2, bam = c.sim.pairs_bam(1, c.tb + 1)
        assert frags.tobytes() == tiny.whole[0].tobytes()
        assert (f1, f2) == tiny.whole[1:3]
        assert bam == tiny.whole[3]
        if option == "overlap":
            assert c.sim.last_kernel_launches("bam_write") == 3
        a1, a2, abam = c.sim.adapter_only_pairs_bam(0, 150)
        assert (a1, a2, abam) == tiny.sim.adapter_only_pairs_bam(0, 150)
    finally:
        c.close()


def test_adapter_only_pairs(tiny):
    f1, f2, bam = tiny.sim.adapter_only_pairs_bam(0, 150)
    assert (f1, f2) == tiny.sim.adapter_only_pairs(0, 150)
    assert tiny.sim.last_kernel_launches("bam_write") == 0
    s1, s2, sam = tiny.sim.adapter_only_pairs_sam(0, 150)
    text, records = decode_bam(bam, tiny.names)
    assert text == sam and len(records) == 300
    fastq = [x.split(b"\n") for x in (f1, f2)]
    for i, (r, line) in enumerate(zip(records, text.splitlines())):
        pair, seg = divmod(i, 2)
        assert (r["ref_id"], r["next_ref_id"], r["pos"], r["next_pos"], r["mapq"], r["bin"], r["n_cigar"], r["tlen"]) == (-1, -1, -1, -1, 0, UNMAPPED_BIN, 0, 0)
        assert r["flag"] == (141 if seg else 77)
        f = line.split(b"\t")
        assert f[9] == fastq[seg][4 * pair + 1] and f[10] == fastq[seg][4 * pair + 3]          # FASTQ orientation (TINY's offset is 33)
    assert tiny.sim.adapter_only_pairs_bam(10, 0) == (b"", b"", b"")


def test_enospc_leaves_the_buffer_alone(tiny):
    frags, f1, f2, bam = tiny.whole
    dev = tiny.sim.device
    r1, r2 = api.DeviceArray(dev, len(f1)), api.DeviceArray(dev, len(f2))
    short = api.DeviceArray.from_numpy(dev, np.full(len(bam) - 1, MARKER, np.uint8))
    try:
        n, l1, l2, lb, rc = tiny.sim.pairs_bam_device(1, tiny.tb + 1, r1, r2, short)
        assert rc == api.RSQ_ENOSPC and (n, l1, l2, lb) == (len(frags), len(f1), len(f2), len(bam))
        assert np.all(short.to_numpy(np.uint8, len(bam) - 1) == MARKER)
        # a FASTQ buffer one byte short: the BAM records are not written either
        full = api.DeviceArray.from_numpy(dev, np.full(len(bam), MARKER, np.uint8))
        r1s = api.DeviceArray(dev, len(f1) - 1)
        n, l1, l2, lb, rc = tiny.sim.pairs_bam_device(1, tiny.tb + 1, r1s, r2, full)
        assert rc == api.RSQ_ENOSPC and (l1, l2, lb) == (len(f1), len(f2), len(bam))
        assert np.all(full.to_numpy(np.uint8, len(bam)) == MARKER)
        # buffers of exactly the needed sizes
        n, l1, l2, lb, rc = tiny.sim.pairs_bam_device(1, tiny.tb + 1, r1, r2, full)
        assert rc == api.RSQ_OK and full.to_numpy(np.uint8, lb).tobytes() == bam
        r1s.free()
        full.free()
    finally:
        for d in (r1, r2, short):
            d.free()


def test_a_reference_with_variants_is_refused(workdir):
    import parity_cases as P
    ppath, fpath, seqs = P.make_inputs(workdir, "tiny_e2e", synth.TINY, [5000, 80, 3210])
    vcf = workdir / "bam_refused.vcf"
    P.write_vcf(vcf, seqs, [(0, 99, 1, "ACGT"[(int(seqs[0][1][99]) + 1) % 4], "0|1"), (2, 1500, 1, "ACGT"[(int(seqs[2][1][1500]) + 2) % 4], "1|1")])
    c = Case(workdir, "tiny_e2e", synth.TINY, [5000, 80, 3210], 7, 3000, vcf=str(vcf))
    try:
        n, l1, l2, lb, rc = c.sim.pairs_bam_device(1, 2, None, None, None)
        assert rc == api.RSQ_EINVAL and "variants" in api.lib().rsq_last_error().decode()
        l = C.c_size_t()
        assert api.lib().rsq_sim_adapter_only_pairs_bam(c.sim.h, 0, 10, None, 0, C.byref(l), None, 0, C.byref(l), None, 0, C.byref(l), None) == api.RSQ_EINVAL
        assert "variants" in api.lib().rsq_last_error().decode()
        assert len(c.sim.pairs(1, 2)[0]) > 0                      # the plain call serves it
    finally:
        c.close()


@pytest.mark.parametrize("name_len,refused", [(197, False), (198, True)])
def test_a_read_name_that_could_exceed_254_bytes_is_refused(workdir, name_len, refused):
    """decided at the call from the widest every field can be: "ReseqRead" (9) + block (10) _ number (10) : pos (4) : name : pos (4) : tile (5) :1337:1337 = 57 + name"""
    c = Case(workdir, f"bam_name_{name_len}", synth.TINY, [5000], 7, 1000, names=["n" * name_len + " rest of the id"])
    try:
        n, l1, l2, lb, rc = c.sim.pairs_bam_device(1, c.tb + 1, None, None, None)
        if refused:
            assert rc == api.RSQ_EINVAL and "254" in api.lib().rsq_last_error().decode() and (n, lb) == (0, 0)
            l = C.c_size_t()
            assert api.lib().rsq_sim_adapter_only_pairs_bam(c.sim.h, 0, 10, None, 0, C.byref(l), None, 0, C.byref(l), None, 0, C.byref(l), None) == api.RSQ_EINVAL
            assert len(c.sim.pairs_sam(1, c.tb + 1)[0]) > 0           # SAM text has no such limit
        else:
            assert rc == api.RSQ_ENOSPC and n > 0
            frags, f1, f2, bam = c.sim.pairs_bam(1, c.tb + 1)
            text, records = decode_bam(bam, c.names)
            assert text == c.sim.pairs_sam(1, c.tb + 1)[3] and max(r["l_read_name"] for r in records) <= 255
    finally:
        c.close()


def test_read_length_150(workdir):
    """P0: 38-word rows (150 is no multiple of four: every reversed word comes from two neighbours, 75 packed bytes are no whole words) and real record sizes"""
    c = Case(workdir, "sam_p0", synth.P0, [20000], 11, 1500, no_substitutions=True, prof_seed=103741084, ref_seed=2)
    try:
        frags, f1, f2, bam = c.sim.pairs_bam(1, c.tb + 1)
        sf, s1, s2, sam = c.sim.pairs_sam(1, c.tb + 1)
        assert 1000 < len(frags) < 2000 and sf.tobytes() == frags.tobytes() and (s1, s2) == (f1, f2)
        text, records = decode_bam(bam, c.names)
        assert text == sam and len(records) == 2 * len(frags)
        assert {r["l_seq"] for r in records} == {150} and {r["flag"] & 0x10 for r in records} == {0, 0x10}
    finally:
        c.close()


def members(data):
    """the gzip members of `data`: [(its bytes, its content)]"""
    out = []
    while data:
        d = zlib.decompressobj(31)
        content = d.decompress(data)
        assert d.eof
        out.append((data[:len(data) - len(d.unused_data)], content))
        data = d.unused_data
    return out


def test_command_line(workdir):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    c = tiny_case(workdir, replace_n_seed=7, base_identifier="ReseqRead")          # the API's bytes of the same run: the command's seed (also ReplaceN's), pair count and base identifier
    try:
        frags, f1, f2, bam = c.sim.pairs_bam(1, c.tb + 1)
        a1, a2, abam = c.sim.adapter_only_pairs_bam(0, c.info.adapter_only_pairs)
        header, names, fpath, ppath = c.ref.bam_header(), c.names, c.fpath, c.ppath
    finally:
        c.close()
    assert len(frags) > 2000 and len(a1) > 0
    out = {k: str(workdir / f"truth_bam_cli_{k}") for k in ("p1", "p2", "b1", "b2", "bam", "t1", "t2", "tbam", "tsam", "x1", "x2", "xbam")}
    common = [exe, "illuminaPE", "-R", fpath, "-s", ppath, "--numReads", "3000", "--seed", "7"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True)
    read = lambda path: open(path, "rb").read()
    assert run(["-1", out["p1"], "-2", out["p2"]]).returncode == 0
    assert run(["-1", out["b1"], "-2", out["b2"], "--truthBam", out["bam"]]).returncode == 0
    r = run(["-1", out["t1"], "-2", out["t2"], "--truthBam", out["tbam"], "--truthSam", out["tsam"]])
    assert r.returncode == 0, r.stderr
    for m in "12":                                                 # the FASTQ files are unchanged by the option
        assert read(out["p" + m]) == read(out["b" + m]) == read(out["t" + m]) == (f1 + a1 if m == "1" else f2 + a2)
    for path in (out["bam"], out["tbam"]):
        packed = read(path)
        parts = members(packed)
        assert len(parts) >= 2 and all(m[3] == 4 and m[12:14] == b"BC" for m, _ in parts)          # BGZF: FEXTRA with the BC field
        assert packed.endswith(api.gzip_eof_member()) and parts[-1][1] == b""
        content = b"".join(text for _, text in parts)
        assert content == header + bam + abam
        text, refs, used = decode_bam_header(content)
        assert [n for n, _ in refs] == names and used == len(header)
        assert text + decode_bam(content[used:], names)[0] == read(out["tsam"])          # the --truthSam file of the same run, header text included
    # refusals: nothing is simulated, no file is left
    for extra, message in ((["--gpus", "2"], "one worker only"), (["-V", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test-var.vcf")], "variants"),
                           (["--hostGzip"], "hostGzip")):
        r = run(["-1", out["x1"], "-2", out["x2"], "--truthBam", out["xbam"]] + extra)
        assert r.returncode != 0 and message in r.stderr, r.stderr
        assert not any(os.path.exists(p) for p in (out["x1"], out["x2"], out["xbam"]))
