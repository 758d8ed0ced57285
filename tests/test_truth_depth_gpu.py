"""Truth depth on the device (rsq_sim_depth_*, `reseq illuminaPE --truthDepth`; reseq_amd/csrc/rsq_depth.h): the depth a run accumulates against
tests/truth_depth.py depth_from_sam applied to the SAM text rsq_sim_pairs_sam writes for the same pairs (which the truth tests check against their own
statements), whatever call simulates the pairs and however the blocks are cut; the bedGraph text against bedgraph_from_depth, however the sequence is cut."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from reseq_amd import api, synth
from test_truth_md_gpu import GoldenCase
from test_truth_sam_gpu import Case, inflate_members, long_name_case, tiny_case
from test_truth_variants_gpu import VarCase
from truth_depth import bedgraph_from_depth, depth_from_sam

pytestmark = pytest.mark.gpu

TILE = 4096


def run_depth(sim, simulate, text=False):
    """a depth run around simulate(): ([depth per sequence], what simulate returned, depth_add launches of the last call[, the bedGraph text])"""
    sim.depth_begin()
    try:
        out = simulate()
        launches = sim.last_kernel_launches("depth_add")
        sim.depth_finish()
        assert sim.last_kernel_launches("depth_scan") == 1
        depths = [sim.depth(s) for s in range(len(sim.sequence_lengths()))]
        return (depths, out, launches, sim.depth_bedgraph()) if text else (depths, out, launches)
    finally:
        sim.depth_end()


def same(a, b):
    return len(a) == len(b) and all(x.dtype == np.uint32 and x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def records_depth(case, sam):
    return depth_from_sam(sam, case.sim.sequence_lengths(), case.names)


@pytest.fixture(scope="module")
def tiny(workdir):
    """TINY over all blocks through pairs_sam with a run open: the reference every test below shares"""
    c = tiny_case(workdir)
    c.depths, c.whole, c.launches, c.text = run_depth(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1), text=True)
    c.want = records_depth(c, c.whole[3])
    yield c
    c.close()


def test_equals_the_records(tiny):
    frags, f1, f2, sam = tiny.whole
    assert 2000 < len(frags) < 4000 and [len(d) for d in tiny.depths] == [5000, 80, 3210]
    assert same(tiny.depths, tiny.want)
    # a change of TINY must not quietly weaken the tests: the classes the case has to meet
    lines = [l.split(b"\t") for l in sam.splitlines()]
    cigars = [f[5] for f in lines]
    assert any(b"D" in c for c in cigars) and any(b"I" in c for c in cigars)
    assert {int(f[1]) & 0x10 for f in lines} == {0, 0x10}, "both strands"
    assert max(int(d.max()) for d in tiny.want) >= 2, "overlapping mates"
    assert any((d == 0).any() for d in tiny.want), "a zero-depth run"


def test_depth_on_the_first_base_of_a_sequence(workdir):
    """The class "non-zero depth on the first and on the last base of some sequence" is not met by TINY's own seed (7: its coverage begins at positions 4 and 1 and
    ends at 4992 and 3204), so the first base is met here, by the same case under seed 17 (fragments start at position 0 of sequences 0 and 2).  The LAST base is
    met by no simulated case: over seeds 1 .. 59 of this case the host emulation places no fragment that ends at its sequence's end (the largest end lies 5 bases
    in front of it).  That class -- the -1 on a sequence's extra word -- is met by tests/test_truth_depth.py (a crafted read that reaches the last base, every
    sequence, both strands) and, for the array's layout on the device, by test_scan_seams below."""
    c = Case(workdir, "tiny_e2e", synth.TINY, [5000, 80, 3210], 17, 3000)
    try:
        got, out, _ = run_depth(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1))
        want = records_depth(c, out[3])
        assert same(got, want) and want[0][0] > 0 and want[2][0] > 0
    finally:
        c.close()


def test_the_truth_call_does_not_matter(tiny, workdir):
    from test_truth_bam_sorted_gpu import run_sorted
    sim, tb = tiny.sim, tiny.tb
    assert tiny.launches == 1
    plain, out, launches = run_depth(sim, lambda: sim.pairs(1, tb + 1))
    assert same(plain, tiny.want) and launches == 1 and out[1:] == tiny.whole[1:3]
    bam, out, launches = run_depth(sim, lambda: sim.pairs_bam(1, tb + 1))
    assert same(bam, tiny.want) and launches == 1
    sorted_, out, _ = run_depth(sim, lambda: run_sorted(sim, [1, 2, 7, tb + 1]))
    assert same(sorted_, tiny.want) and (out[2], out[3]) == tiny.whole[1:3]
    # with no run open: no launch, and the bytes of a simulator that never began a run
    pf, p1, p2 = sim.pairs(1, tb + 1)
    assert sim.last_kernel_launches("depth_add") == 0 and all(sim.last_kernel_launches(k) == 0 for k in ("depth_scan", "depth_lines", "depth_text"))
    after = sim.pairs_sam(1, tb + 1)
    assert sim.last_kernel_launches("depth_add") == 0
    fresh = tiny_case(workdir)
    try:
        ff, f1, f2 = fresh.sim.pairs(1, tb + 1)
        fs = fresh.sim.pairs_sam(1, tb + 1)
    finally:
        fresh.close()
    assert (pf.tobytes(), p1, p2) == (ff.tobytes(), f1, f2) and after[1:] == fs[1:] == tiny.whole[1:] and after[0].tobytes() == fs[0].tobytes()


@pytest.mark.parametrize("option,value", [("cuts", 0), ("overlap", 3), ("image_tiles", 1)])
def test_cuts_and_options(tiny, workdir, rsq_options, option, value):
    if option != "cuts":
        rsq_options(option, value)
    c = tiny_case(workdir)
    try:
        if option == "image_tiles":
            assert c.sim.fill_plan()["image_tiles"] == 1
        bounds = [1, 4, c.tb + 1] if option == "cuts" else [1, c.tb + 1]
        got, out, _ = run_depth(c.sim, lambda: [c.sim.pairs_sam(lo, hi) for lo, hi in zip(bounds, bounds[1:])])
        assert same(got, tiny.want)
        assert b"".join(o[3] for o in out) == tiny.whole[3] and all(len(o[0]) for o in out)
    finally:
        c.close()


def test_enospc_then_repeat(tiny):
    """a call that returns RSQ_ENOSPC adds nothing: repeated with room, its pairs count once"""
    frags, f1, f2, sam = tiny.whole
    sim, dev, tb = tiny.sim, tiny.sim.device, tiny.tb
    r1, r2 = api.DeviceArray(dev, len(f1)), api.DeviceArray(dev, len(f2))
    short, full = api.DeviceArray(dev, len(sam) - 1), api.DeviceArray(dev, len(sam))

    def sam_calls():
        n, l1, l2, ls, rc = sim.pairs_sam_device(1, tb + 1, r1, r2, short)
        assert rc == api.RSQ_ENOSPC and ls == len(sam) and sim.last_kernel_launches("depth_add") == 0
        n, l1, l2, ls, rc = sim.pairs_sam_device(1, tb + 1, r1, r2, full)
        assert rc == api.RSQ_OK and full.to_numpy(np.uint8, ls).tobytes() == sam and sim.last_kernel_launches("depth_add") == 1

    def sorted_calls():
        sim.bam_sorted_begin(0)
        n, l1, l2, ls, nr, rc = sim.pairs_bam_sorted_device(1, tb + 1, None, None, None)
        assert rc == api.RSQ_ENOSPC and ls > 1
        tight, room = api.DeviceArray(dev, ls - 1), api.DeviceArray(dev, ls)
        try:
            assert sim.pairs_bam_sorted_device(1, tb + 1, r1, r2, tight)[5] == api.RSQ_ENOSPC and sim.last_kernel_launches("depth_add") == 0
            got = sim.pairs_bam_sorted_device(1, tb + 1, r1, r2, room)
            assert got[5] == api.RSQ_OK and got[3] == ls and sim.last_kernel_launches("depth_add") == 1
        finally:
            tight.free()
            room.free()
        sim.bam_sorted_flush()

    try:
        assert same(run_depth(sim, sam_calls)[0], tiny.want)
        assert same(run_depth(sim, sorted_calls)[0], tiny.want)
    finally:
        for d in (r1, r2, short, full):
            d.free()


# ------------------------------------------------------------------------------------------------ variants
def counting_deletions(sam):
    """the same records with every D element read as M: what the depth would be if deletions counted"""
    lines = []
    for line in sam.splitlines():
        f = line.split(b"\t")
        f[5] = f[5].replace(b"D", b"M")
        lines.append(b"\t".join(f))
    return b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("kind", ["mixed", "ends", "subs", "golden"])
def test_variants(workdir, kind):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    c = {"mixed": lambda: VarCase(workdir, "depth_main", 7, 31), "ends": lambda: VarCase(workdir, "depth_ends", 11, 43, ends=40),
         "subs": lambda: VarCase(workdir, "depth_subs", 7, 17, kind="subs"), "golden": lambda: GoldenCase(workdir, golden)}[kind]()
    try:
        got, out, launches = run_depth(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1))
        frags, f1, f2, sam = out
        want = records_depth(c, sam)
        assert len(frags) > 1000 and launches == 1 and same(got, want)
        # rsq_sim_truth_variants only authorises the truth calls: the plain call accumulates the same depth without it
        c.sim.truth_variants(False)
        plain, _, _ = run_depth(c.sim, lambda: c.sim.pairs(1, c.tb + 1))
        assert same(plain, want)
        with_d = records_depth(c, counting_deletions(sam))
        if kind in ("mixed", "ends"):                             # positions an allele deleted: fewer counts than if D were counted
            cigars = [l.split(b"\t")[5] for l in sam.splitlines()]
            assert sum(b"D" in x for x in cigars) > 100 and sum(b"I" in x for x in cigars) > 100
            fewer = [int((w < d).sum()) for w, d in zip(want, with_d)]
            assert sum(fewer) > 10, fewer
            s = int(np.argmax(fewer))
            p = int(np.flatnonzero(want[s] < with_d[s])[0])
            assert got[s][p] == want[s][p] < with_d[s][p]
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ the prefix sum's seams
def test_scan_seams(workdir):
    """sequence ends on, one before and one behind a tile boundary of the flat array (a word per base and one per sequence), and more tiles than the tile-sums
    scan has threads"""
    lengths = [TILE * 1025 - 1, TILE, TILE]
    # flat: sequence 0's extra word is the last of tile 1024, sequence 1 begins ON the boundary and its extra word lies on the next one, sequence 2 begins one behind
    # it and its last base lies on a boundary
    starts = np.cumsum([0] + [n + 1 for n in lengths])
    assert (starts[1] - 1) % TILE == TILE - 1 and starts[1] % TILE == 0 and (starts[1] + lengths[1]) % TILE == 0 and starts[2] % TILE == 1 and (starts[2] + lengths[2] - 1) % TILE == 0
    assert sum(lengths) > TILE * 1024
    c = Case(workdir, "depth_seams", synth.TINY, lengths, 7, 4000)
    try:
        c.sim.depth_begin()
        out = c.sim.pairs_sam(1, c.tb + 1)
        c.sim.depth_finish()
        want = records_depth(c, out[3])
        assert 2000 < len(out[0]) < 6000 and same([c.sim.depth(s) for s in range(3)], want)
        assert all(int(w.sum()) > 0 for w in want), "reads on every sequence"
        # windows in any order, at any place
        for s, lo, hi in ((2, 1000, 1001), (0, TILE * 1024 - 3, lengths[0]), (1, 0, TILE), (0, 0, 5), (1, 77, 77)):
            assert (c.sim.depth(s, lo, hi) == want[s][lo:hi]).all()
    finally:
        c.sim.depth_end()
        c.close()


# ------------------------------------------------------------------------------------------------ bedGraph
def pieces_text(sim, seq, length, piece):
    """the sequence's text fetched in pieces of `piece` positions through the device call, with room for each; the lines' total"""
    out, lines, dst = [], 0, api.DeviceArray(sim.device, 1 << 20)
    try:
        for lo in range(0, length, piece):
            n, k, rc = sim.depth_bedgraph_device(seq, lo, min(lo + piece, length), dst)
            assert rc == api.RSQ_OK, (seq, lo, rc)
            out.append(dst.to_numpy(np.uint8, n).tobytes())
            lines += k
    finally:
        dst.free()
    return b"".join(out), lines


def test_bedgraph(tiny):
    sim, lengths = tiny.sim, tiny.sim.sequence_lengths()
    want = bedgraph_from_depth(tiny.names, tiny.want)
    assert tiny.text == want
    per_seq = [bedgraph_from_depth([n], [d]) for n, d in zip(tiny.names, tiny.want)]
    # the lines of each sequence tile [0, length)
    for name, text, length in zip(tiny.names, per_seq, lengths):
        rows = [l.split(b"\t") for l in text.splitlines()]
        assert all(r[0] == name for r in rows) and int(rows[0][1]) == 0 and int(rows[-1][2]) == length
        assert all(int(a[2]) == int(b[1]) and a[3] != b[3] for a, b in zip(rows, rows[1:])) and all(int(r[1]) < int(r[2]) for r in rows)
    # the inputs: runs that cross a piece seam, runs that end exactly at one
    d = tiny.want[0]
    seams = np.concatenate([np.arange(piece, len(d), piece) for piece in (7, TILE, TILE + 1)])
    assert (d[seams] == d[seams - 1]).any() and (d[seams] != d[seams - 1]).any()
    sim.depth_begin()
    try:
        sim.pairs(1, tiny.tb + 1)
        sim.depth_finish()
        for piece, seqs in ((1, (1, 2)), (7, (0, 1, 2)), (TILE, (0, 1, 2)), (TILE + 1, (0, 1, 2)), (1 << 30, (0, 1, 2))):
            for s in seqs:
                text, lines = pieces_text(sim, s, lengths[s], piece)
                assert text == per_seq[s] and lines == len(per_seq[s].splitlines()), (piece, s)
        assert sim.last_kernel_launches("depth_text") == 1 and sim.last_kernel_launches("depth_lines") >= 1
        # RSQ_ENOSPC leaves the carried start unchanged: the piece can be repeated, and the next one continues it
        big = api.DeviceArray(sim.device, 1 << 20)
        try:
            cut = int(np.flatnonzero(d[1:] == d[:-1])[5]) + 1                    # a seam inside a run
            first = sim.depth_bedgraph_device(0, 0, cut, big)
            head = big.to_numpy(np.uint8, first[0]).tobytes()
            need, lines, rc = sim.depth_bedgraph_device(0, cut, lengths[0], None)
            assert rc == api.RSQ_ENOSPC and need == len(per_seq[0]) - len(head) and lines == len(per_seq[0].splitlines()) - first[1]
            small = api.DeviceArray.from_numpy(sim.device, np.full(need - 1, 0xA7, np.uint8))
            assert sim.depth_bedgraph_device(0, cut, lengths[0], small)[2] == api.RSQ_ENOSPC and (small.to_numpy(np.uint8, need - 1) == 0xA7).all()
            small.free()
            n, _, rc = sim.depth_bedgraph_device(0, cut, lengths[0], big)
            assert rc == api.RSQ_OK and head + big.to_numpy(np.uint8, n).tobytes() == per_seq[0]
            # a piece that does not continue the one before: RSQ_ESTATE; lo == 0 always restarts
            assert sim.depth_bedgraph_device(0, 0, 100, big)[2] == api.RSQ_OK
            assert sim.depth_bedgraph_device(0, 101, 200, big)[2] == api.RSQ_ESTATE
            assert sim.depth_bedgraph_device(2, 100, 200, big)[2] == api.RSQ_ESTATE
            assert sim.depth_bedgraph_device(0, 100, 200, big)[2] == api.RSQ_OK
            assert sim.depth_bedgraph_device(0, 100, 200, big)[2] == api.RSQ_ESTATE
            assert sim.depth_bedgraph_device(0, 0, lengths[0] + 1, big)[2] == api.RSQ_EINVAL and sim.depth_bedgraph_device(3, 0, 1, big)[2] == api.RSQ_EINVAL
            n, _, rc = sim.depth_bedgraph_device(2, 0, lengths[2], big)
            assert rc == api.RSQ_OK and big.to_numpy(np.uint8, n).tobytes() == per_seq[2]
        finally:
            big.free()
        # windows of the counts, in any order
        for s, lo, hi in ((2, 1000, 1001), (0, 4990, 5000), (1, 0, 80), (0, 0, 5), (1, 77, 77)):
            assert (sim.depth(s, lo, hi) == tiny.want[s][lo:hi]).all()
        assert sim.depth_counts_device(0, 10, 5001, big) == api.RSQ_EINVAL
    finally:
        sim.depth_end()


@pytest.mark.parametrize("name_len", [150, 600])
def test_bedgraph_with_long_names(workdir, name_len):
    """64 lines with a name of 150 characters fit the writer's image of at most 32 KiB, with one of 600 they do not and every lane writes its line straight to
    memory: both routes write the same lines"""
    c = long_name_case(workdir) if name_len == 150 else Case(workdir, "depth_long_name", synth.TINY, [6000], 7, 1500, names=["n" * 600 + " rest of the id"])
    try:
        got, out, _, text = run_depth(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1), text=True)
        want = records_depth(c, out[3])
        assert len(out[0]) > 1000 and same(got, want) and text == bedgraph_from_depth(c.names, want) and len(c.names[0]) == name_len
        assert 64 * (name_len + 34) + 16 > 32768 or name_len == 150
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ state
def test_state(tiny, workdir):
    sim, L = tiny.sim, api.lib()
    error = lambda: L.rsq_last_error().decode()
    assert L.rsq_sim_depth_finish(sim.h, None) == api.RSQ_ESTATE and sim.depth_counts_device(0, 0, 1, None) == api.RSQ_ESTATE
    assert sim.depth_bedgraph_device(0, 0, 1, None)[2] == api.RSQ_ESTATE
    sim.depth_begin()
    try:
        assert L.rsq_sim_depth_begin(sim.h) == api.RSQ_ESTATE and "open" in error()
        assert sim.depth_counts_device(0, 0, 1, None) == api.RSQ_ESTATE, "differences are no depths"
        n, b1, b2 = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert L.rsq_sim_job_generate(sim.h, 1, 2, 0, C.byref(n), C.byref(b1), C.byref(b2), None) == api.RSQ_ESTATE and "depth run" in error()
        assert L.rsq_sim_job_compress(sim.h, C.byref(b1), C.byref(b2)) == api.RSQ_ESTATE
        assert len(sim.adapter_only_pairs(0, 50)[0]) > 0 and sim.last_kernel_launches("depth_add") == 0      # adapter-only pairs are unmapped: nothing to add
        sim.depth_finish()
        assert L.rsq_sim_depth_finish(sim.h, None) == api.RSQ_ESTATE
        assert all(not sim.depth(s).any() for s in range(3)), "no pairs call: all zero"
        assert sim.depth_bedgraph() == b"".join(b"%s\t0\t%d\t0\n" % (name, n) for name, n in zip(tiny.names, sim.sequence_lengths()))
        assert sim.pairs_device(1, 2, None, None)[3] == api.RSQ_ESTATE and "rsq_sim_depth_end" in error()
        assert sim.pairs_sam_device(1, 2, None, None, None)[4] == api.RSQ_ESTATE and sim.pairs_bam_device(1, 2, None, None, None)[4] == api.RSQ_ESTATE
        sim.bam_sorted_begin(0)
        assert sim.pairs_bam_sorted_device(1, 2, None, None, None)[5] == api.RSQ_ESTATE
        sim.bam_sorted_flush()
    finally:
        sim.depth_end()
    sim.depth_end()                                               # without a run: nothing to free
    assert len(sim.pairs(1, 2)[0]) > 0
    # allele coordinates and a depth run exclude each other
    c = VarCase(workdir, "depth_state", 7, 31)
    try:
        c.sim.truth_variants(False)
        c.sim.depth_begin()
        assert L.rsq_sim_truth_alleles(c.sim.h, 1) == api.RSQ_ESTATE and "depth" in error()
        c.sim.depth_end()
        c.sim.truth_alleles(True)
        assert L.rsq_sim_depth_begin(c.sim.h) == api.RSQ_EINVAL and "allele" in error()
        c.sim.truth_alleles(False)
        c.sim.depth_begin()
        c.sim.depth_end()
    finally:
        c.close()
    # before rsq_sim_prepare
    prof, ref = api.Profile(tiny.ppath), api.Reference(tiny.fpath, 0)
    raw = api.Simulator(prof, ref, 0)
    try:
        assert L.rsq_sim_depth_begin(raw.h) == api.RSQ_ESTATE
    finally:
        raw.close()
        ref.close()
        prof.close()


# ------------------------------------------------------------------------------------------------ the command line
def test_command_line(tiny, workdir):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    out = {k: str(workdir / f"depth_cli_{k}") for k in ("p1", "p2", "s1", "s2", "sam", "sdepth", "n1", "n2", "ndepth", "g1", "g2", "gdepth", "x1", "x2", "xdepth", "xsam")}
    common = [exe, "illuminaPE", "-R", tiny.fpath, "-s", tiny.ppath, "--numReads", "3000", "--seed", "7", "--batchBlocks", "3"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True)
    read = lambda path: open(path, "rb").read()
    assert run(["-1", out["p1"], "-2", out["p2"]]).returncode == 0
    r = run(["-1", out["s1"], "-2", out["s2"], "--truthSam", out["sam"], "--truthDepth", out["sdepth"]])
    assert r.returncode == 0, r.stderr
    assert run(["-1", out["n1"], "-2", out["n2"], "--truthDepth", out["ndepth"]]).returncode == 0
    assert run(["-1", out["g1"], "-2", out["g2"], "--truthDepth", out["gdepth"] + ".gz", "-j", "1"]).returncode == 0
    for m in "12":
        assert read(out["p" + m]) == read(out["s" + m]) == read(out["n" + m]) == read(out["g" + m])
    sam = read(out["sam"])
    lengths = {m.group(1): int(m.group(2)) for m in re.finditer(rb"@SQ\tSN:(\S+)\tLN:(\d+)\n", sam)}
    assert list(lengths.values()) == [5000, 80, 3210]
    text = bedgraph_from_depth(list(lengths), depth_from_sam(sam, lengths))
    assert read(out["sdepth"]) == text and len(text.splitlines()) > 1000
    assert read(out["ndepth"]) == text
    packed = read(out["gdepth"] + ".gz")
    assert packed[3] == 4 and packed.endswith(api.gzip_eof_member()) and inflate_members(packed) == text      # BGZF members made on the device
    # refusals: nothing is simulated, no file is left
    golden_vcf = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test-var.vcf")
    for extra, message in ((["--truthDepth", out["xdepth"], "--gpus", "2"], "one worker only"), (["--truthDepth", out["xdepth"] + ".bz2"], "bzip2"),
                           (["--truthDepth", out["xdepth"], "--truthSam", out["xsam"], "-V", golden_vcf, "--truthAlleles"], "--truthAlleles"),
                           (["--truthDepth", out["xdepth"], "--truthSam", out["xsam"], "--truthBam", out["xsam"] + ".bam"], "at most one")):
        r = run(["-1", out["x1"], "-2", out["x2"]] + extra)
        assert r.returncode != 0 and "--truthDepth" in r.stderr and message in r.stderr, r.stderr
        assert not any(os.path.exists(p) for p in (out["x1"], out["x2"], out["xdepth"], out["xdepth"] + ".bz2", out["xsam"]))
