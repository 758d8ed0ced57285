"""The simulation report on the device (rsq_sim_stats_*, `reseq illuminaPE --simStats`; reseq_amd/csrc/rsq_stats.h): the tables a run accumulates against
tests/sim_stats.py applied to the texts the same calls write -- the call's own fragments and FASTQ texts (every table but mismatch) and its SAM text with XC, XE
and MD (every table but fragment_length) -- whatever call simulates the pairs, however the blocks are cut and whatever the testing options say.  Every count is
exact: a seam bug shows as a count off by one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim_stats
from reseq_amd import api, synth
from test_truth_sam_gpu import Case, tiny_case
from test_truth_variants_gpu import VarCase
from truth_depth import depth_from_sam

pytestmark = pytest.mark.gpu

KERNELS = ("stats_rows", "stats_mates")


def dims_of(sim):
    y = sim.stats_layout()
    return (int(y.read_length[0]), int(y.read_length[1])), int(y.insert_to), int(y.n_quality), int(y.n_tiles), int(y.phred_offset)


def run_stats(sim, simulate):
    """a stats run around simulate(): (the tables, what simulate returned, the two kernels' launches of the last call, the dimensions)"""
    sim.stats_begin()
    try:
        out = simulate()
        launches = tuple(sim.last_kernel_launches(k) for k in KERNELS)
        return sim.stats(), out, launches, dims_of(sim)
    finally:
        sim.stats_end()


def same(got, want, names=sim_stats.TABLES):
    for name in names:
        assert got[name].dtype == np.uint64 and got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        assert (got[name] == want[name]).all(), (name, np.argwhere(got[name] != want[name])[:8].tolist())
    return True


def statements(case, out, dims, tiles):
    """(the tables from the fragments and the FASTQ texts, the tables from the SAM text) of one pairs_sam call, or of several calls' texts joined"""
    frags, f1, f2, sam = out
    lengths, F, Q, T, phred = dims
    assert phred == case.phred_offset and T == len(tiles)
    return sim_stats.from_fastq(frags, f1, f2, lengths, F, Q, T, phred, tiles), sim_stats.from_sam(sam, lengths, F, Q, T, tiles)


def check_call(case, got, out, dims, tiles):
    """every table equals both statements (mismatch: the SAM side; fragment_length: the fragments), and the tables agree among themselves"""
    fq, sm = statements(case, out, dims, tiles)
    same(got, fq, [n for n in sim_stats.TABLES if n != "mismatch"])
    same(got, sm, [n for n in sim_stats.TABLES if n != "fragment_length"])
    L = max(dims[0])
    longer = np.cumsum(got["read_length"][:, ::-1], axis=1)[:, ::-1]              # reads of length >= p ...
    for s in (0, 1):
        for p in range(L):                                                       # ... so longer[s][p + 1] is the reads with a base at cycle p
            assert int(got["base_quality"][s, p].sum()) == int(got["base_call"][s, p].sum()) == int(longer[s, p + 1]), (s, p)
    assert int(got["pairs"].sum()) == len(out[0]) and int(got["strand"].sum()) == int(got["tile"].sum()) == int(got["fragment_length"].sum()) == int(got["pairs"][0])
    assert not got["bad"][0]
    return sm


@pytest.fixture(scope="module")
def tiny(workdir):
    """TINY over all blocks through pairs_sam with truth_md on and a run open: the reference every test below shares"""
    c = tiny_case(workdir)
    c.tiles = synth.TINY["tiles"]
    c.sim.truth_md(True)
    c.got, c.whole, c.launches, c.dims = run_stats(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1))
    yield c
    c.close()


def test_equals_the_statements(tiny):
    frags, f1, f2, sam = tiny.whole
    assert 2000 < len(frags) < 4000 and tiny.launches == (1, 1)
    lengths, F, Q, T, phred = tiny.dims
    assert 20 < max(lengths) <= synth.TINY["read_len_max"] + 1 and 40 < F <= synth.TINY["ins_to"] and Q == synth.TINY["qual_to"] and T == 3 and phred == 33
    got = tiny.got
    check_call(tiny, got, tiny.whole, tiny.dims, tiny.tiles)
    # a change of TINY must not quietly weaken the tests: the classes the case has to meet
    assert np.count_nonzero(got["read_length"][0]) > 3 and np.count_nonzero(got["read_length"][1]) > 3, "several read lengths"
    assert all(int(got[name].sum()) > 0 for name in ("insertion", "deletion", "adapter", "tail")), "I, D, S and H"
    assert int(got["pairs"][0]) > 0 and (got["strand"] > 0).all(), "both strands"
    assert int(got["base_call"][:, :, 4].sum()) > 0, "an N call"
    reverse = [l.split(b"\t") for l in sam.splitlines() if int(l.split(b"\t")[1]) & 0x10]
    assert any(not l[-1][5:].isdigit() for l in reverse) and int(got["mismatch"].sum()) > 0, "mismatches on a reverse mate"
    assert (got["tile"] > 0).all() and got["base_quality"][:, :, 2].any() and got["base_quality"][:, :, Q - 1].any()


def test_other_seeds_and_the_adapter_only_class(tiny, workdir):
    """The class "an adapter-only pair" -- a pair whose Fragment::len is 0 inside a pairs call -- is met by no seed of TINY: the sieve of this case emits no such
    fragment under seed 7 nor under 17, 3, 5, 11 or 23 (pairs[1] == 0 in all of them; the adapter-only pairs of a run come from rsq_sim_adapter_only_pairs, which
    the report does not count).  The class is met on crafted rows by tests/test_sim_stats.py test_an_adapter_only_pair (a pair without a fragment, and a fragment
    of length 0).  Here two of those seeds are held to the statements as well, and a seed that does simulate such a pair is held to them like any other."""
    assert int(tiny.got["pairs"][1]) == 0, "TINY now simulates a fragment of length 0: assert the class in test_equals_the_statements and drop this note"
    for seed in (17, 3):
        c = Case(workdir, "tiny_e2e", synth.TINY, [5000, 80, 3210], seed, 3000)
        try:
            c.sim.truth_md(True)
            got, out, _, dims = run_stats(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1))
            check_call(c, got, out, dims, synth.TINY["tiles"])
            assert int(got["pairs"].sum()) == len(out[0]) > 2000
        finally:
            c.close()


def test_the_call_does_not_matter(tiny, workdir):
    from test_truth_bam_sorted_gpu import run_sorted
    sim, tb = tiny.sim, tiny.tb
    got, out, launches, _ = run_stats(sim, lambda: sim.pairs(1, tb + 1))
    assert same(got, tiny.got) and launches == (1, 1) and out[1:] == tiny.whole[1:3]
    got, out, launches, _ = run_stats(sim, lambda: sim.pairs_bam(1, tb + 1))
    assert same(got, tiny.got) and launches == (1, 1)
    got, out, _, _ = run_stats(sim, lambda: run_sorted(sim, [1, 2, 7, tb + 1]))
    assert same(got, tiny.got) and (out[2], out[3]) == tiny.whole[1:3]
    # with no run open: no launch, and the bytes of a simulator that never began a run
    pf, p1, p2 = sim.pairs(1, tb + 1)
    assert all(sim.last_kernel_launches(k) == 0 for k in KERNELS)
    after = sim.pairs_sam(1, tb + 1)
    assert all(sim.last_kernel_launches(k) == 0 for k in KERNELS)
    fresh = tiny_case(workdir)
    try:
        fresh.sim.truth_md(True)
        ff, f1, f2 = fresh.sim.pairs(1, tb + 1)
        fs = fresh.sim.pairs_sam(1, tb + 1)
    finally:
        fresh.close()
    assert (pf.tobytes(), p1, p2) == (ff.tobytes(), f1, f2) and after[1:] == fs[1:] == tiny.whole[1:] and after[0].tobytes() == fs[0].tobytes()


def test_block_cuts_and_snapshots(tiny):
    """blocks cut as [1, 4, tb + 1]: a snapshot after the first cut is the statement of the first cut alone, the final one the whole"""
    sim, tb = tiny.sim, tiny.tb
    sim.stats_begin()
    try:
        first = sim.pairs_sam(1, 4)
        snap = sim.stats()
        assert len(first[0]) > 0
        check_call(tiny, snap, first, tiny.dims, tiny.tiles)
        rest = sim.pairs_sam(4, tb + 1)
        assert len(rest[0]) > 0 and first[3] + rest[3] == tiny.whole[3]
        assert same(sim.stats(), tiny.got) and same(sim.stats(), tiny.got), "a snapshot changes nothing"
    finally:
        sim.stats_end()


@pytest.mark.parametrize("options", [{"overlap": 3}, {"image_tiles": 1}, {"stats_chunk": 4, "stats_slab": 64, "stats_groups": 3}, {"stats_form": 1, "stats_chunk": 8, "stats_groups": 40}])
def test_options(tiny, workdir, rsq_options, options):
    for k, v in options.items():
        rsq_options(k, v)
    c = tiny_case(workdir)
    try:
        if "image_tiles" in options:
            assert c.sim.fill_plan()["image_tiles"] == 1
        c.sim.truth_md(True)
        got, out, launches, _ = run_stats(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1))
        assert same(got, tiny.got) and launches == (1, 1) and out[3] == tiny.whole[3]
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
        assert rc == api.RSQ_ENOSPC and ls == len(sam) and all(sim.last_kernel_launches(k) == 0 for k in KERNELS)
        assert not any(v.any() for v in sim.stats().values())
        n, l1, l2, ls, rc = sim.pairs_sam_device(1, tb + 1, r1, r2, full)
        assert rc == api.RSQ_OK and full.to_numpy(np.uint8, ls).tobytes() == sam

    try:
        got, _, launches, _ = run_stats(sim, sam_calls)
        assert same(got, tiny.got) and launches == (1, 1)
    finally:
        for d in (r1, r2, short, full):
            d.free()


def test_a_depth_run_and_a_stats_run_together(tiny):
    sim, tb = tiny.sim, tiny.tb
    lengths = sim.sequence_lengths()
    sim.depth_begin()
    try:
        got, out, launches, _ = run_stats(sim, lambda: sim.pairs_sam(1, tb + 1))
        assert sim.last_kernel_launches("depth_add") == 1 and launches == (1, 1)
        sim.depth_finish()
        depths = [sim.depth(s) for s in range(len(lengths))]
    finally:
        sim.depth_end()
    assert same(got, tiny.got) and out[3] == tiny.whole[3]
    want = depth_from_sam(tiny.whole[3], lengths, tiny.names)
    assert all((d == w).all() for d, w in zip(depths, want)) and sum(int(w.sum()) for w in want) > 0


@pytest.mark.parametrize("mode", ["variants", "alleles"])
def test_a_reference_with_variants(workdir, mode):
    """mismatch equals the MD-derived statement (the records of rsq_sim_truth_variants), the other tables theirs; with rsq_sim_truth_alleles on, the calls write
    other records and the report is the same"""
    c = VarCase(workdir, "stats_main", 7, 31)
    try:
        c.sim.truth_md(True)
        got, out, launches, dims = run_stats(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1))
        sm = check_call(c, got, out, dims, synth.TINY["tiles"])
        cigars = [l.split(b"\t")[5] for l in out[3].splitlines()]
        assert launches == (1, 1) and sum(b"D" in x for x in cigars) > 100 and sum(b"I" in x for x in cigars) > 100 and int(sm["mismatch"].sum()) > 100
        if mode == "alleles":
            c.sim.truth_md(False)
            c.sim.truth_variants(False)
            c.sim.truth_alleles(True)
            in_alleles, out_alleles, _, _ = run_stats(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1))
            assert same(in_alleles, got) and out_alleles[1:3] == out[1:3] and out_alleles[3] != out[3]
    finally:
        c.close()


def test_tiles_at_150_cycles(workdir, rsq_options):
    """P0 with three tiles: 151 x (Q + 5) counters exceed one default chunk of the rows kernel, the reads are binned by tile, the tile table matches"""
    cfg = synth.p0_with_tiles(3)
    c = Case(workdir, "p0_tiles3", cfg, [30000], 11, 1500, prof_seed=21, ref_seed=2)
    try:
        c.sim.truth_md(True)
        got, out, launches, dims = run_stats(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1))
        lengths, F, Q, T, phred = dims
        assert lengths[0] > 64 and T == 3 and launches == (1, 1) and 1000 < len(out[0]) < 2500, "more positions than the largest chunk holds"
        check_call(c, got, out, dims, cfg["tiles"])
        assert (got["tile"] > 0).all() and int(got["base_quality"][:, lengths[0] - 2].sum()) > 0, "the last cycle lies in the last chunk"
    finally:
        c.close()


def test_state(tiny):
    sim, L = tiny.sim, api.lib()
    error = lambda: L.rsq_last_error().decode()
    layout = api.StatsLayout()
    assert L.rsq_sim_stats_layout(sim.h, C.byref(layout)) == api.RSQ_ESTATE and L.rsq_sim_stats_counts(sim.h, (C.c_uint64 * 8)(), 8, None) == api.RSQ_ESTATE
    sim.stats_begin()
    try:
        assert L.rsq_sim_stats_begin(sim.h) == api.RSQ_ESTATE and "open" in error()
        n, b1, b2 = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert L.rsq_sim_job_generate(sim.h, 1, 2, 0, C.byref(n), C.byref(b1), C.byref(b2), None) == api.RSQ_ESTATE and "stats run" in error()
        assert L.rsq_sim_job_compress(sim.h, C.byref(b1), C.byref(b2)) == api.RSQ_ESTATE
        assert L.rsq_sim_stats_counts(sim.h, (C.c_uint64 * 8)(), 8, None) == api.RSQ_ENOSPC
        assert len(sim.adapter_only_pairs(0, 50)[0]) > 0 and all(sim.last_kernel_launches(k) == 0 for k in KERNELS)      # the adapter-only calls are not counted
        assert not any(v.any() for v in sim.stats().values()), "no pairs call: all zero"
        offsets = sorted((int(t.offset), int(t.segments) * int(t.dim[0]) * int(t.dim[1])) for t in sim.stats_layout().table)
        assert offsets[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(offsets, offsets[1:])) and sum(offsets[-1]) == sim.stats_layout().words, "the tables tile the array"
    finally:
        sim.stats_end()
    sim.stats_end()                                               # without a run: nothing to free
    assert len(sim.pairs(1, 2)[0]) > 0
    prof, ref = api.Profile(tiny.ppath), api.Reference(tiny.fpath, 0)
    raw = api.Simulator(prof, ref, 0)
    try:
        assert L.rsq_sim_stats_begin(raw.h) == api.RSQ_ESTATE
    finally:
        raw.close()
        ref.close()
        prof.close()


def test_command_line(tiny, workdir):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    out = {k: str(workdir / f"stats_cli_{k}") for k in ("p1", "p2", "plain", "g1", "g2", "gz", "t1", "t2", "both", "sam", "bam", "d1", "d2", "with_depth", "dsam", "depth",
                                                         "x1", "x2", "x")}
    common = [exe, "illuminaPE", "-R", tiny.fpath, "-s", tiny.ppath, "--numReads", "3000", "--seed", "7", "--batchBlocks", "3"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True)
    r = run(["-1", out["p1"], "-2", out["p2"], "--simStats", out["plain"]])
    assert r.returncode == 0, r.stderr
    assert run(["-1", out["g1"], "-2", out["g2"], "--simStats", out["gz"] + ".gz", "-j", "1"]).returncode == 0
    # a batch is simulated once for --truthSam and once for --truthBam: counted once
    r = run(["-1", out["t1"], "-2", out["t2"], "--simStats", out["both"], "--truthSam", out["sam"], "--truthBam", out["bam"], "--truthMD"])
    assert r.returncode == 0, r.stderr
    # --truthDepth takes one of the two truth outputs beside it
    r = run(["-1", out["d1"], "-2", out["d2"], "--simStats", out["with_depth"], "--truthSam", out["dsam"], "--truthDepth", out["depth"]])
    assert r.returncode == 0, r.stderr
    read = lambda path: open(path, "rb").read()
    text = read(out["plain"])
    assert text.startswith(b"#reseq_amd simStats v1\n#read_length\t%d\t%d\n#insert_to\t%d\n#n_quality\t%d\n#n_tiles\t3\n#phred_offset\t33\n" % (tiny.dims[0] + tiny.dims[1:3])) and read(out["both"]) == text == read(out["with_depth"])
    assert read(out["gz"] + ".gz")[:2] == b"\x1f\x8b" and sim_stats.report_tables(out["gz"] + ".gz")[1].keys() == tiny.got.keys()
    # the report parses back to the API's arrays for the same seed: the block calls' pairs (the adapter-only calls are not counted)
    for path in (out["plain"], out["gz"] + ".gz"):
        dims, tables = sim_stats.report_tables(path)
        assert (tuple(dims["read_length"]), dims["insert_to"][0], dims["n_quality"][0], dims["n_tiles"][0], dims["phred_offset"][0]) == tiny.dims
        same(tables, tiny.got)
    # refusals: nothing is simulated, no file is left
    for extra, message in ((["--simStats", out["x"], "--gpus", "2"], "one worker only"), (["--simStats", out["x"] + ".bz2"], "bzip2")):
        r = run(["-1", out["x1"], "-2", out["x2"]] + extra)
        assert r.returncode != 0 and "--simStats" in r.stderr and message in r.stderr, r.stderr
        assert not any(os.path.exists(p) for p in (out["x1"], out["x2"], out["x"], out["x"] + ".bz2"))
