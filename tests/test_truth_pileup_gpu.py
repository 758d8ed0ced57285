"""Truth pileup on the device (rsq_sim_pileup_*, `reseq illuminaPE --truthPileup`; reseq_amd/csrc/rsq_pileup.h): the table a run accumulates against
tests/truth_pileup.py pileup_from_sam applied to the SAM text rsq_sim_pairs_sam writes for the same pairs (which the truth tests check against their own
statements), whatever call simulates the pairs and however the blocks are cut; the TSV text against pileup_text, however the sequence is cut; the depth column
against a depth run and the mismatches against a stats run open around the same call.  All comparisons are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from reseq_amd import api, synth
from test_truth_md_gpu import GoldenCase, letters_of
from test_truth_sam_gpu import Case, inflate_members, long_name_case, tiny_case
from test_truth_variants_gpu import VarCase
from truth_pileup import DEL, DEPTH, INS, header_line, pileup_from_sam, pileup_text

pytestmark = pytest.mark.gpu

KERNELS = ("pileup_add", "pileup_scan", "pileup_rows", "pileup_lines", "pileup_text")


def run_pileup(sim, simulate, strands=False, text=False):
    """a pileup run around simulate(): ([table per sequence], what simulate returned, pileup_add launches of the last call[, the sites' text, all rows' text])"""
    sim.pileup_begin(strands)
    try:
        out = simulate()
        launches = sim.last_kernel_launches("pileup_add")
        sim.pileup_finish()
        assert sim.last_kernel_launches("pileup_scan") == (2 if strands else 1), "once per strand set"
        tables = [sim.pileup(s) for s in range(len(sim.sequence_lengths()))]
        assert sim.last_kernel_launches("pileup_rows") == 1
        return (tables, out, launches, sim.pileup_text(), sim.pileup_text(all_rows=True)) if text else (tables, out, launches)
    finally:
        sim.pileup_end()


def same(a, b):
    return len(a) == len(b) and all(x.dtype == np.uint32 and x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def records_pileup(case, sam, strands):
    return pileup_from_sam(sam, dict(zip(case.names, letters_of(case))), strands)


def folded(tables):
    """forward + reverse as an unstranded table"""
    return [t.sum(axis=1, dtype=np.uint32)[:, None, :] for t in tables]


@pytest.fixture(scope="module")
def tiny(workdir):
    """TINY over all blocks through pairs_sam with a run open, unstranded and per strand: the reference every test below shares"""
    c = tiny_case(workdir)
    c.tables, c.whole, c.launches, c.sites, c.all_rows = run_pileup(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1), text=True)
    c.stranded, whole, _, c.s_sites, c.s_all_rows = run_pileup(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1), strands=True, text=True)
    assert whole[1:] == c.whole[1:]
    c.letters = letters_of(c)
    c.want = records_pileup(c, c.whole[3], False)
    c.s_want = records_pileup(c, c.whole[3], True)
    yield c
    c.close()


def test_equals_the_records(tiny):
    frags, f1, f2, sam = tiny.whole
    assert 2000 < len(frags) < 4000 and [t.shape for t in tiny.tables] == [(5000, 1, 8), (80, 1, 8), (3210, 1, 8)]
    assert [t.shape for t in tiny.stranded] == [(5000, 2, 8), (80, 2, 8), (3210, 2, 8)]
    assert same(tiny.tables, tiny.want) and same(tiny.stranded, tiny.s_want) and same(folded(tiny.stranded), tiny.tables)
    # a change of TINY must not quietly weaken the tests: the classes the case has to meet
    lines = [l.split(b"\t") for l in sam.splitlines()]
    cigars = [f[5] for f in lines]
    assert any(b"D" in c for c in cigars) and any(b"I" in c for c in cigars)
    assert {int(f[1]) & 0x10 for f in lines} == {0, 0x10}, "both strands"
    assert all(t[:, s].any() for t in tiny.s_want[::2] for s in (0, 1)), "counts on both strands"
    assert max(int(t[:, :, DEPTH].max()) for t in tiny.want) >= 2, "overlapping mates"
    assert any(t[:, :, INS].any() for t in tiny.want) and any(t[:, :, DEL].any() for t in tiny.want), "a row with ins > 0, one with del > 0"
    code = np.zeros(256, np.int64)
    code[list(b"ACGT")] = [1, 2, 3, 4]
    mismatches = sum(int(t[:, 0, 1:6].sum()) - int(t[np.arange(len(t)), 0, code[np.frombuffer(l, np.uint8)]].sum()) for t, l in zip(tiny.want, tiny.letters))
    assert mismatches > 100, "mismatches"


@pytest.mark.parametrize("kind", ["mixed", "ends", "subs", "golden"])
def test_variants(workdir, kind):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    c = {"mixed": lambda: VarCase(workdir, "depth_main", 7, 31), "ends": lambda: VarCase(workdir, "depth_ends", 11, 43, ends=40),
         "subs": lambda: VarCase(workdir, "depth_subs", 7, 17, kind="subs"), "golden": lambda: GoldenCase(workdir, golden)}[kind]()
    try:
        got, out, launches = run_pileup(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1))
        frags, f1, f2, sam = out
        want = records_pileup(c, sam, False)
        assert len(frags) > 1000 and launches == 1 and same(got, want)
        stranded, out2, _ = run_pileup(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1), strands=True)
        assert out2[3] == sam and same(stranded, records_pileup(c, sam, True)) and same(folded(stranded), got)
        # rsq_sim_truth_variants only authorises the truth calls: the plain call accumulates the same table without it
        c.sim.truth_variants(False)
        plain, _, _ = run_pileup(c.sim, lambda: c.sim.pairs(1, c.tb + 1))
        assert same(plain, want)
        if kind in ("mixed", "ends"):
            cigars = [l.split(b"\t")[5] for l in sam.splitlines()]
            assert sum(b"D" in x for x in cigars) > 100 and sum(b"I" in x for x in cigars) > 100
        if hasattr(c, "vcf"):
            # at a substitution variant's position the non-reference letter's count is non-zero
            letters, hits, candidates = letters_of(c), 0, 0
            index = {n: i for i, n in enumerate(c.names)}
            for line in open(c.vcf):
                f = line.split("\t")
                if line[:1] == "#" or len(f) < 5:
                    continue
                s, p = index[f[0].encode()], int(f[1]) - 1
                for alt in f[4].split(","):
                    if len(f[3]) == 1 and len(alt) == 1 and alt in "ACGT" and letters[s][p:p + 1] == f[3].encode() and got[s][p, 0, DEPTH] >= 8:
                        candidates += 1
                        hits += int(got[s][p, 0, 1 + "ACGT".index(alt)] > 0)
            assert hits >= 1 if candidates else kind != "subs", (hits, candidates)
    finally:
        c.close()


def test_cross_checks_between_the_three_runs(tiny):
    """depth, stats and pileup runs open around ONE call"""
    sim, tb = tiny.sim, tiny.tb
    for strands in (False, True):
        sim.depth_begin()
        sim.stats_begin()
        sim.pileup_begin(strands)
        try:
            out = sim.pairs_sam(1, tb + 1)
            assert out[1:] == tiny.whole[1:]
            assert [sim.last_kernel_launches(k) for k in ("depth_add", "stats_mates", "pileup_add")] == [1, 1, 1]
            report = sim.stats()
            sim.depth_finish()
            sim.pileup_finish()
            tables = [sim.pileup(s) for s in range(3)]
            depths = [sim.depth(s) for s in range(3)]
        finally:
            sim.pileup_end()
            sim.stats_end()
            sim.depth_end()
        assert same(tables, tiny.stranded if strands else tiny.tables)
        assert all((t[:, :, DEPTH].sum(axis=1, dtype=np.uint32) == d).all() for t, d in zip(tables, depths))
        code = np.zeros(256, np.int64)
        code[list(b"ACGT")] = [1, 2, 3, 4]
        non_ref = sum(int(t[:, :, 1:6].sum()) - int(t[np.arange(len(t)), :, code[np.frombuffer(l, np.uint8)]].sum()) for t, l in zip(tables, tiny.letters))
        assert int(report["bad"].sum()) == 0 and non_ref == int(report["mismatch"].sum()) > 0


def test_the_call_does_not_matter(tiny, workdir):
    from test_truth_bam_sorted_gpu import run_sorted
    sim, tb = tiny.sim, tiny.tb
    assert tiny.launches == 1
    plain, out, launches = run_pileup(sim, lambda: sim.pairs(1, tb + 1))
    assert same(plain, tiny.want) and launches == 1 and out[1:] == tiny.whole[1:3]
    bam, out, launches = run_pileup(sim, lambda: sim.pairs_bam(1, tb + 1), strands=True)
    assert same(bam, tiny.s_want) and launches == 1
    sorted_, out, _ = run_pileup(sim, lambda: run_sorted(sim, [1, 2, 7, tb + 1]))
    assert same(sorted_, tiny.want) and (out[2], out[3]) == tiny.whole[1:3]
    cut, out, launches = run_pileup(sim, lambda: [sim.pairs_sam(lo, hi) for lo, hi in zip([1, 2, 7], [2, 7, tb + 1])], strands=True)
    assert same(cut, tiny.s_want) and launches == 1 and b"".join(o[3] for o in out) == tiny.whole[3]


def test_no_run_open(tiny, workdir):
    """no launch of any pileup kernel, the bytes of a simulator that never began a run; depth and stats results do not change beside a pileup run"""
    sim, tb = tiny.sim, tiny.tb
    pf, p1, p2 = sim.pairs(1, tb + 1)
    assert all(sim.last_kernel_launches(k) == 0 for k in KERNELS)
    after = sim.pairs_sam(1, tb + 1)
    assert all(sim.last_kernel_launches(k) == 0 for k in KERNELS)
    fresh = tiny_case(workdir)
    try:
        ff, f1, f2 = fresh.sim.pairs(1, tb + 1)
        fs = fresh.sim.pairs_sam(1, tb + 1)
        assert all(fresh.sim.last_kernel_launches(k) == 0 for k in KERNELS)
    finally:
        fresh.close()
    assert (pf.tobytes(), p1, p2) == (ff.tobytes(), f1, f2) and after[1:] == fs[1:] == tiny.whole[1:] and after[0].tobytes() == fs[0].tobytes()

    def depth_and_stats(with_pileup):
        sim.depth_begin()
        sim.stats_begin()
        if with_pileup:
            sim.pileup_begin(True)
        try:
            sim.pairs(1, tb + 1)
            report = sim.stats()
            sim.depth_finish()
            return [sim.depth(s) for s in range(3)], sim.depth_bedgraph(), report
        finally:
            sim.pileup_end()
            sim.stats_end()
            sim.depth_end()
    (d0, b0, r0), (d1, b1, r1) = depth_and_stats(False), depth_and_stats(True)
    assert same(d0, d1) and b0 == b1 and r0.keys() == r1.keys() and all((r0[k] == r1[k]).all() for k in r0)


@pytest.mark.parametrize("option,value", [("overlap", 3), ("image_tiles", 1)])
def test_options(tiny, workdir, rsq_options, option, value):
    rsq_options(option, value)
    c = tiny_case(workdir)
    try:
        if option == "image_tiles":
            assert c.sim.fill_plan()["image_tiles"] == 1
        got, out, launches = run_pileup(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1), strands=True)
        assert same(got, tiny.s_want) and launches == 1 and out[3] == tiny.whole[3]
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
        assert rc == api.RSQ_ENOSPC and ls == len(sam) and sim.last_kernel_launches("pileup_add") == 0
        n, l1, l2, ls, rc = sim.pairs_sam_device(1, tb + 1, r1, r2, full)
        assert rc == api.RSQ_OK and full.to_numpy(np.uint8, ls).tobytes() == sam and sim.last_kernel_launches("pileup_add") == 1

    try:
        assert same(run_pileup(sim, sam_calls)[0], tiny.want)
    finally:
        for d in (r1, r2, short, full):
            d.free()


# ------------------------------------------------------------------------------------------------ text
def pieces_text(sim, seq, length, piece, all_rows):
    """the sequence's text fetched in pieces of `piece` positions through the device call, with room for each; the lines' total"""
    out, lines, dst = [], 0, api.DeviceArray(sim.device, 1 << 20)
    try:
        for lo in range(0, length, piece):
            n, k, rc = sim.pileup_text_device(seq, lo, min(lo + piece, length), dst, all_rows)
            assert rc == api.RSQ_OK, (seq, lo, rc)
            out.append(dst.to_numpy(np.uint8, n).tobytes())
            lines += k
    finally:
        dst.free()
    return b"".join(out), lines


@pytest.mark.parametrize("strands", [False, True])
def test_text(tiny, strands):
    sim, lengths = tiny.sim, tiny.sim.sequence_lengths()
    want = tiny.s_want if strands else tiny.want
    texts = {a: pileup_text(tiny.names, tiny.letters, want, a) for a in (False, True)}
    assert (tiny.s_sites if strands else tiny.sites) == texts[False] and (tiny.s_all_rows if strands else tiny.all_rows) == texts[True]
    assert 100 < len(texts[False].splitlines()) < len(texts[True].splitlines()) <= sum(lengths)
    per_seq = {a: [pileup_text([n], [l], [t], a) for n, l, t in zip(tiny.names, tiny.letters, want)] for a in (False, True)}
    sim.pileup_begin(strands)
    try:
        sim.pairs(1, tiny.tb + 1)
        sim.pileup_finish()
        for piece, seqs, modes in ((1, (1,), (False, True)), (63, (0, 1, 2), (False,)), (64, (0, 1, 2), (True,)), (65, (0, 1, 2), (False,)), (4095, (0, 2), (True,)),
                                   (4096, (0, 2), (False, True)), (4097, (0, 2), (False,)), (1 << 30, (0, 1, 2), (False, True))):
            for s in seqs:
                for a in modes:
                    text, lines = pieces_text(sim, s, lengths[s], piece, a)
                    assert text == per_seq[a][s] and lines == len(per_seq[a][s].splitlines()), (piece, s, a)
        assert sim.last_kernel_launches("pileup_text") == 1 and sim.last_kernel_launches("pileup_lines") >= 1
        # pieces in any order
        tail = pieces_text(sim, 0, lengths[0], 1 << 30, True)[0]
        dst = api.DeviceArray(sim.device, 1 << 20)
        try:
            b = sim.pileup_text_device(0, 2000, lengths[0], dst, True)
            second = dst.to_numpy(np.uint8, b[0]).tobytes()
            a = sim.pileup_text_device(0, 0, 2000, dst, True)
            assert a[2] == b[2] == api.RSQ_OK and dst.to_numpy(np.uint8, a[0]).tobytes() + second == tail
            # a cap one byte short: RSQ_ENOSPC with the exact need, nothing written; then it succeeds
            need, lines, rc = sim.pileup_text_device(0, 0, lengths[0], None, False)
            assert rc == api.RSQ_ENOSPC and need == len(per_seq[False][0]) and lines == len(per_seq[False][0].splitlines())
            small = api.DeviceArray.from_numpy(sim.device, np.full(need - 1, 0xA7, np.uint8))
            got = sim.pileup_text_device(0, 0, lengths[0], small, False)
            assert got == (need, lines, api.RSQ_ENOSPC) and (small.to_numpy(np.uint8, need - 1) == 0xA7).all()
            small.free()
            exact = api.DeviceArray(sim.device, need)
            n, _, rc = sim.pileup_text_device(0, 0, lengths[0], exact, False)
            assert rc == api.RSQ_OK and exact.to_numpy(np.uint8, n).tobytes() == per_seq[False][0]
            exact.free()
            # an empty window, a window without a line
            assert sim.pileup_text_device(1, 77, 77, None, True) == (0, 0, api.RSQ_OK)
            # windows of the counts, in any order
            for s, lo, hi in ((2, 1000, 1001), (0, 4990, 5000), (1, 0, 80), (0, 0, 5), (1, 77, 77), (0, 1, 4098)):
                assert (sim.pileup(s, lo, hi) == want[s][lo:hi]).all()
        finally:
            dst.free()
    finally:
        sim.pileup_end()


@pytest.mark.parametrize("name_len", [150, 600])
def test_text_with_long_names(workdir, name_len):
    """64 lines with a name of 150 characters fit the writer's image of at most 32 KiB, with one of 600 they do not and every lane writes its line straight to
    memory: both routes write the same lines"""
    c = long_name_case(workdir) if name_len == 150 else Case(workdir, "depth_long_name", synth.TINY, [6000], 7, 1500, names=["n" * 600 + " rest of the id"])
    try:
        for strands in (False, True):
            got, out, _, sites, all_rows = run_pileup(c.sim, lambda: c.sim.pairs_sam(1, c.tb + 1), strands=strands, text=True)
            want = records_pileup(c, out[3], strands)
            letters = letters_of(c)
            assert len(out[0]) > 1000 and same(got, want) and len(c.names[0]) == name_len
            assert sites == pileup_text(c.names, letters, want, False) and all_rows == pileup_text(c.names, letters, want, True) and len(all_rows.splitlines()) > 1000
        assert 64 * (name_len + 14 + 88) + 16 > 32768 or name_len == 150
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ states and arguments
def test_state(tiny, workdir):
    sim, L = tiny.sim, api.lib()
    error = lambda: L.rsq_last_error().decode()
    assert L.rsq_sim_pileup_finish(sim.h, None) == api.RSQ_ESTATE and sim.pileup_counts_device(0, 0, 1, None) == api.RSQ_ESTATE
    assert sim.pileup_text_device(0, 0, 1, None)[2] == api.RSQ_ESTATE
    assert L.rsq_sim_pileup_begin(sim.h, 2) == api.RSQ_EINVAL and "flags" in error()
    sim.pileup_end()                                              # without a run: RSQ_OK
    sim.pileup_begin()
    try:
        assert L.rsq_sim_pileup_begin(sim.h, 0) == api.RSQ_ESTATE and "open" in error()
        assert sim.pileup_counts_device(0, 0, 1, None) == api.RSQ_ESTATE and sim.pileup_text_device(0, 0, 1, None)[2] == api.RSQ_ESTATE
        n, b1, b2 = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert L.rsq_sim_job_generate(sim.h, 1, 2, 0, C.byref(n), C.byref(b1), C.byref(b2), None) == api.RSQ_ESTATE and "pileup run" in error()
        assert L.rsq_sim_job_compress(sim.h, C.byref(b1), C.byref(b2)) == api.RSQ_ESTATE
        assert L.rsq_sim_job_write(sim.h, b"/dev/null", 0, b"/dev/null", 0, 0) == api.RSQ_ESTATE and "pileup run" in error()
        host = np.zeros(16, np.uint8)
        assert L.rsq_sim_job_read(sim.h, 0, 0, 16, host.ctypes.data, None) == api.RSQ_ESTATE and "pileup run" in error()
        assert len(sim.adapter_only_pairs(0, 50)[0]) > 0 and sim.last_kernel_launches("pileup_add") == 0      # adapter-only pairs are unmapped: nothing to add
        sim.pileup_finish()
        assert L.rsq_sim_pileup_finish(sim.h, None) == api.RSQ_ESTATE
        assert all(not sim.pileup(s).any() for s in range(3)), "no pairs call: all zero"
        assert sim.pileup_text() == b"" and sim.pileup_text(all_rows=True) == b""
        assert sim.pairs_device(1, 2, None, None)[3] == api.RSQ_ESTATE and "rsq_sim_pileup_end" in error()
        assert sim.pairs_sam_device(1, 2, None, None, None)[4] == api.RSQ_ESTATE and sim.pairs_bam_device(1, 2, None, None, None)[4] == api.RSQ_ESTATE
        sim.bam_sorted_begin(0)
        assert sim.pairs_bam_sorted_device(1, 2, None, None, None)[5] == api.RSQ_ESTATE
        sim.bam_sorted_flush()
        # arguments
        big = api.DeviceArray(sim.device, 1 << 16)
        try:
            assert sim.pileup_counts_device(3, 0, 1, big) == api.RSQ_EINVAL and sim.pileup_counts_device(0, 2, 1, big) == api.RSQ_EINVAL
            assert sim.pileup_counts_device(0, 10, 5001, big) == api.RSQ_EINVAL and sim.pileup_counts_device(1, 0, 80, big) == api.RSQ_OK
            assert sim.pileup_text_device(3, 0, 1, big)[2] == api.RSQ_EINVAL and sim.pileup_text_device(0, 2, 1, big)[2] == api.RSQ_EINVAL
            assert sim.pileup_text_device(0, 0, 5001, big)[2] == api.RSQ_EINVAL
            ln, lines = C.c_size_t(), C.c_uint64()
            assert L.rsq_sim_pileup_text(sim.h, 0, 0, 10, 2, big.ptr, big.nbytes, C.byref(ln), C.byref(lines), None) == api.RSQ_EINVAL and "flags" in error()
        finally:
            big.free()
    finally:
        sim.pileup_end()
    sim.pileup_end()
    assert len(sim.pairs(1, 2)[0]) > 0
    # allele coordinates and a pileup run exclude each other
    c = VarCase(workdir, "depth_state", 7, 31)
    try:
        c.sim.truth_variants(False)
        c.sim.pileup_begin()
        assert L.rsq_sim_truth_alleles(c.sim.h, 1) == api.RSQ_ESTATE and "pileup" in error()
        c.sim.pileup_end()
        c.sim.truth_alleles(True)
        assert L.rsq_sim_pileup_begin(c.sim.h, 0) == api.RSQ_EINVAL and "allele" in error()
        c.sim.truth_alleles(False)
        c.sim.pileup_begin(True)
        c.sim.pileup_end()
    finally:
        c.close()
    # before rsq_sim_prepare
    prof, ref = api.Profile(tiny.ppath), api.Reference(tiny.fpath, 0)
    raw = api.Simulator(prof, ref, 0)
    try:
        assert L.rsq_sim_pileup_begin(raw.h, 0) == api.RSQ_ESTATE
    finally:
        raw.close()
        ref.close()
        prof.close()


# ------------------------------------------------------------------------------------------------ the command line
def test_command_line(tiny, workdir):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    keys = ("p1", "p2", "s1", "s2", "sam", "spile", "g1", "g2", "gpile", "b1", "b2", "bpile", "d1", "d2", "ddepth", "t1", "t2", "tstats", "a1", "a2", "apile", "adepth", "astats",
            "x1", "x2", "xpile", "xsam")
    out = {k: str(workdir / f"pileup_cli_{k}") for k in keys}
    common = [exe, "illuminaPE", "-R", tiny.fpath, "-s", tiny.ppath, "--numReads", "3000", "--seed", "7", "--batchBlocks", "3"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True)
    read = lambda path: open(path, "rb").read()
    assert run(["-1", out["p1"], "-2", out["p2"]]).returncode == 0
    r = run(["-1", out["s1"], "-2", out["s2"], "--truthSam", out["sam"], "--truthPileup", out["spile"]])
    assert r.returncode == 0, r.stderr
    r = run(["-1", out["g1"], "-2", out["g2"], "--truthPileup", out["gpile"] + ".gz", "-j", "1"])
    assert r.returncode == 0, r.stderr
    r = run(["-1", out["b1"], "-2", out["b2"], "--truthPileup", out["bpile"] + ".gz", "--truthPileupStrands", "--truthPileupAll"])
    assert r.returncode == 0, r.stderr
    for m in "12":
        assert read(out["p" + m]) == read(out["s" + m]) == read(out["g" + m]) == read(out["b" + m])
    assert read(out["sam"]).count(b"\n") > 5000
    # against the command's own records; its batches simulate the pairs of the blocks 1 .. tb, the run the fixture made: header + pileup_text()
    refs = dict(zip(tiny.names, tiny.letters))
    text = header_line(False) + pileup_text(tiny.names, tiny.letters, pileup_from_sam(read(out["sam"]), refs, False), False)
    assert read(out["spile"]) == text and len(text.splitlines()) > 100
    assert text == header_line(False) + tiny.sites
    packed = read(out["gpile"] + ".gz")
    assert packed[3] == 4 and packed.endswith(api.gzip_eof_member()) and inflate_members(packed) == text      # BGZF members made on the device
    packed = read(out["bpile"] + ".gz")
    assert packed.endswith(api.gzip_eof_member()) and inflate_members(packed) == header_line(True) + tiny.s_all_rows
    assert tiny.s_all_rows == pileup_text(tiny.names, tiny.letters, pileup_from_sam(read(out["sam"]), refs, True), True)
    # beside --truthDepth and --simStats: all three files equal their solo runs
    assert run(["-1", out["d1"], "-2", out["d2"], "--truthDepth", out["ddepth"]]).returncode == 0
    assert run(["-1", out["t1"], "-2", out["t2"], "--simStats", out["tstats"]]).returncode == 0
    r = run(["-1", out["a1"], "-2", out["a2"], "--truthPileup", out["apile"], "--truthDepth", out["adepth"], "--simStats", out["astats"]])
    assert r.returncode == 0, r.stderr
    assert read(out["apile"]) == text and read(out["adepth"]) == read(out["ddepth"]) and read(out["astats"]) == read(out["tstats"]) and len(read(out["tstats"])) > 1000
    # refusals: nothing is simulated, no file is left
    golden_vcf = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test-var.vcf")
    for extra, message in ((["--truthPileup", out["xpile"], "--gpus", "2"], "one worker only"), (["--truthPileup", out["xpile"] + ".bz2"], "bzip2"),
                           (["--truthPileup", out["xpile"], "--truthSam", out["xsam"], "-V", golden_vcf, "--truthAlleles"], "--truthAlleles"),
                           (["--truthPileup", out["xpile"], "--truthSam", out["xsam"], "--truthBam", out["xsam"] + ".bam"], "at most one"),
                           (["--truthPileupStrands"], "--truthPileupStrands"), (["--truthPileupAll"], "--truthPileupAll")):
        r = run(["-1", out["x1"], "-2", out["x2"]] + extra)
        assert r.returncode != 0 and "--truthPileup" in r.stderr and message in r.stderr, r.stderr
        assert not any(os.path.exists(p) for p in (out["x1"], out["x2"], out["xpile"], out["xpile"] + ".bz2", out["xsam"]))
