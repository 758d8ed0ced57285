#!/usr/bin/env python3
"""What the truth pileup costs: python tools/bench_truth_pileup.py [pairs] [steps] -- bench.py's headline workload (E. coli-sized reference, P0, 10 M pairs per step,
one call per step) through rsq_sim_pairs without a run and, in the same process on the same simulator, with a pileup run open (unstranded, then per strand), and
with a depth and a stats run open (the two kernels that make the same two walks separately): pairs/s of each, kernel ms of pileup_add beside depth_add and
stats_mates (of the last step), of pileup_scan (rsq_sim_pileup_finish), of pileup_rows over the whole reference, and of pileup_lines + pileup_text over the whole
reference in pieces of 4 Mi positions in both row modes, with the text's bytes and lines.  One JSON line."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reseq_amd import api, synth, workloads  # noqa: E402

argv = sys.argv[1:]
pairs = int(argv[0]) if len(argv) > 0 else 10_000_000
steps = int(argv[1]) if len(argv) > 1 else 3
PIECE = 4 << 20
tmp = tempfile.mkdtemp(prefix="rsq_pileup_")
ppath, fpath = os.path.join(tmp, "p0.rsqp"), os.path.join(tmp, "ref.fa")
workloads.p0_profile(ppath)
genome = max(200_000, int(4_641_652 * pairs / 10_000_000))
synth.write_fasta(fpath, synth.make_reference(2, [genome], gc=0.508, names=[f"synthEcoli0 len={genome}"]))

prof, ref = api.Profile(ppath), api.Reference(fpath, 11)
sim = api.Simulator(prof, ref, 0)
info = sim.prepare(11, pairs)
lo, hi = 1, info.total_blocks + 1
n, l1, l2, rc = sim.pairs_device(lo, hi, None, None)
assert rc == api.RSQ_ENOSPC, rc
r1, r2 = api.DeviceArray(0, l1 + 4096), api.DeviceArray(0, l2 + 4096)
KERNELS = ("fill_reads", "format_write", "depth_add", "stats_rows", "stats_mates", "pileup_add")


def sync():
    api.lib().rsq_dev_download(0, (api.C.c_char * 8)(), r1.ptr, 8)          # a copy on the null stream: waits for the device


def timed():
    """seconds per rsq_sim_pairs call over the whole reference, and the kernels of the last one"""
    for _ in range(2):                                                       # warm-up: workspaces grown, the formatter's image sized
        assert sim.pairs_device(lo, hi, r1, r2)[3] == api.RSQ_OK
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        assert sim.pairs_device(lo, hi, r1, r2)[3] == api.RSQ_OK
    sync()
    seconds = (time.perf_counter() - t0) / steps
    launches = {k: sim.last_kernel_launches(k) for k in KERNELS}
    return seconds, {k: round(sim.last_kernel_ms(k), 3) for k in KERNELS if launches[k]}


def whole_text(all_rows, text):
    """the whole reference's text in pieces: (bytes, lines, pileup_lines ms, pileup_text ms, seconds of the calls)"""
    out = [0, 0, 0.0, 0.0]
    sync()
    t0 = time.perf_counter()
    for a in range(0, length, PIECE):
        nbytes, nlines, rc = sim.pileup_text_device(0, a, min(a + PIECE, length), text, all_rows)
        assert rc == api.RSQ_OK, rc
        out[0] += nbytes
        out[1] += nlines
        out[2] += sim.last_kernel_ms("pileup_lines")
        if sim.last_kernel_launches("pileup_text"):
            out[3] += sim.last_kernel_ms("pileup_text")
    sync()
    return out + [time.perf_counter() - t0]


def pileup_run(strands):
    sim.pileup_begin(strands)
    seconds, kernels = timed()
    sim.pileup_finish()
    scan_ms = sim.last_kernel_ms("pileup_scan")
    sets = 2 if strands else 1
    rows = api.DeviceArray(0, 32 * sets * min(PIECE, length))
    rows_ms = 0.0
    for a in range(0, length, PIECE):
        assert sim.pileup_counts_device(0, a, min(a + PIECE, length), rows) == api.RSQ_OK
        rows_ms += sim.last_kernel_ms("pileup_rows")
    rows.free()
    texts = {}
    for all_rows in (False, True):
        need = max(sim.pileup_text_device(0, a, min(a + PIECE, length), None, all_rows)[0] for a in range(0, length, PIECE))
        text = api.DeviceArray(0, need + 4096)
        nbytes, nlines, lines_ms, text_ms, s = whole_text(all_rows, text)
        text.free()
        texts["all" if all_rows else "sites"] = {"bytes": nbytes, "lines": nlines, "pileup_lines_ms": round(lines_ms, 3), "pileup_text_ms": round(text_ms, 3),
                                                 "GB_per_s_pileup_text": round(nbytes / text_ms / 1e6, 1) if text_ms else None, "ms_of_the_calls": round(s * 1e3, 2)}
    sim.pileup_end()
    return {"pairs_per_s": round(n / seconds), "ms_per_call": round(seconds * 1e3, 2), "kernels_of_a_call": kernels, "pileup_scan_ms": round(scan_ms, 3),
            "pileup_rows_ms": round(rows_ms, 3), "planes_bytes": 32 * sets * (length + 1), "text": texts}


length = sim.sequence_lengths()[0]
before_s, before_kernels = timed()
unstranded = pileup_run(False)
stranded = pileup_run(True)
sim.depth_begin()
sim.stats_begin()
both_s, both_kernels = timed()
sim.stats_end()
sim.depth_end()
after_s, after_kernels = timed()
print(json.dumps({
    "workload": f"P0, one sequence of {genome} bases, {n} pairs per call", "steps": steps,
    "no_run": {"pairs_per_s_before": round(n / before_s), "pairs_per_s_after": round(n / after_s), "ms_per_call_before": round(before_s * 1e3, 2),
               "ms_per_call_after": round(after_s * 1e3, 2), "kernels_of_a_call": after_kernels},
    "pileup_run": unstranded, "pileup_run_per_strand": stranded,
    "depth_and_stats_runs": {"pairs_per_s": round(n / both_s), "ms_per_call": round(both_s * 1e3, 2), "kernels_of_a_call": both_kernels},
}))
for d in (r1, r2):
    d.free()
sim.close()
ref.close()
prof.close()
