#!/usr/bin/env python3
"""What the truth depth costs: python tools/bench_truth_depth.py [pairs] [steps] -- bench.py's headline workload (E. coli-sized reference, P0, 10 M pairs per step,
one call per step) through rsq_sim_pairs without a depth run and, in the same process on the same simulator, with one open (rsq_sim_depth_begin): pairs/s of
both, in the order without / with / without again (the two runs without one show the run-to-run spread), kernel ms of depth_add beside format_write (of the last
step), of depth_scan (rsq_sim_depth_finish), and of depth_lines + depth_text over the whole reference in pieces of 4 Mi positions, with the text's bytes and the
GB/s of the text kernel and of the bedGraph calls as a whole.  One JSON line."""
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
tmp = tempfile.mkdtemp(prefix="rsq_depth_")
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
    launches = {k: sim.last_kernel_launches(k) for k in ("fill_reads", "format_write", "depth_add")}
    return seconds, {k: {"ms": round(sim.last_kernel_ms(k), 3) if launches[k] else None, "launches": launches[k]} for k in launches}


before_s, before_kernels = timed()
sim.depth_begin()
open_s, open_kernels = timed()
counted_calls = steps + 2
sim.depth_finish()
scan_ms = sim.last_kernel_ms("depth_scan")
# the whole reference's text, in pieces: the first round sizes the buffer, the second is timed
length = sim.sequence_lengths()[0]
need = max(sim.depth_bedgraph_device(0, a, min(a + PIECE, length), None)[0] for a in range(0, length, PIECE))
text = api.DeviceArray(0, need + 4096)
lines_ms = text_ms = 0.0
text_bytes = text_lines = 0
sync()
t0 = time.perf_counter()
for a in range(0, length, PIECE):
    nbytes, nlines, rc = sim.depth_bedgraph_device(0, a, min(a + PIECE, length), text)
    assert rc == api.RSQ_OK, rc
    text_bytes += nbytes
    text_lines += nlines
    lines_ms += sim.last_kernel_ms("depth_lines")
    if sim.last_kernel_launches("depth_text"):
        text_ms += sim.last_kernel_ms("depth_text")
sync()
bedgraph_s = time.perf_counter() - t0
mean_depth = float(sim.depth(0, 0, min(length, 1 << 20)).mean())
sim.depth_end()
after_s, after_kernels = timed()
print(json.dumps({
    "workload": f"P0, one sequence of {genome} bases, {n} pairs per call", "steps": steps,
    "pairs_per_s": {"no_run_before": round(n / before_s), "run_open": round(n / open_s), "no_run_after": round(n / after_s)},
    "ms_per_call": {"no_run_before": round(before_s * 1e3, 2), "run_open": round(open_s * 1e3, 2), "no_run_after": round(after_s * 1e3, 2)},
    "kernels_of_a_call_without_a_run": after_kernels, "kernels_of_a_call_with_a_run": open_kernels,
    "depth_add_atomics_per_s": round(4 * n / (open_kernels["depth_add"]["ms"] * 1e-3)) if open_kernels["depth_add"]["ms"] else None,
    "depth_scan_ms": round(scan_ms, 3), "depth_array_bytes": 4 * (length + 1),
    "bedgraph": {"pieces": -(-length // PIECE), "bytes": text_bytes, "lines": text_lines, "depth_lines_ms": round(lines_ms, 3), "depth_text_ms": round(text_ms, 3),
                 "GB_per_s_depth_text": round(text_bytes / text_ms / 1e6, 1) if text_ms else None, "ms_of_the_calls": round(bedgraph_s * 1e3, 2),
                 "GB_per_s_of_the_calls": round(text_bytes / bedgraph_s / 1e9, 2)},
    "calls_counted_in_the_run": counted_calls, "mean_depth_of_the_first_Mi_positions": round(mean_depth, 1),
}))
for d in (r1, r2, text):
    d.free()
sim.close()
ref.close()
prof.close()
