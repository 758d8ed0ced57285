#!/usr/bin/env python3
"""What the simulation report costs: python tools/bench_sim_stats.py [pairs] [steps] [rounds] -- bench.py's headline workload (E. coli-sized reference, P0, 10 M pairs
per step, one call per step) through rsq_sim_pairs without a stats run and, in the same process on the same simulator, with one open (rsq_sim_stats_begin): pairs/s
of both, in the order without / with / without again (the two runs without one show the run-to-run spread), and kernel ms of stats_rows and stats_mates beside
format_write of the same call.  A second simulator in the same process runs the rows kernel in its direct form (option stats_form 1: every lane of a wave at the same
word, no staging); the two forms' kernel times are taken in interleaved rounds, and their tables must be equal.  One JSON line."""
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
rounds = int(argv[2]) if len(argv) > 2 else 3
tmp = tempfile.mkdtemp(prefix="rsq_stats_")
ppath, fpath = os.path.join(tmp, "p0.rsqp"), os.path.join(tmp, "ref.fa")
workloads.p0_profile(ppath)
genome = max(200_000, int(4_641_652 * pairs / 10_000_000))
synth.write_fasta(fpath, synth.make_reference(2, [genome], gc=0.508, names=[f"synthEcoli0 len={genome}"]))

prof, ref = api.Profile(ppath), api.Reference(fpath, 11)
KERNELS = ("fill_reads", "format_write", "stats_rows", "stats_mates")


def simulator(form):
    api.set_option("stats_form", form)
    sim = api.Simulator(prof, ref, 0)
    info = sim.prepare(11, pairs)
    return sim, 1, info.total_blocks + 1


sim, lo, hi = simulator(0)
direct, _, _ = simulator(1)
api.set_option("stats_form", 0)
n, l1, l2, rc = sim.pairs_device(lo, hi, None, None)
assert rc == api.RSQ_ENOSPC, rc
r1, r2 = api.DeviceArray(0, l1 + 4096), api.DeviceArray(0, l2 + 4096)


def sync():
    api.lib().rsq_dev_download(0, (api.C.c_char * 8)(), r1.ptr, 8)          # a copy on the null stream: waits for the device


def timed(s):
    """seconds per rsq_sim_pairs call over the whole reference, and the kernels of the last one"""
    for _ in range(2):                                                       # warm-up: workspaces grown, the formatter's image sized
        assert s.pairs_device(lo, hi, r1, r2)[3] == api.RSQ_OK
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        assert s.pairs_device(lo, hi, r1, r2)[3] == api.RSQ_OK
    sync()
    seconds = (time.perf_counter() - t0) / steps
    launches = {k: s.last_kernel_launches(k) for k in KERNELS}
    return seconds, {k: {"ms": round(s.last_kernel_ms(k), 3) if launches[k] else None, "launches": launches[k]} for k in launches}


before_s, before_kernels = timed(sim)
sim.stats_begin()
open_s, open_kernels = timed(sim)
tables = sim.stats()
layout = sim.stats_layout()
sim.stats_end()
after_s, after_kernels = timed(sim)

# the two forms of the rows kernel, one call each per round, interleaved
forms = {"skewed": [], "direct": []}
mates = []
same = None
for _ in range(rounds):
    for name, s in (("skewed", sim), ("direct", direct)):
        s.stats_begin()
        assert s.pairs_device(lo, hi, r1, r2)[3] == api.RSQ_OK
        forms[name].append(round(s.last_kernel_ms("stats_rows"), 3))
        if name == "skewed":
            mates.append(round(s.last_kernel_ms("stats_mates"), 3))
        t = s.stats()
        s.stats_end()
        if name == "skewed":
            one = t
        else:
            same = all((one[k] == t[k]).all() for k in t)
            assert same, "the two forms of the rows kernel count differently"
calls = steps + 2
scale = 10_000_000 / n
print(json.dumps({
    "workload": f"P0, one sequence of {genome} bases, {n} pairs per call", "steps": steps,
    "pairs_per_s": {"no_run_before": round(n / before_s), "run_open": round(n / open_s), "no_run_after": round(n / after_s)},
    "ms_per_call": {"no_run_before": round(before_s * 1e3, 2), "run_open": round(open_s * 1e3, 2), "no_run_after": round(after_s * 1e3, 2)},
    "kernels_of_a_call_without_a_run": after_kernels, "kernels_of_a_call_with_a_run": open_kernels,
    "ms_per_10M_pairs": {k: round(open_kernels[k]["ms"] * scale, 3) for k in ("format_write", "stats_rows", "stats_mates") if open_kernels[k]["ms"]},
    "stats_rows_ms_by_form_interleaved": forms, "stats_mates_ms": mates, "forms_count_the_same": same,
    "dimensions": {"read_length": list(layout.read_length), "insert_to": layout.insert_to, "n_quality": layout.n_quality, "n_tiles": layout.n_tiles, "counters": int(layout.words)},
    "calls_counted_in_the_run": calls, "base_quality_increments": int(tables["base_quality"].sum()), "pairs_counted": int(tables["pairs"].sum()),
    "bad": int(tables["bad"][0]),
}))
for d in (r1, r2):
    d.free()
sim.close()
direct.close()
ref.close()
prof.close()
