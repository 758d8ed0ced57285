#!/usr/bin/env python3
"""What the truth alignments cost: python tools/bench_truth_sam.py [pairs] [steps] -- bench.py's headline workload (E. coli-sized reference, P0, 10 M pairs per
step, one call per step) through rsq_sim_pairs and through rsq_sim_pairs_sam: pairs/s of both, kernel ms and launches of format_write, sam_sizes and sam_write
(of the last step), the bytes of the three texts and the two writers' bytes/s.  One JSON line.

--bam: the same through rsq_sim_pairs_bam beside them -- its pairs/s, kernel ms of bam_sizes / bam_write, the bytes per pair of SAM and BAM, and what the device's
deflater (rsq_sim_gzip_device) makes of both and of the BAM bytes' first 256 MiB against zlib level 1 on those same bytes.

--bam --sorted: the sorted call beside them (rsq_sim_bam_sorted_begin + one rsq_sim_pairs_bam_sorted over all blocks, which hands out every mapped record) -- its
pairs/s, kernel ms of bam_sort_keys / bam_sort / bam_gather / bam_index beside bam_write, and the bytes/s of bam_gather (the bytes it writes; it reads as many)."""
import json
import os
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reseq_amd import api, synth, workloads  # noqa: E402

with_bam, with_sorted = "--bam" in sys.argv, "--sorted" in sys.argv
assert with_bam or not with_sorted, "--sorted goes with --bam"
argv = [a for a in sys.argv[1:] if a not in ("--bam", "--sorted")]
pairs = int(argv[0]) if len(argv) > 0 else 10_000_000
steps = int(argv[1]) if len(argv) > 1 else 3
tmp = tempfile.mkdtemp(prefix="rsq_sam_")
ppath, fpath = os.path.join(tmp, "p0.rsqp"), os.path.join(tmp, "ref.fa")
workloads.p0_profile(ppath)
genome = max(200_000, int(4_641_652 * pairs / 10_000_000))
synth.write_fasta(fpath, synth.make_reference(2, [genome], gc=0.508, names=[f"synthEcoli0 len={genome}"]))
prof, ref = api.Profile(ppath), api.Reference(fpath, 11)
sim = api.Simulator(prof, ref, 0)
info = sim.prepare(11, pairs)
lo, hi = 1, info.total_blocks + 1
n, l1, l2, ls, rc = sim.pairs_sam_device(lo, hi, None, None, None)
assert rc == api.RSQ_ENOSPC, rc
r1, r2, sam = api.DeviceArray(0, l1 + 4096), api.DeviceArray(0, l2 + 4096), api.DeviceArray(0, ls + 4096)


def sync():
    api.lib().rsq_dev_download(0, (api.C.c_char * 8)(), r1.ptr, 8)      # a copy on the null stream: waits for the device


def timed(call):
    call()                                                             # warm-up: workspaces grown, the writers' images sized from this call's longest record
    call()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = call()
        assert out[-1] == api.RSQ_OK, out
    sync()
    return (time.perf_counter() - t0) / steps


def kernels(names):                                                    # (a kernel the last call did not launch has no time)
    launches = {k: sim.last_kernel_launches(k) for k in names}
    return {k: {"ms": round(sim.last_kernel_ms(k), 3) if launches[k] else None, "launches": launches[k]} for k in names}


plain_s = timed(lambda: sim.pairs_device(lo, hi, r1, r2))
plain_kernels = kernels(("format_write", "sam_sizes", "sam_write"))
sam_s = timed(lambda: sim.pairs_sam_device(lo, hi, r1, r2, sam))
sam_kernels = kernels(("fill_reads", "format_write", "sam_sizes", "sam_write"))
gbps = lambda nbytes, ms: round(nbytes / ms / 1e6, 1) if ms else None
bam_part = {}
if with_bam:
    _, _, _, lb, rc = sim.pairs_bam_device(lo, hi, None, None, None)
    assert rc == api.RSQ_ENOSPC, rc
    bam = api.DeviceArray(0, lb + 4096)
    bam_s = timed(lambda: sim.pairs_bam_device(lo, hi, r1, r2, bam))
    bam_kernels = kernels(("fill_reads", "format_write", "bam_sizes", "bam_write", "sam_sizes", "sam_write"))
    packed = api.DeviceArray(0, api.lib().rsq_gzip_bound(max(ls, lb)))

    def deflated(d, nbytes):                                           # the device's members of d[0, nbytes): (bytes, ms of the call)
        sync()
        t0 = time.perf_counter()
        out, rc = sim.gzip_device(d, nbytes, packed, packed.nbytes)
        sync()
        assert rc == api.RSQ_OK, rc
        return out, round((time.perf_counter() - t0) * 1e3, 2)

    sam_gz, sam_gz_ms = deflated(sam, ls)
    bam_gz, bam_gz_ms = deflated(bam, lb)
    head = min(lb, 256 << 20)                                          # zlib runs on one host thread: a leading stretch, the same bytes for both
    head_gz, _ = deflated(bam, head)
    head_zlib = len(zlib.compress(bam.to_numpy(api.np.uint8, head).tobytes(), 1))
    bam_part = {
        "pairs_per_s_bam": round(n / bam_s), "ms_per_call_bam": round(bam_s * 1e3, 2), "kernels_of_a_bam_call": bam_kernels,
        "bytes_per_pair": {"sam": round(ls / n, 1), "bam": round(lb / n, 1)}, "bam_bytes": lb, "GB_per_s_bam_write": gbps(lb, bam_kernels["bam_write"]["ms"]),
        "gzip_device": {"sam": sam_gz, "bam": bam_gz, "sam_ratio": round(sam_gz / ls, 4), "bam_ratio": round(bam_gz / lb, 4), "sam_ms": sam_gz_ms, "bam_ms": bam_gz_ms},
        "bam_first_bytes": {"bytes": head, "gzip_device": head_gz, "zlib_level_1": head_zlib},
    }
    if with_sorted:
        def sorted_call():
            sim.bam_sorted_begin(0)
            return sim.pairs_bam_sorted_device(lo, hi, r1, r2, bam)

        sorted_s = timed(sorted_call)
        final_bytes, n_records = sorted_call()[3:5]
        sorted_kernels = kernels(("fill_reads", "format_write", "bam_sizes", "bam_write", "bam_sort_keys", "bam_sort", "bam_gather", "bam_index"))
        held_bytes, n_mapped, n_unmapped, rc = sim.bam_sorted_flush_device(None)
        bam_part.update({
            "pairs_per_s_bam_sorted": round(n / sorted_s), "ms_per_call_bam_sorted": round(sorted_s * 1e3, 2), "kernels_of_a_sorted_call": sorted_kernels,
            "sorted_call": {"records": n_records, "bytes": final_bytes, "held_for_the_flush_bytes": held_bytes},
            "GB_per_s_bam_gather": gbps(final_bytes + held_bytes, sorted_kernels["bam_gather"]["ms"]),
            "GB_per_s_bam_write_in_the_sorted_call": gbps(lb, sorted_kernels["bam_write"]["ms"]),
        })
    packed.free()
    bam.free()
print(json.dumps({
    "workload": f"P0, one sequence of {genome} bases, {n} pairs per call", "steps": steps,
    "pairs_per_s": {"rsq_sim_pairs": round(n / plain_s), "rsq_sim_pairs_sam": round(n / sam_s)},
    "ms_per_call": {"rsq_sim_pairs": round(plain_s * 1e3, 2), "rsq_sim_pairs_sam": round(sam_s * 1e3, 2)},
    "kernels_of_a_plain_call": plain_kernels, "kernels_of_a_sam_call": sam_kernels,
    "bytes": {"fastq1": l1, "fastq2": l2, "sam": ls},
    "GB_per_s": {"format_write": gbps(l1 + l2, sam_kernels["format_write"]["ms"]), "sam_write": gbps(ls, sam_kernels["sam_write"]["ms"])},
    **bam_part,
}))
for d in (r1, r2, sam):
    d.free()
sim.close()
