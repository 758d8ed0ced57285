#!/usr/bin/env python3
"""What the truth alignments cost: python tools/bench_truth_sam.py [pairs] [steps] -- bench.py's headline workload (E. coli-sized reference, P0, 10 M pairs per
step, one call per step) through rsq_sim_pairs and through rsq_sim_pairs_sam: pairs/s of both, kernel ms and launches of format_write, sam_sizes and sam_write
(of the last step), the bytes of the three texts and the two writers' bytes/s.  One JSON line.

--md: the truth calls again with rsq_sim_truth_md set (NM:i and MD:Z on every mapped record), beside the ones above -- "with_md": pairs/s, kernel ms of the sizes
and the write kernel and bytes per pair of the SAM call and, where --bam / --sorted are given, of theirs; with --variants in both halves.

--bam: the same through rsq_sim_pairs_bam beside them -- its pairs/s, kernel ms of bam_sizes / bam_write, the bytes per pair of SAM and BAM, and what the device's
deflater (rsq_sim_gzip_device) makes of both and of the BAM bytes' first 256 MiB against zlib level 1 on those same bytes.

--bam --sorted: the sorted call beside them (rsq_sim_bam_sorted_begin + one rsq_sim_pairs_bam_sorted over all blocks, which hands out every mapped record) -- its
pairs/s, kernel ms of bam_sort_keys / bam_sort / bam_gather / bam_index beside bam_write, and the bytes/s of bam_gather (the bytes it writes; it reads as many).

--variants: everything above twice in one run, on the same reference -- "without_variants" as ever, and "with_variants": a synthetic phased VCF at the human-sized
configuration's density (workloads.human_sized: 4.4 variants per 3100 bases, one in eleven an insertion or a deletion of at most 20 bases, two alleles) with
rsq_sim_truth_variants set -- and "variants_over_plain", the ratios of the truth kernels' times.  The simulators differ in more than the truth kernels (the sieve
and the read kernel walk the alleles), so the ratios to read are those of sam_sizes / sam_write / bam_sizes / bam_write.

--variants --alleles: in the "with_variants" half also "in_allele_coordinates" -- the SAM call (with --bam: and the BAM call) of the SAME simulator with
rsq_sim_truth_alleles in place of rsq_sim_truth_variants: pairs/s, kernel ms of the sizes and the write kernel, bytes per pair, to be read beside the half's own
reference-coordinate figures and the plain calls of "without_variants" -- and "alleles_fasta": the bytes of the alleles' FASTA text of that reference
(rsq_sim_alleles_fasta, the whole text in one call), the kernel's ms (the median of the steps) and GB/s of text written."""
import json
import os
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reseq_amd import api, synth, workloads  # noqa: E402

with_bam, with_sorted, with_variants, with_md = "--bam" in sys.argv, "--sorted" in sys.argv, "--variants" in sys.argv, "--md" in sys.argv
with_alleles = "--alleles" in sys.argv
assert with_bam or not with_sorted, "--sorted goes with --bam"
assert with_variants or not with_alleles, "--alleles goes with --variants"
argv = [a for a in sys.argv[1:] if a not in ("--bam", "--sorted", "--variants", "--md", "--alleles")]
pairs = int(argv[0]) if len(argv) > 0 else 10_000_000
steps = int(argv[1]) if len(argv) > 1 else 3
tmp = tempfile.mkdtemp(prefix="rsq_sam_")
ppath, fpath = os.path.join(tmp, "p0.rsqp"), os.path.join(tmp, "ref.fa")
workloads.p0_profile(ppath)
genome = max(200_000, int(4_641_652 * pairs / 10_000_000))
seqs = synth.make_reference(2, [genome], gc=0.508, names=[f"synthEcoli0 len={genome}"])
synth.write_fasta(fpath, seqs)


def write_vcf(path):
    """workloads.human_sized's call set at its density, over the benchmark's one sequence"""
    rng = api.np.random.default_rng(11)
    codes, letters = seqs[0][1], api.np.frombuffer(b"ACGT", api.np.uint8)
    pos = api.np.unique(rng.integers(1, genome - 50, int(genome * 4.4e6 / 3.1e9)))
    pos = pos[api.np.concatenate(([True], api.np.diff(pos) > 25))]
    kinds, gts = rng.random(len(pos)) < 1.0 / 11.0, rng.integers(0, 3, len(pos))
    lines = ["##fileformat=VCFv4.2", f"##contig=<ID=synthEcoli0,length={genome}>", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1"]
    for p0, is_indel, g in zip(pos.tolist(), kinds.tolist(), gts.tolist()):
        ref = chr(letters[codes[p0]])
        if not is_indel:
            alt = chr(letters[(codes[p0] + 1 + p0 % 3) % 4])
        elif p0 & 1:
            alt = ref + letters[rng.integers(0, 4, 1 + p0 % 20)].tobytes().decode()
        else:
            ref, alt = letters[codes[p0:p0 + 2 + p0 % 20]].tobytes().decode(), ref
        lines.append(f"synthEcoli0\t{p0 + 1}\t.\t{ref}\t{alt}\t.\tPASS\t.\tGT\t{('0|1', '1|0', '1|1')[g]}")
    open(path, "w").write("\n".join(lines) + "\n")
    return len(pos)


def measure(vcf):
    """the whole measurement on a fresh simulator; vcf: the variant file, with the opt-in for its truth alignments"""
    prof, ref = api.Profile(ppath), api.Reference(fpath, 11)
    if vcf:
        ref.read_variants(vcf)
    sim = api.Simulator(prof, ref, 0)
    if vcf:
        sim.truth_variants(True)
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
    alleles_part = {}
    if vcf and with_alleles:
        if with_sorted:                                                    # the switch does not change inside a sorted run: hand out what the last one holds
            held = api.DeviceArray(0, sim.bam_sorted_flush_device(None)[0] + 4096)
            assert sim.bam_sorted_flush_device(held)[3] == api.RSQ_OK
            held.free()
        sim.truth_variants(False)
        sim.truth_alleles(True)
        _, _, _, ls_al, rc = sim.pairs_sam_device(lo, hi, None, None, None)
        assert rc == api.RSQ_ENOSPC, rc
        sam_al = api.DeviceArray(0, ls_al + 4096)
        al_s = timed(lambda: sim.pairs_sam_device(lo, hi, r1, r2, sam_al))
        in_alleles = {"pairs_per_s_sam": round(n / al_s), "ms_per_call_sam": round(al_s * 1e3, 2), "kernels_of_a_sam_call": kernels(("sam_sizes", "sam_write")),
                      "bytes_per_pair": {"sam": round(ls_al / n, 1)}}
        in_alleles["GB_per_s_sam_write"] = gbps(ls_al, in_alleles["kernels_of_a_sam_call"]["sam_write"]["ms"])
        sam_al.free()
        if with_bam:
            _, _, _, lb_al, rc = sim.pairs_bam_device(lo, hi, None, None, None)
            assert rc == api.RSQ_ENOSPC, rc
            bam_al = api.DeviceArray(0, lb_al + 4096)
            al_s = timed(lambda: sim.pairs_bam_device(lo, hi, r1, r2, bam_al))
            in_alleles.update({"pairs_per_s_bam": round(n / al_s), "ms_per_call_bam": round(al_s * 1e3, 2), "kernels_of_a_bam_call": kernels(("bam_sizes", "bam_write"))})
            in_alleles["bytes_per_pair"]["bam"] = round(lb_al / n, 1)
            in_alleles["GB_per_s_bam_write"] = gbps(lb_al, in_alleles["kernels_of_a_bam_call"]["bam_write"]["ms"])
            bam_al.free()
        sim.truth_alleles(False)
        sim.truth_variants(True)
        text_bytes = ref.alleles_fasta_size()
        text = api.DeviceArray(0, text_bytes + 16)
        fasta_ms = []
        for _ in range(steps + 2):                                         # (the first call uploads the records' table)
            assert sim.alleles_fasta_device(0, text_bytes, text) == api.RSQ_OK
            fasta_ms.append(sim.last_kernel_ms("alleles_fasta"))
        text.free()
        fasta_ms = sorted(fasta_ms[2:])
        alleles_part = {"in_allele_coordinates": in_alleles,
                        "alleles_fasta": {"bytes": text_bytes, "ms": round(fasta_ms[len(fasta_ms) // 2], 4), "ms_of_every_step": [round(x, 4) for x in fasta_ms],
                                          "GB_per_s": gbps(text_bytes, fasta_ms[len(fasta_ms) // 2])}}
    md_part = {}
    if with_md:
        if with_sorted:                                                    # the switch does not change inside a sorted run: hand out what the last one holds
            held = api.DeviceArray(0, sim.bam_sorted_flush_device(None)[0] + 4096)
            assert sim.bam_sorted_flush_device(held)[3] == api.RSQ_OK
            held.free()
        sim.truth_md(True)
        _, _, _, ls_md, rc = sim.pairs_sam_device(lo, hi, None, None, None)
        assert rc == api.RSQ_ENOSPC, rc
        sam_md = api.DeviceArray(0, ls_md + 4096)
        md_s = timed(lambda: sim.pairs_sam_device(lo, hi, r1, r2, sam_md))
        md_part = {"pairs_per_s_sam": round(n / md_s), "ms_per_call_sam": round(md_s * 1e3, 2), "kernels_of_a_sam_call": kernels(("sam_sizes", "sam_write")),
                   "bytes_per_pair": {"sam": round(ls_md / n, 1)}}
        md_part["GB_per_s_sam_write"] = gbps(ls_md, md_part["kernels_of_a_sam_call"]["sam_write"]["ms"])
        sam_md.free()
        if with_bam:
            _, _, _, lb_md, rc = sim.pairs_bam_device(lo, hi, None, None, None)
            assert rc == api.RSQ_ENOSPC, rc
            bam_md = api.DeviceArray(0, lb_md + 4096)
            md_s = timed(lambda: sim.pairs_bam_device(lo, hi, r1, r2, bam_md))
            md_part.update({"pairs_per_s_bam": round(n / md_s), "ms_per_call_bam": round(md_s * 1e3, 2), "kernels_of_a_bam_call": kernels(("bam_sizes", "bam_write"))})
            md_part["bytes_per_pair"]["bam"] = round(lb_md / n, 1)
            md_part["GB_per_s_bam_write"] = gbps(lb_md, md_part["kernels_of_a_bam_call"]["bam_write"]["ms"])
            if with_sorted:
                def sorted_md_call():
                    sim.bam_sorted_begin(0)
                    return sim.pairs_bam_sorted_device(lo, hi, r1, r2, bam_md)

                md_s = timed(sorted_md_call)
                md_part.update({"pairs_per_s_bam_sorted": round(n / md_s), "ms_per_call_bam_sorted": round(md_s * 1e3, 2),
                                "kernels_of_a_sorted_call": kernels(("bam_sizes", "bam_write", "bam_sort_keys", "bam_sort", "bam_gather", "bam_index"))})
            bam_md.free()
    result = {
        "workload": f"P0, one sequence of {genome} bases, {n} pairs per call", "steps": steps,
        "pairs_per_s": {"rsq_sim_pairs": round(n / plain_s), "rsq_sim_pairs_sam": round(n / sam_s)},
        "ms_per_call": {"rsq_sim_pairs": round(plain_s * 1e3, 2), "rsq_sim_pairs_sam": round(sam_s * 1e3, 2)},
        "kernels_of_a_plain_call": plain_kernels, "kernels_of_a_sam_call": sam_kernels,
        "bytes": {"fastq1": l1, "fastq2": l2, "sam": ls},
        "GB_per_s": {"format_write": gbps(l1 + l2, sam_kernels["format_write"]["ms"]), "sam_write": gbps(ls, sam_kernels["sam_write"]["ms"])},
        **bam_part,
        **alleles_part,
    }
    if with_md:
        result["with_md"] = md_part
    for d in (r1, r2, sam):
        d.free()
    sim.close()
    ref.close()
    prof.close()
    return result


if with_variants:
    n_variants = write_vcf(os.path.join(tmp, "variants.vcf"))
    plain, var = measure(None), measure(os.path.join(tmp, "variants.vcf"))

    def ms(result, call, kernel):
        return (result.get(call) or {}).get(kernel, {}).get("ms")

    ratios = {}
    for call, kernel in (("kernels_of_a_sam_call", "sam_sizes"), ("kernels_of_a_sam_call", "sam_write"), ("kernels_of_a_bam_call", "bam_sizes"), ("kernels_of_a_bam_call", "bam_write"),
                         ("kernels_of_a_sorted_call", "bam_sort_keys")):
        a, b = ms(plain, call, kernel), ms(var, call, kernel)
        if a and b:
            ratios[kernel] = round(b / a, 3)
    print(json.dumps({"variants": n_variants, "without_variants": plain, "with_variants": var, "variants_over_plain": ratios}))
else:
    print(json.dumps(measure(None)))
