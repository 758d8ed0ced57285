#!/usr/bin/env python3
"""What writing the alleles costs: python tools/bench_alleles_fasta.py [bases] [samples] [steps] -- one synthetic sequence of `bases` bases (default 200 M), a phased
VCF at the human-sized configuration's density (workloads.human_sized: 4.4 variants per 3100 bases, one in eleven an insertion or a deletion of at most 20 bases)
with `samples` samples (default 1: two alleles), and rsq_sim_alleles_fasta over the whole text in one call and in pieces of 64 MiB as the command line fetches it:
kernel ms (the median of the steps), GB/s of text written, and the bytes the kernel must read by the shapes -- the packed reference once per allele (a quarter byte
per base) and the alleles' map entries (16 bytes each).  One JSON line.  The simulator is only created: the text needs nothing of the pre-pass."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reseq_amd import api, synth, workloads  # noqa: E402

np = api.np
bases = (int(sys.argv[1]) if len(sys.argv) > 1 else 200_000_000) // 70 * 70
samples = int(sys.argv[2]) if len(sys.argv) > 2 else 1
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
tmp = tempfile.mkdtemp(prefix="rsq_alleles_")
ppath, fpath, vpath = os.path.join(tmp, "p0.rsqp"), os.path.join(tmp, "ref.fa"), os.path.join(tmp, "variants.vcf")
workloads.p0_profile(ppath)
rng = np.random.default_rng(11)
codes = rng.integers(0, 4, bases).astype(np.uint8)
letters = np.frombuffer(b"ACGT", np.uint8)
with open(fpath, "wb") as f:
    lines = np.full((bases // 70, 71), 10, np.uint8)                       # lines of 70 letters and a line end
    lines[:, :70] = letters[codes].reshape(-1, 70)
    f.write(b">synth0 len=%d\n" % bases)
    f.write(lines.tobytes())
    del lines
pos = np.unique(rng.integers(1, bases - 50, int(bases * 4.4e6 / 3.1e9)))
pos = pos[np.concatenate(([True], np.diff(pos) > 25))]
is_indel = rng.random(len(pos)) < 1.0 / 11.0
entries = 0
with open(vpath, "w") as f:
    f.write(f"##fileformat=VCFv4.2\n##contig=<ID=synth0,length={bases}>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"S{i + 1}" for i in range(samples)) + "\n")
    genotypes = rng.integers(0, 3, (len(pos), samples))
    for i, p0 in enumerate(pos.tolist()):
        ref = chr(letters[codes[p0]])
        if not is_indel[i]:
            alt = chr(letters[(codes[p0] + 1 + p0 % 3) % 4])
        elif p0 & 1:
            alt = ref + letters[rng.integers(0, 4, 1 + p0 % 20)].tobytes().decode()
        else:
            ref, alt = letters[codes[p0:p0 + 2 + p0 % 20]].tobytes().decode(), ref
        gts = [("0|1", "1|0", "1|1")[g] for g in genotypes[i]]
        entries += sum(2 if g == "1|1" else 1 for g in gts) * max(len(ref), 1)
        f.write(f"synth0\t{p0 + 1}\t.\t{ref}\t{alt}\t.\tPASS\t.\tGT\t" + "\t".join(gts) + "\n")

prof, ref = api.Profile(ppath), api.Reference(fpath, 11)
num_alleles = ref.read_variants(vpath)
sim = api.Simulator(prof, ref, 0)
total = ref.alleles_fasta_size()
dst = api.DeviceArray(0, total + 16)


def median_ms(call):
    times = []
    for _ in range(steps + 2):
        times.append(call())
    times = sorted(times[2:])
    return times[len(times) // 2]


def whole():
    assert sim.alleles_fasta_device(0, total, dst) == api.RSQ_OK
    return sim.last_kernel_ms("alleles_fasta")


def in_pieces(piece=64 << 20):
    ms = 0.0
    for at in range(0, total, piece):
        assert sim.alleles_fasta_device(at, min(piece, total - at), dst.ptr.value + at) == api.RSQ_OK
        ms += sim.last_kernel_ms("alleles_fasta")
    return ms


whole_ms, pieces_ms = median_ms(whole), median_ms(in_pieces)
must_read = num_alleles * bases // 4 + 16 * entries
print(json.dumps({"workload": f"one sequence of {bases} bases, {len(pos)} VCF records, {num_alleles} alleles", "text_bytes": total, "ms_whole_text": round(whole_ms, 4),
                  "GB_per_s_whole_text": round(total / whole_ms / 1e6, 1), "ms_in_64MiB_pieces": round(pieces_ms, 4), "GB_per_s_in_64MiB_pieces": round(total / pieces_ms / 1e6, 1),
                  "bytes_it_must_read": must_read, "of_which_map_entries_about": 16 * entries}))
dst.free()
sim.close()
ref.close()
prof.close()
