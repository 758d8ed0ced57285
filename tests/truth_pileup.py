"""What the truth pileup (include/reseq_amd.h rsq_sim_pileup_*; reseq_amd/csrc/rsq_pileup.h) must be, from the truth records alone: the table is a pure function of
the SAM text rsq_sim_pairs_sam writes for the same pairs and of the reference as loaded, the TSV text a pure function of the table.  Shared by
tests/test_truth_pileup.py (the per-lane function on the CPU) and tests/test_truth_pileup_gpu.py (the device); it shares no arithmetic with the kernels.

The rule (DESIGN.md 4.8 "Truth pileup"): only mapped records count, a record's strand is its FLAG 0x10.  r = POS - 1, q = 0, over the CIGAR as written:
nM: per column depth[r] += 1 and base[SEQ[q]][r] += 1, ++r, ++q; nD: del[r .. r + n) += 1, r += n; nI: ins[max(r, 1) - 1] += 1 (one per element), q += n; nS: q += n."""
import re

import numpy as np

_ELEMENT = re.compile(rb"(\d+)([MIDNSHP=X])")
COLUMNS = ("depth", "A", "C", "G", "T", "N", "del", "ins")
DEPTH, DEL, INS = 0, 6, 7
_BASE = {65: 1, 67: 2, 71: 3, 84: 4, 78: 5}          # A C G T N -> the column


def pileup_from_sam(text, refs, strands):
    """[a uint32 array [len, S, 8] per sequence]; refs: {RNAME: the sequence's letters} in order (only the lengths are used: the reference letter's count is
    counted like any other); strands: S = 2, the records without 0x10 and then those with it, else S = 1"""
    index = {name: i for i, name in enumerate(refs)}
    sets = 2 if strands else 1
    tables = [np.zeros((len(r), sets, 8), np.uint32) for r in refs.values()]
    for line in text.split(b"\n"):
        if not line or line[:1] == b"@":
            continue
        f = line.split(b"\t")
        flag = int(f[1])
        if flag & 0x4:
            continue
        t = tables[index[f[2]]]
        s = 1 if strands and flag & 0x10 else 0
        r, q, seq = int(f[3]) - 1, 0, f[9]
        assert f[5] == b"*" or b"".join(n + op for n, op in _ELEMENT.findall(f[5])) == f[5], f[5]
        for n, op in _ELEMENT.findall(f[5]):
            n = int(n)
            if op == b"M":
                assert 0 <= r and r + n <= len(t), (f[:6], len(t))
                for k in range(n):
                    t[r + k, s, DEPTH] += 1
                    t[r + k, s, _BASE[seq[q + k]]] += 1
                r += n
                q += n
            elif op == b"D":
                assert 0 <= r and r + n <= len(t), (f[:6], len(t))
                t[r:r + n, s, DEL] += 1
                r += n
            elif op == b"I":
                t[max(r, 1) - 1, s, INS] += 1
                q += n
            elif op == b"S":
                q += n
            else:
                raise AssertionError(f[5])
        assert q == len(seq), f[:10]
    return tables


def pileup_text(names, letters, tables, all_rows):
    """the TSV text without the header line: per sequence in order, per kept position "<name>\\t<pos, 1-based>\\t<ref letter>" and the eight values of every
    strand set.  Sites (default): a row is kept if any value other than the depth and the reference letter's own count is non-zero; all_rows: if any value is."""
    out = []
    for name, ref, t in zip(names, letters, tables):
        t = np.asarray(t)
        if all_rows:
            keep = t.reshape(len(t), -1).any(axis=1)
        else:
            own = np.array([_BASE[c] for c in ref], np.int64) if len(ref) else np.zeros(0, np.int64)
            other = t.copy()
            other[:, :, DEPTH] = 0
            other[np.arange(len(t)), :, own] = 0
            keep = other.reshape(len(t), -1).any(axis=1)
        for p in np.flatnonzero(keep).tolist():
            out.append(b"%s\t%d\t%c\t%s\n" % (name, p + 1, ref[p], b"\t".join(b"%d" % v for v in t[p].reshape(-1).tolist())))
    return b"".join(out)


def header_line(strands):
    """the header line the command writes in front of the text"""
    cols = [c + s for s in (("+", "-") if strands else ("",)) for c in COLUMNS]
    return ("#chrom\tpos\tref\t" + "\t".join(cols) + "\n").encode()
