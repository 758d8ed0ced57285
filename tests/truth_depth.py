"""What the truth depth (include/reseq_amd.h rsq_sim_depth_*; reseq_amd/csrc/rsq_depth.h) must be, from the truth records alone: the depth is a pure function of
the SAM text rsq_sim_pairs_sam writes for the same pairs, the bedGraph text a pure function of the depth.  Shared by tests/test_truth_depth.py (the per-lane
function on the CPU) and tests/test_truth_depth_gpu.py (the device); it shares no arithmetic with the kernels."""
import re

import numpy as np

_ELEMENT = re.compile(rb"(\d+)([MIDNSHP=X])")


def depth_from_sam(text, lengths, names=None):
    """[a uint32 array per sequence]: for every MAPPED record of the SAM text (header lines are skipped) one count on every reference position under an M element
    of its CIGAR, from POS on; D moves the position without counting, I and S neither.  lengths: the sequences' lengths, {RNAME: length} (in order) or a list
    beside `names`"""
    if not isinstance(lengths, dict):
        lengths = dict(zip(names, lengths))
    index = {name: i for i, name in enumerate(lengths)}
    depths = [np.zeros(n, np.uint32) for n in lengths.values()]
    starts, ends = [[] for _ in depths], [[] for _ in depths]
    for line in text.split(b"\n"):
        if not line or line[:1] == b"@":
            continue
        f = line.split(b"\t")
        if int(f[1]) & 0x4:
            continue
        seq, r = index[f[2]], int(f[3]) - 1
        assert f[5] == b"*" or b"".join(n + op for n, op in _ELEMENT.findall(f[5])) == f[5], f[5]
        for n, op in _ELEMENT.findall(f[5]):
            n = int(n)
            if op == b"M":
                assert 0 <= r and r + n <= len(depths[seq]), (f[:6], len(depths[seq]))
                starts[seq].append(r)
                ends[seq].append(r + n)
            if op in (b"M", b"D"):
                r += n
    for d, s, e in zip(depths, starts, ends):
        if not s:
            continue
        s, n = np.array(s, np.int64), np.array(e, np.int64) - np.array(s, np.int64)
        first = np.cumsum(n) - n                                  # every position under every M element, one np.add.at for the sequence
        np.add.at(d, np.repeat(s - first, n) + np.arange(int(n.sum())), 1)
    return depths


def bedgraph_from_depth(names, depths):
    """the bedGraph text: per sequence in order one line "<name>\\t<start>\\t<end>\\t<depth>\\n" per maximal run of equal depth, 0-based half-open, zero runs included"""
    out = []
    for name, d in zip(names, depths):
        d = np.asarray(d)
        if not len(d):
            continue
        cuts = np.concatenate([[0], np.flatnonzero(d[1:] != d[:-1]) + 1, [len(d)]])
        out += [b"%s\t%d\t%d\t%d\n" % (name, a, b, int(d[a])) for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist())]
    return b"".join(out)
