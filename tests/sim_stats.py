"""What the simulation report (include/reseq_amd.h rsq_sim_stats_*; reseq_amd/csrc/rsq_stats.h) must be, stated in numpy from the texts a pairs call writes: every
table is a pure function of the call's fragments and FASTQ texts (`from_fastq`), and -- all but the fragment-length table -- of its SAM text with the tags XC, XE
and MD (`from_sam`; the MD string itself is checked against tests/truth_md.py md_nm by the tests of the tags).  Shared by tests/test_sim_stats.py (the per-lane
functions on the CPU) and tests/test_sim_stats_gpu.py (the device); it shares no arithmetic with the kernels."""
import gzip
import re

import numpy as np

TABLES = ("pairs", "strand", "tile", "fragment_length", "read_length", "errors_per_read", "base_quality", "base_call", "insertion", "deletion", "adapter", "tail",
          "mismatch", "bad")
PER_SEGMENT = ("read_length", "errors_per_read", "base_quality", "base_call", "insertion", "deletion", "adapter", "tail", "mismatch")
_ELEMENT = re.compile(rb"(\d+)([MIDSH])")
_MD = re.compile(rb"(\d+)|\^([ACGTN]+)|([ACGTN])")
_CODE = np.full(256, 255, np.uint8)
_CODE[list(b"ACGTN")] = range(5)
_COMPLEMENT = bytes.maketrans(b"ACGTN", b"TGCAN")


def empty(lengths, F, Q, T):
    """zeroed tables for segments with read lengths up to lengths[s] - 1 (L_s = lengths[s]), fragment lengths up to F, quality values below Q, T tiles"""
    L = max(lengths)
    shape = dict(pairs=(2,), strand=(2,), tile=(T,), fragment_length=(F + 1,), read_length=(2, L + 1), errors_per_read=(2, L + 1), base_quality=(2, L, Q),
                 base_call=(2, L, 5), insertion=(2, L), deletion=(2, L), adapter=(2, L), tail=(2, L), mismatch=(2, L), bad=(1,))
    return {name: np.zeros(shape[name], np.uint64) for name in TABLES}


def add_cigar(t, seg, cigar, L):
    """the id's own CIGAR (the XC tag), walked with q = 0: M moves on; I, S and H mark their cycles; D adds its length at min(q, L - 1)"""
    elements = [(int(n), op) for n, op in _ELEMENT.findall(cigar)]
    assert b"".join(b"%d%s" % e for e in elements) == cigar, cigar
    q = 0
    for n, op in elements:
        if op == b"D":
            t["deletion"][seg, min(q, L - 1)] += n
            continue
        if op != b"M":
            assert q + n <= L, (cigar, L)
            t[{b"I": "insertion", b"S": "adapter", b"H": "tail"}[op]][seg, q:q + n] += 1
        q += n
    return q


def add_read(t, seg, seq, quality_values, cigar, errors, L):
    """one read as the FASTQ line has it: seq its letters, quality_values its qualities without the offset"""
    n = len(seq)
    assert n <= L and add_cigar(t, seg, cigar, L) == n, (cigar, n)
    t["read_length"][seg, n] += 1
    t["errors_per_read"][seg, min(errors, L)] += 1
    codes = _CODE[np.frombuffer(seq, np.uint8)]
    assert (codes < 5).all() and (quality_values < t["base_quality"].shape[2]).all()
    np.add.at(t["base_call"], (seg, np.arange(n), codes), 1)
    np.add.at(t["base_quality"], (seg, np.arange(n), quality_values), 1)


def add_frags(t, frags):
    """the per-pair tables that need the fragment list: pairs, strand, fragment_length"""
    lengths = np.asarray(frags["len"]).astype(np.int64)
    has = lengths > 0
    t["pairs"] += np.array([has.sum(), (~has).sum()], np.uint64)
    t["strand"] += np.bincount(np.asarray(frags["strand"])[has].astype(np.int64), minlength=2).astype(np.uint64)
    t["fragment_length"] += np.bincount(lengths[has], minlength=len(t["fragment_length"])).astype(np.uint64)


def from_fastq(frags, fastq1, fastq2, lengths, F, Q, T, phred_offset, tiles):
    """every table but mismatch; tiles: the profile's tile numbers in order"""
    t = empty(lengths, F, Q, T)
    add_frags(t, frags)
    tile_index = {int(v): i for i, v in enumerate(tiles)}
    for seg, text in enumerate((fastq1, fastq2)):
        lines = text.split(b"\n")
        assert lines[-1] == b"" and len(lines) % 4 == 1 and (len(lines) - 1) // 4 == len(frags)
        for i in range(0, len(lines) - 1, 4):
            qname, cigar, errors = lines[i][1:].split(b" ")
            add_read(t, seg, lines[i + 1], np.frombuffer(lines[i + 3], np.uint8).astype(np.int64) - phred_offset, cigar, int(errors[1:]), lengths[seg])
            if seg == 0 and int(frags["len"][i // 4]) > 0:
                t["tile"][tile_index[int(qname.split(b":")[-3])]] += 1
    return t


def mismatch_cycles(cigar, md, reverse, read_len):
    """the cycles of the M columns MD names as mismatches: cigar [(n, op)] of the SAM record, md its MD string"""
    at, wrong = 0, []                                          # index among the record's M columns
    for run, deleted, base in _MD.findall(md):
        if run:
            at += int(run)
        elif base:
            wrong.append(at)
            at += 1
    q, m, place = 0, 0, {}
    for n, op in cigar:
        if op == b"M":
            for k in range(n):
                place[m + k] = q + k
            m += n
        if op in (b"M", b"I", b"S"):
            q += n
    assert q == read_len and at == m, (cigar, md)
    return [read_len - 1 - place[w] if reverse else place[w] for w in wrong]


def from_sam(text, lengths, F, Q, T, tiles):
    """every table but fragment_length from SAM text with XC, XE and (mapped records) MD: two records a pair, the mate of segment 0 first"""
    t = empty(lengths, F, Q, T)
    tile_index = {int(v): i for i, v in enumerate(tiles)}
    lines = [l for l in text.split(b"\n") if l and l[:1] != b"@"]
    assert len(lines) % 2 == 0
    for line in lines:
        f = line.split(b"\t")
        flag = int(f[1])
        seg = 1 if flag & 0x80 else 0
        tags = {x[:2]: x[5:] for x in f[11:]}
        reverse = bool(flag & 0x10)
        seq, qual = (f[9].translate(_COMPLEMENT)[::-1], f[10][::-1]) if reverse else (f[9], f[10])
        add_read(t, seg, seq, np.frombuffer(qual, np.uint8).astype(np.int64) - 33, tags[b"XC"], int(tags[b"XE"]), lengths[seg])
        mapped = not flag & 0x4
        if seg == 0:
            t["pairs"][0 if mapped else 1] += 1
            if mapped:
                t["strand"][1 if reverse else 0] += 1           # (the mate of segment 0 reads the reverse strand when the fragment's strand is 1)
                t["tile"][tile_index[int(f[0].split(b":")[-3])]] += 1
        if mapped:
            cigar = [(int(n), op) for n, op in _ELEMENT.findall(f[5])] if f[5] != b"*" else []
            for c in mismatch_cycles(cigar, tags[b"MD"], reverse, len(seq)):
                t["mismatch"][seg, c] += 1
    return t


def parse_report(path):
    """(dimensions {name: [int]}, tables {name: {(segment, i, j): count}}) of a --simStats file; checks the order of its lines"""
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        lines = f.read().split(b"\n")
    assert lines[0] == b"#reseq_amd simStats v1" and lines[-1] == b""
    dims, tables, keys = {}, {}, []
    for line in lines[1:-1]:
        f = line.split(b"\t")
        if line[:1] == b"#":
            assert not keys, "the '#' lines come first"
            dims[f[0][1:].decode()] = [int(x) for x in f[1:]]
            continue
        name, index, count = f[0].decode(), tuple(None if x == b"." else int(x) for x in f[1:4]), int(f[4])
        assert count > 0 and len(f) == 5
        tables.setdefault(name, {})[index] = count
        keys.append((TABLES.index(name),) + tuple(-1 if x is None else x for x in index))
    assert keys == sorted(keys) and len(set(keys)) == len(keys), "tables by id, indices ascending"
    return dims, tables


def report_tables(path):
    """the report as arrays shaped like `empty`'s"""
    dims, tables = parse_report(path)
    t = empty(dims["read_length"], dims["insert_to"][0], dims["n_quality"][0], dims["n_tiles"][0])
    for name, cells in tables.items():
        for (seg, i, j), count in cells.items():
            assert (seg is not None) == (name in PER_SEGMENT) and (j is not None) == (name in ("base_quality", "base_call")) and (i is None) == (name == "bad")
            index = tuple(x for x in (seg, 0 if i is None else i, j) if x is not None)
            t[name][index] = count
    return dims, t
