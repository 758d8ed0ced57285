"""The case tables of tests/hostemu/kernel_trial.cpp, what every case must give, and the checkers (tests/test_kernel_trial.py shows that each of them has teeth,
tests/test_kernel_trial_gpu.py runs the trial on the device).

The trial runs the library's cooperative kernels alone -- the scan, the sorted BAM's radix passes, cut, gather and index kernels, the bins' plan and scatter, the
FASTA record starts; the truth depth's in-place prefix sum (depthscan) and bedGraph text (bedgraph), the truth pileup's rows and TSV text (pileup), the simulation
report's rows kernel and its ballot-aggregated adds (stats): device-only code that the host emulation replaces with a loop.  The references here are plain numpy and
plain loops, written from what the kernels are meant to give (an exclusive prefix sum, a stable sort, a copy, a histogram, a cumulative sum, a bedGraph line ...),
not from their code; the texts are those of tests/truth_depth.py and tests/truth_pileup.py.  The arrays of the last four families lie between guard bytes, which the
checkers compare; a depth, pileup or reference array may exist from a position `base` on only (the trial moves the address back), so positions of ten digits need
no large array.  Every comparison is exact: integers and bytes,
no tolerance.  Seeds are fixed.

A case: sixteen parameter words and blobs (the trial's head comment has the file format); reference(case) gives the result blobs a right kernel leaves, in the
trial's form, check(case, blobs) the complaints about a result (none: it is right)."""
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hostemu", "kernel_trial.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "reseq_amd", "csrc")
WARNINGS = ["-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-result"]       # tests/hostemu/Makefile: TRIALFLAGS
FAMILIES = ["scan", "sort", "gather", "index", "bins", "fasta", "depthscan", "bedgraph", "pileup", "stats"]
CHILD_LIMIT = 120                            # seconds per child process: test_portable_gpu.py's

M32 = 0xFFFFFFFF
GUARD8, GUARD32, GUARD64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
DIR = np.dtype([("key", "<u8"), ("off", "<u8"), ("size", "<u4"), ("span", "<u4")])            # BamDirEntry
RUN = np.dtype([("ref", "<u4"), ("bin", "<u4"), ("begin", "<u8")])                             # BamRunStart
FRAGMENT_BYTES = 24                                                                            # sizeof(Fragment): the trial refuses a case of another size


class Case:
    def __init__(self, name, par, blobs, **facts):
        self.name, self.par, self.blobs = name, [int(p) for p in par], [np.ascontiguousarray(b) for b in blobs]
        self.__dict__.update(facts)

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------------------------------- files and the program
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], U64).tobytes())
        for c in cases:
            assert len(c.par) <= 16
            f.write(np.array(c.par + [0] * (16 - len(c.par)), U64).tobytes())
            for b in c.blobs:
                raw = b.tobytes()
                f.write(np.array([len(raw)], U64).tobytes() + raw + b"\0" * (-len(raw) % 8))


def read_blobs(path):
    """every blob of a result file, as bytes"""
    raw, at, out = np.fromfile(path, U8), 0, []
    while at < len(raw):
        size = int(raw[at:at + 8].view(U64)[0])
        out.append(raw[at + 8:at + 8 + size])
        at += 8 + size + (-size % 8)
    return out


def results_of(family, cases, blobs):
    """the blobs case by case"""
    out, at = [], 0
    for c in cases:
        k = _BLOBS[family](c) if family in _BLOBS else len(reference(family, c))
        out.append(blobs[at:at + k])
        at += k
    assert at == len(blobs), (family, at, len(blobs))
    return out


def library_arch():
    return re.search(r"^ARCH \?= (\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)


def build(directory, hipcc):
    """the trial for the library's architecture with the library's flags (tests/hostemu/Makefile builds the same for build())"""
    exe = os.path.join(str(directory), "kernel_trial")
    subprocess.run([hipcc, "-x", "hip", f"--offload-arch={library_arch()}", "-O3", "-std=c++17", "-ffp-contract=off", "-Werror", *WARNINGS, "-o", exe, SOURCE], check=True)
    return exe


def _offsets(sizes):
    """n + 1 offsets in uint64: the exclusive prefix sum and the total"""
    return np.concatenate([np.zeros(1, U64), np.cumsum(sizes, dtype=U64)])


def _same(what, got, want):
    """a complaint if the blob `got` is not the array `want`"""
    got = np.frombuffer(np.ascontiguousarray(got).tobytes(), U8)
    raw = np.frombuffer(np.ascontiguousarray(want).tobytes(), U8)
    if len(got) != len(raw):
        return [f"{what}: {len(got)} bytes, not {len(raw)}"]
    if want.dtype.names is None and want.dtype.itemsize > 1:
        g = got.view(want.dtype)
        bad = np.flatnonzero(g != want.ravel())
        return [f"{what}: {len(bad)} wrong, the first at {bad[0]}: {int(g[bad[0]]):#x}, not {int(want.ravel()[bad[0]]):#x}"] if len(bad) else []
    bad = np.flatnonzero(got != raw)
    return [f"{what}: {len(bad)} bytes wrong, the first at byte {bad[0]}: {int(got[bad[0]]):#x}, not {int(raw[bad[0]]):#x}"] if len(bad) else []


def _compare(names, got, want):
    if len(got) != len(want):
        return [f"{len(got)} result blobs, not {len(want)}"]
    return [line for name, g, w in zip(names, got, want) for line in _same(name, g, w)]


# ------------------------------------------------------------------------------------------------------------------------- scan
SCAN_TILE = 4096                             # kScanTile; kScanTilesBlock = 1024 tiles and more give a thread of k_scan_tiles two tiles
SCAN_N = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 5, 1024 * 4096, 1024 * 4096 + 1]
SCAN_INIT = [None, 0, (1 << 32) - 5, (1 << 40) + 3]


def scan_cases():
    rng = np.random.default_rng(4096)
    cases = []

    def add(kind, n, arrays, init, in_shift=0, out_shift=0, longest=0):
        total = n * arrays
        if kind == "small":
            v = rng.integers(0, 600, total)
        elif kind == "zero":
            v = np.zeros(total)
        elif kind == "ones":
            v = np.full(total, M32)
        elif kind == "spike":                # 2^31 at the last place of a tile and at the first of the next
            v = rng.integers(0, 600, total)
            for at in range(SCAN_TILE - 1, total - 1, SCAN_TILE):
                v[at] = v[at + 1] = 1 << 31
        else:
            v = np.arange(total) * 3 + 1     # a ramp
        cases.append(Case(f"scan {kind} n={n} arrays={arrays} init={init} in+{in_shift} out+{out_shift}", [n, arrays, init is not None, init or 0, in_shift, out_shift, longest],
                          [v.astype(U32)], n=n, arrays=arrays, init=init, longest=longest))

    for k, n in enumerate(SCAN_N[:-2]):      # every n, the inits and one or two arrays in turn (n odd: the second array is not aligned)
        add("small", n, 1 + k % 2, SCAN_INIT[k % 4])
        add("small", n, 2 - k % 2, SCAN_INIT[(k + 2) % 4])
    for n in (1, 64, 4097):
        add("zero", n, 1 + n % 2, None, longest=5)                   # longest stays what it was
    add("ones", 4097, 2, (1 << 32) - 5)
    add("spike", 4097, 1, None)
    add("spike", 3 * 4096 + 5, 2, (1 << 40) + 3)
    add("ramp", 4097, 1, 0)
    add("ramp", 1024 * 4096, 1, (1 << 40) + 3)                       # 1024 tiles: the last n with one tile a thread
    add("ones", 1024 * 4096 + 1, 1, None)                            # 1025 tiles: two a thread, half the threads without any; sums of 2^54
    add("small", 1024 * 4096 + 1, 2, (1 << 32) - 5)
    for n in (4095, 4096, 4097):             # in 0 .. 3 elements and out 0 or 1 element behind a 16-byte boundary
        for in_shift in range(4):
            for out_shift in range(2):
                add("small", n, 1 + (in_shift + out_shift) % 2, SCAN_INIT[(in_shift + n) % 4], in_shift, out_shift)
    return cases


def scan_reference(c):
    """out[i] = init + sum(in[:i]) for i = 0 .. n in uint64, between two guard words on either side; the totals; the largest element (or what longest held)"""
    v = c.blobs[0].reshape(c.arrays, c.n)
    outs, totals = [], np.full(2, GUARD64, U64)
    for k in range(c.arrays):
        first = 0 if c.init is None else c.init + k                  # (the trial gives the second array the first one's init + 1)
        out = _offsets(v[k]) + U64(first)
        totals[k] = out[-1]
        outs.append(np.concatenate([np.full(2, GUARD64, U64), out, np.full(2, GUARD64, U64)]))
    return outs + [totals, np.array([max(c.longest, int(v.max()))], U32)]


def scan_check(c, got):
    return _compare([f"out[{k}] (two guard words in front)" for k in range(c.arrays)] + ["totals", "longest"], got, scan_reference(c))


# ------------------------------------------------------------------------------------------------------------------------- sort
SORT_TILE = 1024                             # kBamSortTile
SORT_PLANS = {(1, 255): 2, (3, 5000): 2, (3, 140000): 3, (25, 250_000_000): 5, (3000, M32): 6, (1 << 20, M32): 7}      # (n_seqs, longest): passes
SORT_N = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4 * 1024 + 1, 100 * 1024 + 77]
SORT_SHAPES = ["uniform", "equal", "alternating", "ascending", "descending", "runs64", "runs256", "distinct64", "unmapped"]
CUT_ALL = (1 << 64) - 1                      # kBamCutAll
SORT_OUT_OF_ORDER = 3                        # what the trial puts where k_bam_cut reads the count of records out of order


def sort_plan(n_seqs, longest):
    pos_bits = int(longest).bit_length()
    bits = pos_bits + int(n_seqs).bit_length()
    return pos_bits, bits, (bits + 7) // 8


def _key_of_packed(packed, n_seqs, longest):
    """the key whose digits are, as far as the plan's range lets them, those of `packed`"""
    pos_bits = sort_plan(n_seqs, longest)[0]
    pos = packed & ((1 << pos_bits) - 1)
    pos = np.where(pos > longest, pos & ((1 << (pos_bits - 1)) - 1), pos)
    return (((packed >> pos_bits) % n_seqs) << 32 | pos).astype(U64)


def sort_keys(shape, n, n_seqs, longest, rng):
    uniform = (rng.integers(0, n_seqs, n).astype(U64) << U64(32)) | rng.integers(0, longest + 1, n).astype(U64)
    if n >= 4:                               # (some key several times, whatever the range: the cut that equals a key has something to hold)
        uniform[[n // 3, n // 2, n - 1]] = uniform[0]
    i = np.arange(n, dtype=np.int64)
    passes = sort_plan(n_seqs, longest)[2]
    if shape == "uniform":
        return uniform
    if shape == "equal":
        return np.full(n, uniform[0], U64)
    if shape == "alternating":
        return uniform[:2][i % 2] if n > 1 else uniform
    if shape == "ascending":
        return np.sort(uniform)
    if shape == "descending":
        return np.sort(uniform)[::-1].copy()
    if shape in ("runs64", "runs256"):       # every digit the same along a run, another one in the next run
        run = i // int(shape[4:])
        return _key_of_packed(sum(((run * 37 + 11 * p + 5) & 0xFF) << (8 * p) for p in range(passes)), n_seqs, longest)
    if shape == "distinct64":                # i times an odd number: 64 different digits in any 64 consecutive items
        return _key_of_packed(sum(((i * (2 * p + 3) + p) & 0xFF) << (8 * p) for p in range(passes)), n_seqs, longest)
    assert shape == "unmapped"
    return np.where(rng.random(n) < 0.1, U64(n_seqs << 32), uniform)


def sort_cases():
    rng = np.random.default_rng(1024)
    cases = []

    def add(shape, n, plan):
        n_seqs, longest = plan
        keys = sort_keys(shape, n, n_seqs, longest, rng)
        unmapped = n_seqs << 32
        mapped = keys[keys < U64(unmapped)]
        values, counts = np.unique(keys, return_counts=True)
        cuts = [0, int(keys.min()), int(values[np.argmax(counts)]), int(mapped.max()) + 1 if len(mapped) else 0, unmapped, CUT_ALL]
        cases.append(Case(f"sort {shape} n={n} plan={plan}", [n, n_seqs, longest, SORT_OUT_OF_ORDER], [keys, rng.integers(1, 500, n).astype(U32), np.array(cuts, U64)],
                          n=n, plan=plan, unmapped=unmapped))

    for plan in SORT_PLANS:                  # every number of passes
        add("uniform", 4 * 1024 + 1, plan)
    # every key shape at the plan with the seam inside a digit and at the human-sized one; every n once, the runs over more than one tile
    for plan, sizes in (((3, 5000), [1, 63, 64, 65, 255, 1025, 4 * 1024 + 1, 1023, 1024]), ((25, 250_000_000), [256, 257, 100 * 1024 + 77, 1023, 1025, 4 * 1024 + 1, 4 * 1024 + 1, 1024, 4 * 1024 + 1])):
        for shape, n in zip(SORT_SHAPES, sizes):
            add(shape, n, plan)
    return cases


def sort_reference(c):
    """the stable order, the keys in it, k_bam_cut's six words per cut, the plan"""
    keys, sizes, cuts = c.blobs
    order = np.argsort(keys, kind="stable")
    sorted_keys = keys[order]
    at = _offsets(sizes[order])
    words = []
    for cut in cuts:
        n_final = c.n if int(cut) == CUT_ALL else int(np.searchsorted(sorted_keys, cut, side="left"))      # a key equal to the cut is held
        n_mapped = int(np.searchsorted(sorted_keys[:n_final], U64(c.unmapped), side="left"))
        words += [n_final, n_mapped, at[n_final], at[n_mapped], at[c.n], SORT_OUT_OF_ORDER]
    return [sorted_keys, order.astype(U32), np.array(words, U64), np.array(sort_plan(*c.plan), U32)]


def sort_check(c, got):
    return _compare(["sorted keys", "order", "cut words", "plan"], got, sort_reference(c))


# ------------------------------------------------------------------------------------------------------------------------- gather
GATHER_SIZES = [1, 15, 16, 17, 31, 32, 33, 36, 100, 255, 256, 257, 271, 272, 273, 400, 700]
MARKER = 64


def _gather_case(name, rng, sizes, src_mod, n_final, out_lead, held_lead, gaps=True):
    """records of `sizes` in their order in the sorted stream; record j lies in the staging buffer at an offset of src_mod[j] mod 16 (None: any), the staging
    buffer in another order than the stream"""
    n = len(sizes)
    stage_order = rng.permutation(n)
    off = np.zeros(n, np.int64)
    at = 0
    for j in stage_order:
        at += int(rng.integers(0, 40)) if gaps else 0
        if src_mod[j] is not None:
            at += (src_mod[j] - at) % 16
        off[j] = at
        at += sizes[j]
    stage = rng.integers(0, 256, at).astype(U8)
    entries = np.zeros(n, DIR)
    entries["key"], entries["off"], entries["size"], entries["span"] = rng.integers(0, 1 << 40, n), off, sizes, rng.integers(0, 1000, n)
    idx = rng.permutation(n).astype(U32)     # the directory in a third order: entry idx[j] is record j of the stream
    directory = np.zeros(n, DIR)
    directory[idx] = entries
    total, final = int(np.sum(sizes)), int(np.sum(sizes[:n_final]))
    return Case(name, [n, n_final, final, total - final, out_lead, held_lead], [directory, idx, stage], n=n, n_final=n_final, out_lead=out_lead, held_lead=held_lead, entries=entries)


def gather_cases():
    rng = np.random.default_rng(16)
    cases = []
    big = [s for s in GATHER_SIZES if s >= 36]
    for n in (1, 15, 16, 17):
        for n_final in sorted({0, n // 2, n}):
            sizes = np.array([GATHER_SIZES[(j * 5 + n + n_final) % len(GATHER_SIZES)] for j in range(n)])
            cases.append(_gather_case(f"gather n={n} final={n_final}", rng, sizes, [None] * n, n_final, int(rng.integers(0, 16)), int(rng.integers(0, 16))))
    # every (source, destination) pair of offsets mod 16 for records with aligned words in the middle: a small record in front of each moves the destination on
    for n_final_of, out_lead, held_lead in ((lambda n: n, 0, 0), (lambda n: n // 2, 5, 11), (lambda n: 0, 3, 0)):
        sizes, src, at = [], [], 0
        for k, pair in enumerate(rng.permutation(256)):
            s, d = int(pair) // 16, int(pair) % 16
            fill = (d - at - 1) % 16 + 1                             # 1 .. 16 bytes
            sizes += [fill, big[k % len(big)]]
            src += [None, s]
            at += fill + sizes[-1]
        n = len(sizes)
        cases.append(_gather_case(f"gather pairs final={n_final_of(n)} of {n}", rng, np.array(sizes), src, n_final_of(n), out_lead, held_lead))
    # the sizes at which the head and the tail meet, at every destination offset; no gaps in the staging buffer: its last record ends where the buffer does
    sizes, at = [], 0
    for d in range(16):
        for s in GATHER_SIZES[:8]:
            fill = (d - at - 1) % 16 + 1
            sizes += [fill, s]
            at += fill + s
    cases.append(_gather_case("gather short sizes", rng, np.array(sizes), [None] * len(sizes), len(sizes) // 2, 0, 7, gaps=False))
    return cases


def gather_pairs(c):
    """(source, destination) offsets mod 16 of the records of 36 bytes and more, with the destinations on 16-byte boundaries plus the case's leads"""
    e = c.entries
    at = np.concatenate([[0], np.cumsum(e["size"].astype(np.int64))])[:-1]
    dst = np.where(np.arange(c.n) < c.n_final, at + c.out_lead, at - at[c.n_final] + c.held_lead if c.n_final < c.n else 0)
    return {(int(s) % 16, int(d) % 16) for s, d, size in zip(e["off"], dst, e["size"]) if size >= 36}


def gather_reference(c):
    """out: the final records in the stream's order; held: the others; both between 64 marker bytes; the held records' directory; the scanned sizes"""
    stage, e = c.blobs[2], c.entries
    records = [stage[int(o):int(o) + int(s)] for o, s in zip(e["off"], e["size"])]
    marker = np.full(MARKER, GUARD8, U8)
    out = np.concatenate([marker] + records[:c.n_final] + [marker])
    held = np.concatenate([marker] + records[c.n_final:] + [marker])
    at = _offsets(e["size"])
    held_dir = np.zeros(c.n - c.n_final + 1, DIR)
    held_dir[:-1] = e[c.n_final:]
    held_dir["off"][:-1] = at[c.n_final:-1] - at[c.n_final]
    held_dir[-1:] = np.frombuffer(bytes([GUARD8]) * DIR.itemsize, DIR)
    return [out, held, held_dir, at]


def gather_check(c, got):
    want = gather_reference(c)
    if len(got) != 4:
        return [f"{len(got)} result blobs, not 4"]
    lines = []
    for name, g, w in (("out", got[0], want[0]), ("held", got[1], want[1])):
        g = np.frombuffer(np.ascontiguousarray(g).tobytes(), U8)
        if len(g) != len(w):
            lines.append(f"{name}: {len(g)} bytes, not {len(w)}")
            continue
        lines += _same(f"{name}: the marker in front", g[:MARKER], w[:MARKER]) + _same(f"{name}: the marker behind", g[-MARKER:], w[-MARKER:])
        lines += _same(f"{name}: the records", g[MARKER:-MARKER], w[MARKER:-MARKER])
    return lines + _same("held directory (one guard entry behind)", got[2], want[2]) + _same("scanned sizes", got[3], want[3])


# ------------------------------------------------------------------------------------------------------------------------- index
INDEX_SEQ_LEN = [300_000, 50_000, 200_000]   # the middle one without records
WINDOW_SHIFT = 14
NO_OFFSET = (1 << 64) - 1                    # kBamNoOffset
INDEX_SPANS = [1, 30, 150, 16384, 40000]
INDEX_N = [1, 255, 256, 257, 3000]
STREAM_AT = (1 << 33) + 12345


def reg2bin(beg, end):
    """SAM specification 5.3"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def _index_case(name, rng, records):
    """records: (sequence, position, span), made the sorted stream here (stable by sequence and position)"""
    records = sorted(records, key=lambda r: (r[0], r[1]))
    n = len(records)
    entries = np.zeros(n, DIR)
    entries["key"] = [(s << 32) | p for s, p, _ in records]
    entries["span"] = [span for _, _, span in records]
    entries["size"] = rng.integers(50, 400, n)
    entries["off"] = rng.integers(0, 1 << 30, n)
    idx = rng.permutation(n).astype(U32)
    directory = np.zeros(n, DIR)
    directory[idx] = entries
    at = _offsets(entries["size"])
    window_first = np.concatenate([[0], np.cumsum([(l >> WINDOW_SHIFT) + 1 for l in INDEX_SEQ_LEN])]).astype(U64)
    return Case(name, [n, STREAM_AT, len(INDEX_SEQ_LEN)], [directory, idx, at, window_first], n=n, records=records, at=at, window_first=window_first)


def index_cases():
    rng = np.random.default_rng(16384)
    cases = []
    # a short record behind a long one that reaches further (twice over), then records in the windows the long ones cover, one past every seam
    cases.append(_index_case("index a short record behind a long one", rng, [
        (0, 100, 40000), (0, 200, 30), (0, 300, 16384), (0, 310, 1), (0, 16383, 1), (0, 16384, 1), (0, 16390, 40000), (0, 20000, 30), (0, 33000, 150), (0, 40000, 1),
        (0, 131071, 1), (0, 131071, 2), (0, 131072, 150), (0, 299990, 30), (0, 299999, 1), (2, 0, 1), (2, 16383, 150), (2, 199000, 40000)]))

    def place(seq):
        length = INDEX_SEQ_LEN[seq]
        kind = rng.integers(0, 4)
        if kind == 0:
            return int(rng.integers(16384 - 200, 16384 + 200))
        if kind == 1:
            return int(rng.integers(131072 - 200, 131072 + 200))
        if kind == 2:
            return int(rng.integers(length - 200, length))
        return int(rng.integers(0, length))

    for n in INDEX_N:
        records = []
        for _ in range(n):
            seq = 0 if rng.random() < 0.6 else 2
            records.append((seq, place(seq), INDEX_SPANS[int(rng.integers(0, len(INDEX_SPANS)))]))
        cases.append(_index_case(f"index n={n}", rng, records))
    return cases


def index_reference(c):
    """by plain loops: where (sequence, bin) changes; those records' runs; the smallest offset per 16 kb window over the records that overlap it"""
    flags = np.zeros(c.n, U32)
    runs = []
    windows = np.full(int(c.window_first[-1]) + 1, NO_OFFSET, U64)   # (the last: what the trial leaves behind the windows)
    before = None
    for i, (seq, pos, span) in enumerate(c.records):
        here = (seq, reg2bin(pos, pos + span))
        offset = STREAM_AT + int(c.at[i])
        if here != before:
            flags[i] = 1
            runs.append((seq, here[1], offset))
        before = here
        first, n_windows = int(c.window_first[seq]), int(c.window_first[seq + 1] - c.window_first[seq])
        for w in range(pos >> WINDOW_SHIFT, min(((pos + span - 1) >> WINDOW_SHIFT) + 1, n_windows)):
            windows[first + w] = min(int(windows[first + w]), offset)
    run_blob = np.zeros(len(runs) + 1, RUN)
    run_blob[:-1] = np.array(runs, RUN)
    run_blob[-1:] = np.frombuffer(bytes([GUARD8]) * RUN.itemsize, RUN)
    return [flags, run_blob, windows]


def index_check(c, got):
    return _compare(["flags", "runs (one guard entry behind)", "windows"], got, index_reference(c))


# ------------------------------------------------------------------------------------------------------------------------- bins
BIN_KEYS_LDS = 4096                          # kBinKeysLds: more keys take the counting and scattering kernels' other branch
BINS_KEYS = [1, 2, 3, 96, 192, 1023, 1024, 1025, 4096, 4097]
BINS_N = [1, 4095, 4096, 4097, 3 * 4096 + 5, 40 * 4096 + 1]          # a scatter workgroup takes 4096 items
BINS_SHAPES = ["uniform", "first", "last", "once", "half"]


def bins_cases():
    rng = np.random.default_rng(64)
    cases = []

    def add(shape, n, n_keys, pairs, frags=False):
        if shape == "uniform":
            keys = rng.integers(0, n_keys, n)
        elif shape == "first":
            keys = np.zeros(n)
        elif shape == "last":
            keys = np.full(n, n_keys - 1)
        elif shape == "once":                # every key once
            n = n_keys
            keys = rng.permutation(n_keys)
        else:                                # every other key without items
            keys = rng.integers(0, (n_keys + 1) // 2, n) * 2
        n_bins = 2 * n_keys if pairs else n_keys
        blobs = [keys.astype(U16), rng.integers(0, 256, (n, FRAGMENT_BYTES)).astype(U8) if frags else np.zeros(0, U8)]
        cases.append(Case(f"bins {shape} n={n} keys={n_keys} bins={n_bins}" + (" with fragments" if frags else ""), [n, n_keys, n_bins, frags], blobs, n=n, n_keys=n_keys, n_bins=n_bins,
                          frags=frags))

    for k, n_keys in enumerate(BINS_KEYS):
        add("uniform", BINS_N[k % len(BINS_N)], n_keys, k % 2 == 0)
        add("uniform", BINS_N[(k + 3) % len(BINS_N)], n_keys, k % 2 == 1)
    for k, n in enumerate(BINS_N):
        add("uniform", n, 96, k % 2 == 1)
    for n_keys in (1, 3, 1025, 4096, 4097):
        for k, shape in enumerate(BINS_SHAPES[1:]):
            add(shape, 3 * 4096 + 5, n_keys, (k + n_keys) % 2 == 0)
    add("uniform", 4097, 192, True, frags=True)
    return cases


def bins_reference(c):
    """the small arrays as the library lays them out and a guard word; the cursors before the scatter; one right perm (a bin's items in rising order -- the kernel
    may leave them in any order) and a guard word; the fragments in that order"""
    keys = c.blobs[0].astype(np.int64)
    hist = np.bincount(keys, minlength=c.n_keys)
    first = np.concatenate([[0], np.cumsum(hist)])[:-1]
    bin_count = hist[np.arange(c.n_bins) % c.n_keys]
    chunk_ptr = np.concatenate([[0], np.cumsum((bin_count + 63) // 64)])
    zeros = np.zeros(c.n_bins)
    small = np.concatenate([hist, first + hist, first[np.arange(c.n_bins) % c.n_keys], bin_count, zeros, zeros, chunk_ptr, [GUARD32]]).astype(U32)
    perm = np.argsort(keys, kind="stable")
    frags = c.blobs[1].reshape(-1, FRAGMENT_BYTES)[perm] if c.frags else np.zeros(0, U8)
    return [small, first.astype(U32), np.concatenate([perm, [GUARD32]]).astype(U32), frags]


def bins_check(c, got):
    """The order of a bin's items comes from atomics and is not fixed: perm must be a permutation of 0 .. n whose stretch [bin_first[k], + hist[k]) holds, as a set,
    exactly the items of key k -- that is: the keys along perm rise -- and the fragments must follow perm as it is."""
    want = bins_reference(c)
    if len(got) != 4:
        return [f"{len(got)} result blobs, not 4"]
    lines = _same("hist, cursor, bin_first, bin_count, next_chunk, workers, chunk_ptr and a guard word", got[0], want[0]) + _same("the plan's cursors", got[1], want[1])
    perm = np.frombuffer(np.ascontiguousarray(got[2]).tobytes(), U8)
    if len(perm) != 4 * (c.n + 1):
        return lines + [f"perm: {len(perm)} bytes, not {4 * (c.n + 1)}"]
    perm = perm.view(U32)
    if perm[-1] != GUARD32:
        lines.append("perm: the guard word behind it is overwritten")
    perm = perm[:-1].astype(np.int64)
    if not np.array_equal(np.sort(perm), np.arange(c.n)):
        return lines + ["perm is no permutation of the items"]
    keys = c.blobs[0].astype(np.int64)
    bad = np.flatnonzero(keys[perm] != np.sort(keys))
    if len(bad):
        lines.append(f"perm: {len(bad)} items outside their bins, the first at {bad[0]}: item {perm[bad[0]]} of key {keys[perm[bad[0]]]} in the bin of key {np.sort(keys)[bad[0]]}")
    if c.frags:
        lines += _same("the fragments in perm's order", got[3], c.blobs[1].reshape(-1, FRAGMENT_BYTES)[perm])
    else:
        lines += _same("no fragments", got[3], np.zeros(0, U8))
    return lines


# ------------------------------------------------------------------------------------------------------------------------- fasta starts
FASTA_TILE = 4096                            # kTileBytes; a lane takes two words of 8 bytes, a step 1024 bytes, a workgroup four tiles
FASTA_SEAMS = [8, 16, 24, 1016, 1024, 1032, 4088, 4096, 4104, 12288, 16384]
FASTA_LENGTHS = [1, 2, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385]
FASTA_SHIFTS = [0, 1, 5, 15]
GT, NL, CR, A = (ord(ch) for ch in ">\n\rA")


def fasta_cases():
    rng = np.random.default_rng(62)
    cases = []

    def add(name, text, shift=0):
        cases.append(Case(f"fasta {name} +{shift}", [shift], [np.asarray(text, U8)], shift=shift))

    for b in FASTA_SEAMS:                    # a '>' on either side of every seam, behind a line end and behind what is none
        for o in (b - 1, b, b + 1):
            for front, name in ((NL, "\\n>"), (CR, "\\r>"), (A, "A>"), (GT, ">>")):
                for shift in FASTA_SHIFTS:
                    text = np.full(20000, A, U8)
                    text[o - 1], text[o] = front, GT
                    add(f"{name} at {o}", text, shift)
    for length in FASTA_LENGTHS:             # the text ends next to the seams: with a start as its last byte, with a line end as its last byte
        text = np.full(length, A, U8)
        text[-1] = GT
        if length > 1:
            text[-2] = NL
        add(f"{length} bytes, a start the last", text)
        text = np.full(length, A, U8)
        text[-1] = NL
        add(f"{length} bytes, a line end the last", text, shift=length % 16)
    for name, unit in (("\\n> repeated", [NL, GT]), (">\\n repeated", [GT, NL]), ("all >", [GT]), ("all \\n", [NL])):
        add(name, np.tile(np.array(unit, U8), 20000 // len(unit)))
    for k in range(40):
        add(f"random {k}", rng.choice(np.array([GT, NL, CR, A], U8), int(rng.integers(1, 70001)), p=[0.3, 0.3, 0.1, 0.3]), shift=int(rng.integers(0, 16)) if k % 2 else 0)
    return cases


def fasta_reference(c):
    """the starts: a '>' at offset 0 or behind a line feed (tests/test_fasta_records.py: records_of); their counts per tile; the starts, the text's length and a
    guard word; k_fasta_lead's flag: a byte that is no line end in front of the first start"""
    text = c.blobs[0]
    behind_nl = np.concatenate([[True], text[:-1] == NL])
    starts = np.flatnonzero((text == GT) & behind_nl)
    counts = np.bincount(starts // FASTA_TILE, minlength=-(-len(text) // FASTA_TILE)).astype(U32)
    lead = text[:starts[0] if len(starts) else len(text)]
    flag = int(np.any((lead != NL) & (lead != CR)))
    return [counts, np.concatenate([starts, [len(text), GUARD32]]).astype(U32), np.array([0, 0, flag, 0], U32)]


def fasta_check(c, got):
    return _compare(["counts per tile", "starts, the text's length, a guard word", "summary"], got, fasta_reference(c))


# ------------------------------------------------------------------------------------------------------------------------- guarded arrays, text through the image
def _guarded(a):
    """the array as the trial emits it: MARKER guard bytes in front and behind"""
    marker = np.full(MARKER, GUARD8, U8)
    return np.concatenate([marker, np.frombuffer(np.ascontiguousarray(a).tobytes(), U8), marker])


def _same_guarded(what, got, want):
    """complaints about a guarded blob: its size, the guards, the array (want: the guarded reference, dtype: the array's)"""
    got = np.frombuffer(np.ascontiguousarray(got).tobytes(), U8)
    raw = np.frombuffer(np.ascontiguousarray(want[0]).tobytes(), U8)
    if len(got) != len(raw):
        return [f"{what}: {len(got)} bytes, not {len(raw)}"]
    lines = _same(f"{what}: the guard in front", got[:MARKER], raw[:MARKER]) + _same(f"{what}: the guard behind", got[-MARKER:], raw[-MARKER:])
    return lines + _same(what, got[MARKER:-MARKER].view(want[1]) if want[1] != U8 else got[MARKER:-MARKER], raw[MARKER:-MARKER].view(want[1]))


def _name_of(length):
    """a sequence name of so many characters"""
    return (b"chr" + b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ_.-" * (length // 60 + 1))[:length] if length > 1 else b"X"


IMAGE_MAX = 32 * 1024                        # kDepthLdsMax, kPileupLdsMax


def depth_lds_bytes(name_len):
    """rsq_depth.h: 64 lines of a name and three numbers at their widest, whole 128 bytes, at most 32 KiB"""
    return min(IMAGE_MAX, (64 * (name_len + 34) + 16 + 127) & ~127)


def pileup_lds_bytes(name_len, sets):
    """rsq_pileup.h: 64 lines at their widest"""
    return min(IMAGE_MAX, (64 * (name_len + 14 + 88 * sets) + 16 + 127) & ~127)


def text_waves(pieces, lead, lds):
    """(skew, bytes, through the image) of every wave of 64 lines: pieces: the lines (bytes) of every piece, written one behind the other from `lead` bytes behind a
    16-byte boundary on; a wave goes through the image if skew + bytes <= lds, else its lanes write straight to memory (WaveImage of rsq_format.h)"""
    out, at = [], lead
    for lines in pieces:
        for first in range(0, len(lines), 64):
            size = sum(len(line) for line in lines[first:first + 64])
            out.append((at % 16, size, at % 16 + size <= lds))
            at += size
    return out


# ------------------------------------------------------------------------------------------------------------------------- depth: the in-place prefix sum
DEPTH_TILE = 4096                            # kDepthTile; kDepthTilesBlock = 1024: more tiles give a thread of k_depth_tiles two and three
DEPTHSCAN_TILES = [1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 3000]
DEPTHSCAN_KINDS = ["random", "ones", "pairs", "spike", "zero"]


def depthscan_cases():
    rng = np.random.default_rng(20)
    cases = []

    def add(kind, tiles):
        n = tiles * DEPTH_TILE
        if kind == "random":                 # all 32 bits: the sums wrap at every few words
            v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
        elif kind == "ones":
            v = np.full(n, M32, U32)
        elif kind == "pairs":                # the product's: +1 where an M run begins, 0xFFFFFFFF behind it
            starts = rng.integers(0, n - 301, n // 40)
            ends = starts + rng.integers(1, 301, len(starts))
            v = (np.bincount(starts, minlength=n) - np.bincount(ends, minlength=n)).astype(np.int64).astype(U32)
        elif kind == "spike":                # 2^31 on the last word of every tile and on the first of the next
            v = rng.integers(0, 600, n).astype(U32)
            v[DEPTH_TILE - 1::DEPTH_TILE] = 1 << 31
            v[DEPTH_TILE::DEPTH_TILE] = 1 << 31
        else:
            v = np.zeros(n, U32)
        cases.append(Case(f"depthscan {kind} tiles={tiles}", [tiles], [v], tiles=tiles, kind=kind))

    for tiles in DEPTHSCAN_TILES:
        add("random", tiles)
    for kind in DEPTHSCAN_KINDS[1:]:
        for tiles in (1, 1025, 2049):
            add(kind, tiles)
    return cases


def depthscan_reference(c):
    """the inclusive prefix sum modulo 2^32; tile_sums: the exclusive prefixes of the tiles' totals modulo 2^32"""
    total = np.cumsum(c.blobs[0], dtype=U64)
    ends = total[DEPTH_TILE - 1::DEPTH_TILE]
    return [_guarded((total & U64(M32)).astype(U32)), _guarded((np.concatenate([np.zeros(1, U64), ends[:-1]]) & U64(M32)).astype(U32))]


def depthscan_check(c, got):
    if len(got) != 2:
        return [f"{len(got)} result blobs, not 2"]
    want = depthscan_reference(c)
    return _same_guarded("the prefix sums", got[0], (want[0], U32)) + _same_guarded("tile_sums", got[1], (want[1], U32))


# ------------------------------------------------------------------------------------------------------------------------- depth: bedGraph text
BED_VALUES = sorted({v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)} | {0, M32})        # 0, 9, 10, 99, 100, ... 999 999 999, 1 000 000 000, 4 294 967 295
BED_NAMES = [1, 150, 490, 600]
BED_PIECES = [1, 7, 255, 256, 257, None]     # positions a piece; None: the whole window
BED_LINES = [1, 63, 64, 65, 128, 129]        # lines a piece
BED_MIXED_BASE = 9_990_016                   # seven digits throughout the mixed-route case


def _bed_case(name, d, base, name_len, bounds, lead, **facts):
    """d: the depths of [base, base + len(d)); the word at len repeats the last one: that a run ends at len must not come from the array"""
    d = np.asarray(d, U32)
    c = Case(f"bedgraph {name} base={base} name={name_len} +{lead}", [base + len(d), base, lead, 0], [np.concatenate([d, d[-1:]]), np.frombuffer(_name_of(name_len), U8), np.array(bounds, U64)],
             base=base, len=base + len(d), name_len=name_len, lead=lead, bounds=[int(b) for b in bounds], **facts)
    c.lines = bed_lines(c)
    c.par[3] = sum(len(line) for _, line in c.lines)
    return c


def bed_lines(c):
    """(where the run ends, its line) of every maximal run of equal depth of the window, by a plain loop"""
    d, name = c.blobs[0][:-1].tolist(), c.blobs[1].tobytes()
    out, start = [], c.base
    for b in range(c.base + 1, c.len + 1):
        if b == c.len or d[b - c.base] != d[b - 1 - c.base]:
            out.append((b, b"%s\t%d\t%d\t%d\n" % (name, start, b, d[b - 1 - c.base])))
            start = b
    return out


def bed_pieces(c):
    """the lines of every piece: the runs that end in (lo, hi]"""
    return [[line for end, line in c.lines if lo < end <= hi] for lo, hi in zip(c.bounds[:-1], c.bounds[1:])]


def _steps(lo, hi, step):
    return list(range(lo, hi, step)) + [hi]


def bedgraph_cases():
    rng = np.random.default_rng(34)
    cases = []

    def runs(n, longest=9, values=(0, 1, 2, 3, 7, 12, 150)):
        """n positions in runs of 1 .. longest, neighbours of different depth"""
        out, last = [], None
        while len(out) < n:
            v = values[int(rng.integers(0, len(values)))]
            if v != last:
                out += [v] * int(rng.integers(1, longest + 1))
                last = v
        return np.array(out[:n])

    own = lambda n, a=3, b=8: np.where(np.arange(n) % 2 == 0, a, b)                  # every position a run of its own
    # run shapes
    cases.append(_bed_case("one run, pieces without a line", np.full(1000, 7), 0, 150, [0, 256, 512, 1000], 3))
    cases.append(_bed_case("every position its own run", own(600), 0, 150, [0, 600], 0))
    cases.append(_bed_case("pieces of 1 63 64 65 128 129 lines", own(450), 0, 150, np.concatenate([[0], np.cumsum(BED_LINES)]), 9))
    cases.append(_bed_case("a seam inside a run, a seam on a run's end", np.repeat([3, 5, 2, 8], 100), 0, 150, [0, 150, 200, 400], 0))
    cases.append(_bed_case("a last run of depth 0", np.concatenate([runs(300), np.zeros(40)]), 0, 150, [0, 100, 340], 0))
    cases.append(_bed_case("a last run of non-zero depth", np.concatenate([runs(300), np.full(40, 5)]), 0, 150, [0, 100, 340], 0))
    # piece sizes
    for size, n in zip(BED_PIECES, (40, 150, 1100, 1100, 1100, 1100)):
        cases.append(_bed_case(f"pieces of {size}", runs(n), 0, 150, _steps(0, n, size or n), 5))
    # depth values of every width, each between two others
    values = np.array(BED_VALUES + BED_VALUES[::-1][1:] + BED_VALUES[1::3])
    assert np.all(values[1:] != values[:-1])
    cases.append(_bed_case("depths of every width", values, 0, 150, [0, 17, len(values)], 2))
    # positions that gain a digit inside the window; the last position a sequence can have
    for power in (7, 8, 9):
        base = (10 ** power - 300) // 32 * 32
        cases.append(_bed_case(f"positions around 10^{power}", runs(10 ** power + 300 - base, 4), base, 150, [base, 10 ** power - 1, 10 ** power, 10 ** power + 300], power))
    base = (M32 - 500) // 32 * 32
    cases.append(_bed_case("a window that ends at 4294967295", runs(M32 - base, 4, BED_VALUES[-4:]), base, 150, [base, M32 - 256, M32], 13))
    # names: through the image (1, 150), straight (600: whole waves of 64 lines only -- fewer lines of a last wave would fit the image)
    for lead in range(16):
        cases.append(_bed_case("alignments", runs(300), 0, 150, [0, 131, 300], lead))
    for lead in (0, 5, 11):
        cases.append(_bed_case("a short name", runs(300), 0, 1, [0, 131, 300], lead))
        cases.append(_bed_case("a long name", own(192, 4, M32), 0, 600, [0, 64, 192], lead))
        cases.append(_bed_case("a name at the image's cap", runs(500), 0, 490, [0, 131, 500], lead))
    # both routes in one launch, name 490: a wave of narrow lines (through the image), one of the widest depths (straight), one of exactly the image's size
    # (through the image at skew 0 only), narrow ones again
    d = np.concatenate([own(64, 1, 2), own(64, M32, 10 ** 9), own(64, 1000, 2000), own(64, 1, 2), own(20, 3, 4)])
    probe = _bed_case("probe", d, BED_MIXED_BASE, 490, [BED_MIXED_BASE, BED_MIXED_BASE + len(d)], 0)
    exact_at = sum(size for _, size, _ in text_waves(bed_pieces(probe), 0, IMAGE_MAX)[:2])
    for lead in ((-exact_at) % 16, (1 - exact_at) % 16):
        cases.append(_bed_case("both routes", d, BED_MIXED_BASE, 490, [BED_MIXED_BASE, BED_MIXED_BASE + len(d)], lead, mixed=True))
    return cases


def bedgraph_reference(c):
    """{lines, bytes, carry} per piece by a plain loop; the text: tests/truth_depth.py's bedgraph_from_depth of the window (a window from 0 on: the function knows
    no other; test_kernel_trial.py holds that the loop's lines are its text), guarded"""
    from truth_depth import bedgraph_from_depth
    per_piece, carry = [], c.base
    for lo, hi in zip(c.bounds[:-1], c.bounds[1:]):
        ends = [(end, line) for end, line in c.lines if lo < end <= hi]
        carry = ends[-1][0] if ends else carry
        per_piece += [len(ends), sum(len(line) for _, line in ends), carry]
    text = b"".join(line for end, line in c.lines if end <= c.bounds[-1]) if c.base else bedgraph_from_depth([c.blobs[1].tobytes()], [c.blobs[0][:-1]])
    return [np.array(per_piece, U64), _guarded(np.frombuffer(text, U8))]


def bedgraph_check(c, got):
    if len(got) != 2:
        return [f"{len(got)} result blobs, not 2"]
    want = bedgraph_reference(c)
    return _same("lines, bytes and carry per piece", got[0], want[0]) + _same_guarded("the text", got[1], (want[1], U8))


# ------------------------------------------------------------------------------------------------------------------------- pileup: rows and TSV text
PILEUP_NAMES = [1, 150, 450, 600]
PILEUP_KEPT = [0, 1, 63, 64, 65, 129]        # kept lines a piece
PILEUP_MIXED_BASE = 1_000_000                # seven digits throughout the mixed-route cases
LETTERS = b"ACGT"
DEPTH, DEL, INS = 0, 6, 7                    # the columns of a row: depth, A, C, G, T, N, del, ins


def _row(ref, calls=(0, 0, 0, 0, 0), dele=0, ins=0, depth=None):
    """the full counts of one strand set: the five calls (the reference letter's own among them), the depth their sum"""
    return [sum(calls) if depth is None else depth, *calls, dele, ins]


def _pileup_case(name, v, ref, base, all_rows, name_len, bounds, lead, rows_shift=0, **facts):
    """v: the full counts [n][sets][8] (uint32); ref: the reference codes [n].  The planes as a run stores them: plane 0 the depth, the plane of the reference's own
    letter 0 (its count is the depth less the other calls, modulo 2^32), the others the counts."""
    v, ref = np.asarray(v, np.int64).astype(U32), np.asarray(ref, np.int64)
    n, sets = v.shape[:2]
    planes = np.ascontiguousarray(v.transpose(1, 2, 0))                # [sets][8][n]
    planes[:, 1 + ref, np.arange(n)] = 0
    packed = np.zeros((n + 31) // 32, U64)
    for k in range(32):
        part = ref[k::32].astype(U64) << U64(2 * k)
        packed[:len(part)] |= part
    c = Case(f"pileup {name} base={base} sets={sets} all={int(all_rows)} name={name_len} +{lead} rows+{rows_shift}", [n, base, sets, all_rows, lead, rows_shift, 0],
             [planes, packed, np.frombuffer(_name_of(name_len), U8), np.array(bounds, U64)], n=n, base=base, sets=sets, all=bool(all_rows), name_len=name_len, lead=lead,
             rows_shift=rows_shift, bounds=[int(b) for b in bounds], v=v, ref=ref, **facts)
    assert c.bounds[0] == base and c.bounds[-1] == base + n
    c.keep, c.lines = pileup_lines(c)
    c.par[6] = sum(len(line) for line in c.lines if line)
    return c


def pileup_lines(c):
    """by a plain loop over the positions: the predicate and the kept rows' lines (b"" for the others).  Sites: a value other than the depth and the reference
    letter's own count is non-zero, in any strand set; all: any value is"""
    name, keep, lines = c.blobs[2].tobytes(), [], []
    for i, (row, ref) in enumerate(zip(c.v.tolist(), c.ref.tolist())):
        kept = any(x for s in row for k, x in enumerate(s) if c.all or k not in (DEPTH, 1 + ref))
        keep.append(kept)
        lines.append(b"%s\t%d\t%c\t%s\n" % (name, c.base + i + 1, LETTERS[ref], b"\t".join(b"%d" % x for s in row for x in s)) if kept else b"")
    return np.array(keep), lines


def pileup_pieces(c):
    return [[line for line in c.lines[lo - c.base:hi - c.base] if line] for lo, hi in zip(c.bounds[:-1], c.bounds[1:])]


def _digits(width, k=0):
    """a number of so many digits"""
    return min(10 ** (width - 1) + k, M32) if width else 0


def pileup_cases():
    rng = np.random.default_rng(88)
    cases = []
    zero = _row(0)

    def random_rows(n, sets, kept):
        """rows with a depth and the reference letter's own count; those of `kept` (a mask) with one other value more, in one strand set"""
        ref = rng.integers(0, 4, n)
        v = np.zeros((n, sets, 8), np.int64)
        for i in range(n):
            for s in range(sets):
                v[i, s, 1 + ref[i]] = v[i, s, DEPTH] = rng.integers(0, 60)
            if kept[i]:
                s, k = int(rng.integers(0, sets)), int(rng.choice([c for c in range(1, 8) if c != 1 + ref[i]]))
                v[i, s, k] += rng.integers(1, 30)
                v[i, s, DEPTH] += v[i, s, k] if k < DEL else 0
        return v, ref

    # the predicate
    for sets in (1, 2):
        rows, refs = [], []
        for ref in range(4):
            rows.append([zero] * sets)                                         # never kept
            rows.append([_row(ref, [3 * (k == ref) for k in range(5)])] + [zero] * (sets - 1))      # the depth and the letter's own count: under all only
            for k in range(5):                                                 # a single 1 in each of A, C, G, T, N, del and ins
                rows.append([_row(ref, [int(j == k) for j in range(5)])] + [zero] * (sets - 1))
            rows.append([_row(ref, dele=1)] + [zero] * (sets - 1))
            rows.append([_row(ref, ins=1)] + [zero] * (sets - 1))
            if sets == 2:                                                      # the only non-zero call, del or ins in the reverse set
                own = _row(ref, [2 * (k == ref) for k in range(5)])
                for first in (zero, own):
                    rows.append([first, _row(ref, [int(j == (ref + 1) % 4) for j in range(5)])])
                    rows.append([first, _row(ref, [0, 0, 0, 0, 1])])
                    rows.append([first, _row(ref, dele=1)])
                    rows.append([first, _row(ref, ins=1)])
                    rows.append([first, own])                                  # ... and nothing but the own count there
            refs += [ref] * (len(rows) - len(refs))
        for all_rows in (0, 1):
            cases.append(_pileup_case("the predicate", rows, refs, 0, all_rows, 150, [0, 7, len(rows)], 4 * all_rows, predicate=True))
    # counts of 1 .. 10 digits in every column; the depth 4294967295 with nothing else
    for sets in (1, 2):
        rows, refs = [], []
        for width in range(1, 11):
            for col in range(8):
                ref = (width + col) % 4
                calls = [0] * 5
                if col == DEPTH:
                    calls[ref] = _digits(width, 3)
                elif col < DEL:
                    calls[col - 1] = _digits(width, col)
                row = _row(ref, calls, _digits(width, 1) if col == DEL else 0, _digits(width, 2) if col == INS else 0)
                rows.append([zero] * (sets - 1) + [row])
                refs.append(ref)
        rows.append([_row(2, [0, 0, M32, 0, 0])] + [zero] * (sets - 1))
        refs.append(2)
        cases.append(_pileup_case("counts of every width", rows, refs, 0, 1, 150, [0, len(rows)], 7, rows_shift=sets - 1, widths=True))
    # ten-digit positions, the window crossing 10^9: the widest row a run can hold -- three calls, N, del and ins of ten digits, the letter's own count what the
    # depth leaves: nine --, and the line the image is sized for, every column ten digits: a depth below the other calls' sum, the own count modulo 2^32
    base = (10 ** 9 - 40) // 32 * 32
    for sets in (1, 2):
        rows, refs = [], []
        for i in range(96):
            ref = i % 4
            calls = [10 ** 9 + i] * 5
            calls[ref] = M32 - 4 * (10 ** 9 + i)
            widest = _row(ref, calls, M32 - i, 10 ** 9 + i)
            calls[ref] = (10 ** 9 - 4 * (10 ** 9 + i)) % (1 << 32)
            sized_for = _row(ref, calls, M32, M32 - i, depth=10 ** 9)
            rows.append([sized_for if i % 3 == 2 else widest] * sets)
            refs.append(ref)
        cases.append(_pileup_case("the widest lines, positions around 10^9", rows, refs, base, 0, 150, [base, 10 ** 9 - 1, base + 96], 1, rows_shift=1, widest=True))
    for power in (7, 8):
        base = (10 ** power - 100) // 32 * 32
        v, ref = random_rows(200, 2, rng.random(200) < 0.5)
        cases.append(_pileup_case(f"positions around 10^{power}", v, ref, base, 0, 150, [base, 10 ** power - 1, 10 ** power, base + 200], power))
    # kept lines a piece: 0, 1, 63, 64, 65, 129
    sizes, kept = [50, 10, 100, 64, 80, 200], []
    for size, lines in zip(sizes, PILEUP_KEPT):
        mask = np.zeros(size, bool)
        mask[rng.permutation(size)[:lines]] = True
        kept.append(mask)
    v, ref = random_rows(sum(sizes), 1, np.concatenate(kept))
    cases.append(_pileup_case("pieces of 0 1 63 64 65 129 lines", v, ref, 0, 0, 150, np.concatenate([[0], np.cumsum(sizes)]), 6, kept_per_piece=True))
    v, ref = random_rows(100_000, 1, rng.random(100_000) < 0.001)
    cases.append(_pileup_case("sparse", v, ref, 0, 0, 150, [0, 4096, 100_000], 0, sparse=True))
    v, ref = random_rows(1000, 2, np.ones(1000, bool))
    cases.append(_pileup_case("every row kept", v, ref, 0, 0, 150, [0, 257, 1000], 10, rows_shift=1))
    # names and alignments (600: whole waves of 64 lines only -- fewer lines of a last wave would fit the image)
    for lead in range(16):
        v, ref = random_rows(300, 1 + lead % 2, rng.random(300) < 0.7)
        cases.append(_pileup_case("alignments", v, ref, 0, lead % 4 == 3, 150, [0, 131, 300], lead, rows_shift=lead % 2))
    for lead in (0, 5, 11):
        v, ref = random_rows(300, 2, rng.random(300) < 0.7)
        cases.append(_pileup_case("a short name", v, ref, 0, 0, 1, [0, 131, 300], lead))
        v, ref = random_rows(192, 1, np.ones(192, bool))
        cases.append(_pileup_case("a long name", v, ref, 0, 0, 600, [0, 64, 192], lead))
        v, ref = random_rows(500, 1 + (lead > 0), rng.random(500) < 0.7)
        cases.append(_pileup_case("a name at the image's cap", v, ref, 0, 0, 450, [0, 131, 500], lead))
    # both routes in one launch, name 450: a wave of narrow lines (through the image), one of the widest (straight), one of exactly the image's size (512 bytes a
    # line: through the image at skew 0 only), narrow ones again
    for sets in (1, 2):
        narrow = [_row(0, [0, 1, 0, 0, 0])] * sets
        wide = [_row(1, [10 ** 9, M32 - 3 * 10 ** 9, 10 ** 9, 0, 10 ** 9], M32, M32)] * sets
        exact = [_row(2, [10000] * 5, 10 ** 6, 10 ** 5)] if sets == 1 else [_row(2, [1, 1, 0, 1, 1], 1, 1), _row(2, [100] * 5, 10 ** 4, 10 ** 3)]
        rows = [narrow] * 64 + [wide] * 64 + [exact] * 64 + [narrow] * 84
        refs = [0] * 64 + [1] * 64 + [2] * 64 + [0] * 84
        bounds = [PILEUP_MIXED_BASE, PILEUP_MIXED_BASE + len(rows)]
        probe = _pileup_case("probe", rows, refs, PILEUP_MIXED_BASE, 0, 450, bounds, 0)
        exact_at = sum(size for _, size, _ in text_waves(pileup_pieces(probe), 0, IMAGE_MAX)[:2])
        for lead in ((-exact_at) % 16, (1 - exact_at) % 16):
            cases.append(_pileup_case("both routes", rows, refs, PILEUP_MIXED_BASE, 0, 450, bounds, lead, mixed=True))
    return cases


def pileup_reference(c):
    """the rows: the full counts; per piece the flags, the lines' sizes, {lines, bytes}, the kept positions, the lines' places and the text's length; the text
    (tests/truth_pileup.py's pileup_text over the rows for a window from 0 on -- it knows no other; test_kernel_trial.py holds that the loop's lines are its text)"""
    from truth_pileup import pileup_text
    out = [_guarded(c.v)]
    for lo, hi in zip(c.bounds[:-1], c.bounds[1:]):
        lines = c.lines[lo - c.base:hi - c.base]
        sizes = np.array([len(line) for line in lines], U32)
        kept = np.flatnonzero(c.keep[lo - c.base:hi - c.base])
        out += [_guarded(c.keep[lo - c.base:hi - c.base].astype(U32)), _guarded(sizes), np.array([len(kept), sizes.sum()], U64), _guarded((kept + lo).astype(U32)),
                _guarded(_offsets(sizes[kept]) if len(kept) else np.zeros(0, U64))]
    text = b"".join(c.lines) if c.base or getattr(c, "widest", False) else pileup_text([c.blobs[2].tobytes()], [bytes(LETTERS[r] for r in c.ref)], [c.v], c.all)
    return out + [_guarded(np.frombuffer(text, U8))]


def pileup_check(c, got):
    want = pileup_reference(c)
    if len(got) != len(want):
        return [f"{len(got)} result blobs, not {len(want)}"]
    lines = _same_guarded("the rows", got[0], (want[0], U32))
    for k in range(len(c.bounds) - 1):
        g, w = got[1 + 5 * k:6 + 5 * k], want[1 + 5 * k:6 + 5 * k]
        lines += _same_guarded(f"piece {k}: flags", g[0], (w[0], U32)) + _same_guarded(f"piece {k}: sizes", g[1], (w[1], U32)) + _same(f"piece {k}: lines and bytes", g[2], w[2])
        lines += _same_guarded(f"piece {k}: line_pos", g[3], (w[3], U32)) + _same_guarded(f"piece {k}: offsets", g[4], (w[4], U64))
    return lines + _same_guarded("the text", got[-1], (want[-1], U8))


# ------------------------------------------------------------------------------------------------------------------------- the report: rows, shared adds
STATS_PAIRS = [1, 63, 64, 65, 255, 257, 1025, 5000]
STATS_SLABS = [64, 100, 1024]
STATS_LENGTHS = [(1, 1), (3, 5), (4, 0), (150, 151), (301, 30)]
STATS_CHUNKS = [4, 8, 52, 64, 0]             # 0: the library's choice (stats_rows_geometry)
STATS_Q = [1, 2, 41, 42, 94, 250]
STATS_BLOCK = 256                            # kStatsMatesBlock


def stats_layout(len0, len1, Q):
    """rsq_stats.h's StatsLayout for F = 0 and one tile: pairs[2] strand[2] tile[1] read_length[2][L + 1] errors_per_read[2][L + 1] insertion, deletion, adapter,
    tail, mismatch [2][L] bad[1] fragment_length[1] base_quality[2][L][Q] base_call[2][L][5] -> where base_quality, base_call and bad begin, the words"""
    L = max(len0, len1)
    bad = 5 + 4 * (L + 1) + 10 * L
    quality = bad + 2
    call = quality + 2 * L * Q
    return quality, call, bad, call + 10 * L


def _rows_case(name, rng, n_pairs, lengths, Q=42, phred=33, chunk=0, slab=0, groups=0, skew=1, row_words=None, read_lens=None, hot=False, below=False, **facts):
    """word-major seq and qual arrays [word][row] of 2 n_pairs reads with a pitch above them; 0xFF in every byte behind a read's last base and in the rows beyond"""
    L = max(lengths)
    row_words = row_words or (L + 3) // 4 + 1
    reads, pitch, cycles = 2 * n_pairs, 2 * n_pairs + 7, 4 * row_words
    lens = np.concatenate([np.full(n_pairs, lengths[0]), np.full(n_pairs, lengths[1])])
    if read_lens is not None:
        lens = rng.choice(read_lens, reads)
    elif not hot:
        lens = np.where(rng.random(reads) < 0.3, rng.integers(0, L + 1, reads), lens)
    if hot:
        bases, quals = np.full((cycles, reads), 2), np.full((cycles, reads), phred + min(Q - 1, 30))
    else:
        bases = np.where(rng.random((cycles, reads)) < 0.01, rng.integers(5, 256, (cycles, reads)), rng.integers(0, 5, (cycles, reads)))
        quals = phred + np.where(rng.random((cycles, reads)) < 0.01, Q + rng.integers(0, 3, (cycles, reads)), rng.integers(0, Q, (cycles, reads)))
        if below:
            quals = np.where(rng.random((cycles, reads)) < 0.02, rng.integers(0, phred, (cycles, reads)), quals)
    seq, qual = np.full((cycles, pitch), 0xFF, U8), np.full((cycles, pitch), 0xFF, U8)
    inside = np.arange(cycles)[:, None] < lens[None, :]
    seq[:, :reads][inside] = bases[inside]
    qual[:, :reads][inside] = np.minimum(quals, 255)[inside]

    def words(a):                            # [cycle][row] bytes -> [word][row] little-endian words
        return np.ascontiguousarray(a.reshape(row_words, 4, pitch).transpose(0, 2, 1)).view(U32).reshape(row_words, pitch)
    units = sum(-(-l // chunk) for l in lengths) if chunk else None
    return Case(f"stats rows {name} pairs={n_pairs} lengths={lengths} Q={Q} phred={phred} chunk={chunk} slab={slab} groups={groups} skew={skew} row_words={row_words}",
                [0, n_pairs, lengths[0], lengths[1], Q, phred, row_words, pitch, chunk, slab, groups, skew], [words(seq), words(qual), lens.astype(U16)], kind="rows", n_pairs=n_pairs,
                lengths=lengths, Q=Q, phred=phred, chunk=chunk, slab=slab, groups=groups, skew=skew, row_words=row_words, pitch=pitch, units=units, hot=hot, below=below,
                slabs=-(-n_pairs // (slab or 1024)), **facts)


def _shared_case(name, rounds, words, image_words, groups=1, **facts):
    """rounds: [round][256][{index, on, index2, v}]"""
    rounds = np.ascontiguousarray(rounds, U32)
    return Case(f"stats shared {name} words={words} image={image_words} groups={groups}", [1, words, image_words, groups], [rounds], kind="shared", words=words, image_words=image_words,
                groups=groups, rounds=rounds, **facts)


def stats_cases():
    rng = np.random.default_rng(250)
    cases = []
    for k, n in enumerate(STATS_PAIRS):
        cases.append(_rows_case("pairs", rng, n, (150, 151), slab=STATS_SLABS[k % 3], skew=k % 2))
    k = 0
    for slab in STATS_SLABS:                 # 257 pairs: five slabs of 64, three of 100, one of 1024; chunk 8 over (30, 21): 4 + 3 units
        units, slabs = 7, -(-257 // slab)
        for groups in (1, 2, units - 1, units, units + 1, 3 * units + 1, units * slabs + 3):
            cases.append(_rows_case("groups", rng, 257, (30, 21), chunk=8, slab=slab, groups=groups, skew=k % 2))
            k += 1
    for lengths in STATS_LENGTHS:
        for chunk in STATS_CHUNKS:
            cases.append(_rows_case("lengths", rng, 130, lengths, chunk=chunk, slab=100, skew=k % 2))
            k += 1
    for Q in STATS_Q:
        for skew in (0, 1):
            cases.append(_rows_case("Q", rng, 200, (150, 151), Q=Q, skew=skew))
    for phred in (33, 64):
        cases.append(_rows_case("characters below the offset", rng, 130, (30, 21), phred=phred, below=True, skew=phred == 33))
    # read lengths: 0, longer than the segment's L, longer than 4 row_words (rows of five words under reads of up to 30)
    cases.append(_rows_case("read lengths", rng, 130, (30, 21), chunk=8, slab=64, read_lens=[0, 1, 3, 4, 5, 20, 21, 22, 29, 30, 31, 40, 1000], skew=1, lens=True))
    cases.append(_rows_case("read lengths", rng, 130, (30, 21), chunk=8, slab=64, read_lens=[0, 1, 3, 4, 5, 20, 21, 22, 29, 30, 31, 40, 1000], skew=0, lens=True))
    cases.append(_rows_case("rows shorter than the reads", rng, 130, (30, 30), chunk=12, row_words=5, read_lens=[0, 19, 20, 21, 25, 30], skew=1, short_rows=True))
    cases.append(_rows_case("rows shorter than the reads", rng, 130, (30, 30), row_words=5, read_lens=[0, 19, 20, 21, 25, 30], skew=0, short_rows=True))
    for skew in (0, 1):                      # 5000 reads add to one counter a cycle
        cases.append(_rows_case("one counter", rng, 2500, (301, 301), hot=True, skew=skew))
    # the shared adds: a workgroup of four waves; per round a lane's {index, on, index2, v}
    words, image = 700, 300
    lane = np.arange(STATS_BLOCK) % 64
    wave = np.arange(STATS_BLOCK) // 64

    def round_of(index, on, index2=None, v=None):
        r = np.zeros((STATS_BLOCK, 4), np.int64)
        r[:, 0], r[:, 1] = index, on
        r[:, 2] = rng.integers(0, words, STATS_BLOCK) if index2 is None else index2
        r[:, 3] = rng.integers(0, 4, STATS_BLOCK) if v is None else v
        return r

    rounds = [round_of(5, 1), round_of(image + 7, 1),                          # all 64 lanes on one index, in the image and in memory
              round_of(10 + lane, 1), round_of(image - 32 + lane, 1),          # 64 different indices, the second on both sides of image_words
              round_of(3, 0),                                                  # nobody
              round_of(4, lane == 0), round_of(4, lane == 63),                 # one lane
              round_of(20 + lane % 2, 1), round_of(np.where(lane % 2, image, image - 1), 1),      # two indices interleaved
              round_of(30 + wave, lane % 3 != 0)]
    rounds += [round_of(rng.integers(0, words, STATS_BLOCK) // rng.integers(1, 40), rng.random(STATS_BLOCK) < 0.7) for _ in range(40)]
    cases.append(_shared_case("patterns", rounds, words, image, classes=True))
    cases.append(_shared_case("patterns, three workgroups", rounds, words, image, groups=3))
    cases.append(_shared_case("patterns, no image", rounds, words, 0))
    cases.append(_shared_case("patterns, all in the image", rounds, words, words))
    cases.append(_shared_case("1000 rounds onto one counter", [round_of(9, 1, 9, 1) for _ in range(1000)], words, image, hot=True))
    cases.append(_shared_case("1000 rounds onto one counter in memory", [round_of(image, 1, image, 1) for _ in range(1000)], words, image, hot=True))
    return cases


def stats_reference(c):
    """rows: per segment, row and cycle c < min(read_len, L of the segment, 4 row_words) the quality byte less the offset (uint32) counts in base_quality[seg][c][q] if
    below Q, else in bad; the base byte in base_call[seg][c][b] if below 5, else in bad; every other table stays zero.  shared: np.bincount"""
    if c.kind == "shared":
        r = c.rounds.reshape(-1, 4).astype(np.int64)
        counts = np.bincount(r[r[:, 1] != 0, 0], minlength=c.words) + np.bincount(r[:, 2], weights=r[:, 3], minlength=c.words).astype(np.int64)
        return [_guarded((counts * c.groups).astype(U64))]
    quality, call, bad, words = stats_layout(c.lengths[0], c.lengths[1], c.Q)
    L, n, cycles = max(c.lengths), c.n_pairs, 4 * c.row_words
    counts = np.zeros(words, np.int64)
    seq, qual, lens = c.blobs

    def per_cycle(a):                        # [word][row] words -> [cycle][row] bytes
        return a.view(U8).reshape(c.row_words, c.pitch, 4).transpose(0, 2, 1).reshape(cycles, c.pitch).astype(np.int64)
    for seg in (0, 1):
        rows = slice(seg * n, (seg + 1) * n)
        upto = np.minimum(np.minimum(lens[rows].astype(np.int64), c.lengths[seg]), cycles)
        cycle, row = np.nonzero(np.arange(cycles)[:, None] < upto[None, :])
        q = (per_cycle(qual)[:, rows][cycle, row] - c.phred) & M32
        b = per_cycle(seq)[:, rows][cycle, row]
        counts[bad] += np.count_nonzero(q >= c.Q) + np.count_nonzero(b >= 5)
        counts += np.bincount(quality + ((seg * L + cycle) * c.Q + q)[q < c.Q], minlength=words)
        counts += np.bincount(call + ((seg * L + cycle) * 5 + b)[b < 5], minlength=words)
    return [np.array([quality, call, bad, words], U32), _guarded(counts.astype(U64))]


def stats_check(c, got):
    want = stats_reference(c)
    if len(got) != len(want):
        return [f"{len(got)} result blobs, not {len(want)}"]
    if c.kind == "shared":
        return _same_guarded("the counts", got[0], (want[0], U64))
    lines = _same("the layout: base_quality, base_call, bad, words", got[0], want[0]) + _same_guarded("the counts", got[1], (want[1], U64))
    g = np.frombuffer(np.ascontiguousarray(got[1]).tobytes(), U8)
    if len(g) == len(want[1]):
        quality, call, bad, words = stats_layout(c.lengths[0], c.lengths[1], c.Q)
        g, w = g[MARKER:-MARKER].view(U64), want[1][MARKER:-MARKER].view(U64)
        for name, lo, hi in (("the tables that stay zero", 0, bad), ("bad", bad, bad + 1), ("fragment_length", bad + 1, quality), ("base_quality", quality, call), ("base_call", call, words)):
            wrong = np.flatnonzero(g[lo:hi] != w[lo:hi])
            if len(wrong):
                lines.append(f"{name}: {len(wrong)} counters wrong, the first at {wrong[0]}: {int(g[lo + wrong[0]])}, not {int(w[lo + wrong[0]])}")
    return lines


# -------------------------------------------------------------------------------------------------------------------------
_CASES = {"scan": scan_cases, "sort": sort_cases, "gather": gather_cases, "index": index_cases, "bins": bins_cases, "fasta": fasta_cases, "depthscan": depthscan_cases,
          "bedgraph": bedgraph_cases, "pileup": pileup_cases, "stats": stats_cases}
_REFERENCE = {"scan": scan_reference, "sort": sort_reference, "gather": gather_reference, "index": index_reference, "bins": bins_reference, "fasta": fasta_reference,
              "depthscan": depthscan_reference, "bedgraph": bedgraph_reference, "pileup": pileup_reference, "stats": stats_reference}
_CHECK = {"scan": scan_check, "sort": sort_check, "gather": gather_check, "index": index_check, "bins": bins_check, "fasta": fasta_check, "depthscan": depthscan_check,
          "bedgraph": bedgraph_check, "pileup": pileup_check, "stats": stats_check}
# the result blobs of a case, where they follow from the case without its reference (the large ones)
_BLOBS = {"depthscan": lambda c: 2, "bedgraph": lambda c: 2, "pileup": lambda c: 2 + 5 * (len(c.bounds) - 1), "stats": lambda c: 1 if c.kind == "shared" else 2}
_made = {}


def cases(family):
    """the family's table, made once"""
    if family not in _made:
        _made[family] = _CASES[family]()
    return _made[family]


def reference(family, case):
    return _REFERENCE[family](case)


def check(family, case, got):
    return _CHECK[family](case, got)


def run(exe, family, directory):
    """the trial as a fresh child process over the family's table -> (the result blobs case by case, or None; the finished process)"""
    inputs, results = os.path.join(str(directory), family + "_in.bin"), os.path.join(str(directory), family + "_out.bin")
    write_cases(inputs, cases(family))
    done = subprocess.run([exe, family, inputs, results], capture_output=True, text=True, timeout=CHILD_LIMIT)
    return (results_of(family, cases(family), read_blobs(results)) if done.returncode == 0 else None), done
