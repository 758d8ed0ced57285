"""The case tables of tests/hostemu/kernel_trial.cpp, what every case must give, and the checkers (tests/test_kernel_trial.py shows that each of them has teeth,
tests/test_kernel_trial_gpu.py runs the trial on the device).

The trial runs the library's cooperative kernels alone -- the scan, the sorted BAM's radix passes, cut, gather and index kernels, the bins' plan and scatter, the
FASTA record starts: device-only code that the host emulation replaces with a loop.  The references here are plain numpy and plain loops, written from what the
kernels are meant to give (an exclusive prefix sum, a stable sort, a copy, a histogram ...), not from their code.  Every comparison is exact: integers and bytes,
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
FAMILIES = ["scan", "sort", "gather", "index", "bins", "fasta"]
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
        k = len(reference(family, c))
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


# -------------------------------------------------------------------------------------------------------------------------
_CASES = {"scan": scan_cases, "sort": sort_cases, "gather": gather_cases, "index": index_cases, "bins": bins_cases, "fasta": fasta_cases}
_REFERENCE = {"scan": scan_reference, "sort": sort_reference, "gather": gather_reference, "index": index_reference, "bins": bins_reference, "fasta": fasta_reference}
_CHECK = {"scan": scan_check, "sort": sort_check, "gather": gather_check, "index": index_check, "bins": bins_check, "fasta": fasta_check}
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
