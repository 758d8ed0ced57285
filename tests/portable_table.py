"""The table of inputs of tests/hostemu/portable_trial.cpp (every primitive of reseq_amd/csrc/rsq_portable.h), what each record must give -- written here from the
primitives' stated meaning, in plain Python, not from the header --, and how the two programs of that one source are built and run.
A record is eight words (operation, six arguments, a spare), a result four."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hostemu", "portable_trial.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "reseq_amd", "csrc")

OPS = ["base_letters", "complement_letters", "bam_nibbles", "perm_bytes", "byte_reverse", "bam_pack", "align_bytes", "bytes_at",
       "div_small", "popcount64", "lowest_set_bit64", "bit_reverse32", "bit_reverse64", "clamp_from_zero",
       "fma2", "fma1", "mul_add2",
       "load64_align1", "load64_align2", "load128_align2", "load32_align1", "load32_align4", "load64_align1_lds",
       "store64_align1", "image_or", "wave_any"]                 # the order of portable_trial.cpp's enum Op
OP = {name: i for i, name in enumerate(OPS)}
BUF = bytes((i * 37 + 11) & 0xFF for i in range(64))             # portable_trial.cpp buf_byte
M32 = 0xFFFFFFFF
WORDS = [0, M32, 0x80000000, 0x01020304]


# ------------------------------------------------------------------------------------------------------------------------- single precision, exactly
def f32(bits):
    return Fraction(float(np.array([bits], np.uint32).view(np.float32)[0]))


def round_f32(v):
    """the bits of the float nearest to the rational v, ties to even; v's magnitude is 0 or within the normal range"""
    if v == 0:
        return 0
    sign, v = (0x80000000, -v) if v < 0 else (0, v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    q = v / Fraction(2) ** (e - 23)                              # in [2^23, 2^24)
    n = q.numerator // q.denominator
    rest = q - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1):
        n += 1
    if n == 1 << 24:
        n, e = 1 << 23, e + 1
    assert -126 <= e <= 127, "outside the normal range: the table keeps away from it"
    return sign | ((e + 127) << 23) | (n - (1 << 23))


def fused(a, b, c):
    return round_f32(f32(a) * f32(b) + f32(c))


def unfused(a, b, c):
    return round_f32(f32(round_f32(f32(a) * f32(b))) + f32(c))


def bits_of(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


# ------------------------------------------------------------------------------------------------------------------------- the table
def records():
    rng = np.random.default_rng(20260)
    rows = []

    def add(op, *args):
        rows.append([OP[op]] + [int(a) & M32 for a in args] + [0] * (7 - len(args)))

    def pairs():
        return [(a, b) for a in WORDS for b in WORDS] + [tuple(int(x) for x in rng.integers(0, 1 << 32, 2)) for _ in range(64)]

    # the three table lookups: all 4096 words whose bytes are 0 to 7
    for w in range(4096):
        codes = (w & 7) | ((w >> 3) & 7) << 8 | ((w >> 6) & 7) << 16 | ((w >> 9) & 7) << 24
        add("base_letters", codes)
        add("complement_letters", codes)
        add("bam_nibbles", codes, 0)
        add("bam_nibbles", codes, 1)
    # perm_bytes: the selectors the code uses beside the lookups (byte swap, byte pack, bytes_at's five), and every single selector byte of the contract
    selectors = [0x00010203, 0x06040200] + [0x03020100 + at * 0x01010101 for at in range(5)]
    selectors += [v << (8 * k) for k in range(4) for v in range(8)] + [(0x07070707 & ~(7 << (8 * k))) | v << (8 * k) for k in range(4) for v in range(8)]
    for hi, lo in pairs()[12:28]:
        for sel in selectors:
            add("perm_bytes", hi, lo, sel)
        for k in range(4):                                       # a selector byte outside the contract spoils its own byte of the result (masked: argument 3) and no other
            for s in (8, 12, 15, 0xA5, 0xFF):
                add("perm_bytes", hi, lo, (0x05020700 & ~(0xFF << (8 * k))) | s << (8 * k), 0xFF << (8 * k))
    for hi, lo in pairs():
        add("byte_reverse", lo)
        add("byte_reverse", hi)
        for n in range(4):
            add("align_bytes", hi, lo, n)
        for at in range(5):
            add("bytes_at", hi, lo, at)
    nibbles = np.array([0, 1, 2, 4, 8, 15, 3, 9], np.uint32)
    for _ in range(64):
        n = nibbles[rng.integers(0, 8, 8)]
        add("bam_pack", sum(int(c) << (8 * k) for k, c in enumerate(n[:4])), sum(int(c) << (8 * k) for k, c in enumerate(n[4:])))
    for c in (0, 15):
        add("bam_pack", c * 0x01010101, (15 - c) * 0x01010101)
    # div_small: x around q d for the smallest and the largest quotients, inside x < 2^24 and x / d < 2^17
    for d in list(range(1, 301)) + [65535]:
        for q in (0, 1, 1 << 16, (1 << 17) - 1):
            for x in (q * d - 1, q * d, q * d + 1):
                if 0 <= x < 1 << 24 and x // d < 1 << 17:
                    add("div_small", x, d)
    # bits: every one-bit word and 256 random words
    words64 = [1 << k for k in range(64)]                        # (the random ones shifted up by 0 to 63 bits, so that the lowest set bit is anywhere; none is zero)
    words64 += [((int(x) | 1) << int(k)) & (1 << 64) - 1 for x, k in zip(rng.integers(0, 1 << 64, 256, dtype=np.uint64), rng.integers(0, 64, 256))]
    for x in words64:
        for op in ("popcount64", "lowest_set_bit64", "bit_reverse64"):
            add(op, x, x >> 32)
    add("popcount64", 0, 0)
    add("bit_reverse64", 0, 0)
    for x in [1 << k for k in range(32)] + [int(x) for x in rng.integers(0, 1 << 32, 256)] + [0]:
        add("bit_reverse32", x)
    for d in (-(1 << 31), -70000, -1, 0, 1, 5, 6, 7, 1000, (1 << 31) - 1):
        for last in (0, 6, (1 << 31) - 1):
            add("clamp_from_zero", d, last)
    # single precision: operands whose fused and unfused results differ in the last bit, random ones, and the screen's boundary factors 2^-60 and 2^29
    # (rsq_core.h "screened draw": values are 0 or in [2^-60, 2^29]); no result leaves the normal range
    triples = []
    while len(triples) < 64:
        a, b = (bits_of(x) for x in rng.uniform(1.0, 2.0, 2).astype(np.float32))
        c = bits_of(np.float32(rng.uniform(0.5, 4.0)))
        if abs(fused(a, b, c) - unfused(a, b, c)) == 1:
            triples.append((a, b, c))
    for _ in range(32):
        triples.append(tuple(bits_of(x) for x in (rng.normal(0, 100, 3)).astype(np.float32)))
    lo, hi, eps = 2.0 ** -60, 2.0 ** 29, 1 + 2.0 ** -23
    for a, b, c in ((lo, lo, 0.0), (lo, lo, 2.0 ** -120), (lo * eps, lo * eps, 2.0 ** -119), (hi, hi, 0.0), (hi, hi, 2.0 ** 58), (hi / eps, hi / eps, 2.0 ** 57 * eps), (lo, hi, 2.0 ** -31),
                    (lo * eps, hi / eps, 2.0 ** -30), (0.0, hi, 2.0 ** -30), (hi, 0.0, 0.0), (hi * 1.5, hi / eps, lo), (lo * 1.75, 1.0 + 2.0 ** -12, lo * eps)):
        triples.append(tuple(bits_of(np.float32(x)) for x in (a, b, c)))
    for i, (a, b, c) in enumerate(triples):
        a2, b2, c2 = triples[(i + 7) % len(triples)]
        add("fma2", a, a2, b, b2, c, c2)
        add("mul_add2", a, a2, b, b2, c, c2)
        add("fma1", a, 0, b, 0, c, 0)
    # loads: every offset in steps of the stated alignment at which the load stays inside the 64 bytes; the store likewise
    for op, size, step in (("load64_align1", 8, 1), ("load64_align2", 8, 2), ("load128_align2", 16, 2), ("load32_align1", 4, 1), ("load32_align4", 4, 4), ("load64_align1_lds", 8, 1)):
        for off in range(0, 64 - size + 1, step):
            add(op, off)
    for off in range(0, 57):
        v = int(rng.integers(0, 1 << 63)) * 2 + 1
        add("store64_align1", off, v, v >> 32)
    # the image: 64 lanes OR into four words that keep what they hold
    for first, v in ((0, 1), (1, 0x00010000), (2, 0x80000001), (3, 0), (0, 0x00F00000)):
        add("image_or", first, v)
    # any lane of the wave: no lane, the first, the last, one in the middle, many; all 64 lanes there, or fewer
    for mask in (0, 1, 1 << 63, 1 << 17, 1 << 16, int(rng.integers(0, 1 << 63))):
        for lanes in (1, 17, 64):
            add("wave_any", mask, mask >> 32, lanes)
    return np.array(rows, np.uint32)


# ------------------------------------------------------------------------------------------------------------------------- what every record must give
def _bytes(w):
    return [(w >> (8 * k)) & 0xFF for k in range(4)]


def _word(bs):
    return sum(b << (8 * k) for k, b in enumerate(bs))


def _lookup(table):
    return lambda a: [_word(table[b] for b in _bytes(a[0])), 0, 0, 0]


def _x64(a):
    return a[0] | a[1] << 32


def _signed(w):
    return w - (1 << 32) if w >> 31 else w


def _load(size):
    def load(a):
        v = int.from_bytes(BUF[a[0]:a[0] + size], "little")
        assert a[0] + size <= 64
        return [(v >> (32 * k)) & M32 for k in range(4)]
    return load


def _store(a):
    v = (a[1] | a[2] << 32).to_bytes(8, "little")
    return [int.from_bytes(v[:4], "little"), int.from_bytes(v[4:], "little"), sum(v), 0]


MEANING = {
    "base_letters": _lookup([ord(c) for c in "ACGTNNNN"]),
    "complement_letters": _lookup([ord(c) for c in "TGCANNNN"]),
    "bam_nibbles": lambda a: _lookup([8, 4, 2, 1, 15, 15, 15, 15] if a[1] else [1, 2, 4, 8, 15, 15, 15, 15])(a),
    "perm_bytes": lambda a: [_word((_bytes(a[1]) + _bytes(a[0]))[s] if s < 8 else 0 for s in _bytes(a[2])) & ~a[3] & M32, 0, 0, 0],
    "byte_reverse": lambda a: [int.from_bytes(a[0].to_bytes(4, "little"), "big"), 0, 0, 0],
    "bam_pack": lambda a: [_word((c[0] << 4 | c[1]) for c in zip(*[iter(_bytes(a[0]) + _bytes(a[1]))] * 2)), 0, 0, 0],
    "align_bytes": lambda a: [((a[0] << 32 | a[1]) >> (8 * a[2])) & M32, 0, 0, 0],
    "bytes_at": lambda a: [((a[0] << 32 | a[1]) >> (8 * a[2])) & M32, 0, 0, 0],
    "div_small": lambda a: [a[0] // a[1], 0, 0, 0],
    "popcount64": lambda a: [bin(_x64(a)).count("1"), 0, 0, 0],
    "lowest_set_bit64": lambda a: [(_x64(a) & -_x64(a)).bit_length() - 1, 0, 0, 0],
    "bit_reverse32": lambda a: [int(format(a[0], "032b")[::-1], 2), 0, 0, 0],
    "bit_reverse64": lambda a: [int(format(_x64(a), "064b")[::-1], 2) & M32, int(format(_x64(a), "064b")[::-1], 2) >> 32, 0, 0],
    "clamp_from_zero": lambda a: [min(max(_signed(a[0]), 0), _signed(a[1])), 0, 0, 0],
    "fma2": lambda a: [fused(a[0], a[2], a[4]), fused(a[1], a[3], a[5]), 0, 0],
    "fma1": lambda a: [fused(a[0], a[2], a[4]), 0, 0, 0],
    "mul_add2": lambda a: [unfused(a[0], a[2], a[4]), unfused(a[1], a[3], a[5]), 0, 0],
    "load64_align1": _load(8), "load64_align2": _load(8), "load128_align2": _load(16), "load32_align1": _load(4), "load32_align4": _load(4), "load64_align1_lds": _load(8),
    "store64_align1": _store,
}


def expected(table):
    """[records, 4] uint32; the image's records in the table's order, as the programs run them"""
    out, image = [], [0, 0, 0, 0]
    for row in table:
        name, a = OPS[row[0]], [int(x) for x in row[1:7]]
        if name == "image_or":
            for lane in range(64):
                image[(a[0] + lane) & 3] |= ((a[1] << (lane & 31)) | (a[1] >> ((32 - lane) & 31))) & M32
            out.append(list(image))
        elif name == "wave_any":
            here = _x64(a) & ((1 << a[2]) - 1)
            out.append([int(here != 0), 0, 0, 0])
        else:
            out.append(MEANING[name](a))
    return np.array(out, np.uint64).astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------- the two programs
WARNINGS = ["-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]


def build_host(directory, sanitize):
    """portable_trial.cpp as a stand-alone host program; sanitize: with the address and undefined-behaviour sanitizers"""
    exe = os.path.join(str(directory), "portable_trial_san" if sanitize else "portable_trial_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, *WARNINGS, "-o", exe, SOURCE], check=True)
    return exe


def library_arch():
    return re.search(r"^ARCH \?= (\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)


def find_hipcc():
    return shutil.which("hipcc") or next((p for p in ("/opt/rocm/bin/hipcc",) if os.path.exists(p)), None)


def build_device(directory, hipcc):
    """the same source for the library's architecture, with the library's floating-point flags and no sanitizer"""
    exe = os.path.join(str(directory), "portable_trial_device")
    subprocess.run([hipcc, "-x", "hip", f"--offload-arch={library_arch()}", "-O3", "-std=c++17", "-ffp-contract=off", *WARNINGS, "-o", exe, SOURCE], check=True)
    return exe


def run(exe, table, directory, name, timeout=None):
    """the program as a fresh child process over the table -> (its results [records, 4], the finished process)"""
    inputs, results = os.path.join(str(directory), name + "_in.bin"), os.path.join(str(directory), name + "_out.bin")
    table.tofile(inputs)
    done = subprocess.run([exe, inputs, results], capture_output=True, text=True, timeout=timeout)
    got = np.fromfile(results, np.uint32).reshape(-1, 4) if done.returncode == 0 else None
    return got, done
