"""xor3 and RSQ_KEEP_IN_SGPR of reseq_amd/csrc/rsq_portable.h -- the three-input xor of Philox's rounds (one v_bitop3_b32 on the device, two xors on the host) and
the scalar barrier behind which a kernel forms the round keys (nothing on the host) -- by the scheme of tests/test_portable_counter.py:
tests/hostemu/xor3_trial.cpp, one source and two programs, evaluates them over a table, and both the host forms (g++ with -fsanitize=address,undefined, a program
of its own) and the device forms (hipcc for the library's architecture; 1, 63, 64 and 65 active lanes) must give what the primitives mean, computed here in plain
Python: a ^ b ^ c, and the value that went in."""
import os
import subprocess

import numpy as np
import pytest

import portable_table as T

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu", "xor3_trial.cpp")
M32 = 0xFFFFFFFF
LANES = (1, 63, 64, 65)                                          # xor3_trial.cpp kLanes


def table():
    triples = [(0, 0, 0), (M32, M32, M32), (M32, 0, 0), (0, M32, 0), (0, 0, M32), (M32, M32, 0), (M32, 0, M32), (0, M32, M32)]
    for bit in range(32):                                        # a single bit in each operand
        triples += [(1 << bit, 0, 0), (0, 1 << bit, 0), (0, 0, 1 << bit)]
    mixes = (0x80000000, 0x01020304, 0, M32)
    triples += [(a, b, c) for a in mixes for b in mixes for c in mixes]
    rng = np.random.default_rng(20240917)
    triples += [tuple(int(x) for x in row) for row in rng.integers(0, 2 ** 32, size=(256, 3), dtype=np.uint64)]
    return np.array(triples, np.uint32)


def rotate_left(v, n):
    n &= 31
    return ((v << n) | (v >> ((32 - n) & 31))) & M32


def expected(triples):
    out = []
    for lanes in LANES:
        for a, b, c in triples.tolist():
            for lane in range(lanes):
                al, bl, cl = (a + lane) & M32, b ^ ((lane * 0x01000193) & M32), rotate_left(c, lane)
                out.append((al ^ bl ^ cl, a, (a + 4 * 0x9E3779B9) & M32, lane))
    return np.array(out, np.uint64).astype(np.uint32)


def run(exe, directory, name):
    inputs, results = os.path.join(str(directory), name + "_in.bin"), os.path.join(str(directory), name + "_out.bin")
    triples = table()
    triples.tofile(inputs)
    done = subprocess.run([exe, inputs, results], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and f"{len(triples)} records" in done.stdout, (done.returncode, done.stdout, done.stderr[-2000:])
    return np.fromfile(results, np.uint32).reshape(-1, 4)


def check(got):
    want = expected(table())
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(bad), [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:8]])


def test_the_table_has_the_cases():
    t = table()
    assert len(t) == 8 + 96 + 64 + 256 and len({tuple(r) for r in t.tolist()}) >= 8 + 96 + 64 + 256 - 11      # the mixes repeat the eight 0 / all-ones triples and three single bits
    want = expected(t)
    assert len(want) == len(t) * sum(LANES)
    assert (want[:len(t), 0] == t[:, 0] ^ t[:, 1] ^ t[:, 2]).all(), "lane 0 of a record is its own triple"


def test_the_host_forms(tmp_path):
    exe = str(tmp_path / "xor3_trial_san")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *T.WARNINGS, "-o", exe, SOURCE], check=True)
    check(run(exe, tmp_path, "san"))


@pytest.mark.gpu
def test_the_device_forms(tmp_path):
    hipcc = T.find_hipcc()
    assert hipcc, "hipcc is needed to build the device program"
    exe = str(tmp_path / "xor3_trial_device")
    subprocess.run([hipcc, "-x", "hip", f"--offload-arch={T.library_arch()}", "-O3", "-std=c++17", "-ffp-contract=off", *T.WARNINGS, "-o", exe, SOURCE], check=True)
    check(run(exe, tmp_path, "device"))
