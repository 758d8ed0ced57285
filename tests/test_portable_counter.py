"""counter_add of reseq_amd/csrc/rsq_portable.h -- the addition into a counter in device memory that the truth depth rests on (rsq_depth.h): an atomic without a
result on the device, a plain add on the host -- by the scheme of tests/test_portable.py: tests/hostemu/counter_trial.cpp, one source and two programs, evaluates it
over a table, and both the host form (g++ with -fsanitize=address,undefined, a program of its own) and the device form (hipcc for the library's architecture) must
give what the primitive means, computed here in plain Python."""
import os
import subprocess

import numpy as np
import pytest

import portable_table as T

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu", "counter_trial.cpp")
M32 = 0xFFFFFFFF
# (first counter, the word lane 0 adds): sums that wrap, a -1 (what the depth adds behind an element), nothing, a word whose rotations carry into every counter
TABLE = np.array([(0, 1), (1, M32), (2, 0x80000001), (3, 0), (0, 0x00F00000), (2, M32), (1, 0x7FFFFFFF), (3, 0xDEADBEEF)], np.uint32)


def expected(table):
    out, counters = [], [0, 0, 0, 0]
    for first, v in table.tolist():
        for lane in range(64):
            k = (first + lane) & 3
            counters[k] = (counters[k] + (((v << (lane & 31)) | (v >> ((32 - lane) & 31))) & M32)) & M32
        out.append(list(counters))
    return np.array(out, np.uint64).astype(np.uint32)


def run(exe, directory, name):
    inputs, results = os.path.join(str(directory), name + "_in.bin"), os.path.join(str(directory), name + "_out.bin")
    TABLE.tofile(inputs)
    done = subprocess.run([exe, inputs, results], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and f"{len(TABLE)} records" in done.stdout, (done.returncode, done.stdout, done.stderr[-2000:])
    return np.fromfile(results, np.uint32).reshape(len(TABLE), 4)


def test_the_table_wraps():
    want = expected(TABLE)
    assert want.shape == (len(TABLE), 4) and len({tuple(r) for r in want.tolist()}) >= len(TABLE) - 1
    assert (want[1].astype(np.int64) < want[0].astype(np.int64)).any(), "an addition of -1 takes a counter down: the sum is modulo 2^32"


def test_the_host_form_adds(tmp_path):
    exe = str(tmp_path / "counter_trial_san")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *T.WARNINGS, "-o", exe, SOURCE], check=True)
    got, want = run(exe, tmp_path, "san"), expected(TABLE)
    assert (got == want).all(), (got.tolist(), want.tolist())


@pytest.mark.gpu
def test_the_device_form_adds(tmp_path):
    hipcc = T.find_hipcc()
    assert hipcc, "hipcc is needed to build the device program"
    exe = str(tmp_path / "counter_trial_device")
    subprocess.run([hipcc, "-x", "hip", f"--offload-arch={T.library_arch()}", "-O3", "-std=c++17", "-ffp-contract=off", *T.WARNINGS, "-o", exe, SOURCE], check=True)
    got, want = run(exe, tmp_path, "device"), expected(TABLE)
    assert (got == want).all(), (got.tolist(), want.tolist())
