"""Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11) in plain Python, from the paper -- independent of
reseq_amd/csrc/rsq_core.h and of the oracle -- and how tests/hostemu/philox_steps_trial.cpp is built and run (tests/test_philox_words.py,
tests/test_philox_steps_gpu.py)."""
import os
import subprocess

import numpy as np

import portable_table as T

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu", "philox_steps_trial.cpp")
M32 = 0xFFFFFFFF
M0, M1 = 0xD2511F53, 0xCD9E8D57                                  # the two multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                                  # the key schedule's increments (golden ratio, sqrt(3) - 1)
CHOICES = 5                                                      # philox_steps_trial.cpp kChoices


def philox4x32_10(seed, c0, c1, c2, c3):
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + W0) & M32, (k1 + W1) & M32
    return c0, c1, c2, c3


def build_host(directory):
    exe = os.path.join(str(directory), "philox_steps_trial_san")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *T.WARNINGS, "-o", exe, SOURCE], check=True)
    return exe


def build_device(directory, hipcc):
    exe = os.path.join(str(directory), "philox_steps_trial_device")
    subprocess.run([hipcc, "-x", "hip", f"--offload-arch={T.library_arch()}", "-O3", "-std=c++17", "-ffp-contract=off", *T.WARNINGS, "-Wno-unused-result", "-o", exe, SOURCE], check=True)
    return exe


def run(exe, mode, inputs_array, n_records, directory, name):
    """the program as a fresh child process -> its results, four words a row"""
    inputs, results = os.path.join(str(directory), name + "_in.bin"), os.path.join(str(directory), name + "_out.bin")
    np.asarray(inputs_array, np.uint32).tofile(inputs)
    done = subprocess.run([exe, mode, inputs, results], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and f"{n_records} records" in done.stdout, (done.returncode, done.stdout, done.stderr[-2000:])
    return np.fromfile(results, np.uint32).reshape(-1, 4)


def job_words(seed, c3base, first, steps, lanes):
    """a job of the `steps` mode: its header and the lanes' (c0, c1, c2)"""
    return [seed & M32, seed >> 32, c3base, first, steps, len(lanes)] + [w for lane in lanes for w in lane]


def job_expected(seed, c3base, first, steps, lanes):
    """[lane][step] -> four words, once (every choice of the program must give the same)"""
    return np.array([philox4x32_10(seed, c0, c1, c2, c3base | (first + t)) for c0, c1, c2 in lanes for t in range(steps)], np.uint64).astype(np.uint32)
