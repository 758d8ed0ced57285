"""The random words of reseq_amd/csrc/rsq_core.h on the CPU: philox() and Stream::step through tests/hostemu/philox_steps_trial.cpp (a program of its own, g++ with
-fsanitize=address,undefined) against a Philox4x32-10 written from the paper in plain Python (tests/philox_reference.py) and against the oracle's.  philox() forms
its three-way xors with xor3 and may pass its round keys through a barrier that is nothing on the host (rsq_portable.h): every choice of the barrier the trial
instantiates must give the same words.  The device forms: tests/test_philox_steps_gpu.py."""
import numpy as np
import pytest

import oracle_lib as O
import philox_reference as R

M32 = R.M32


def counters():
    """(seed, c0, c1, c2, c3): all zero, all ones, the domain tag alone (the top bits of c3), each with the other's key, and 1000 seeded random ones"""
    fixed = [(0, 0, 0, 0, 0), (2 ** 64 - 1, M32, M32, M32, M32), (0, 0, 0, 0, 0xF8000000), (0x0123456789ABCDEF, 0, 0, 0, 0xF8000000), (0, M32, M32, M32, M32), (2 ** 64 - 1, 0, 0, 0, 0),
             (0, 0, 0, 0, 0x10000000), (1, 0, 0, 0, 0), (1 << 32, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1)]
    rng = np.random.default_rng(4711)
    return fixed + [(int(rng.integers(0, 2 ** 64, dtype=np.uint64)), *(int(x) for x in rng.integers(0, 2 ** 32, size=4, dtype=np.uint64))) for _ in range(1000)]


@pytest.fixture(scope="module")
def trial(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp("philox_words"))


def test_the_reference_is_philox4x32_10():
    # the known-answer vectors of the Random123 distribution (kat_vectors: philox4x32 10)
    assert R.philox4x32_10(0, 0, 0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert R.philox4x32_10(2 ** 64 - 1, M32, M32, M32, M32) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert R.philox4x32_10((0x299F31D0 << 32) | 0xA4093822, 0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_philox_words(trial, tmp_path):
    cs = counters()
    got = R.run(trial, "words", [w for seed, *c in cs for w in (seed & M32, seed >> 32, *c)], len(cs), tmp_path, "words")
    want = np.array([R.philox4x32_10(*c) for c in cs], np.uint64).astype(np.uint32)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(bad), [(cs[i], got[i].tolist(), want[i].tolist()) for i in bad[:4]])
    for c, words in zip(cs, got.tolist()):
        assert words == list(O.lib().orc_philox4x32_10(*c).w), c


def test_the_steps_of_a_read(trial, tmp_path):
    """Stream::step(s) for s = 0 ... 320 of one stream: the sequence a read walks (two draws ahead of its iterations, then one per iteration)"""
    seed, c3base, lanes = 0x5DEECE66D1234567, 0x1A020000, [(123456, 3, (7 << 16) | 301)]
    got = R.run(trial, "steps", R.job_words(seed, c3base, 0, 321, lanes), 1, tmp_path, "steps")
    want = R.job_expected(seed, c3base, 0, 321, lanes)
    assert got.shape == (R.CHOICES * 321, 4)
    for choice in range(R.CHOICES):
        assert (got[choice * 321:(choice + 1) * 321] == want).all(), choice
    assert got[:321].tolist() == [list(O.lib().orc_philox4x32_10(seed, *lanes[0], c3base | s).w) for s in range(321)]
