"""The random words of reseq_amd/csrc/rsq_core.h on the device: tests/hostemu/philox_steps_trial.cpp compiled by hipcc for the library's architecture.  A kernel
walks Stream::step(2 + t), t = 0 ... 159, in a LOOP -- the read kernel's form, so the compiler places the round keys and hoists what is constant as it does there --
with a wave-uniform seed, distinct counters per lane and 1, 63, 64, 65 and 129 active lanes, once for every choice of philox's key barrier that the tree uses
(and both ends of the range); every word must be what the Philox4x32-10 of tests/philox_reference.py gives.  A second kernel runs philox() with a seed per lane
(the form without the barrier that every other caller takes) over the counters of tests/test_philox_words.py."""
import numpy as np
import pytest

import philox_reference as R
import portable_table as T
from test_philox_words import counters

STEPS, FIRST = 160, 2
LANE_COUNTS = (1, 63, 64, 65, 129)


def lane_counters(n):
    """distinct (c0, c1, c2) per lane: a fragment's start, its sequence, its length and duplicate number (pair_stream, rsq_reads.h); lane 0 and the last lane of the
    largest job at the ends of the range"""
    lanes = [((1000003 * lane + 17) & R.M32, lane % 5, ((lane % 3) << 16) | (150 + lane)) for lane in range(n)]
    lanes[0] = (0, 0, 0)
    if n == max(LANE_COUNTS):
        lanes[-1] = (R.M32, R.M32, R.M32)
    return lanes


@pytest.fixture(scope="module")
def device_trial(tmp_path_factory):
    hipcc = T.find_hipcc()
    assert hipcc, "hipcc is needed to build the device program"
    return R.build_device(tmp_path_factory.mktemp("philox_steps"), hipcc)


@pytest.mark.gpu
def test_the_step_loop_of_every_key_choice(device_trial, tmp_path):
    jobs = [(0x5DEECE66D1234567, 0x1A020000), (0, 0x10000000), (2 ** 64 - 1, 0xF8000000)]      # (seed, c3base): a pair's, all-zero and all-ones keys
    words, want = [], []
    longest = R.job_expected(jobs[0][0], jobs[0][1], FIRST, STEPS, lane_counters(max(LANE_COUNTS))[:-1])      # the lanes of a smaller job are the first of the largest one's
    for j, (seed, c3base) in enumerate(jobs):
        for n in LANE_COUNTS if j == 0 else (65,):
            lanes = lane_counters(n)
            words += R.job_words(seed, c3base, FIRST, STEPS, lanes)
            if j == 0:
                want.append(longest[:n * STEPS] if n < max(LANE_COUNTS) else np.concatenate([longest, R.job_expected(seed, c3base, FIRST, STEPS, lanes[-1:])]))
            else:
                want.append(R.job_expected(seed, c3base, FIRST, STEPS, lanes))
    n_jobs = len(LANE_COUNTS) + len(jobs) - 1
    got = R.run(device_trial, "steps", words, n_jobs, tmp_path, "steps")
    assert len(got) == R.CHOICES * sum(len(w) for w in want)
    at = 0
    for j, w in enumerate(want):
        for choice in range(R.CHOICES):
            part = got[at:at + len(w)]
            bad = np.flatnonzero((part != w).any(axis=1))
            assert not len(bad), (j, choice, len(bad), [(int(i) // STEPS, int(i) % STEPS, part[i].tolist(), w[i].tolist()) for i in bad[:4]])
            at += len(w)


@pytest.mark.gpu
def test_philox_words_with_a_seed_per_lane(device_trial, tmp_path):
    cs = counters()
    got = R.run(device_trial, "words", [w for seed, *c in cs for w in (seed & R.M32, seed >> 32, *c)], len(cs), tmp_path, "words")
    want = np.array([R.philox4x32_10(*c) for c in cs], np.uint64).astype(np.uint32)
    assert got.shape == want.shape and (got == want).all(), np.flatnonzero((got != want).any(axis=1))[:8].tolist()
