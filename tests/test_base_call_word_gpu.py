"""The base call decided by the random word alone (reseq_amd/csrc/rsq_reads.h ScreenTables::base_call_word) on the device: byte for byte against the host emulation,
which tests/test_base_call_word.py holds against the oracle, with option base_call_word 0 and 1, on both builds of the read kernels (compiled for the profile at run
time, and the library's own instantiation), for calls of 1, 63, 64, 65 and 129 pairs (a wave's last chunk is partial), together with the switches that change what
the image holds or how the kernel addresses (rate_rows 1, image_tiles 1, force_exact, wide_rows 1); a case with variants and a seqToIllumina case (the other two
kernels share ScreenTables); and one call of a few thousand pairs of profile P0, where the word decides 99 % of the base calls, with the option off and on."""
import numpy as np
import pytest

import parity_cases as P
from backends import EmuBackend, GpuBackend, set_option_everywhere
from reseq_amd import synth

pytestmark = pytest.mark.gpu

PAIR_COUNTS = (1, 63, 64, 65, 129)
LENGTHS = [150 + 37 * (i % 7) + 11 * (i % 5) for i in range(40)]        # a few fragments per block: runs of blocks with exactly the wanted number exist
SEED, NUM_PAIRS = 5, 300


@pytest.fixture
def word_option():
    """set(value) of option base_call_word; back to its default 1 afterwards"""
    yield lambda value: set_option_everywhere("base_call_word", value)
    set_option_everywhere("base_call_word", 1)


@pytest.fixture(scope="module")
def expected(workdir):
    """inputs, the emulation's normalization, and per wanted pair count a block range that holds as many fragments, with the emulation's fragments and texts"""
    ppath, fpath, _ = P.make_inputs(workdir, "base_call_word", synth.TINY, LENGTHS)
    emu = EmuBackend(ppath, fpath)
    info = emu.prepare(SEED, NUM_PAIRS)
    blocks = info["total_blocks"]
    counts = [emu.L.emu_sieve(emu.h, lo, lo + 1, None, 0) for lo in range(1, blocks + 1)]
    before = np.concatenate([[0], np.cumsum(counts)])
    ranges = {n: next((lo + 1, hi + 1) for lo in range(blocks) for hi in range(lo + 1, blocks + 1) if before[hi] - before[lo] == n) for n in PAIR_COUNTS}
    want = {n: emu.pairs(*ranges[n]) for n in PAIR_COUNTS}
    out = dict(ppath=ppath, fpath=fpath, normalization=(info["bias_normalization"], emu.thresholds()), ranges=ranges, want=want)
    emu.close()
    return out


def check(expected, keys=PAIR_COUNTS):
    for key in keys:
        g = GpuBackend(expected["ppath"], expected["fpath"])
        try:
            g.prepare(SEED, NUM_PAIRS)
            g.set_normalization(*expected["normalization"])
            frags, r1, r2 = g.pairs(*expected["ranges"][key])
        finally:
            g.close()
        want = expected["want"][key]
        assert frags.tobytes() == want[0].tobytes(), key
        assert r1 == want[1] and r2 == want[2], key


@pytest.mark.parametrize("word", [1, 0])
@pytest.mark.parametrize("specialize", [1, 0])
def test_pair_counts_equal_the_emulation(expected, rsq_options, word_option, specialize, word):
    rsq_options("specialize", specialize)
    word_option(word)
    check(expected)


@pytest.mark.parametrize("word", [1, 0])
@pytest.mark.parametrize("option", ["rate_rows", "image_tiles", "force_exact", "wide_rows"])
@pytest.mark.parametrize("specialize", [1, 0])
def test_with_the_switches_of_the_image(expected, rsq_options, word_option, specialize, option, word):
    """rate_rows 1: one error-rate row beside the scalars; image_tiles 1: the binned kernel, an image per tile; force_exact: the word decides nothing;
    wide_rows 1: the cursor's 64-bit form"""
    rsq_options("specialize", specialize)
    rsq_options(option, 1)
    word_option(word)
    check(expected)


@pytest.mark.parametrize("word", [1, 0])
def test_variants_and_records(workdir, word_option, word):
    """k_fill_reads with variants and k_fill_records draw through the same ScreenTables"""
    word_option(word)
    P.case_variants_indels(GpuBackend, workdir)
    P.case_error_model_tiny(GpuBackend, workdir)


def test_p0_equal_with_the_option_off_and_on(workdir, word_option):
    """about 3000 pairs of P0 (64 kb): the same fragments and the same FASTQ bytes whether the word decides the base calls or every one reads its rows"""
    ppath, fpath, _ = P.make_inputs(workdir, "base_call_word_p0", synth.P0, [64000], prof_seed=103741084, ref_seed=4)
    got = {}
    for word in (0, 1):
        word_option(word)
        g = GpuBackend(ppath, fpath)
        try:
            info = g.prepare(17, 3000)
            got[word] = g.pairs(1, info["total_blocks"] + 1)
        finally:
            g.close()
    assert 2000 < len(got[1][0]) < 4000
    assert got[0][0].tobytes() == got[1][0].tobytes()
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2]
