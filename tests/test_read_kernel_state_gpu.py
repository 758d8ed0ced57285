"""The read kernels' per-lane state (reseq_amd/csrc/rsq_reads.h: WaveReadOut, WaveFragmentSrc) on the device, byte for byte against the host emulation, which
keeps the pointer forms (ReadOut, FragmentSrc).  TINY profile, both builds of the kernels (compiled for the profile at run time, and the library's own
instantiation), calls of 1, 63, 64, 65 and 129 pairs: a wave's last chunk is partial, and the arrays' pitch (the reads rounded up to 64) is 64, 128, 192 and 320.
TINY's inserts begin at 12 bases and its reads reach 30: fragments shorter than the read run the adapter part and the tail in the general step loop; its indel rates
put deletions in most waves, so read positions lag and the lanes of a wave store different words in one step."""
import numpy as np
import pytest

import parity_cases as P
from backends import EmuBackend, GpuBackend
from reseq_amd import synth

pytestmark = pytest.mark.gpu

PAIR_COUNTS = (1, 63, 64, 65, 129)
# 40 sequences of 150 to 416 bases, a block of start positions each: a few fragments per block, so that runs of blocks with exactly the wanted number exist
LENGTHS = [150 + 37 * (i % 7) + 11 * (i % 5) for i in range(40)]
SEED, NUM_PAIRS = 3, 300


@pytest.fixture(scope="module")
def expected(workdir):
    """inputs, the emulation's normalization, and per wanted pair count the block range that holds as many fragments with the emulation's fragments and texts"""
    ppath, fpath, _ = P.make_inputs(workdir, "kernel_state", synth.TINY, LENGTHS)
    emu = EmuBackend(ppath, fpath)
    info = emu.prepare(SEED, NUM_PAIRS)
    blocks = info["total_blocks"]
    counts = [emu.L.emu_sieve(emu.h, lo, lo + 1, None, 0) for lo in range(1, blocks + 1)]
    before = np.concatenate([[0], np.cumsum(counts)])
    ranges = {}
    for n in PAIR_COUNTS:
        ranges[n] = next((lo + 1, hi + 1) for lo in range(blocks) for hi in range(lo + 1, blocks + 1) if before[hi] - before[lo] == n)
    want = {n: emu.pairs(*ranges[n]) for n in PAIR_COUNTS}
    want["all"] = emu.pairs(1, blocks + 1)
    ranges["all"] = (1, blocks + 1)
    adapter_only = emu.adapter_only_pairs(5, 65)
    out = dict(ppath=ppath, fpath=fpath, normalization=(info["bias_normalization"], emu.thresholds()), ranges=ranges, want=want, adapter_only=adapter_only)
    emu.close()
    for n in PAIR_COUNTS:
        assert len(want[n][0]) == n
    text = want["all"][1] + want["all"][2]
    cigars = [line.split(b" ")[-2] if b" " in line else b"" for line in text.split(b"\n")[0::4]]
    assert any(b"D" in c for c in cigars) and any(b"I" in c for c in cigars) and any(b"S" in c for c in cigars) and any(b"H" in c for c in cigars)
    assert (want["all"][0]["len"] < 30).any()                     # fragments shorter than the longest read
    return out


def gpu_pairs(expected, key):
    g = GpuBackend(expected["ppath"], expected["fpath"])
    try:
        g.prepare(SEED, NUM_PAIRS)
        g.set_normalization(*expected["normalization"])
        return g.pairs(*expected["ranges"][key]), g.adapter_only_pairs(5, 65)
    finally:
        g.close()


def check(expected, keys=PAIR_COUNTS + ("all",)):
    for key in keys:
        (frags, r1, r2), adapter_only = gpu_pairs(expected, key)
        want = expected["want"][key]
        assert frags.tobytes() == want[0].tobytes(), key
        assert r1 == want[1] and r2 == want[2], key
        assert adapter_only == expected["adapter_only"], key


@pytest.mark.parametrize("specialize", [1, 0])
def test_pair_counts_equal_the_emulation(expected, rsq_options, specialize):
    rsq_options("specialize", specialize)
    check(expected)


@pytest.mark.parametrize("specialize", [1, 0])
def test_every_draw_behind_the_screen(expected, rsq_options, specialize):
    """force_exact: every draw takes the double-precision call, the state lives across three calls per step"""
    rsq_options("specialize", specialize)
    rsq_options("force_exact", 1)
    check(expected, (65, 129))


@pytest.mark.parametrize("specialize", [1, 0])
def test_one_staged_rate_row(expected, rsq_options, specialize):
    """rate_rows 1: only row 0 of the error-rate margins is in the image, a position with a systematic error rate reads margin 3 from L2"""
    rsq_options("specialize", specialize)
    rsq_options("rate_rows", 1)
    check(expected, (65, 129))


@pytest.mark.parametrize("specialize", [1, 0])
def test_wide_addresses(expected, rsq_options, specialize):
    """wide_rows 1: the cursor's 64-bit form, which a call takes by itself only from 4 GB of raw arrays on (28 M reads)"""
    rsq_options("specialize", specialize)
    rsq_options("wide_rows", 1)
    check(expected, (1, 65, 129))


@pytest.mark.parametrize("specialize", [1, 0])
def test_records(workdir, rsq_options, specialize):
    """33 seqToIllumina records through k_fill_records: rows of the raw arrays chosen per lane by the records' segment"""
    rsq_options("specialize", specialize)
    ppath, _, _ = P.make_inputs(workdir, "kernel_state_em", synth.TINY, [100], prof_seed=5)
    arrays = synth.make_profile(synth.TINY, seed=5)
    rec = synth.make_error_model_input(21, 33, 30, arrays, zero_frac=0.6)
    emu = EmuBackend(ppath, None)
    emu.prepare(13)
    want = emu.error_model(rec, first_index=17)
    emu.close()
    g = GpuBackend(ppath, None)
    try:
        g.prepare(13)
        got = g.error_model(rec, first_index=17)
    finally:
        g.close()
    assert len(got) == 33 and got == want
