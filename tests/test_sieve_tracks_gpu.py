"""The sieve's candidate kernel with the pre-pass's surrounding-bias tracks kept (reseq_amd/csrc/rsq_sim.hip DevicePrepass::bias_partials, rsq_sim::SieveTracks;
rsq_sieve.h k_sieve_finish<0, 1>, BiasTracks): a cell's two surrounding factors come from the tracks instead of surrounding_forward / surrounding_reverse and the
sur_bias table.  Fragments and both FASTQ texts byte for byte against the host emulation (whose cells are sieve_cell on the reference) and against the device with
option sieve_tracks_mb 0; every case asserts through rsq_sim_last_kernel_launches ("sieve_tracks" / "sieve_tracks_off") which of the two the call took.

Inputs as in tests/test_sieve_gaps_lds_gpu.py: TINY, references of 5000 / 80 / 3210 bases in two coverage groups, seed 7, 3000 pairs asked.  A simulator takes one
reference for its lifetime (a second rsq_sim_import_reference is refused), so "tracks of an earlier pre-pass" are those of an earlier rsq_sim_prepare of the same
simulator: a whole pre-pass, then a sharded one over a part of the blocks, then a whole one with another seed and pair count."""
import numpy as np
import pytest

import parity_cases as P
from backends import EmuBackend, GpuBackend, set_option_everywhere
from reseq_amd import sharding, synth

pytestmark = pytest.mark.gpu

EDITS = {"no_substitutions": True}
LENGTHS = [5000, 80, 3210]
BIASES = [1.0, 1.0, 3.0]
TRACKS_MB_DEFAULT = 4096


@pytest.fixture
def tracks_mb():
    """set(value) of option sieve_tracks_mb, back to its default afterwards"""
    def set_(value):
        set_option_everywhere("sieve_tracks_mb", value)

    yield set_
    set_option_everywhere("sieve_tracks_mb", TRACKS_MB_DEFAULT)


class Inputs:
    def __init__(self, workdir, tag="sieve_tracks", lengths=LENGTHS, biases=BIASES):
        self.ppath, self.fpath, seqs = P.make_inputs(workdir, tag, synth.TINY, lengths)
        self.lengths = lengths
        names = [n.split(" ")[0] for n, _ in seqs]
        self.bias_file = workdir / f"{tag}.tsv"
        self.bias_file.write_text("".join(f"{n}\t{b}\n" for n, b in zip(names, biases)))

    def backend(self, cls):
        b = cls(self.ppath, self.fpath, 0, EDITS)
        b.set_ref_bias_file(self.bias_file)
        return b


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2] == b[2]


def took(gpu):
    on, off = gpu.sim.last_kernel_launches("sieve_tracks"), gpu.sim.last_kernel_launches("sieve_tracks_off")
    assert (on > 0) != (off > 0), (on, off)
    return on > 0


@pytest.fixture(scope="module")
def inputs(workdir):
    return Inputs(workdir)


@pytest.fixture(scope="module")
def whole(inputs):
    """the emulation's whole job, computed once: (info, thresholds, (fragments, text 1, text 2))"""
    emu = inputs.backend(EmuBackend)
    info = emu.prepare(7, 3000, 0.0, 3)
    out = (info, emu.thresholds(), emu.pairs(1, info["total_blocks"] + 1))
    emu.close()
    return out


def device_run(inputs, whole, want_tracks):
    info, thresholds, _ = whole
    g = inputs.backend(GpuBackend)
    try:
        g.prepare(7, 3000, 0.0, 3)
        g.set_normalization(info["bias_normalization"], thresholds)      # the tracks do not depend on the normalisation: they stay
        out = g.pairs(1, info["total_blocks"] + 1)
        assert took(g) == want_tracks
        return out
    finally:
        g.close()


def test_kept_tracks_equal_the_emulation_and_the_device_without_them(inputs, whole, tracks_mb):
    info, _, want = whole
    assert info["n_groups"] == 2 and 2000 < len(want[0]) < 4000
    ends = want[0]["start"] + want[0]["len"]
    assert (want[0]["start"] < 10).any() and (np.array(LENGTHS)[want[0]["seq"]] - ends < 10).any()      # cells whose surroundings wrap around a sequence end
    on = device_run(inputs, whole, True)
    assert same(on, want)
    tracks_mb(0)
    off = device_run(inputs, whole, False)
    assert same(off, on)


def test_a_budget_of_one_mb_on_a_reference_that_needs_more(workdir, tracks_mb):
    """16 bytes per position of the share and of the reach behind it (a chunk of the bias sums and an insert length): 70 000 bases need more than 2^20 bytes"""
    big = Inputs(workdir, "sieve_tracks_big", [70000], [1.0])
    emu = big.backend(EmuBackend)
    try:
        info = emu.prepare(7, 3000, 0.0, 3)
        whole = (info, emu.thresholds(), emu.pairs(1, info["total_blocks"] + 1))
    finally:
        emu.close()
    assert 70000 * 16 > 1 << 20 and len(whole[2][0]) > 2000
    tracks_mb(1)
    assert same(device_run(big, whole, False), whole[2])
    tracks_mb(TRACKS_MB_DEFAULT)
    assert same(device_run(big, whole, True), whole[2])


def test_a_sharded_prepare_keeps_its_share(inputs, whole):
    """two ranks in one process (rsq_sim_prepare_plan .. rsq_sim_prepare_finish): each keeps the tracks of its blocks and the reach behind them, and a call
    inside its blocks takes them"""
    info, thresholds, _ = whole
    emu = inputs.backend(EmuBackend)
    ranks = [inputs.backend(GpuBackend) for _ in range(2)]
    try:
        emu.prepare(7, 3000, 0.0, 3)
        for b in ranks:
            b.seq_len = LENGTHS
            b.ref_seq_bias_ = b.ref_seq_bias
            b.ref_seq_bias = lambda b=b: b.ref_seq_bias_(len(LENGTHS))
        _, ranges, _ = sharding.sharded_prepare_in_process(ranks, 7, 3000, 0.0, 3)
        assert all(lo < hi for lo, hi in ranges) and ranges[0][1] == ranges[1][0]
        for b, (lo, hi) in zip(ranks, ranges):
            b.set_normalization(info["bias_normalization"], thresholds)
            want = emu.pairs(lo, hi)
            assert len(want[0]) > 300
            assert same(b.pairs(lo, hi), want) and took(b)
            if hi - lo > 2:                                          # a call strictly inside the share
                assert same(b.pairs(lo + 1, hi - 1), emu.pairs(lo + 1, hi - 1)) and took(b)
    finally:
        emu.close()
        for b in ranks:
            b.close()


def test_no_tracks_of_an_earlier_prepare_survive(inputs, whole):
    """one simulator: a whole pre-pass, a sharded one over the last blocks only (its tracks begin inside the reference), a whole one with another seed and
    pair count; after each the calls equal the emulation prepared the same way"""
    info, thresholds, want = whole
    tb = info["total_blocks"]
    emu, first = inputs.backend(EmuBackend), inputs.backend(EmuBackend)
    g = inputs.backend(GpuBackend)
    try:
        g.prepare(7, 3000, 0.0, 3)
        g.set_normalization(info["bias_normalization"], thresholds)
        assert same(g.pairs(1, tb + 1), want) and took(g)
        # a sharded pre-pass in which this simulator is the second of two ranks (the first is an emulation): its share begins inside the reference
        first.seq_len = LENGTHS
        bias_of = first.ref_seq_bias
        first.ref_seq_bias = lambda: bias_of(len(LENGTHS))
        _, ranges, _ = sharding.sharded_prepare_in_process([first, g], 7, 3000, 0.0, 3)
        lo, hi = ranges[1]
        assert 1 < lo < hi == tb + 1
        g.set_normalization(info["bias_normalization"], thresholds)
        emu.prepare(7, 3000, 0.0, 3)
        part = emu.pairs(lo, hi)
        assert len(part[0]) > 300
        assert same(g.pairs(lo, hi), part) and took(g)
        # a whole pre-pass again, another job
        other = emu.prepare(11, 2000, 0.0, 3)
        g.prepare(11, 2000, 0.0, 3)
        g.set_normalization(other["bias_normalization"], emu.thresholds())
        again = emu.pairs(1, tb + 1)
        assert len(again[0]) != len(want[0])
        assert same(g.pairs(1, tb + 1), again) and took(g)
    finally:
        emu.close()
        first.close()
        g.close()
