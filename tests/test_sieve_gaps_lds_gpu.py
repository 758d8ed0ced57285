"""The sieve's gap walk on LDS copies of its coverage group's tables (reseq_amd/csrc/rsq_sieve.h: k_sieve_gaps_lds) against the host emulation, whose walk is
sieve_gaps on the tables in memory, and against the device's own walk in memory (k_sieve_gaps: option sieve_lds 0, and an LDS budget below the profile's need):
fragments and both FASTQ texts byte for byte -- the read ids carry every sieve result.

Inputs: TINY on references of 5000 / 80 / 3210 bases (short last blocks, and a sequence shorter than the longest insert, which gets no block), seed 7, 3000 pairs
asked, and a file of reference sequence biases that puts the first and the third sequence into different coverage groups (SplitCoverageGroups: a new group where the
bias is more than twice the group's first).  A block has 1000 start position slots and a tile of the walk 256, so the tile of slots 4864..5119 covers the end of the
first sequence and the start of the third.  A tile is served with the tables of its first slot's group; its lanes of another group -- here the start positions 0..119
of the third sequence -- walk the tables in memory.  Two placements, so that either group is the staged one of that tile:
  third_high    biases 1, 1, 3
  third_low     biases 3, 3, 1"""
import numpy as np
import pytest

import parity_cases as P
from backends import EmuBackend, GpuBackend, set_option_everywhere
from reseq_amd import synth

pytestmark = pytest.mark.gpu

EDITS = {"no_substitutions": True}
LENGTHS = [5000, 80, 3210]
BIASES = {"third_high": [1.0, 1.0, 3.0], "third_low": [3.0, 3.0, 1.0]}
BLOCK, TILE = 1000, 256
LDS_PER_LENGTH = 20                      # kSieveLdsPerLength


@pytest.fixture
def sieve_options():
    """set(name, value) for the sieve's options, back to their defaults afterwards (sieve_lds is on by default)"""
    defaults = {"sieve_lds": 1, "sieve_lds_bytes": 0}
    changed = []

    def set_(name, value):
        set_option_everywhere(name, value)
        changed.append(name)

    yield set_
    for name in changed:
        set_option_everywhere(name, defaults[name])


def coverage_groups(bias):
    """SplitCoverageGroups (rsq_pack.h plan_bias_normalization) restated"""
    order = sorted((b, i) for i, b in enumerate(bias))
    groups, start, g = [0] * len(bias), order[0][0], 0
    for b, i in order:
        if b > 2 * start:
            start, g = b, g + 1
        groups[i] = g
    return groups


def with_blocks(insert_to):
    """the sequences that get blocks: those no shorter than the longest insert"""
    return [i for i, n in enumerate(LENGTHS) if n >= insert_to]


def slot_groups(groups, insert_to):
    """per start position slot of the whole job: (the coverage group of its sequence, -1 for the dead slots behind a sequence's end; its sequence)"""
    live, seq = [], []
    for i in with_blocks(insert_to):
        n = -(-LENGTHS[i] // BLOCK) * BLOCK
        live += [groups[i]] * LENGTHS[i] + [-1] * (n - LENGTHS[i])
        seq += [i] * n
    return np.array(live), np.array(seq)


class Job:
    def __init__(self, workdir, placement):
        self.ppath, self.fpath, seqs = P.make_inputs(workdir, "sieve_lds", synth.TINY, LENGTHS)
        names = [n.split(" ")[0] for n, _ in seqs]
        self.bias_file = workdir / f"sieve_lds_{placement}.tsv"
        self.bias_file.write_text("".join(f"{n}\t{b}\n" for n, b in zip(names, BIASES[placement])))
        self.placement = placement
        self.emu = self._prepared(EmuBackend)
        self.info = self.emu.info()
        self.tb = self.info["total_blocks"]
        self.frags, self.r1, self.r2 = self.emu.pairs(1, self.tb + 1)

    def _prepared(self, cls):
        b = cls(self.ppath, self.fpath, 0, EDITS)
        b.set_ref_bias_file(self.bias_file)
        b.prepare(7, 3000, 0.0, 3)
        return b

    def device(self):
        """a fresh simulator on the device (it takes the options as they are now), with the emulation's normalisation"""
        g = self._prepared(GpuBackend)
        assert g.info()["total_blocks"] == self.tb and g.info()["n_groups"] == 2
        g.set_normalization(self.info["bias_normalization"], self.emu.thresholds())
        return g

    def close(self):
        self.emu.close()


@pytest.fixture(scope="module", params=list(BIASES))
def job(request, workdir):
    j = Job(workdir, request.param)
    yield j
    j.close()


def test_the_inputs_put_a_tile_across_two_groups(job):
    """a change of TINY or of the block size must not quietly weaken the cases below"""
    groups = coverage_groups(BIASES[job.placement])
    assert list(job.emu.ref_seq_bias(3)) == BIASES[job.placement] and job.info["n_groups"] == 2 and len(set(groups)) == 2
    per_group = np.bincount(np.array(groups)[job.frags["seq"]], minlength=2)
    assert per_group.min() > 300, per_group                         # both groups have pairs
    sg, seq_of_slot = slot_groups(groups, job.info["insert_to"])
    assert len(sg) == job.tb * BLOCK
    strangers = {}                                                   # tile -> its live slots of another group than its first slot's sequence
    for tile in range(-(-len(sg) // TILE)):
        live = sg[tile * TILE:(tile + 1) * TILE]
        other = np.flatnonzero((live >= 0) & (live != groups[seq_of_slot[tile * TILE]]))
        if len(other):
            strangers[tile] = other + tile * TILE
    want_tile, want_seq = 4864 // TILE, 2
    assert list(strangers) == [want_tile]                            # the straddling tile exists
    assert sg[want_tile * TILE] == groups[0] and set(seq_of_slot[strangers[want_tile]]) == {want_seq} and int(strangers[want_tile][0]) == 5 * BLOCK
    # pairs come out of the lanes that walk in memory beside the staged ones
    in_strangers = (job.frags["seq"] == want_seq) & (job.frags["start"] < len(strangers[want_tile]))
    assert in_strangers.sum() > 0
    assert (job.info["insert_to"] - synth.TINY["ins_from"]) * LDS_PER_LENGTH > 1024      # the budget of test_a_budget_below_the_need... is below the need


def run(job, want_lds):
    g = job.device()
    try:
        out = g.pairs(1, job.tb + 1)
        lds, mem = g.sim.last_kernel_launches("sieve_gaps_lds"), g.sim.last_kernel_launches("sieve_gaps_mem")
        assert (lds > 0, mem > 0) == (want_lds, not want_lds), (lds, mem)
        return out
    finally:
        g.close()


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2] == b[2]


def test_lds_walk_equals_the_emulation_and_the_walk_in_memory(job, sieve_options):
    assert 2000 < len(job.frags) < 4000
    on = run(job, True)
    assert same(on, (job.frags, job.r1, job.r2))
    sieve_options("sieve_lds", 0)
    off = run(job, False)
    assert same(off, on)


def test_a_budget_below_the_need_takes_the_walk_in_memory(job, sieve_options):
    sieve_options("sieve_lds_bytes", 1024)
    assert same(run(job, False), (job.frags, job.r1, job.r2))


def test_sub_ranges_of_blocks(job):
    """calls that begin and end inside the job: the tiles are counted from the call's first block, so other tiles straddle"""
    g = job.device()
    try:
        for lo, hi in ((2, 8), (5, 7), (6, job.tb + 1)):
            want = job.emu.pairs(lo, hi)
            assert same(g.pairs(lo, hi), want), (lo, hi)
            assert g.sim.last_kernel_launches("sieve_gaps_lds") > 0
    finally:
        g.close()
