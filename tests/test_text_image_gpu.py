"""The text writers' wave image (WaveImage, reseq_amd/csrc/rsq_format.h) where a wave's text does NOT fit it: k_format_write, k_sam_write and k_record_text_waves
then write straight to HBM, and a later call has a larger image.  No other input of the suite has records that long.

The reference has four sequences of 2500 bases whose names are 1, 300, 600 and 1200 characters long (TINY, seed 7, 3000 pairs, the oracle's normalisation:
2953 pairs, R1's id lines of 43 to 1272 bytes, spread evenly over the names).  The routes, from the code's arithmetic (a test cannot observe them; it asserts the
text):
  FASTQ  the first call of a simulator has an image for records of 480 bytes: records with the 1- and 300-character names fit it, the 600-character name falls
         back and fits on the next call (the image is then sized from the longest record of the call before), the 1200-character name never fits the 16 KB cap.
  SAM    a pair's text carries the name four times (QNAME and RNAME of both records); the first image holds pairs of 1100 bytes: the 1-character name fits, the
         300-character name falls back and then fits, the 600- and 1200-character names never fit the 32 KB cap.
  binned rows (option image_tiles = 1: PERM) have a slot of the image per record and go through it only if all 16 of a wave fit theirs: with four names next to
         no wave does, hence the second reference with names of 1 and 600 characters, whose waves get from fallback to image on the second call.
A call for the sizes (the Python helpers make one in front of theirs) writes nothing but already leaves its longest record to the next call, so every test first
makes one writing call of its own into buffers sized from the expected text: that is the call with the first image."""
import numpy as np
import pytest

import oracle_lib as O
import parity_cases as P
from backends import GpuBackend
from reseq_amd import api, synth
from test_truth_sam import sam_text

pytestmark = pytest.mark.gpu

MARKER = 0xA7
REFERENCES = {"four": [c * n for c, n in zip("abcd", (1, 300, 600, 1200))], "two": ["a", "c" * 600]}


class Expected:
    """the oracle's fragments and FASTQ text of one reference, and its normalisation for the device"""

    def __init__(self, workdir, which):
        self.tag, self.names = "long_names_" + which, REFERENCES[which]
        self.lengths = [2500] * len(self.names)
        _, _, seqs = P.make_inputs(workdir, self.tag, synth.TINY, self.lengths, names=self.names)
        oprof = O.Profile(str(workdir / (self.tag + ".rsqp")))
        oref = O.Reference(seqs)
        osim = O.Sim(oprof, oref, 7, 3000, 0.0, b"", 0, None)
        try:
            self.tb = osim.total_blocks()
            self.norm = osim.bias_normalization(), osim.thresholds()
            self.frags = osim.sieve(1, self.tb + 1)
            self.r1, self.r2 = osim.create_reads(self.frags)
        finally:
            osim.close()
            oref.close()
            oprof.close()
        self.sam = sam_text(self.frags, self.r1, self.r2, [n.encode() for n in self.names], synth.TINY["phred_offset"])

    def simulator(self, workdir):
        """a fresh one (first image), prepared like the oracle"""
        ppath, fpath, _ = P.make_inputs(workdir, self.tag, synth.TINY, self.lengths, names=self.names)
        b = GpuBackend(ppath, fpath)
        b.prepare(7, 3000)
        b.set_normalization(*self.norm)
        return b


@pytest.fixture(scope="module")
def expected(workdir):
    made = {}

    def get(which):
        if which not in made:
            made[which] = Expected(workdir, which)
        return made[which]
    return get


def test_the_inputs_are_what_the_routes_assume(expected):
    e = expected("four")
    ids = [len(line) for line in e.r1.split(b"\n")[0::4] if line]                     # of R1
    per_name = np.bincount(e.frags["seq"], minlength=4)
    print(len(e.frags), "pairs, id lines", min(ids), "..", max(ids), "bytes, per name", per_name)
    assert len(e.frags) == 2953 and (min(ids), max(ids)) == (43, 1272) and per_name.min() > 600


def set_row_order(rsq_options, b_of, binned):
    if binned:
        rsq_options("image_tiles", 1)
    b = b_of()
    if binned:
        assert b.fill_plan()["image_tiles"] == 1
    return b


@pytest.mark.parametrize("binned,which", [(0, "four"), (1, "four"), (1, "two")])
def test_pairs(expected, workdir, rsq_options, binned, which):
    e = expected(which)
    b = set_row_order(rsq_options, lambda: e.simulator(workdir), binned)
    dev = b.sim.device
    r1, r2 = api.DeviceArray(dev, len(e.r1)), api.DeviceArray(dev, len(e.r2))
    try:
        n, l1, l2, rc = b.sim.pairs_device(1, e.tb + 1, r1, r2)                  # the first image
        assert rc == api.RSQ_OK and (n, l1, l2) == (len(e.frags), len(e.r1), len(e.r2))
        assert r1.to_numpy(np.uint8, l1).tobytes() == e.r1 and r2.to_numpy(np.uint8, l2).tobytes() == e.r2
        for call in range(2):
            frags, f1, f2 = b.pairs(1, e.tb + 1)
            assert frags.tobytes() == e.frags.tobytes(), call
            assert f1 == e.r1 and f2 == e.r2, call
    finally:
        r1.free()
        r2.free()
        b.close()


@pytest.mark.parametrize("binned", [0, 1])
def test_pairs_sam(expected, workdir, rsq_options, binned):
    e = expected("four")
    b = set_row_order(rsq_options, lambda: e.simulator(workdir), binned)
    dev = b.sim.device
    bufs = [api.DeviceArray(dev, len(t)) for t in (e.r1, e.r2, e.sam)]
    try:
        n, l1, l2, ls, rc = b.sim.pairs_sam_device(1, e.tb + 1, *bufs)           # the first images
        assert rc == api.RSQ_OK and (n, l1, l2, ls) == (len(e.frags), len(e.r1), len(e.r2), len(e.sam))
        assert [d.to_numpy(np.uint8, len(t)).tobytes() for d, t in zip(bufs, (e.r1, e.r2, e.sam))] == [e.r1, e.r2, e.sam]
        for call in range(2):
            frags, f1, f2, sam = b.sim.pairs_sam(1, e.tb + 1)
            assert frags.tobytes() == e.frags.tobytes() and f1 == e.r1 and f2 == e.r2, call      # e.r1, e.r2: what test_pairs has from pairs()
            assert sam == e.sam, call                                                              # the statement, applied to these fragments and FASTQ texts
    finally:
        for d in bufs:
            d.free()
        b.close()


@pytest.fixture(scope="module")
def records(workdir):
    """case_error_model_tiny's 400 records, their ids 5, 600 and 1200 bytes long in turn, and the text from the oracle's reads"""
    ppath, _, _ = P.make_inputs(workdir, "em_tiny", synth.TINY, [100], prof_seed=5)
    rec = synth.make_error_model_input(9, 400, 30, synth.make_profile(synth.TINY, seed=5), zero_frac=0.7)
    oprof = O.Profile(ppath)
    exp = O.error_model_only(oprof, 13, rec, first_index=17)
    oprof.close()
    ids = [(b"r%04d" % i).ljust((5, 600, 1200)[i % 3], b"x") for i in range(400)]
    want = b"".join(b"@" + ids[i] + b" " + e[2].encode() + b" E%d\n" % e[3] + bytes(b"ACGTN"[c] for c in e[0]) + b"\n+\n" + e[1] + b"\n" for i, e in enumerate(exp))
    return ppath, rec, ids, want


@pytest.mark.parametrize("binned", [0, 1])
def test_error_model_fastq(records, rsq_options, binned):
    ppath, rec, ids, want = records

    def fresh():
        b = GpuBackend(ppath, None)
        b.prepare(13)
        return b
    b = set_row_order(rsq_options, fresh, binned)
    try:
        assert b.sim.error_model_fastq(rec, ids, first_index=17, text_len=len(want)) == want      # the first image
        for call in range(2):
            assert b.error_model_fastq(rec, ids, first_index=17) == want, call
    finally:
        b.close()


def test_enospc_comes_before_the_fallback_writes(expected, workdir):
    """an R1 buffer one byte short on a fresh simulator, whose waves would mostly write straight to HBM: sizes reported, nothing written to it (the capacity is
    checked per file: R2, which fits, is written)"""
    e = expected("four")
    b = e.simulator(workdir)
    dev = b.sim.device
    r1 = api.DeviceArray.from_numpy(dev, np.full(len(e.r1) - 1, MARKER, np.uint8))
    r2 = api.DeviceArray(dev, len(e.r2))
    try:
        n, l1, l2, rc = b.sim.pairs_device(1, e.tb + 1, r1, r2)
        assert rc == api.RSQ_ENOSPC and (n, l1, l2) == (len(e.frags), len(e.r1), len(e.r2))
        assert np.all(r1.to_numpy(np.uint8, len(e.r1) - 1) == MARKER)
    finally:
        r1.free()
        r2.free()
        b.close()
