"""The text kernels' image writers on the device (reseq_amd/csrc/rsq_format.h: ImageSink, image_header, image_line_part in k_format_write, k_record_text_waves and
k_sam_write): the FASTQ text of rsq_sim_pairs and the SAM text of rsq_sim_pairs_sam byte for byte against the host emulation, whose writer is format_record
(rsq_text.h) -- the SAM text against the statement of tests/test_truth_sam.py applied to the emulation's FASTQ text, the emulation writes no SAM.  The inputs are
those of tests/test_truth_sam_gpu.py (TINY's 30-base reads on references of 5000 / 80 / 3210 bases, seed 7, 3000 pairs asked, no substitution errors): leading and
trailing D, I, adapter parts, tails and all four residues of the read length modulo four."""
import numpy as np
import pytest

import parity_cases as P
from backends import EmuBackend, GpuBackend
from reseq_amd import api, synth
from test_truth_sam import sam_text

pytestmark = pytest.mark.gpu

EDITS = {"no_substitutions": True}
LENGTHS = [5000, 80, 3210]


class Both:
    """the host emulation and the device on the same inputs, the device with the emulation's normalisation"""

    def __init__(self, workdir, num_pairs, names=None, tag="tiny_e2e", lengths=LENGTHS):
        self.ppath, self.fpath, self.seqs = P.make_inputs(workdir, tag, synth.TINY, lengths, names=names)
        self.emu = EmuBackend(self.ppath, self.fpath, 0, EDITS)
        self.gpu = GpuBackend(self.ppath, self.fpath, 0, EDITS)
        self.tb = self.emu.prepare(7, num_pairs)["total_blocks"]
        assert self.gpu.prepare(7, num_pairs)["total_blocks"] == self.tb
        self.gpu.set_normalization(self.emu.info()["bias_normalization"], self.emu.thresholds())
        self.names = [self.gpu.ref.sequence_name(i).encode() for i in range(self.gpu.ref.num_sequences())]
        self.frags, self.r1, self.r2 = self.emu.pairs(1, self.tb + 1)

    def sam(self, frags, r1, r2):
        return sam_text(frags, r1, r2, self.names, synth.TINY["phred_offset"])

    def close(self):
        self.gpu.close()
        self.emu.close()


@pytest.fixture(scope="module")
def whole(workdir):
    """the emulation's text of the 3000 pairs, computed once"""
    b = Both(workdir, 3000)
    text = (b.frags, b.r1, b.r2, b.sam(b.frags, b.r1, b.r2), b.emu.adapter_only_pairs(0, 17))
    b.close()
    return text


@pytest.mark.parametrize("binned", [0, 1])
def test_pairs_and_sam_equal_the_emulation(whole, workdir, rsq_options, binned):
    frags, r1, r2, sam, _ = whole
    if binned:
        rsq_options("image_tiles", 1)
    b = Both(workdir, 3000)
    try:
        if binned:
            assert b.gpu.fill_plan()["image_tiles"] == 1
        assert 2000 < len(frags) < 4000
        residues = {len(line) % 4 for line in r1.split(b"\n")[1::4]}
        cigars = b" ".join(line.split(b" ")[1] for line in r1.split(b"\n")[0::4] if line)
        assert residues == {0, 1, 2, 3} and b"D" in cigars and b"I" in cigars and b"S" in cigars and b"H" in cigars      # a change of TINY must not quietly weaken this test
        gf, g1, g2 = b.gpu.pairs(1, b.tb + 1)
        assert gf.tobytes() == frags.tobytes()
        assert g1 == r1 and g2 == r2
        sf, s1, s2, gsam = b.gpu.sim.pairs_sam(1, b.tb + 1)
        assert sf.tobytes() == frags.tobytes() and s1 == r1 and s2 == r2
        assert gsam == sam
    finally:
        b.close()


@pytest.mark.parametrize("binned", [0, 1])
@pytest.mark.parametrize("n", [1, 16, 17])
def test_a_partial_wave_a_full_one_and_one_record_over(whole, workdir, rsq_options, binned, n):
    """n adapter-only pairs exactly (a wave takes 16 records), and the pairs of a simulation that was asked for n"""
    if binned:
        rsq_options("image_tiles", 1)
    b = Both(workdir, n)
    try:
        a1, a2 = b.emu.adapter_only_pairs(0, n)
        assert a1.count(b"\n") == 4 * n
        if n == 17:
            assert (a1, a2) == whole[4]                              # adapter-only pairs do not depend on the pairs asked for
        assert b.gpu.adapter_only_pairs(0, n) == (a1, a2)
        g1, g2, gsam = b.gpu.sim.adapter_only_pairs_sam(0, n)
        assert (g1, g2) == (a1, a2) and gsam == b.sam(None, a1, a2)
        assert b.gpu.adapter_only_pairs(2 ** 32 - 5, n) == b.emu.adapter_only_pairs(2 ** 32 - 5, n)      # read numbers across 2^32
        gf, g1, g2 = b.gpu.pairs(1, b.tb + 1)
        assert gf.tobytes() == b.frags.tobytes() and (g1, g2) == (b.r1, b.r2)
        if len(b.frags):
            sf, s1, s2, gsam = b.gpu.sim.pairs_sam(1, b.tb + 1)
            assert (s1, s2) == (b.r1, b.r2) and gsam == b.sam(b.frags, b.r1, b.r2)
    finally:
        b.close()


def test_error_model_records_from_fasta_text(workdir):
    """33 records (two waves and one record) through rsq_sim_error_model_fasta: the ids are read where they stand in the FASTA text, at any alignment"""
    ppath, _, _ = P.make_inputs(workdir, "em_tiny", synth.TINY, [100], prof_seed=5)
    rec = synth.make_error_model_input(9, 33, 30, synth.make_profile(synth.TINY, seed=5), zero_frac=0.7)
    r = rec["rate"].astype(np.int64)                                 # what survives the file (parity_cases._error_model_fasta)
    rec["rate"] = np.where(r > 86, r - r % 2, r).astype(np.uint8)
    ids = [("r%d" % i) + "x" * (i % 9) + (" more words" if i % 5 == 0 else "") for i in range(33)]
    emu, gpu = EmuBackend(ppath, None), GpuBackend(ppath, None)
    try:
        emu.prepare(13)
        gpu.prepare(13)
        exp = emu.error_model(rec, first_index=17)
        want = b"".join(b"@" + ids[i].encode() + b" " + e[2].encode() + b" E%d\n" % e[3] + bytes(b"ACGTN"[c] for c in e[0]) + b"\n+\n" + e[1] + b"\n" for i, e in enumerate(exp))
        text = P.fasta_of_records(rec, ids, wrap_every=3)
        for skew in (0, 1, 2, 3):
            got, k, used = gpu.error_model_fasta(text, first_index=17, skew=skew)
            assert (k, used) == (33, len(text)) and got == want, skew
        assert gpu.error_model_fastq(rec, [i.encode() for i in ids], first_index=17) == want
    finally:
        gpu.close()
        emu.close()


def test_a_long_name_sends_some_waves_down_the_fallback(workdir):
    """two sequences, the second's name 600 characters long: on a fresh simulator the image holds records of 480 bytes, so the waves of the first sequence's
    records go through it and those of the second are written straight to memory (from the code's arithmetic, as in tests/test_text_image_gpu.py); the call
    after has an image for all of them"""
    b = Both(workdir, 3000, names=["a", "c" * 600], tag="sink_long_name", lengths=[2500, 2500])
    dev = b.gpu.sim.device
    r1, r2 = api.DeviceArray(dev, len(b.r1)), api.DeviceArray(dev, len(b.r2))
    try:
        per_name = np.bincount(b.frags["seq"], minlength=2)
        assert per_name.min() > 300
        n, l1, l2, rc = b.gpu.sim.pairs_device(1, b.tb + 1, r1, r2)                      # the first image
        assert rc == api.RSQ_OK and (n, l1, l2) == (len(b.frags), len(b.r1), len(b.r2))
        assert r1.to_numpy(np.uint8, l1).tobytes() == b.r1 and r2.to_numpy(np.uint8, l2).tobytes() == b.r2
        gf, g1, g2 = b.gpu.pairs(1, b.tb + 1)
        assert (g1, g2) == (b.r1, b.r2)
    finally:
        r1.free()
        r2.free()
        b.close()
