"""The scan that places the records' text (reseq_amd/csrc/rsq_scan.h: k_scan_tile_sums, k_scan_tiles, k_scan_apply) at the ends of its tiles, and the longest
record's size, which its first pass now finds (it sizes the text kernel's LDS image of the next call): seqToIllumina records through rsq_sim_error_model_fastq, where
the number of records is exact -- n = 1, T - 1, T, T + 1 and 3 T + 5 for the tile of T = 4096 elements -- against the host emulation's records, byte for byte.
The last record has the longest id by far, so the maximum lies in the last, partial tile; every n runs twice on one simulator: the second call's image is sized
by the first call's maximum, and both calls size their text exactly (a wrong offset or a wrong total would end in RSQ_ENOSPC or in other bytes)."""
import numpy as np
import pytest

import parity_cases as P
from backends import EmuBackend, GpuBackend
from reseq_amd import synth

pytestmark = pytest.mark.gpu

TILE = 4096                                  # kScanTile
SIZES = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
FIRST = 17


@pytest.fixture(scope="module")
def records(workdir):
    """3 T + 5 records of 30 bases and the emulation's result for them, computed once: a record's draws depend on its index alone, so the first n records of the
    result are the result of the first n records"""
    ppath, _, _ = P.make_inputs(workdir, "scan_tiny", synth.TINY, [100], prof_seed=5)
    n = max(SIZES)
    rec = synth.make_error_model_input(9, n, 30, synth.make_profile(synth.TINY, seed=5), zero_frac=0.7)
    r = rec["rate"].astype(np.int64)
    rec["rate"] = np.where(r > 86, r - r % 2, r).astype(np.uint8)
    emu = EmuBackend(ppath, None)
    try:
        emu.prepare(13)
        exp = emu.error_model(rec, first_index=FIRST)
    finally:
        emu.close()
    return ppath, rec, exp


def ids_for(n):
    ids = [("r%d" % i) + "x" * (i % 9) for i in range(n)]
    ids[-1] = "last" + "y" * 700                                     # longer than the 480 bytes a fresh simulator's image holds per record
    return ids


def text_of(ids, exp):
    return b"".join(b"@" + ids[i].encode() + b" " + e[2].encode() + b" E%d\n" % e[3] + bytes(b"ACGTN"[c] for c in e[0]) + b"\n+\n" + e[1] + b"\n" for i, e in enumerate(exp[:len(ids)]))


@pytest.mark.parametrize("n", SIZES)
def test_records_at_the_ends_of_the_scan_tiles(records, n):
    ppath, rec, exp = records
    part = {k: v[:n] for k, v in rec.items()}
    ids = ids_for(n)
    want = text_of(ids, exp)
    gpu = GpuBackend(ppath, None)
    try:
        gpu.prepare(13)
        for call in (0, 1):
            got = gpu.error_model_fastq(part, [i.encode() for i in ids], first_index=FIRST)
            assert len(got) == len(want) and got == want, (n, call)
    finally:
        gpu.close()
