"""The address arithmetic of the wave kernels' per-lane state (reseq_amd/csrc/rsq_reads.h) without a GPU: WaveReadOut forms one 32-bit byte offset from word
and row against wave-uniform array bases, and takes the 64-bit form when the host finds the arrays 4 GB or longer (RawLayout::wide, read_out_is_wide);
WaveFragmentSrc keeps element indices of the lane's first template word and first error entry, 32 bits and a few high bits (2^40 words, 2^48 entries: beyond any device).  tests/hostemu/read_out_trial.cpp
(built here with g++) forms these addresses beside the pointer forms they replace -- WordColumn::at through RawLayout, FragmentSrc's words + word_off and
sys_ -- from made-up bases, so nothing is allocated at the sizes asked for; and it replays iterations through ReadOut and WaveReadOut into real small arrays."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def trial(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("read_out_trial") / "libread_out_trial.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-shared", "-o", out,
                    os.path.join(HERE, "hostemu", "read_out_trial.cpp")], check=True)
    L = C.CDLL(out)
    L.read_out_trial_wide.argtypes = [C.c_uint64, C.c_uint64]
    L.read_out_trial_word.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    L.read_out_trial_word.restype = None
    L.read_out_trial_source.restype = None
    L.read_out_trial_source.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    L.read_out_trial_replay.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    return L


READ_WORDS = 38           # 2 x 150 bp reads: 150 bases in rows of 16 bytes -> 38 words (the ops need fewer)
PITCHES = [1, 63, 64, 65, 1 << 26]


def word_offsets(trial, words, pitch, row, w):
    out = (C.c_uint64 * 2)()
    trial.read_out_trial_word(words, pitch, row, w, out)
    return out[0], out[1]


@pytest.mark.parametrize("pitch", PITCHES)
def test_word_addresses_equal_the_columns(trial, pitch):
    """first and last word of rows at both ends of the pitch: the cursor's address is WordColumn::at's, and is what the layout says"""
    for row in sorted({0, 1, pitch // 2, pitch - 1}):
        for w in (0, 1, READ_WORDS - 1):
            got, want = word_offsets(trial, READ_WORDS, pitch, row, w)
            assert got == want == (w * pitch + row) * 4, (pitch, row, w)


def test_wide_is_decided_where_the_last_byte_passes_4_gb(trial):
    """the 32-bit offset is exact while words * pitch * 4 <= 2^32 (the largest offset is 4 bytes below that product)"""
    edge = (1 << 32) // (4 * READ_WORDS)                    # the largest pitch whose arrays stay within 4 GB
    assert READ_WORDS * edge * 4 <= 1 << 32 < READ_WORDS * (edge + 1) * 4
    assert trial.read_out_trial_wide(READ_WORDS, edge) == 0
    assert trial.read_out_trial_wide(READ_WORDS, edge + 1) == 1
    assert trial.read_out_trial_wide(1, 1 << 30) == 0 and trial.read_out_trial_wide(1, (1 << 30) + 1) == 1
    assert trial.read_out_trial_wide(READ_WORDS, 1 << 26) == 1        # 9.5 GB: the largest of PITCHES takes the 64-bit form, the others the 32-bit offset
    assert trial.read_out_trial_wide(READ_WORDS, 20_000_000) == 0     # the flagship workload's 10 M pairs: 3 GB


@pytest.mark.parametrize("delta", [-64, 0, 64, 1 << 20])
def test_rows_on_both_sides_of_4_gb(trial, delta):
    """arrays just within 4 GB take the 32-bit offset up to their last word; just beyond, the 64-bit form: both give the column's address, for the rows and words
    around the place where w * pitch * 4 crosses 2^32"""
    edge = ((1 << 32) // (4 * READ_WORDS)) & ~63            # pitches are multiples of 64
    pitch = edge + delta
    for w in (0, READ_WORDS - 2, READ_WORDS - 1):
        r0 = (1 << 30) - w * pitch                          # the first row of word w at or beyond 4 GB, if the word row reaches that far
        rows = {0, 1, 63, pitch // 3, pitch - 1} | {r for r in (r0 - 1, r0, r0 + 1) if 0 <= r < pitch}
        for row in sorted(rows):
            got, want = word_offsets(trial, READ_WORDS, pitch, row, w)
            assert got == want == (w * pitch + row) * 4, (pitch, row, w)
    # the last word row's last read: the largest address of the arrays
    got, want = word_offsets(trial, READ_WORDS, pitch, pitch - 1, READ_WORDS - 1)
    assert got == want == (READ_WORDS * pitch - 1) * 4
    assert (got >= 1 << 32) == (delta > 0)


def source_indices(trial, word_off, hap_off, sys_off, reverse, first, template_at, k):
    out = (C.c_uint64 * 6)()
    trial.read_out_trial_source(word_off, hap_off, sys_off, reverse, first, (1 << 64) - 1 if template_at is None else template_at, k, out)
    return 0, list(out)


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("sys_off", [0, 12345, (1 << 31) - 160, (1 << 31) - 2, 1 << 31, (1 << 32) - 3, 1 << 32, (3 << 32) + 7])
def test_error_track_positions(trial, reverse, sys_off):
    """a mate whose first error entry lies on either side of 2^31 and of 2^32 entries (a human-sized track has 3.1 x 2^30; bytes are twice that), read over 300
    template bases: every group of four is the entry FragmentSrc's pointer reaches, in the strand's own track"""
    for k in list(range(0, 12)) + [148, 149, 150, 299]:
        rc, o = source_indices(trial, 1000, 0, sys_off, reverse, 5000, None, k)
        assert rc == 0
        assert o[2] == o[3] == sys_off + (k & ~3), (sys_off, k)
        assert o[4] == o[5]


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("word_off,hap_off", [(0, 0), (97_000_000, 0), ((1 << 32) - 2, 0), (1 << 32, 0), (5, 3 * 97_000_000), ((1 << 31) + 9, (1 << 32) + (1 << 31))])
def test_template_words(trial, reverse, word_off, hap_off):
    """the reference's word of every template base, forwards and backwards over word boundaries, with the sequence's first word on either side of 2^32 words and in
    an allele's copy of the reference"""
    first = 3 * 32 + 5 if not reverse else 11 * 32 + 2
    for k in (0, 1, 2, 3, 26, 27, 58, 59, 60, 149, 150):
        rc, o = source_indices(trial, word_off, hap_off, 77, reverse, first, None, k)
        assert rc == 0
        pos = first - 1 - k if reverse else first + k
        assert o[0] == o[1] == hap_off + word_off + (pos >> 5), (word_off, hap_off, k)
        assert o[4] == o[5] == (reverse << 1) | (reverse << 2)


@pytest.mark.parametrize("template_at", [0, 6 * 123_456, (1 << 32) - 6, 1 << 32, (7 << 32) + 12])
def test_converted_templates(trial, template_at):
    """--methylation: the converted template is read forwards from its own word 0 whichever strand the mate reads; its errors stay the strand's"""
    for reverse in (0, 1):
        for k in (0, 31, 32, 150, 191):
            rc, o = source_indices(trial, 1000, 0, (1 << 31) + 5, reverse, 7777, template_at, k)
            assert rc == 0
            assert o[0] == o[1] == template_at + (k >> 5)
            assert o[2] == o[3]
            assert o[4] == o[5] == 1 | (reverse << 1)


def replay_kinds(n_template, n_tail, seed):
    """iterations of a read: bases with some deletions and insertions, then a tail"""
    rng = np.random.default_rng(seed)
    body = rng.choice(np.array([0, 0, 0, 0, 0, 1, 2], np.uint8), size=n_template)
    return np.concatenate([body, np.full(n_tail, 3, np.uint8)])


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("pitch,row", [(1, 0), (63, 62), (64, 0), (65, 64), (192, 100)])
def test_replay_equals_read_out(trial, pitch, row, wide):
    """the words ReadOut stores and the ones WaveReadOut stores, untouched words included: reads whose bases and ops end on and off word boundaries, without an
    iteration, without an op, with a tail"""
    cases = [(0, 0), (0, 5), (1, 0), (3, 0), (4, 0), (15, 0), (16, 0), (17, 0), (31, 1), (32, 0), (33, 7), (150, 0), (163, 12), (160, 16)]
    for i, (n_template, n_tail) in enumerate(cases):
        kinds = replay_kinds(n_template, n_tail, 100 + i)
        rc = trial.read_out_trial_replay(kinds.ctypes.data, len(kinds), pitch, row, wide)
        assert rc == 0, (n_template, n_tail, pitch, row, wide, rc)
