"""What tests/test_kernel_trial_gpu.py rests on, without a GPU: tests/hostemu/kernel_trial.cpp compiles for the library's architecture with the project's warning
flags; the tables of tests/kernel_trial_cases.py hold the cases they are meant to hold; every checker has teeth -- the reference's own result passes it, and the
same result damaged the way a wrong kernel would damage it does not: each of these self-tests is a condition, it must fail its checker --; and the stable order
the sort checker expects is the one of the host loop (bam_sort_trial_sort of tests/hostemu/bam_sort_trial.cpp: bam_sort_pass_host pass by pass), the form that
tests/test_truth_bam_sorted.py holds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kernel_trial_cases as K
from portable_table import find_hipcc


def test_the_trial_compiles_for_the_librarys_architecture(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc to compile the program with")
    assert os.path.getsize(K.build(tmp_path, hipcc)) > 0


def case_of(family, wanted):
    return next(c for c in K.cases(family) if wanted(c))


def reported(family, case, damaged):
    """the reference's own result passes; the damaged one is reported"""
    assert K.check(family, case, K.reference(family, case)) == []
    lines = K.check(family, case, damaged)
    assert lines, (family, case)
    return " ".join(lines)


# ------------------------------------------------------------------------------------------------------------------------- the tables
def test_the_tables_hold_the_cases_they_are_meant_to():
    scan = K.cases("scan")
    assert {c.n for c in scan} == set(K.SCAN_N) and {c.init for c in scan} == set(K.SCAN_INIT) and {c.arrays for c in scan} == {1, 2}
    assert {(c.par[4], c.par[5]) for c in scan if c.n in (4095, 4096, 4097)} >= {(i, o) for i in range(4) for o in range(2)}
    assert any(c.n > 1024 * 4096 and int(K.scan_reference(c)[0][-3]) >> 52 for c in scan)           # sums of 2^54
    sort = K.cases("sort")
    assert {c.n for c in sort} == set(K.SORT_N) and {c.plan for c in sort} == set(K.SORT_PLANS)
    for plan, passes in K.SORT_PLANS.items():                        # the passes the plans were chosen for
        assert K.sort_plan(*plan)[2] == passes
    assert K.sort_plan(3, 5000)[0] % 8 != 0 and K.sort_plan(3, 5000)[0] // 8 == 1        # the seam between position and sequence inside digit 1
    for c in sort:                                                   # the cuts: below all keys, a key, a key that occurs several times, above the mapped keys, above all
        keys, cuts = c.blobs[0], [int(cut) for cut in c.blobs[2]]
        assert cuts[0] == 0 and cuts[1] == keys.min() and cuts[4] == c.unmapped and cuts[5] == K.CUT_ALL and (c.n < 4 or np.count_nonzero(keys == np.uint64(cuts[2])) > 1)
        assert cuts[3] <= c.unmapped and not np.any((keys >= np.uint64(cuts[3])) & (keys < np.uint64(c.unmapped)))
    assert any(np.any(c.blobs[0] == np.uint64(c.unmapped)) and np.any(c.blobs[0] < np.uint64(c.unmapped)) for c in sort)        # unmapped keys among the mapped
    gather = K.cases("gather")
    assert {c.n for c in gather} >= {1, 15, 16, 17} and {int(s) for c in gather for s in c.entries["size"]} >= set(K.GATHER_SIZES)
    everything = {(s, d) for s in range(16) for d in range(16)}
    assert K.gather_pairs(case_of("gather", lambda c: "pairs" in c.name and c.n_final == c.n)) == everything
    assert K.gather_pairs(case_of("gather", lambda c: "pairs" in c.name and c.n_final == 0)) == everything
    assert {"none" if c.n_final == 0 else "all" if c.n_final == c.n else "some" for c in gather} == {"none", "all", "some"}
    index = K.cases("index")
    assert {c.n for c in index} >= set(K.INDEX_N) and {span for c in index for _, _, span in c.records} == set(K.INDEX_SPANS) | {2}
    assert all({seq for seq, _, _ in c.records} <= {0, 2} for c in index)
    bins = K.cases("bins")
    assert {c.n_keys for c in bins} == set(K.BINS_KEYS) and {c.n for c in bins} >= set(K.BINS_N) and {c.n_bins // c.n_keys for c in bins} == {1, 2}
    assert sum(c.frags for c in bins) == 1
    fasta = K.cases("fasta")
    assert {len(c.blobs[0]) for c in fasta} >= set(K.FASTA_LENGTHS) and {c.shift for c in fasta} >= set(K.FASTA_SHIFTS)
    assert {0, 1} == {int(K.fasta_reference(c)[2][2]) for c in fasta}


# ------------------------------------------------------------------------------------------------------------------------- teeth
def test_scan_checker_one_offset_behind_a_2_32_crossing_short_by_2_32():
    c = case_of("scan", lambda c: c.name.startswith("scan ones n=4097"))
    want = K.scan_reference(c)
    out = want[1].copy()
    behind = np.flatnonzero((out[2:-2] >> np.uint64(32)) > (out[2] >> np.uint64(32)))[0] + 2 + 7      # a few offsets behind the first crossing
    assert out[behind] >= 1 << 32
    out[behind] -= np.uint64(1 << 32)
    assert "out[1]" in reported("scan", c, [want[0], out] + want[2:])


def test_scan_checker_a_guard_word_or_the_total_or_the_longest():
    c = case_of("scan", lambda c: c.n == 4096 and c.arrays == 2 and c.par[5] == 1)
    want = K.scan_reference(c)
    for blob, at in ((0, 1), (0, -1), (2, 1), (3, 0)):
        got = [w.copy() for w in want]
        got[blob][at] += 1
        reported("scan", c, got)


def test_sort_checker_two_neighbouring_equal_key_records_swapped():
    c = case_of("sort", lambda c: "alternating" in c.name and c.n > 1024)
    keys, order, words, plan = K.sort_reference(c)
    at = len(order) // 3
    assert keys[at] == keys[at + 1] and order[at] < order[at + 1]
    order = order.copy()
    order[[at, at + 1]] = order[[at + 1, at]]
    assert "order" in reported("sort", c, [keys, order, words, plan])         # the keys are still sorted: only the stable order tells
    words = words.copy()
    words[6 * 2] += 1                                                         # a cut equal to a key: one record of that key taken for final
    assert "cut words" in reported("sort", c, [keys, K.sort_reference(c)[1], words, plan])


def test_gather_checker_one_byte_of_one_record_and_one_guard_byte():
    c = case_of("gather", lambda c: "pairs" in c.name and 0 < c.n_final < c.n)
    want = K.gather_reference(c)
    for blob, name in ((0, "out"), (1, "held")):
        got = [w.copy() for w in want]
        got[blob][K.MARKER + len(got[blob]) // 2] ^= 0x20                     # one byte of one record
        assert f"{name}: the records" in reported("gather", c, got)
        for at, where in ((K.MARKER - 1, "in front"), (-K.MARKER, "behind")):
            got = [w.copy() for w in want]
            got[blob][at] ^= 1                                                # one guard byte
            assert f"{name}: the marker {where}" in reported("gather", c, got)
    got = [w.copy() for w in want]
    got[2]["off"][3] += 1
    assert "held directory" in reported("gather", c, got)


def test_index_checker_one_windows_offset_not_the_minimum_and_one_run_missing():
    c = case_of("index", lambda c: "short record behind" in c.name)
    flags, runs, windows = K.index_reference(c)
    # window 1 of sequence 0 is overlapped by the first record (100, 40000) and by later ones: the offset of a later one is not the minimum
    later = K.STREAM_AT + int(c.at[[r[:2] for r in c.records].index((0, 16384))])
    assert int(windows[1]) == K.STREAM_AT + int(c.at[0]) < later
    damaged = windows.copy()
    damaged[1] = later
    assert "windows" in reported("index", c, [flags, runs, damaged])
    damaged = flags.copy()
    damaged[np.flatnonzero(flags)[2]] = 0
    assert "flags" in reported("index", c, [damaged, runs, windows])
    assert "runs" in reported("index", c, [flags, np.delete(runs, 2), windows])


def test_bins_checker_one_item_placed_in_a_neighbouring_bin():
    c = case_of("bins", lambda c: c.frags)
    small, cursors, perm, frags = K.bins_reference(c)
    first = int(cursors[5])                                                   # the first item of bin 5 and the last of bin 4 change places
    assert c.blobs[0][perm[first]] == 5 and c.blobs[0][perm[first - 1]] == 4
    damaged = perm.copy()
    damaged[[first - 1, first]] = damaged[[first, first - 1]]
    assert "outside their bins" in reported("bins", c, [small, cursors, damaged, frags])
    # the order inside a bin is free -- with the fragments in the same order
    free = perm.copy()
    free[[first, first + 1]] = free[[first + 1, first]]
    assert c.blobs[0][free[first + 1]] == 5
    assert K.check("bins", c, [small, cursors, free, c.blobs[1].reshape(-1, K.FRAGMENT_BYTES)[free[:-1]]]) == []
    assert "fragments" in reported("bins", c, [small, cursors, free, frags])
    twice = perm.copy()
    twice[7] = twice[8]
    assert "no permutation" in reported("bins", c, [small, cursors, twice, frags])
    small = small.copy()
    small[-2] += 1                                                            # the total of the chunks
    assert "chunk_ptr" in reported("bins", c, [small, cursors, perm, frags])


def test_fasta_checker_one_record_start_dropped():
    c = case_of("fasta", lambda c: c.name.startswith("fasta random 7"))
    counts, at, summary = K.fasta_reference(c)
    assert len(at) > 12
    assert "starts" in reported("fasta", c, [counts, np.delete(at, 5), summary])
    damaged = counts.copy()
    damaged[0] -= 1
    assert "counts" in reported("fasta", c, [damaged, at, summary])
    assert "summary" in reported("fasta", c, [counts, at, summary ^ np.array([0, 0, 1, 0], np.uint32)])


# ------------------------------------------------------------------------------------------------------------------------- the host loop
def test_the_expected_order_is_the_host_loops(tmp_path):
    out = str(tmp_path / "libbam_sort_trial.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-shared", "-o", out,
                    os.path.join(K.HERE, "hostemu", "bam_sort_trial.cpp")], check=True)
    L = C.CDLL(out)
    L.bam_sort_trial_sort.restype = C.c_uint32
    L.bam_sort_trial_sort.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    for c in K.cases("sort"):
        keys = c.blobs[0]
        order, sorted_keys, plan = np.zeros(c.n, np.uint32), np.zeros(c.n, np.uint64), np.zeros(2, np.uint32)
        passes = L.bam_sort_trial_sort(keys.ctypes.data, c.n, c.plan[0], c.plan[1], order.ctypes.data, sorted_keys.ctypes.data, plan.ctypes.data)
        want = K.sort_reference(c)
        assert [int(plan[0]), int(plan[1]), passes] == want[3].tolist(), c
        assert np.array_equal(sorted_keys, want[0]) and np.array_equal(order, want[1]), c
