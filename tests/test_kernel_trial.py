"""What tests/test_kernel_trial_gpu.py rests on, without a GPU: tests/hostemu/kernel_trial.cpp compiles for the library's architecture with the project's warning
flags; the tables of tests/kernel_trial_cases.py hold the cases they are meant to hold; every checker has teeth -- the reference's own result passes it, and the
same result damaged the way a wrong kernel would damage it does not: each of these self-tests is a condition, it must fail its checker --; and the stable order
the sort checker expects is the one of the host loop (bam_sort_trial_sort of tests/hostemu/bam_sort_trial.cpp: bam_sort_pass_host pass by pass), the form that
tests/test_truth_bam_sorted.py holds."""
import copy
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
    the_depth_scan_table_holds()
    the_bedgraph_table_holds()
    the_pileup_table_holds()
    the_stats_table_holds()


def digits(values):
    return {len(str(int(v))) for v in values}


def the_depth_scan_table_holds():
    scan = K.cases("depthscan")
    assert [c.tiles for c in scan if c.kind == "random"] == K.DEPTHSCAN_TILES == [1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 3000]
    for kind in K.DEPTHSCAN_KINDS[1:]:
        assert [c.tiles for c in scan if c.kind == kind] == [1, 1025, 2049]
    assert all(len(c.blobs[0]) == c.tiles * K.DEPTH_TILE for c in scan)
    c = case_of("depthscan", lambda c: c.kind == "random" and c.tiles == 3)
    assert int(np.sum(c.blobs[0], dtype=np.uint64)) >> 32 > 1000                          # the sums wrap thousands of times
    c = case_of("depthscan", lambda c: c.kind == "spike" and c.tiles == 1025)
    assert c.blobs[0][K.DEPTH_TILE - 1] == c.blobs[0][K.DEPTH_TILE] == 1 << 31
    c = case_of("depthscan", lambda c: c.kind == "pairs" and c.tiles == 1025)                # the product's: every prefix a small depth, the last one 0
    depth = np.cumsum(c.blobs[0], dtype=np.uint64) & np.uint64(K.M32)
    assert depth[-1] == 0 and 0 < depth.max() < 1000 and np.count_nonzero(c.blobs[0] == K.M32) > 1000


def routes_of(c, pieces, lds):
    """the routes of a text case's waves; the pieces' first bytes fall where the table says"""
    return K.text_waves(pieces, c.lead, lds)


def the_text_routes_hold(cases, pieces_of, lds_of, capped, long_name):
    starts = set()
    for c in cases:
        waves = routes_of(c, pieces_of(c), lds_of(c))
        through = {w[2] for w in waves}
        at = c.lead
        for lines in pieces_of(c):
            if lines:
                starts.add(at % 16)
            at += sum(len(line) for line in lines)
        if c.name_len in (1, 150):
            assert through == {True}, c
        elif c.name_len == long_name:
            assert through == {False}, c
        elif getattr(c, "mixed", False):                                                     # both routes in one launch, neighbours in memory
            assert lds_of(c) == K.IMAGE_MAX and c.name_len == capped and len(pieces_of(c)) == 1
            assert [w[2] for w in waves[:2]] == [True, False] and waves[3][2] and waves[4][2], c
            assert waves[2][1] == K.IMAGE_MAX and waves[2][2] == (waves[2][0] == 0), c       # the wave that fits at skew 0 only
    exact = {routes_of(c, pieces_of(c), lds_of(c))[2][2] for c in cases if getattr(c, "mixed", False)}
    assert exact == {True, False}
    assert starts == set(range(16))                                                          # a piece's first byte on every alignment
    assert {c.lead for c in cases if c.name_len == 150} >= set(range(16))
    for name_len in {c.name_len for c in cases} - {150}:
        assert len({c.lead for c in cases if c.name_len == name_len}) >= 2


def the_bedgraph_table_holds():
    from truth_depth import bedgraph_from_depth
    bed = K.cases("bedgraph")
    assert {c.name_len for c in bed} == set(K.BED_NAMES) == {1, 150, 490, 600}
    assert 64 * (490 + 34) + 16 > K.IMAGE_MAX >= 64 * 511 + 15 and K.depth_lds_bytes(150) == 11904 and K.depth_lds_bytes(490) == K.depth_lds_bytes(600) == K.IMAGE_MAX
    the_text_routes_hold(bed, K.bed_pieces, lambda c: K.depth_lds_bytes(c.name_len), 490, 600)
    per_piece = [K.bedgraph_reference(c)[0].reshape(-1, 3) for c in bed]
    assert {int(n) for p in per_piece for n in p[:, 0]} >= set(K.BED_LINES) | {0}
    assert {hi - lo for c in bed for lo, hi in zip(c.bounds[:-1], c.bounds[1:])} >= {1, 7, 255, 256, 257}
    assert any(len(c.bounds) == 2 and c.len - c.base > 1000 for c in bed)                    # the whole window as one piece
    for c in bed:                                                                            # the loop's lines are bedgraph_from_depth's text; the word at len repeats
        assert c.bounds[0] == c.base and c.bounds[-1] == c.len and c.blobs[0][-1] == c.blobs[0][-2] and c.base % 32 == 0
        if c.base == 0:
            assert b"".join(line for _, line in c.lines) == bedgraph_from_depth([c.blobs[1].tobytes()], [c.blobs[0][:-1]])
    c = case_of("bedgraph", lambda c: "one run" in c.name)
    assert K.bedgraph_reference(c)[0].reshape(-1, 3)[:, 0].tolist() == [0, 0, 1] and len(c.lines) == 1
    c = case_of("bedgraph", lambda c: "its own run" in c.name)
    assert len(c.lines) == c.len
    c = case_of("bedgraph", lambda c: "a seam inside" in c.name)
    ends = {end for end, _ in c.lines}
    assert c.bounds[1] not in ends and c.bounds[2] in ends
    assert case_of("bedgraph", lambda c: "last run of depth 0" in c.name).lines[-1][1].endswith(b"\t340\t0\n")
    assert case_of("bedgraph", lambda c: "last run of non-zero" in c.name).lines[-1][1].endswith(b"\t340\t5\n")
    c = case_of("bedgraph", lambda c: "every width" in c.name)
    assert set(c.blobs[0].tolist()) == set(K.BED_VALUES) and digits(K.BED_VALUES) == set(range(1, 11)) and {0, 9, 10, 999_999_999, 10 ** 9, K.M32} <= set(K.BED_VALUES)
    for power in (7, 8, 9):                                                                  # start and end gain a digit inside the window
        c = case_of("bedgraph", lambda c: f"10^{power}" in c.name)
        fields = [line.split(b"\t") for _, line in c.lines]
        assert {len(f[1]) for f in fields} == {len(f[2]) for f in fields} == {power, power + 1}
    c = case_of("bedgraph", lambda c: c.len == K.M32)
    assert c.lines[-1][1].split(b"\t")[2] == b"4294967295" and max(len(line) for _, line in c.lines) == 150 + 34


def the_pileup_table_holds():
    from truth_pileup import pileup_text
    pile = K.cases("pileup")
    assert {c.name_len for c in pile} == set(K.PILEUP_NAMES) == {1, 150, 450, 600}
    for sets in (1, 2):
        assert 64 * (450 + 14 + 88 * sets) + 16 > K.IMAGE_MAX >= 64 * (450 + 37) + 15 and K.pileup_lds_bytes(450, sets) == K.IMAGE_MAX > K.pileup_lds_bytes(150, sets)
        assert {c.sets for c in pile if getattr(c, "mixed", False)} == {1, 2}
    the_text_routes_hold(pile, K.pileup_pieces, lambda c: K.pileup_lds_bytes(c.name_len, c.sets), 450, 600)
    assert {c.sets for c in pile} == {1, 2} and {c.all for c in pile} == {False, True} and {c.rows_shift for c in pile} == {0, 1}
    for c in pile:                                                                           # the planes are a run's; the loop's lines are pileup_text's
        planes = c.blobs[0].astype(np.int64)
        assert np.all(planes[:, 1 + c.ref, np.arange(c.n)] == 0) and c.base % 32 == 0
        if not getattr(c, "widest", False):
            assert np.all(planes[:, 0] >= planes[:, 1:6].sum(axis=1))
        if c.base == 0:
            assert b"".join(c.lines) == pileup_text([c.blobs[2].tobytes()], [bytes(K.LETTERS[r] for r in c.ref)], [c.v], c.all)
    for sets in (1, 2):                                                                      # the predicate's classes
        sites, every = (case_of("pileup", lambda c: getattr(c, "predicate", False) and c.sets == sets and c.all == a) for a in (False, True))
        v, ref = sites.v.astype(np.int64), sites.ref
        assert np.array_equal(v, every.v) and not np.any(every.keep & ~v.reshape(len(v), -1).any(axis=1)) and np.all(sites.keep <= every.keep)
        assert np.count_nonzero(~every.keep) >= 4 and np.count_nonzero(every.keep & ~sites.keep) >= 4        # all zeros; the depth and the own count only
        singles = {(int(r), int(np.flatnonzero(row[0, 1:])[0]) + 1) for row, r in zip(v, ref) if row[0, 1:].sum() == 1 and not row[1:].any()}
        assert singles == {(r, k) for r in range(4) for k in range(1, 8)}
        if sets == 2:                                                                        # the only non-zero call, del or ins in the reverse set
            other = v.copy()
            other[:, :, 0] = 0
            other[np.arange(len(v)), :, 1 + ref] = 0
            only_reverse = ~other[:, 0].any(axis=1) & other[:, 1].any(axis=1)
            assert {int(np.flatnonzero(o[1])[0]) for o in other[only_reverse]} >= {5, 6, 7} and np.all(sites.keep[only_reverse])
            assert np.any(only_reverse & v[:, 0, 0].astype(bool)) and np.any(only_reverse & ~v[:, 0].any(axis=1))
    for sets in (1, 2):
        c = case_of("pileup", lambda c: getattr(c, "widths", False) and c.sets == sets)
        for col in range(8):
            assert digits(c.v[:, sets - 1, col]) == set(range(1, 11)), col
        assert np.any((c.v[:, 0, 0] == K.M32) & (c.v[:, 0, 3] == K.M32) & (c.v[:, 0, 1:].sum(axis=1) == K.M32))       # the depth with nothing else: the own count
        c = case_of("pileup", lambda c: getattr(c, "widest", False) and c.sets == sets)
        assert max(len(line) for line in c.lines) == 150 + 14 + 88 * sets                    # the line the image is sized for
        assert {len(line.split(b"\t")[1]) for line in c.lines} == {9, 10}
    c = case_of("pileup", lambda c: getattr(c, "kept_per_piece", False))
    assert [int(p[0]) for p in K.pileup_reference(c)[3::5]] == K.PILEUP_KEPT == [0, 1, 63, 64, 65, 129]
    c = case_of("pileup", lambda c: getattr(c, "sparse", False))
    assert c.n == 100_000 and 50 < c.keep.sum() < 200
    assert any(c.keep.all() and c.n >= 1000 for c in pile)
    for power in (7, 8, 9):
        assert any({len(line.split(b"\t")[1]) for line in c.lines if line} == {power, power + 1} for c in pile)


def the_stats_table_holds():
    stats = K.cases("stats")
    rows, shared = [c for c in stats if c.kind == "rows"], [c for c in stats if c.kind == "shared"]
    assert {c.n_pairs for c in rows} >= set(K.STATS_PAIRS) and {c.slab for c in rows} >= set(K.STATS_SLABS) and {c.skew for c in rows} == {0, 1}
    for slab in K.STATS_SLABS:                                                               # the workgroups against the units and their slabs
        some = [c for c in rows if c.name.startswith("stats rows groups ") and c.slab == slab]
        assert {c.units for c in some} == {7} and {c.slabs for c in some} == {-(-257 // slab)}
        assert {c.groups for c in some} == {1, 2, 6, 7, 8, 22, 7 * some[0].slabs + 3}
        assert {c.skew for c in some} == {0, 1}
    assert {(c.lengths, c.chunk) for c in rows if c.name.startswith("stats rows lengths ")} == {(l, k) for l in K.STATS_LENGTHS for k in K.STATS_CHUNKS}
    assert {(c.Q, c.skew) for c in rows if c.chunk == 0 and c.groups == 0 and c.lengths == (150, 151)} >= {(q, s) for q in K.STATS_Q for s in (0, 1)}
    assert {c.phred for c in rows if c.below} == {33, 64}
    for c in rows:
        if c.below:                                                                          # characters below the offset, inside reads
            qual = c.blobs[1].view(np.uint8).reshape(c.row_words, c.pitch, 4)
            assert np.any((qual[0, :2 * c.n_pairs, 0] < c.phred) & (c.blobs[2] > 0))
        want = K.stats_reference(c)[1][K.MARKER:-K.MARKER].view(np.uint64)
        quality, call, bad, words = K.stats_layout(*c.lengths, c.Q)
        assert want[:bad].sum() == 0 and want[bad + 1] == 0 and (c.hot or want[bad] > 0 or max(c.lengths) < 30)
        assert want[quality:call].sum() + want[call:].sum() + want[bad] == 2 * np.minimum(np.minimum(c.blobs[2][:c.n_pairs], c.lengths[0]), 4 * c.row_words).sum(dtype=np.int64) + \
            2 * np.minimum(np.minimum(c.blobs[2][c.n_pairs:], c.lengths[1]), 4 * c.row_words).sum(dtype=np.int64)
    c = case_of("stats", lambda c: c.kind == "rows" and getattr(c, "lens", False))
    assert 0 in c.blobs[2] and np.any(c.blobs[2][:c.n_pairs] > 30) and np.any((c.blobs[2][c.n_pairs:] > 21) & (c.blobs[2][c.n_pairs:] <= 30))
    c = case_of("stats", lambda c: c.kind == "rows" and getattr(c, "short_rows", False))
    assert np.any(c.blobs[2] > 4 * c.row_words) and 4 * c.row_words < min(c.lengths)
    hot = [c for c in rows if c.hot]
    assert {c.skew for c in hot} == {0, 1} and all(2 * c.n_pairs == 5000 and max(c.lengths) == 301 for c in hot)
    for c in hot:
        want = K.stats_reference(c)[1][K.MARKER:-K.MARKER].view(np.uint64)
        assert want.max() == 2500 and np.count_nonzero(want) == 4 * 301
    c = case_of("stats", lambda c: c.kind == "shared" and getattr(c, "classes", False))
    image = c.image_words
    seen = set()
    for r in c.rounds.reshape(-1, 4, 64, 4):                                                 # per round the four waves' lanes
        for w in r:
            index, on = w[:, 0], w[:, 1] != 0
            seen.add("nobody" if not on.any() else "lane 0" if on.tolist() == [True] + [False] * 63 else "lane 63" if on.tolist() == [False] * 63 + [True] else
                     ("one index" if len(set(index)) == 1 else "64 indices" if len(set(index)) == 64 else "two interleaved" if np.all(index[2:] == index[:-2]) and index[0] != index[1]
                      else "several") + (" across the image's end" if index.min() < image <= index.max() else " in memory" if index.min() >= image else "") if on.all() else "some")
    assert seen >= {"nobody", "lane 0", "lane 63", "one index", "one index in memory", "64 indices", "64 indices across the image's end", "two interleaved",
                    "two interleaved across the image's end", "some"}, seen
    assert {(c.image_words == 0, c.image_words == c.words) for c in shared} == {(False, False), (True, False), (False, True)} and {c.groups for c in shared} == {1, 3}
    hot = [c for c in shared if getattr(c, "hot", False)]
    assert len(hot) == 2 and all(len(c.rounds) == 1000 and len(np.unique(c.rounds[:, :, 0])) == 1 for c in hot)
    assert {int(c.rounds[0, 0, 0]) < c.image_words for c in hot} == {True, False}


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


def body(blob, dtype):
    """the array of a guarded blob, a view into it"""
    return blob[K.MARKER:len(blob) - K.MARKER].view(dtype)


def test_depthscan_checker_a_prefix_short_by_one_tiles_sum():
    c = case_of("depthscan", lambda c: c.kind == "random" and c.tiles == 3)
    want = K.depthscan_reference(c)
    out = want[0].copy()
    body(out, np.uint32)[2 * K.DEPTH_TILE:] -= np.sum(c.blobs[0][K.DEPTH_TILE:2 * K.DEPTH_TILE], dtype=np.uint32)      # from tile 2 on, tile 1's sum is missing
    assert "the prefix sums: 4096 wrong, the first at 8192" in reported("depthscan", c, [out, want[1]])
    sums = want[1].copy()
    body(sums, np.uint32)[2] = body(sums, np.uint32)[1]
    assert "tile_sums" in reported("depthscan", c, [want[0], sums])
    for blob, at, where in ((0, K.MARKER - 1, "in front"), (0, -K.MARKER, "behind"), (1, -K.MARKER + 15, "behind")):      # (tile_sums: inside the library's 16 spare bytes)
        got = [w.copy() for w in want]
        got[blob][at] ^= 1
        assert f"the guard {where}" in reported("depthscan", c, got)


def with_text(c, text):
    """the text blob of a case whose kernel wrote `text` into the destination: what it left untouched are guard bytes"""
    return K._guarded(np.frombuffer(text + bytes([K.GUARD8]) * (c.par[3 if c.name.startswith("bedgraph") else 6] - len(text)), np.uint8))


def test_bedgraph_checker_a_run_end_dropped_a_line_one_byte_short_a_guard_byte():
    c = case_of("bedgraph", lambda c: "a seam inside" in c.name)
    numbers, text = K.bedgraph_reference(c)
    # the run end at 100 dropped in piece 0: its run and the next become one line with the second run's depth
    name, lines = c.blobs[1].tobytes(), [line for _, line in c.lines]
    merged = [name + b"\t0\t200\t5\n"] + lines[2:]
    damaged = numbers.copy()
    damaged[0:3] = [0, 0, 0]                                                                  # piece (0, 150]: no line, the carry stays
    damaged[3:5] = [1, len(merged[0])]
    said = reported("bedgraph", c, [damaged, with_text(c, b"".join(merged))])
    assert "lines, bytes and carry" in said and "the text" in said
    # a line written one byte short, the next one shifted
    whole = b"".join(lines)
    short = whole[:len(lines[0]) - 2] + whole[len(lines[0]) - 1:]
    assert "the text: " in reported("bedgraph", c, [numbers, with_text(c, short)])
    for at, where in ((K.MARKER - 1, "in front"), (-K.MARKER, "behind")):
        got = text.copy()
        got[at] = ord("\n")
        assert f"the text: the guard {where}" in reported("bedgraph", c, [numbers, got])


def test_pileup_checker_a_kept_row_missing_under_sites():
    c = case_of("pileup", lambda c: getattr(c, "kept_per_piece", False))
    assert not c.all
    gone = int(np.flatnonzero(c.keep)[70])
    less = copy.copy(c)
    less.keep, less.lines = c.keep.copy(), list(c.lines)
    less.keep[gone], less.lines[gone] = False, b""
    damaged = K.pileup_reference(less)
    damaged[-1] = with_text(c, b"".join(less.lines))
    said = reported("pileup", c, damaged)
    assert "flags" in said and "line_pos" in said and "the text" in said
    want = K.pileup_reference(c)
    for blob, name in ((0, "the rows"), (1, "piece 0: flags"), (len(want) - 1, "the text")):
        for at, where in ((K.MARKER - 1, "in front"), (-K.MARKER, "behind")):
            got = [w.copy() for w in want]
            got[blob][at] ^= 0x40
            assert f"{name}: the guard {where}" in reported("pileup", c, got)
    got = [w.copy() for w in want]
    at = int(np.flatnonzero(c.v[:, 0, 0] != c.v[np.arange(c.n), 0, 1 + c.ref])[0])
    row = body(got[0], np.uint32).reshape(c.n, c.sets, 8)[at, 0]
    row[1 + c.ref[at]] = row[0]                              # the own count not formed: the depth stands in its place
    assert "the rows" in reported("pileup", c, got)


def test_stats_checker_a_count_in_the_neighbouring_cycle_and_bad_off_by_one():
    c = case_of("stats", lambda c: c.kind == "rows" and c.n_pairs == 65)
    layout, counts = K.stats_reference(c)
    quality, call, bad, words = (int(x) for x in layout)
    got = counts.copy()
    at = quality + int(np.flatnonzero(body(counts, np.uint64)[quality:call])[5])
    body(got, np.uint64)[at] -= 1
    body(got, np.uint64)[at + c.Q] += 1                                                      # the same quality one cycle later
    assert "base_quality: 2 counters wrong" in reported("stats", c, [layout, got])
    got = counts.copy()
    body(got, np.uint64)[bad] += 1
    assert "bad: 1 counters wrong" in reported("stats", c, [layout, got])
    got = counts.copy()
    body(got, np.uint64)[3] += 1
    assert "the tables that stay zero" in reported("stats", c, [layout, got])
    got = counts.copy()
    got[-K.MARKER] ^= 1
    assert "the guard behind" in reported("stats", c, [layout, got])
    c = case_of("stats", lambda c: c.kind == "shared" and getattr(c, "classes", False))
    got = K.stats_reference(c)[0].copy()
    body(got, np.uint64)[5] -= 1                                                             # 63 of a wave's 64 equal indices counted
    assert "the counts" in reported("stats", c, [got])


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
