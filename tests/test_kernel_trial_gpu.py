"""The library's cooperative kernels alone on the device, on inputs no simulation makes: tests/hostemu/kernel_trial.cpp, compiled by hipcc for the library's
architecture, runs one family's table of tests/kernel_trial_cases.py per test as a fresh child process under a time limit of its own; its results must be the
plain references' of that module, exactly -- integers and bytes, no tolerance (tests/test_kernel_trial.py shows the checkers' teeth).

  scan     k_scan_tile_sums / k_scan_tiles / k_scan_apply through scan_launch: sums past 2^32 and 2^54, an init above 2^32, 1025 tiles, unaligned in and out
  sort     k_bam_sort_hist / k_bam_sort_scatter through bam_sort_passes, k_bam_cut: two to seven passes, the ballot ranking on crafted digits, six cuts a case
  gather   k_bam_sorted_sizes / k_bam_gather: every (source, destination) alignment, sizes around the head and tail and past 256 bytes, guard bytes
  index    k_bam_index_flags / k_bam_index_runs: records over several 16 kb windows, short ones behind long ones
  bins     bin_count_key / k_bins_plan / k_bin_scatter: several scatter workgroups, more than 1024 bins, both sides of kBinKeysLds
  fasta    tile_starts in k_fasta_count / k_fasta_starts, k_fasta_lead: a start on either side of every seam, texts that end there, unaligned text
  depthscan  k_depth_tile_sums / k_depth_tiles / k_depth_apply: dense values whose sums wrap, spikes on the tile seams, one to three tiles a thread of k_depth_tiles
  bedgraph   k_depth_ends / k_depth_run_ends / k_depth_line_sizes / k_depth_text piece by piece: numbers of one to ten digits, positions up to 4294967295, every
             alignment, names on both sides of the image's cap and a launch whose waves take both routes
  pileup     k_pileup_rows / k_pileup_lines / k_pileup_place / k_pileup_text: the predicate over one and two strand sets, counts of every width, the unaligned
             rows, 0 to 129 kept lines a piece, both routes in one launch
  stats      k_stats_rows in both forms over units, slabs and workgroups of every relation, Q up to 250 with the library's chunk; StatsMatesAdd's shared adds

A child that ends by a signal, by abort, at its limit or with a HIP error in its output stops the module: the family tests after it fail at once and start nothing
on the device."""
import subprocess
import time

import pytest

import kernel_trial_cases as K
from portable_table import find_hipcc

pytestmark = pytest.mark.gpu

STOPPED = []                                 # why no further child is started


@pytest.fixture(scope="module")
def trial(tmp_path_factory):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc to compile the program with")
    return K.build(tmp_path_factory.mktemp("kernel_trial"), hipcc)


def family_holds(trial, tmp_path, family):
    assert not STOPPED, f"not started: {STOPPED[0]}"
    cases = K.cases(family)
    began = time.perf_counter()
    try:
        got, done = K.run(trial, family, tmp_path)
    except subprocess.TimeoutExpired as e:
        STOPPED.append(f"the {family} child was still running after {K.CHILD_LIMIT} s")
        raise AssertionError(STOPPED[0]) from e
    text = done.stdout + done.stderr
    if done.returncode < 0 or done.returncode in (134, 139) or "HIP error" in text:
        STOPPED.append(f"the {family} child ended with status {done.returncode}: {text[-500:]}")
    assert done.returncode == 0 and f"{family}: {len(cases)} cases" in done.stdout, (done.returncode, text[-2000:])
    print(f"{family}: {len(cases)} cases, the child took {time.perf_counter() - began:.2f} s")
    bad = [(c.name, lines) for c, blobs in zip(cases, got) for lines in [K.check(family, c, blobs)] if lines]
    assert not bad, (len(bad), bad[:6])


def test_scan(trial, tmp_path):
    family_holds(trial, tmp_path, "scan")


def test_sort(trial, tmp_path):
    family_holds(trial, tmp_path, "sort")


def test_gather(trial, tmp_path):
    family_holds(trial, tmp_path, "gather")


def test_index(trial, tmp_path):
    family_holds(trial, tmp_path, "index")


def test_bins(trial, tmp_path):
    """(the order of the items inside a bin comes from atomics and is not fixed: kernel_trial_cases.bins_check compares a bin's items as a set)"""
    family_holds(trial, tmp_path, "bins")


def test_fasta_starts(trial, tmp_path):
    family_holds(trial, tmp_path, "fasta")


def test_depth_prefix_sum(trial, tmp_path):
    family_holds(trial, tmp_path, "depthscan")


def test_depth_bedgraph(trial, tmp_path):
    family_holds(trial, tmp_path, "bedgraph")


def test_pileup_rows_and_text(trial, tmp_path):
    family_holds(trial, tmp_path, "pileup")


def test_stats_rows_and_shared_adds(trial, tmp_path):
    """(the sums are integers: the order of the atomics does not show)"""
    family_holds(trial, tmp_path, "stats")
