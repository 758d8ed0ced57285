"""The base call decided by the random word alone (reseq_amd/csrc/rsq_pack.h base_call_word_bounds, rsq_reads.h word_screen_sure and ScreenTables::base_call_word)
without a GPU.  tests/hostemu/base_call_word_trial.cpp (built here with g++, on top of the host emulation) runs

 * made-up base-call tables through the pack-time bound and the lane's check: every word the check calls sure must give the template base through the
   double-precision draw (LogArrayResult::Draw), for every combination of list entries and of the values that share them -- and must stop doing so when the stored
   scalars are cut by 5 %;
 * the parity cases with option base_call_word 0 and 1 against the oracle;
 * profile P0 in the read kernel's grouping of 64 reads per wave: the share of wave-steps in which every base call is decided by the word."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import parity_cases as P

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "reseq_amd", "csrc")


def build_trial(directory):
    out = os.path.join(str(directory), "libbase_call_word_trial.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable", "-shared",
                    "-o", out, os.path.join(HERE, "hostemu", "base_call_word_trial.cpp"), os.path.join(CSRC, "rsq_host.cpp"), "-lz", "-ldl", "-lpthread"], check=True)
    L = C.CDLL(out)
    L.emu_last_error.restype = C.c_char_p
    L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_char_p, C.POINTER(C.c_void_p)]
    L.emu_free.argtypes = [C.c_void_p]
    L.emu_prepare.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_int, C.c_char_p]
    L.emu_get_info.argtypes = [C.c_void_p, C.c_void_p]
    L.emu_sieve.restype = C.c_int64
    L.emu_sieve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]
    L.emu_set_option.argtypes = [C.c_char_p, C.c_longlong]
    L.bcw_share.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.bcw_plan.argtypes = [C.c_void_p, C.c_void_p]
    L.bcw_soundness.argtypes = [C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint32, C.c_double, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def trial(tmp_path_factory):
    return build_trial(tmp_path_factory.mktemp("base_call_word_trial"))


@pytest.fixture
def word_option():
    """set(value) of option base_call_word in the product library and the host emulation; back to its default 1 afterwards"""
    from backends import set_option_everywhere
    yield lambda value: set_option_everywhere("base_call_word", value)
    set_option_everywhere("base_call_word", 1)


# ------------------------------------------------------------------------------------------------------------------------- soundness
# Small ranges, so that every combination can be drawn: qualities 2 .. 6, read positions 0 .. 39 (three buckets of sixteen), 0 .. 4 errors, rates 0 .. 3.
G_FROM = np.array([2, 0, 0, 0], np.uint32)
G_LAST = np.array([4, 39, 4, 3], np.uint32)


def make_table(rng, kind, k, z):
    """rows of the four margins (a list of arrays rows x k), their first values, and the outcome values: column z holds the template base 2"""
    from_ = G_FROM.copy()
    rows = G_LAST + 1
    if kind == "ragged":                                            # the table's own ranges are shorter than the family's at both ends
        from_ = G_FROM + np.array([1, 5, 1, 0], np.uint32)
        rows = np.array([3, 22, 2, 2], np.uint32)
    margins = []
    for n in range(4):
        if kind == "edges":                                         # the ends of the screen's preconditions
            m = np.exp2(rng.choice([-60.0, -31.0, 0.0, 29.0], (rows[n], k)))
        else:
            m = np.exp2(rng.uniform(-14.0, 0.0, (rows[n], k)))
            m[:, z] = np.exp2(rng.uniform(-1.0, 0.0, rows[n]))      # profile-like: the template base is the likely call
        if kind == "zero_rows":
            m[rng.random(rows[n]) < 0.3] = 0.0                      # all-zero rows: prob_sum 0, FillReadPart takes the template base
            m[:, [c for c in range(k) if c != z]] *= rng.random((rows[n], 1)) < 0.8      # and rows with zeros everywhere but in column z
        if kind == "zero_in_z":
            m[rng.integers(0, rows[n]), z] = 0.0                    # no bound for the lanes that can land on such a row
        margins.append(m)
    values = [v for v in (0, 1, 3, 4, 5, 6, 7, 8) if v != 2][:k - 1]
    par0 = np.array(values[:z] + [2] + values[z:], np.uint8)
    return from_, rows, margins, par0


def run_soundness(trial, from_, rows, margins, par0, cut=1.0, base=2):
    k = len(par0)
    values = np.ascontiguousarray(np.concatenate([m.ravel() for m in margins]), np.float64)
    f, r = np.ascontiguousarray(from_, np.uint32), np.ascontiguousarray(rows, np.uint32)
    out = np.zeros(5, np.uint64)
    rc = trial.bcw_soundness(k, par0.ctypes.data, f.ctypes.data, r.ctypes.data, values.ctypes.data, G_FROM.ctypes.data, G_LAST.ctypes.data, base, cut, out.ctypes.data)
    assert rc == 0, trial.emu_last_error().decode()
    return dict(zip(("bound", "sure", "draws", "wrong", "zero_sum"), map(int, out)))


KINDS = ["profile", "ragged", "edges", "zero_rows", "zero_in_z"]


@pytest.mark.parametrize("k,z", [(4, 3), (4, 0), (5, 2), (2, 1), (8, 7)])
@pytest.mark.parametrize("kind", KINDS)
def test_every_sure_word_gives_the_template_base(trial, kind, k, z):
    """template base in the last, the first and a middle column; at the ends of every sure range of words and on both sides of them"""
    rng = np.random.default_rng(100 * k + 10 * z + KINDS.index(kind))
    got = run_soundness(trial, *make_table(rng, kind, k, z))
    assert got["wrong"] == 0, got
    if kind in ("profile", "ragged"):                               # not vacuous: the bound exists and words are sure
        assert got["bound"] == 1 and got["sure"] > 1000 and got["draws"] > 10 * got["sure"], got
        assert got["zero_sum"] == 0, got
    if kind == "zero_rows":
        assert got["zero_sum"] > 0, got                             # sure draws over all-zero rows occurred


def test_a_zero_in_the_template_column_leaves_no_bound(trial):
    """every row of one margin has row[z] = 0 < row[c]: whatever the lane's values, nothing is sure"""
    rng = np.random.default_rng(5)
    from_, rows, margins, par0 = make_table(rng, "profile", 4, 3)
    margins[2][:, 3] = 0.0
    got = run_soundness(trial, from_, rows, margins, par0)
    assert got["sure"] == 0 and got["wrong"] == 0, got
    # a table without the template base among its outcome values, and one outside the screen's preconditions: no bound
    from_, rows, margins, par0 = make_table(rng, "profile", 4, 3)
    assert run_soundness(trial, from_, rows, margins, par0, base=7) == dict(bound=0, sure=0, draws=0, wrong=0, zero_sum=0)
    margins[1][0, 0] = 2.0 ** 30
    assert run_soundness(trial, from_, rows, margins, par0)["bound"] == 0


def test_scalars_cut_by_five_percent_are_caught(trial):
    """negative control: with two outcome columns the product of the scalars is attained by the lane's own rows (one column on the side: sum and maximum are
    that column's ratio), so a bound 5 % below it calls words sure that draw the other column"""
    wrong = 0
    for seed in range(4):
        rng = np.random.default_rng(40 + seed)
        from_, rows, margins, par0 = make_table(rng, "profile", 2, 1)
        for m in margins:
            m[:, 0] = np.exp2(rng.uniform(-4.0, 0.0, len(m)))       # ratios of 1/16 and more: 5 % of the sum is far above the check's own margin of 2^-20
        assert run_soundness(trial, from_, rows, margins, par0)["wrong"] == 0
        wrong += run_soundness(trial, from_, rows, margins, par0, cut=0.95)["wrong"]
    assert wrong > 0


# ------------------------------------------------------------------------------------------------------------------- parity, share
CASES = ["case_sieve_and_reads_tiny", "case_p0_reads", "case_ragged_tables", "case_indel_columns_shuffled", "case_adapter_only", "case_error_model_tiny",
         "case_variants_indels", "case_profile_edits"]


@pytest.mark.parametrize("word", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_parity_with_and_without_the_word_screen(workdir, word_option, case, word):
    from backends import EmuBackend
    word_option(word)
    getattr(P, case)(EmuBackend, workdir)


def p0_share(L, workdir, p0_profile_path, word=1):
    """[draws, sure draws, wave-steps, all-sure wave-steps] of about 1500 pairs of P0 on a 30 kb reference, and the plan"""
    from reseq_amd import synth
    fasta = workdir / "bcw_p0.fa"
    if not fasta.exists():
        synth.write_fasta(fasta, synth.make_reference(2, [30000]))
    assert 0 == L.emu_set_option(b"base_call_word", word)
    h = C.c_void_p()
    try:
        assert 0 == L.emu_create(str(p0_profile_path).encode(), str(fasta).encode(), 0, b"", C.byref(h)), L.emu_last_error().decode()
    finally:
        L.emu_set_option(b"base_call_word", 1)
    try:
        assert 0 == L.emu_prepare(h, 11, 1500, 0.0, 0, b""), L.emu_last_error().decode()
        from backends import FRAGMENT_DTYPE, EmuInfo
        info = EmuInfo()
        L.emu_get_info(h, C.byref(info))
        n = L.emu_sieve(h, 1, info.total_blocks + 1, None, 0)
        frags = np.zeros(max(n, 1), FRAGMENT_DTYPE)
        L.emu_sieve(h, 1, info.total_blocks + 1, frags.ctypes.data, n)
        out, plan = np.zeros(4, np.uint64), np.zeros(7, np.uint32)
        assert 0 == L.bcw_share(h, frags.ctypes.data, n, out.ctypes.data), L.emu_last_error().decode()
        L.bcw_plan(h, plan.ctypes.data)
        return [int(x) for x in out], [int(x) for x in plan]
    finally:
        L.emu_free(h)


def test_p0_all_sure_share(trial, workdir, p0_profile_path):
    """P0, 1500 pairs, seed 11: the word decides 0.9963 of the base calls and every one in 0.801 of the wave-steps (buckets of 16 positions, own entries up to 3
    errors and rate 63; rsq_types.h).  The floor of 0.75 leaves 0.05 for another seed or another build of the profile: 6908 wave-steps, whose reads stay together
    for 150 steps, so the figure moves by about a hundredth between seeds."""
    (draws, sure, steps, all_sure), plan = p0_share(trial, workdir, p0_profile_path)
    print(f"P0: {draws} base-call draws, {sure} decided by the word ({sure / draws:.4f}); {steps} wave-steps, {all_sure} all-sure ({all_sure / steps:.4f}); plan {plan}")
    assert plan[0] == 1 and draws > 400_000
    assert sure > 0.99 * draws
    assert all_sure > 0.75 * steps
    off, _ = p0_share(trial, workdir, p0_profile_path, word=0)
    assert off[0] == draws and off[1] == 0 and off[3] == 0        # option 0: the same draws, none decided by the word
