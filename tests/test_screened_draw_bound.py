"""The read kernel's screened draw (rsq_core.h draw_screened) against the double-precision recipe (draw_rows_k, the reference's LogArrayResult::Draw) on
the CPU: single precision with fused multiply-adds in its running sum, and a band `delta` around every column boundary derived from the rounding count above
the function.  Every draw the screen calls decided must have the double-precision column -- over random tables, over words aimed at the column boundaries,
and over rows at the edges of the screen's preconditions (values 0 or in [2^-60, 2^29], a total of at least 2^-30).  The share the screen leaves to the
double-precision route is reported for profile P0 through the host emulation (tests/hostemu)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def trial_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("screen_trial") / "libscreen_trial.so")
    # the product's floating-point flags: no contraction (the screen's FMAs are explicit builtins)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", out, os.path.join(HERE, "hostemu", "screen_trial.cpp")], check=True)
    L = C.CDLL(out)
    L.screen_trial.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.screen_row_stride.argtypes = [C.c_uint32]
    L.screen_row_stride.restype = C.c_uint32
    return L


def run_trial(L, rows, words):
    """rows: nm x k doubles; returns (decided, screened column, double-precision column) per word"""
    nm, k = rows.shape
    kp = L.screen_row_stride(k)
    padded = np.zeros((nm, kp), np.float64)
    padded[:, :k] = rows
    words = np.ascontiguousarray(words, np.uint32)
    out = np.zeros((len(words), 3), np.int32)
    assert 0 == L.screen_trial(nm, k, padded.ctypes.data, len(words), words.ctypes.data, out.ctypes.data)
    return out[:, 0].astype(bool), out[:, 1], out[:, 2]


def boundary_words(rows, rng, spread=(0, 1, 2, 3, 7, 64, 1 << 10, 1 << 14)):
    """words whose u * T falls on and next to every column boundary: the reference takes column j when B(j) < (1-u) T <= B(j+1)"""
    p = np.prod(rows, axis=0)
    T = p.sum()
    if T == 0:
        return np.zeros(0, np.uint32)
    below = np.concatenate([[0.0], np.cumsum(p)[:-1]])
    centre = np.floor((1.0 - below / T) * 4294967296.0).astype(np.int64)
    offs = np.array([s * d for s in spread for d in (-1, 1)] + [0], np.int64)
    w = (centre[:, None] + offs[None, :]).ravel()
    w = np.concatenate([w, rng.integers(0, 1 << 32, 2000, dtype=np.int64), [0, 1, (1 << 32) - 1]])
    return np.clip(w, 0, (1 << 32) - 1).astype(np.uint32)


def random_rows(rng, nm, k, kind):
    lo, hi = {"profile": (-14.0, 0.0), "wide": (-40.0, 20.0), "edges": (-60.0, 29.0), "small": (-12.0, -7.0)}[kind]
    rows = np.exp2(rng.uniform(lo, hi, (nm, k)))
    if kind == "edges":                                         # the bounds of the preconditions themselves, and zeros
        pick = rng.random((nm, k))
        rows[pick < 0.15] = 2.0 ** -60
        rows[(pick >= 0.15) & (pick < 0.25)] = 2.0 ** 29
        rows[(pick >= 0.25) & (pick < 0.35)] = 0.0
    elif kind != "small":
        rows[rng.random((nm, k)) < 0.05] = 0.0
    if kind == "profile":                                       # as the tables are written: columns by ascending likelihood
        rows = rows[:, np.argsort(np.prod(rows, axis=0), kind="stable")]
    return rows


@pytest.mark.parametrize("nm,k", [(4, 40), (4, 48), (4, 37), (4, 8), (4, 5), (3, 8), (3, 2), (4, 1)])
@pytest.mark.parametrize("kind", ["profile", "wide", "edges", "small"])
def test_every_decided_draw_is_the_double_precision_column(trial_lib, nm, k, kind):
    rng = np.random.default_rng(1000 * nm + 10 * k + ["profile", "wide", "edges", "small"].index(kind))
    decided_total = draws = 0
    for _ in range(25):
        rows = random_rows(rng, nm, k, kind)
        words = boundary_words(rows, rng)
        if not len(words):
            continue
        decided, col, exact = run_trial(trial_lib, rows, words)
        wrong = np.flatnonzero(decided & (col != exact))
        assert not len(wrong), (rows.tolist(), words[wrong[:5]].tolist(), col[wrong[:5]].tolist(), exact[wrong[:5]].tolist())
        draws += len(words)
        decided_total += int(decided.sum())
    if kind in ("profile", "wide") and k > 1:                     # the screen is not vacuous: words aimed at boundaries are a minority of the draws
        assert decided_total > 0.3 * draws, (decided_total, draws)


def test_total_below_the_screens_minimum_is_never_decided(trial_lib):
    """S32 >= 2^-30 is a precondition of the bound: rows whose products sum below it go to double precision"""
    rows = np.full((4, 40), 2.0 ** -9)                          # 40 columns of 2^-36: S = 40 * 2^-36 < 2^-30
    words = np.random.default_rng(7).integers(0, 1 << 32, 5000, dtype=np.int64).astype(np.uint32)
    decided, _, _ = run_trial(trial_lib, rows, words)
    assert not decided.any()


def test_p0_undecided_share(workdir):
    """profile P0 (K = 40, ten quads) through the host emulation: the share of quality draws the screen leaves to double precision.  The FMAs round a
    term more often in the running sum (the band grew from (2Q+24) to (4Q+20) units): about 5.7e-5 before, at most 2e-4 allowed"""
    import parity_cases as P
    from backends import EmuBackend, emu_lib
    stats = np.zeros(8, np.uint64)
    emu_lib().emu_screen_stats(C.c_void_p(stats.ctypes.data))             # reset
    P.case_p0_reads(EmuBackend, workdir)
    emu_lib().emu_screen_stats(C.c_void_p(stats.ctypes.data))
    (q, q_left), (b, b_left) = stats.reshape(4, 2)[:2].tolist()
    print(f"P0 quality draws {q}, undecided {q_left} ({q_left / q:.3g}); base-call draws {b}, undecided {b_left} ({b_left / b:.3g})")
    assert q > 400_000 and b > 400_000
    assert q_left < 2e-4 * q, (q, q_left)
    assert b_left < 2e-4 * b, (b, b_left)
