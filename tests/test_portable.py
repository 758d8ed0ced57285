"""What the host emulation rests on (reseq_amd/csrc/rsq_portable.h): wherever a kernel header's function does one thing on the device and another on the host, both
are one primitive of that header.  Here the HOST forms: tests/hostemu/portable_trial.cpp, a program of its own built with g++ and -fsanitize=address,undefined,
evaluates every primitive over the table of portable_table.py, and every result must be what the primitive's stated meaning gives, computed here in plain Python.
tests/test_portable_gpu.py requires the same words of the device forms."""

import numpy as np
import pytest

import portable_table as T


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("portable")
    table = T.records()
    got, done = T.run(T.build_host(d, sanitize=True), table, d, "san")
    assert done.returncode == 0 and f"{len(table)} records" in done.stdout, (done.returncode, done.stdout, done.stderr[-4000:])
    return table, got, T.expected(table)


def test_the_table_covers_what_it_says():
    table = T.records()
    ops = table[:, 0]
    assert set(ops) == set(range(len(T.OPS))), "every primitive has records"
    for name in ("base_letters", "complement_letters"):
        codes = table[ops == T.OP[name], 1]
        assert len(set(codes)) == 4096 and all(((codes >> (8 * k)) & 0xFF).max() == 7 for k in range(4))
    assert (ops == T.OP["bam_nibbles"]).sum() == 2 * 4096
    sel = table[(ops == T.OP["perm_bytes"]) & (table[:, 4] == 0), 3]
    assert (table[(ops == T.OP["perm_bytes"]) & (table[:, 4] != 0), 3] & 0xF8F8F8F8 != 0).all()
    assert {0x00010203, 0x06040200, 0x03020100, 0x07060504} <= set(sel) and all({(s >> (8 * k)) & 0xFF for s in sel} == set(range(8)) for k in range(4))
    assert set(table[ops == T.OP["align_bytes"], 3]) == {0, 1, 2, 3} and set(table[ops == T.OP["bytes_at"], 3]) == {0, 1, 2, 3, 4}
    div = table[ops == T.OP["div_small"]]
    assert set(div[:, 2]) == set(range(1, 301)) | {65535} and div[:, 1].max() < 1 << 24 and (div[:, 1] // div[:, 2]).max() == (1 << 17) - 1
    assert {(1 << 16) * d for d in (1, 7, 255)} <= set(div[:, 1]) and {(1 << 16) * 7 - 1, (1 << 16) * 7 + 1, 0, 1, 2} <= set(div[:, 1])
    for name, step, size in (("load64_align1", 1, 8), ("load64_align2", 2, 8), ("load128_align2", 2, 16), ("load32_align1", 1, 4), ("load32_align4", 4, 4), ("load64_align1_lds", 1, 8)):
        assert list(table[ops == T.OP[name], 1]) == list(range(0, 64 - size + 1, step)), name
    fma = table[ops == T.OP["fma1"]]
    differ = sum(abs(T.fused(a, b, c) - T.unfused(a, b, c)) == 1 for a, b, c in fma[:, [1, 3, 5]].tolist())
    assert differ >= 64, "operands whose fused and unfused results differ in the last bit"
    assert len(table) < 40000


@pytest.mark.parametrize("name", T.OPS)
def test_a_host_form_gives_what_the_primitive_means(host_results, name):
    table, got, want = host_results
    rows = np.flatnonzero(table[:, 0] == T.OP[name])
    bad = rows[(got[rows] != want[rows]).any(axis=1)]
    assert len(rows) and not len(bad), (name, len(bad), [(table[i, 1:7].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:5]])


def test_fused_and_unfused_are_told_apart(host_results):
    """the host's fma2 / fma1 round once and Float2's own operators twice: on the operands chosen for it the two differ in the last bit, as computed exactly here"""
    table, got, _ = host_results
    f, m = got[table[:, 0] == T.OP["fma2"]], got[table[:, 0] == T.OP["mul_add2"]]
    assert (np.abs(f[:64, 0].astype(np.int64) - m[:64, 0].astype(np.int64)) == 1).all()


def test_outside_its_domain_a_host_form_stops(tmp_path):
    """a shift of 4 through align_bytes (the instruction takes it modulo 4, a plain shift does not) is outside the contract, like a word beyond bytes_at's four, a zero
    word for the lowest set bit and a dividend of 2^24: the host form asserts instead of returning a word the device would not"""
    exe = T.build_host(tmp_path, sanitize=False)
    for name, args in (("align_bytes", (1, 2, 4)), ("bytes_at", (1, 2, 5)), ("lowest_set_bit64", (0, 0)), ("div_small", (1 << 24, 3))):
        row = np.array([[T.OP[name], *args] + [0] * (7 - len(args))], np.uint32)
        got, done = T.run(exe, row, tmp_path, "outside")
        assert done.returncode != 0 and "Assertion" in done.stderr, (name, done.returncode, done.stderr[-500:])
    got, done = T.run(exe, np.array([[T.OP["load64_align1"], 57, 0, 0, 0, 0, 0, 0]], np.uint32), tmp_path, "outside")      # and the program itself refuses an access beside its buffers
    assert done.returncode == 2 and got is None
