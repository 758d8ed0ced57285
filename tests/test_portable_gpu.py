"""The DEVICE forms of reseq_amd/csrc/rsq_portable.h: tests/hostemu/portable_trial.cpp -- the source test_portable.py builds for the host -- compiled by hipcc for
the library's architecture runs the table of portable_table.py through one kernel of one workgroup (the LDS primitives on a few words of LDS), as a fresh child
process under a time limit of its own; its results must be the host program's, word for word.  With test_portable.py (the host forms against their stated
meaning) that is what the host emulation of the kernels' per-lane functions rests on."""
import numpy as np
import pytest

import portable_table as T


@pytest.mark.gpu
def test_the_device_forms_give_the_host_forms_words(tmp_path):
    hipcc = T.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc to compile the program with")
    table = T.records()
    host, done = T.run(T.build_host(tmp_path, sanitize=False), table, tmp_path, "host")
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    device, done = T.run(T.build_device(tmp_path, hipcc), table, tmp_path, "device", timeout=120)
    assert done.returncode == 0 and f"{len(table)} records" in done.stdout, (done.returncode, done.stdout, done.stderr[-2000:])
    assert host.shape == device.shape == (len(table), 4)
    bad = np.flatnonzero((host != device).any(axis=1))
    assert not len(bad), (len(bad), [(T.OPS[table[i, 0]], table[i, 1:7].tolist(), host[i].tolist(), device[i].tolist()) for i in bad[:8]])
    assert (device == T.expected(table)).all()
