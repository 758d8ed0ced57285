"""The truth BAM sorted by coordinate on the device (rsq_sim_pairs_bam_sorted, rsq_sim_bam_sorted_flush, rsq_sim_bam_sorted_index, `reseq illuminaPE --truthBam
... --truthBamSort`).  The oracle is the statement of tests/test_truth_bam_sorted.py applied to the records of rsq_sim_pairs_bam (which tests/test_truth_bam_gpu.py
pins to the SAM text): their stable sort by (refID, pos) with the unmapped behind.  The main test: the sorted stream does not depend on how the blocks are cut
into calls, nor on options overlap and image_tiles."""
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from reseq_amd import api, synth
from test_truth_bam import decode_bam_header
from test_truth_bam_sorted import block_table, build_bai, overlapping, parse_bai, query_bai, sorted_stream, split_records
from test_truth_sam_gpu import MARKER, Case, tiny_case

pytestmark = pytest.mark.gpu

NEW_KERNELS = ("bam_sort_keys", "bam_sort", "bam_gather", "bam_index")


def block_of(record):
    """the block a record's pair was simulated in: a read name is "{base identifier}{block}_{number}:..." """
    return int(re.match(rb"\D*(\d+)_", record["raw"][36:]).group(1))


def expected_of(case):
    """(the sorted stream's bytes, its records, the unsorted call's results)"""
    whole = case.sim.pairs_bam(1, case.tb + 1)
    records = sorted_stream(split_records(whole[3], case.names))
    return b"".join(r["raw"] for r in records), records, whole


def run_sorted(sim, cuts, first_record_offset=0):
    """a sorted run in calls over [cuts[k], cuts[k + 1]) and the flush: (the stream, per call (lo, hi, fragments, records' bytes, records), fastq 1, fastq 2, fragments, flush)"""
    sim.bam_sorted_begin(first_record_offset)
    calls, f1, f2, frags = [], [], [], []
    for lo, hi in zip(cuts, cuts[1:]):
        fr, t1, t2, bam, n_records = sim.pairs_bam_sorted(lo, hi)
        calls.append((lo, hi, fr, bam, n_records))
        f1.append(t1)
        f2.append(t2)
        frags.append(fr.tobytes())
    flush = sim.bam_sorted_flush()
    return b"".join(c[3] for c in calls) + flush[0], calls, b"".join(f1), b"".join(f2), b"".join(frags), flush


@pytest.fixture(scope="module")
def tiny(workdir):
    c = tiny_case(workdir)
    c.expected, c.records, c.whole = expected_of(c)
    yield c
    c.close()


def test_the_case_has_teeth(tiny):
    """a change of TINY must not quietly weaken the tests below"""
    keys = [(r["ref_id"], r["pos"]) for r in tiny.records if r["mapped"]]
    assert any(a == b for a, b in zip(keys, keys[1:])), "neighbouring equal keys: ties"
    # every sequence that has fragments has records: the first and the third (the 80 bases of the second hold no fragment of this profile, so the sorted
    # stream steps over a sequence without records, and the keys of neighbours differ in refID alone)
    assert {r["ref_id"] for r in tiny.records if r["mapped"]} == {int(s) for s in np.unique(tiny.whole[0]["seq"])} == {0, 2}
    sizes = lambda recs: np.concatenate([[0], np.cumsum([len(r["raw"]) for r in recs])])[:-1]
    source, destination = sizes(split_records(tiny.whole[3], tiny.names)), sizes(tiny.records)      # one call: a record's staging offset is its offset in the unsorted stream
    assert {int(x) % 16 for x in source} == set(range(16)) and {int(x) % 16 for x in destination} == set(range(16))
    assert len(tiny.expected) == len(tiny.whole[3]) and tiny.expected != tiny.whole[3]


@pytest.mark.parametrize("cuts", ["one call", "one block per call", "1, 4, end", "an empty range in the middle"])
def test_the_stream_does_not_depend_on_the_calls(tiny, cuts):
    tb = tiny.tb
    bounds = {"one call": [1, tb + 1], "one block per call": list(range(1, tb + 2)), "1, 4, end": [1, 4, tb + 1], "an empty range in the middle": [1, 3, 3, 6, 6, tb + 1]}[cuts]
    stream, calls, f1, f2, frags, flush = run_sorted(tiny.sim, bounds)
    assert stream == tiny.expected
    assert (f1, f2) == tiny.whole[1:3] and frags == tiny.whole[0].tobytes()          # the FASTQ texts and the fragments are those of the unsorted call
    n_unmapped = sum(not r["mapped"] for r in tiny.records)
    assert sum(c[4] for c in calls) + flush[1] + flush[2] == len(tiny.records) and flush[2] == n_unmapped
    if cuts == "one block per call":                                   # a call hands out records it held from the call before: a read name begins with its block
        per_call = [split_records(bam, tiny.names) for lo, hi, fr, bam, n in calls]
        assert [len(p) for p in per_call] == [c[4] for c in calls]
        assert any(block_of(r) < c[0] for c, p in zip(calls[1:], per_call[1:]) for r in p)
        assert any(n != 2 * len(fr) for lo, hi, fr, bam, n in calls)
    if cuts == "an empty range in the middle":
        assert len(calls[1][2]) == 0 and len(calls[3][2]) == 0


@pytest.mark.parametrize("option,value", [("overlap", 3), ("image_tiles", 1)])
def test_pipelined_sub_ranges_and_binned_rows(tiny, workdir, rsq_options, option, value):
    rsq_options(option, value)
    c = tiny_case(workdir)
    try:
        if option == "image_tiles":
            assert c.sim.fill_plan()["image_tiles"] == 1
        for bounds in ([1, c.tb + 1], [1, 4, c.tb + 1]):
            stream, calls, f1, f2, frags, flush = run_sorted(c.sim, bounds)
            assert stream == tiny.expected and (f1, f2) == tiny.whole[1:3] and frags == tiny.whole[0].tobytes()
        if option == "overlap":
            c.sim.bam_sorted_begin(0)
            c.sim.pairs_bam_sorted_device(1, c.tb + 1, None, None, None)
            assert c.sim.last_kernel_launches("bam_write") == 3 and c.sim.last_kernel_launches("bam_sort_keys") == 3
    finally:
        c.close()


def test_parts_without_pairs(workdir, rsq_options):
    """a pipelined truth call some of whose parts hold no pair: 40 pairs on TINY's nine blocks leave a block in the middle (and the last one) empty, and
    option overlap = the number of blocks makes every block a part of its own.  Such a part's text, SAM text and records end where they begin, on the
    workspace it alternates to; the three outputs are those of the call in one part."""
    sparse = lambda: Case(workdir, "tiny_e2e", synth.TINY, [5000, 80, 3210], 7, 40)
    c = sparse()
    try:
        tb = c.tb
        want_sam = c.sim.pairs_sam(1, tb + 1)
        want_sorted = run_sorted(c.sim, [1, tb + 1])
    finally:
        c.close()
    rsq_options("overlap", tb)
    c = sparse()
    try:
        # the teeth: part k of tb parts over [1, tb + 1) is block k + 1 alone
        per_block = [len(c.sim.pairs(b, b + 1)[0]) for b in range(1, tb + 1)]
        assert 0 in per_block[1:-1] and per_block[0] > 0 and sum(per_block) == len(want_sam[0]) > 0, per_block
        filled = sum(n > 0 for n in per_block)
        frags, f1, f2, sam = c.sim.pairs_sam(1, tb + 1)
        assert c.sim.last_kernel_launches("sam_write") == filled
        assert frags.tobytes() == want_sam[0].tobytes() and (f1, f2, sam) == want_sam[1:]
        stream, calls, f1, f2, frags, flush = run_sorted(c.sim, [1, tb + 1])
        assert (stream, f1, f2, frags) == (want_sorted[0], want_sorted[2], want_sorted[3], want_sorted[4]) and flush == want_sorted[5]
        assert len(stream) > 0 and (f1, f2) == want_sam[1:3]
    finally:
        c.close()


def test_launch_counts(tiny):
    sim, tb = tiny.sim, tiny.tb
    new = lambda: {k: sim.last_kernel_launches(k) for k in NEW_KERNELS}
    none = dict.fromkeys(NEW_KERNELS, 0)
    sim.pairs(1, 3)
    assert new() == none
    sim.pairs_sam(1, 3)
    assert new() == none
    sim.pairs_bam(1, 3)
    assert new() == none and sim.last_kernel_launches("bam_write") == 1
    sim.bam_sorted_begin(0)
    sim.pairs_bam_sorted(1, 3)
    assert all(v >= 1 for v in new().values()), new()
    assert sim.last_kernel_launches("sam_sizes") == 0 and sim.last_kernel_launches("sam_write") == 0
    assert sim.last_kernel_launches("bam_sizes") == 1 and sim.last_kernel_launches("bam_write") == 1 and sim.last_kernel_launches("bam_gather") == 1
    sim.pairs_bam(1, 3)                                              # an unsorted call in the middle of a run launches none of them either
    assert new() == none


def test_enospc_and_a_call_out_of_turn(tiny):
    sim, dev, tb = tiny.sim, tiny.sim.device, tiny.tb
    sim.bam_sorted_begin(0)
    out = [sim.pairs_bam_sorted(1, 4)[3]]
    n, l1, l2, lb, nr, rc = sim.pairs_bam_sorted_device(4, 7, None, None, None)
    assert rc == api.RSQ_ENOSPC and n > 0 and lb > 0
    r1, r2 = api.DeviceArray(dev, l1), api.DeviceArray(dev, l2)
    short = api.DeviceArray.from_numpy(dev, np.full(lb - 1, MARKER, np.uint8))
    full = api.DeviceArray.from_numpy(dev, np.full(lb, MARKER, np.uint8))
    try:
        assert sim.pairs_bam_sorted_device(4, 7, r1, r2, short) == (n, l1, l2, lb, nr, api.RSQ_ENOSPC)       # a BAM buffer one byte short
        assert np.all(short.to_numpy(np.uint8, lb - 1) == MARKER)
        # a call out of turn: the run goes on at block 4
        assert sim.pairs_bam_sorted_device(5, 7, r1, r2, full)[5] == api.RSQ_ESTATE and "block 4" in api.lib().rsq_last_error().decode()
        assert np.all(full.to_numpy(np.uint8, lb) == MARKER)
        # repeated with enough room, the call and the rest of the run give the sorted stream
        assert sim.pairs_bam_sorted_device(4, 7, r1, r2, full) == (n, l1, l2, lb, nr, api.RSQ_OK)
        out.append(full.to_numpy(np.uint8, lb).tobytes())
    finally:
        for d in (r1, r2, short, full):
            d.free()
    out.append(sim.pairs_bam_sorted(7, tb + 1)[3])
    out.append(sim.bam_sorted_flush()[0])
    assert b"".join(out) == tiny.expected
    assert sim.bam_sorted_flush() == (b"", 0, 0)                     # nothing is held any more


def three_case(workdir, **kw):
    """tiny_case with a middle sequence long enough to carry fragments: blocks 1-5, 6-7 and 8-11"""
    return Case(workdir, "bam_sorted_three", synth.TINY, [5000, 1500, 3210], 7, 3000, **kw)


def test_records_of_all_three_sequences(workdir):
    """a middle refID with records: its digits are sorted, cuts fall at its first block, inside it and at its end, and it is held across calls"""
    c = three_case(workdir)
    try:
        expected, records, whole = expected_of(c)
        assert {r["ref_id"] for r in records if r["mapped"]} == {0, 1, 2}
        middle = sorted({int(b) for b in whole[0]["block"][whole[0]["seq"] == 1]})          # the middle sequence's blocks
        assert len(middle) == 2 and middle[0] > 4 and middle[1] + 3 <= c.tb
        keys = [(r["ref_id"], r["pos"]) for r in records if r["mapped"]]
        assert any(a == b and a[0] == 1 for a, b in zip(keys, keys[1:])), "ties inside the middle sequence"
        for bounds in ([1, c.tb + 1], list(range(1, c.tb + 2)), [1, middle[0], middle[1], middle[1] + 1, c.tb + 1], [1, 4, middle[1], middle[1], middle[1] + 3, c.tb + 1]):
            stream, calls, f1, f2, frags, flush = run_sorted(c.sim, bounds)
            assert stream == expected, bounds
            assert (f1, f2) == whole[1:3] and frags == whole[0].tobytes()
        per_call = [split_records(call[3], c.names) for call in calls]          # the last cuts: the call that begins at the middle sequence's second block hands out records of its first
        assert any(r["ref_id"] == 1 and block_of(r) == middle[0] for r in per_call[3]) and not per_call[2]
    finally:
        c.close()


def test_long_sequence(workdir):
    """keys of more than 16 position bits (a third 8-bit digit), records across 16384 and 131072, calls of 37 blocks"""
    c = Case(workdir, "bam_sorted_long", synth.TINY, [140000, 80, 3210], 7, 4000)
    try:
        expected, records, whole = expected_of(c)
        bins = {r["bin"] for r in records if r["mapped"]}
        assert any(b < 585 for b in bins) and any(b >= 4681 for b in bins), sorted(bins)[:5]
        assert any(r["pos"] > 131072 for r in records if r["mapped"]) and {r["ref_id"] for r in records if r["mapped"]} == {0, 2}
        bounds = list(range(1, c.tb + 1, 37)) + [c.tb + 1]
        assert len(bounds) > 3
        stream, calls, f1, f2, frags, flush = run_sorted(c.sim, bounds)
        assert stream == expected and (f1, f2) == whole[1:3]
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ the command line
def read_chunk(packed, names, beg, end):
    """the records of the chunk [beg, end) (virtual offsets), inflating from the chunk's block on: [(virtual offset, record)]"""
    text, member_at, at = b"", [], beg >> 16
    while at < len(packed) and at <= end >> 16:
        d = zlib.decompressobj(31)
        member_at.append((len(text), at))
        text += d.decompress(packed[at:])
        assert d.eof
        at = len(packed) - len(d.unused_data)
    out, t = [], beg & 0xFFFF
    while t < len(text):
        text_at, file_at = max(m for m in member_at if m[0] <= t)
        v = file_at << 16 | (t - text_at)
        if v >= end:
            break
        (block_size,) = struct.unpack_from("<i", text, t)
        if t + 4 + block_size > len(text):                            # the chunk's last record ends in a block behind the chunk's last: not asked for here
            break
        out.append((v, split_records(text[t:t + 4 + block_size], names)[0]))
        t += 4 + block_size
    return out


def test_command_line(workdir):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    c = Case(workdir, "bam_sorted_cli", synth.P0, [40000], 11, 1500, prof_seed=103741084, ref_seed=2, replace_n_seed=11, base_identifier="ReseqRead")
    try:
        expected, records, (frags, f1, f2, bam) = expected_of(c)
        a1, a2, abam = c.sim.adapter_only_pairs_bam(0, c.info.adapter_only_pairs)
        header, names, fpath, ppath = c.ref.bam_header_so(1), c.names, c.fpath, c.ppath
    finally:
        c.close()
    out = {k: str(workdir / f"truth_sorted_cli_{k}") for k in ("p1", "p2", "s1", "s2", "x1", "x2")}
    out.update(bam=str(workdir / "truth_sorted_cli.bam"), sam=str(workdir / "truth_sorted_cli.sam"), xbam=str(workdir / "truth_sorted_cli_x.bam"))
    common = [exe, "illuminaPE", "-R", fpath, "-s", ppath, "--numReads", "1500", "--seed", "11"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True)
    read = lambda path: open(path, "rb").read()
    assert run(["-1", out["p1"], "-2", out["p2"]]).returncode == 0
    r = run(["-1", out["s1"], "-2", out["s2"], "--truthBam", out["bam"], "--truthBamSort", "--truthSam", out["sam"]])
    assert r.returncode == 0, r.stderr
    for m in "12":                                                 # the FASTQ files are unchanged by the option
        assert read(out["p" + m]) == read(out["s" + m]) == (f1 + a1 if m == "1" else f2 + a2)
    packed = read(out["bam"])
    block_u, block_c = block_table(packed)
    assert len(block_u) >= 4 and packed.endswith(api.gzip_eof_member())          # at least three blocks and the end-of-file member
    content = b"".join(zlib.decompress(packed[c0:c1], 31) for c0, c1 in zip(block_c, block_c[1:] + [len(packed)]))
    assert content == header + expected + abam
    text, refs, used = decode_bam_header(content)
    assert text.startswith(b"@HD\tVN:1.6\tSO:coordinate\n") and used == len(header)
    assert read(out["sam"]).startswith(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n")          # the SAM file of the same run stays in pair order
    in_file = records + split_records(abam, names)
    n_no_coor = sum(not r["mapped"] for r in in_file)
    assert n_no_coor == 2 * c.info.adapter_only_pairs + sum(not r["mapped"] for r in records)
    bai = read(out["bam"] + ".bai")
    assert bai == build_bai(in_file, len(header), len(names), block_u, block_c, n_no_coor)
    index = parse_bai(bai)
    assert index[1] == n_no_coor
    for beg, end in ((20000, 20100), (16300, 16500), (0, 40000)):      # inside one window, across 16384, the whole sequence
        found = [r for cb, ce in query_bai(index, 0, beg, end) for v, r in read_chunk(packed, names, cb, ce)]
        found = [r for r in found if r["mapped"] and r["pos"] < end and r["pos"] + r["span"] > beg]
        want = overlapping(records, 0, beg, end)
        assert want and [r["raw"] for r in found] == [r["raw"] for r in want], (beg, end)
    # refusals: nothing is simulated, no file is left
    golden_vcf = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test-var.vcf")
    for extra, message in ((["--truthBam", out["xbam"], "--truthBamSort", "--gpus", "2"], "one worker only"), (["--truthBam", out["xbam"], "--truthBamSort", "-V", golden_vcf], "variants"),
                           (["--truthBam", out["xbam"], "--truthBamSort", "--hostGzip"], "hostGzip"), (["--truthBamSort"], "--truthBam")):
        r = run(["-1", out["x1"], "-2", out["x2"]] + extra)
        assert r.returncode != 0 and message in r.stderr, r.stderr
        assert not any(os.path.exists(p) for p in (out["x1"], out["x2"], out["xbam"], out["xbam"] + ".bai"))


def test_command_line_in_batches(workdir):
    """--truthSam beside --truthBam --truthBamSort in batches of one block: a batch's calls are repeated when one of them asks for room, the sorted call --
    which has moved its run on when it returned -- is not; members and records are cut by batch ends at any place"""
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "reseq")
    c = three_case(workdir, replace_n_seed=7, base_identifier="ReseqRead")
    try:
        expected, records, (frags, f1, f2, bam) = expected_of(c)
        sam = c.sim.pairs_sam(1, c.tb + 1)[3]
        a1, a2, abam = c.sim.adapter_only_pairs_bam(0, c.info.adapter_only_pairs)
        asam = c.sim.adapter_only_pairs_sam(0, c.info.adapter_only_pairs)[2]
        header, sam_header, names, fpath, ppath = c.ref.bam_header_so(1), c.ref.sam_header(), c.names, c.fpath, c.ppath
    finally:
        c.close()
    out = {k: str(workdir / f"truth_sorted_batches_{k}") for k in ("1", "2", "sam")}
    out["bam"] = str(workdir / "truth_sorted_batches.bam")
    for batch_blocks in ("1", "4"):
        r = subprocess.run([exe, "illuminaPE", "-R", fpath, "-s", ppath, "--numReads", "3000", "--seed", "7", "-1", out["1"], "-2", out["2"], "--truthBam", out["bam"], "--truthBamSort",
                            "--truthSam", out["sam"], "--batchBlocks", batch_blocks], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        read = lambda path: open(path, "rb").read()
        assert read(out["1"]) == f1 + a1 and read(out["2"]) == f2 + a2 and read(out["sam"]) == sam_header + sam + asam
        packed = read(out["bam"])
        block_u, block_c = block_table(packed)
        content = b"".join(zlib.decompress(packed[c0:c1], 31) for c0, c1 in zip(block_c, block_c[1:] + [len(packed)]))
        assert content == header + expected + abam and packed.endswith(api.gzip_eof_member())
        in_file = records + split_records(abam, names)
        assert read(out["bam"] + ".bai") == build_bai(in_file, len(header), len(names), block_u, block_c, sum(not r["mapped"] for r in in_file))
