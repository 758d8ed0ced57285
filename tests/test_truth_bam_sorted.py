"""The truth BAM sorted by coordinate and its .bai index (reseq_amd/csrc/rsq_bamsort.h; include/reseq_amd.h rsq_sim_pairs_bam_sorted ...) without a GPU.

The statement lives here, in pure Python: `sorted_stream` (the mapped records stably sorted by (refID, pos), the unmapped behind in their order), `build_bai` (SAM
specification 5.2 from the records in file order and the file's BGZF block table), `parse_bai` and `query_bai` (the region query of 5.3: reg2bins plus the linear
index).  tests/hostemu/bam_sort_trial.cpp -- built here with g++ like the other trials -- runs the library's host-callable pieces on crafted inputs: the key of
a mate, a sort pass's tile / digit / rank arithmetic as a loop, the cut, the run and window rules call by call, and the .bai builder.
tests/test_truth_bam_sorted_gpu.py applies the same statement to the device's output."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from reseq_amd import api
from test_truth_bam import decode_bam, decode_bam_header, reg2bin
from test_truth_sam import GOLDEN, HERE, build_trial

NO_OFFSET = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ the statement
def split_records(data, names):
    """the uncompressed records in `data`: [dict(raw, ref_id, pos, span, bin)]; span = max(reference bases, 1), 0 for an unmapped record (the decoder of
    tests/test_truth_bam.py has checked every field on the way)"""
    _, fields = decode_bam(data, names)
    out, at = [], 0
    for f in fields:
        size = 4 + f["block_size"]
        raw = data[at:at + size]
        cigar = struct.unpack_from("<%dI" % f["n_cigar"], raw, 36 + f["l_read_name"])
        span = sum(c >> 4 for c in cigar if (c & 15) in (0, 2))
        mapped = not f["flag"] & 0x4
        out.append(dict(raw=raw, ref_id=f["ref_id"], pos=f["pos"], span=max(span, 1) if mapped else 0, bin=f["bin"], mapped=mapped))
        at += size
    assert at == len(data)
    return out


def sorted_stream(records):
    """the mapped records stably sorted by (refID, pos), then the unmapped ones in their original order"""
    mapped = [r for r in records if r["mapped"]]
    return sorted(mapped, key=lambda r: (r["ref_id"], r["pos"])) + [r for r in records if not r["mapped"]]


def block_table(packed):
    """(uncompressed starts, compressed starts) of the BGZF blocks of a file, read off the members: BSIZE at bytes 16-17, ISIZE in the last four"""
    u, c, at, text = [], [], 0, 0
    while at < len(packed):
        assert packed[at:at + 4] == b"\x1f\x8b\x08\x04" and packed[at + 12:at + 14] == b"BC"
        size = struct.unpack_from("<H", packed, at + 16)[0] + 1
        u.append(text)
        c.append(at)
        text += struct.unpack_from("<I", packed, at + size - 4)[0]
        at += size
    assert at == len(packed)
    return u, c


def virtual_offset(offset, block_u, block_c):
    """the block with the largest start <= offset: an offset at a block's first byte belongs to that block"""
    k = max(i for i, u in enumerate(block_u) if u <= offset)
    assert offset - block_u[k] < 65536
    return block_c[k] << 16 | (offset - block_u[k])


def build_bai(records, first_offset, n_ref, block_u, block_c, n_no_coor):
    """the .bai of a file whose records (file order, each a dict of split_records) begin at the uncompressed offset first_offset"""
    bins = [dict() for _ in range(n_ref)]
    linear = [dict() for _ in range(n_ref)]
    at, last = first_offset, None
    for r in records:
        end = at + len(r["raw"])
        if r["mapped"]:
            chunks = bins[r["ref_id"]].setdefault(r["bin"], [])
            if last == (r["ref_id"], r["bin"]):
                chunks[-1][1] = end                                  # consecutive in the file: the run goes on
            else:
                chunks.append([at, end])
            for w in range(r["pos"] >> 14, ((r["pos"] + r["span"] - 1) >> 14) + 1):
                linear[r["ref_id"]].setdefault(w, at)                # file order: the first record that overlaps the window
            last = (r["ref_id"], r["bin"])
        else:
            last = None
        at = end
    out = [b"BAI\1", struct.pack("<I", n_ref)]
    for ref in range(n_ref):
        out.append(struct.pack("<I", len(bins[ref])))
        for b in sorted(bins[ref]):
            out.append(struct.pack("<II", b, len(bins[ref][b])))
            for beg, end in bins[ref][b]:
                out.append(struct.pack("<QQ", virtual_offset(beg, block_u, block_c), virtual_offset(end, block_u, block_c)))
        n_intv = max(linear[ref]) + 1 if linear[ref] else 0
        out.append(struct.pack("<I", n_intv))
        values, nxt = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):                          # a window no record overlaps takes the value of the next overlapped one
            nxt = linear[ref].get(w, nxt)
            values[w] = virtual_offset(nxt, block_u, block_c)
        out.append(struct.pack("<%dQ" % n_intv, *values))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def parse_bai(data):
    """([per sequence (bins: {bin: [(beg, end)]}, linear: [ioffset])], n_no_coor)"""
    assert data[:4] == b"BAI\1"
    (n_ref,) = struct.unpack_from("<I", data, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<I", data, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<II", data, at)
            at += 8
            assert b not in bins and n_chunk > 0
            bins[b] = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
        (n_intv,) = struct.unpack_from("<I", data, at)
        at += 4
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, data, at))))
        at += 8 * n_intv
    (n_no_coor,) = struct.unpack_from("<Q", data, at)
    assert at + 8 == len(data)
    return refs, n_no_coor


def reg2bins(beg, end):
    """SAM specification 5.3: the bins that may hold records overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def query_bai(index, ref, beg, end):
    """the chunks a reader visits for [beg, end) of sequence `ref`: those of reg2bins' bins that end behind the linear index's offset for beg's window"""
    bins, linear = index[0][ref]
    if not bins:
        return []
    w = beg >> 14
    min_offset = linear[w] if w < len(linear) else (linear[-1] if linear else 0)
    chunks = [c for b in reg2bins(beg, end) for c in bins.get(b, []) if c[1] > min_offset]
    return sorted((max(cb, min_offset), ce) for cb, ce in chunks)


def records_through_index(index, ref, beg, end, by_voffset):
    """the records a reader finds: those that begin inside a visited chunk and overlap; by_voffset: {virtual offset of a record's first byte: record}"""
    chunks = query_bai(index, ref, beg, end)
    found = [r for v, r in sorted(by_voffset.items()) if any(cb <= v < ce for cb, ce in chunks)]
    return [r for r in found if r["mapped"] and r["ref_id"] == ref and r["pos"] < end and r["pos"] + r["span"] > beg]


def overlapping(records, ref, beg, end):
    return [r for r in records if r["mapped"] and r["ref_id"] == ref and r["pos"] < end and r["pos"] + r["span"] > beg]


# ------------------------------------------------------------------------------------------------ the trial
class TrialMate(C.Structure):
    _fields_ = [("q", C.c_uint32), ("t", C.c_uint32), ("lead", C.c_uint32), ("trail", C.c_uint32), ("bytes", C.c_uint32)]


@pytest.fixture(scope="module")
def trial(tmp_path_factory):
    L = build_trial(tmp_path_factory, "bam_sort_trial")
    L.bam_sort_trial_entries.argtypes = [C.c_uint32] * 4 + [C.POINTER(TrialMate), C.c_uint64, C.c_uint32, C.c_void_p]
    L.bam_sort_trial_key.restype = L.bam_sort_trial_unmapped_key.restype = C.c_uint64
    L.bam_sort_trial_key.argtypes = [C.c_uint32, C.c_uint32]
    L.bam_sort_trial_unmapped_key.argtypes = [C.c_uint32]
    L.bam_sort_trial_tile.restype = C.c_uint32
    L.bam_sort_trial_out_of_order.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    L.bam_sort_trial_sort.restype = C.c_uint32
    L.bam_sort_trial_sort.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bam_sort_trial_cut.restype = C.c_uint64
    L.bam_sort_trial_cut.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.bam_sort_trial_index.restype = C.c_uint64
    L.bam_sort_trial_index.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                       C.c_char_p, C.c_uint64]
    return L


def key(ref, pos):
    return ref << 32 | pos


def trial_sort(L, keys, n_seqs, longest):
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    order, out, plan = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint64), np.zeros(2, np.uint32)
    keys_arg = np.ascontiguousarray(keys) if n else np.zeros(1, np.uint64)
    passes = L.bam_sort_trial_sort(keys_arg.ctypes.data, n, n_seqs, longest, order.ctypes.data, out.ctypes.data, plan.ctypes.data)
    return [int(i) for i in order[:n]], [int(k) for k in out[:n]], passes, (int(plan[0]), int(plan[1]))


def test_the_key_of_a_mate(trial):
    """forward: start + D dropped at the left end; reverse: end - template bases + D dropped at the left end (its last in read order); the interval is the one the
    bin is taken from; a fragment of length 0 is unmapped and lies above every mapped key"""
    L = trial
    assert L.bam_sort_trial_key(2, 77) == key(2, 77) and L.bam_sort_trial_unmapped_key(3) == key(3, 0)
    out = np.zeros(8, np.uint64)
    mates = (TrialMate * 2)(TrialMate(30, 32, 2, 0, 111), TrialMate(25, 25, 0, 5, 222))
    for strand in (0, 1):
        L.bam_sort_trial_entries(1, 1000, 200, strand, mates, 5000, 3, out.ctypes.data)
        fwd, rev = (0, 1) if strand == 0 else (1, 0)               # the mate with segment == strand reads forward
        m = [(30, 32, 2, 0), (25, 25, 0, 5)]
        lead_f, trail_f = m[fwd][2], m[fwd][3]
        lead_r, trail_r = m[rev][2], m[rev][3]
        want = {fwd: (key(1, 1000 + lead_f), m[fwd][1] - lead_f - trail_f), rev: (key(1, 1200 - m[rev][1] + trail_r), m[rev][1] - lead_r - trail_r)}
        for seg in (0, 1):
            assert (int(out[4 * seg]), int(out[4 * seg + 3])) == want[seg], (strand, seg)
        assert [int(out[1]), int(out[2]), int(out[5]), int(out[6])] == [5000, 111, 5111, 222]      # mate 1's record lies behind mate 0's
    L.bam_sort_trial_entries(1, 1000, 0, 0, mates, 0, 3, out.ctypes.data)
    assert [int(out[0]), int(out[3]), int(out[4]), int(out[7])] == [key(3, 0), 0, key(3, 0), 0]
    only_d = (TrialMate * 2)(TrialMate(0, 4, 4, 0, 50), TrialMate(9, 9, 0, 0, 60))      # a template part of D alone: no reference bases, the interval is one base
    L.bam_sort_trial_entries(0, 10, 50, 0, only_d, 0, 3, out.ctypes.data)
    assert (int(out[0]), int(out[3])) == (key(0, 14), 1)


def test_the_plan_covers_the_significant_bits_only(trial):
    assert trial_sort(trial, [], 1, 4_641_652)[2:] == (3, (23, 24))          # an E. coli-sized reference: 23 position bits and the bit of the unmapped records
    assert trial_sort(trial, [], 3, 5000)[2:] == (2, (13, 15))
    assert trial_sort(trial, [], 3, 140000)[2:] == (3, (18, 20))
    assert trial_sort(trial, [], 25, 1 << 29)[2:] == (5, (30, 35))


@pytest.mark.parametrize("name", ["none", "one", "no multiple of the tile", "all equal", "top digit only", "refID only", "random with unmapped"])
def test_sort_edge_cases(trial, name):
    rng = np.random.default_rng(5)
    tile = trial.bam_sort_trial_tile()
    n_seqs, longest = 3, 140000
    keys = {"none": [], "one": [key(1, 17)],
            "no multiple of the tile": [key(int(s), int(p)) for s, p in zip(rng.integers(0, 3, 2 * tile + 452), rng.integers(0, 140000, 2 * tile + 452))],
            "all equal": [key(2, 4242)] * (tile + 7),
            "top digit only": [key(int(s), 99) for s in rng.integers(0, 4, tile + 300)],        # 18 position bits: the sequence is all the third digit holds above 65536
            "refID only": [key(int(s), 65536 + 300) for s in rng.integers(0, 3, 3 * tile)],
            "random with unmapped": [key(3, 0) if u else key(int(s), int(p)) for u, s, p in zip(rng.random(5000) < 0.1, rng.integers(0, 3, 5000), rng.integers(0, 64, 5000))]}[name]
    order, out, passes, _ = trial_sort(trial, keys, n_seqs, longest)
    want = sorted(range(len(keys)), key=keys.__getitem__)          # Python's sort is stable: ties keep their order
    assert order == want and out == [keys[i] for i in want] and passes == 3
    if name in ("all equal",):
        assert order == list(range(len(keys)))


def test_cut_edge_cases(trial):
    L = trial
    # two sequences of three and two blocks (blocks are 1-based; the list has the entry behind the last block that the library's has)
    block_seq, first_block = np.array([0, 0, 0, 0, 1, 1, 0], np.uint32), np.array([1, 4], np.uint32)
    keys = sorted([key(0, 0), key(0, 999), key(0, 1000), key(0, 1000), key(0, 1001), key(0, 2999), key(1, 0), key(1, 5), key(1, 1000), key(2, 0), key(2, 0)])
    arr = np.array(keys, np.uint64)
    cut = C.c_uint64()
    final = lambda block: (L.bam_sort_trial_cut(arr.ctypes.data, len(keys), block, 5, 2, block_seq.ctypes.data, first_block.ctypes.data, 1000, C.byref(cut)), cut.value)
    assert final(1) == (0, key(0, 0))                              # nothing lies below the first block
    assert final(2) == (2, key(0, 1000))                           # key == cut goes to the held side
    assert final(3) == (5, key(0, 2000))
    assert final(4) == (6, key(1, 0))                              # a cut at a sequence's first block holds everything of that sequence
    assert final(5) == (8, key(1, 1000))
    assert final(6) == (9, key(2, 0))                              # past the last block every mapped record is final, the unmapped ones (refID n_seqs) stay held
    # the run-time guard: a mapped key below the cut of the call before, or a position the digits do not cover
    assert L.bam_sort_trial_out_of_order(key(0, 999), key(0, 1000), 2, 3000) == 1
    assert L.bam_sort_trial_out_of_order(key(0, 1000), key(0, 1000), 2, 3000) == 0
    assert L.bam_sort_trial_out_of_order(key(2, 0), key(1, 0), 2, 3000) == 0          # unmapped
    assert L.bam_sort_trial_out_of_order(key(1, 4096), key(1, 0), 2, 3000) == 1       # 3000 takes 12 bits


# ------------------------------------------------------------------------------------------------ the index
def crafted_file():
    """records of two sequences with bins of several levels, a sequence without records between them, and a block table of four blocks and the end-of-file member
    with a record that straddles a block's end and one that ends exactly at one"""
    spec = [(0, 100, 50), (0, 100, 30), (0, 16380, 10), (0, 16384, 40), (0, 16400, 1), (0, 131000, 100), (0, 131070, 10), (0, 131072, 5), (0, 200000, 150),
            (2, 5, 100), (2, 49000, 200), (2, 49100, 64), (2, 130000, 2000)]
    rng = np.random.default_rng(3)
    records = [dict(raw=bytes(int(rng.integers(100, 400))), ref_id=r, pos=p, span=s, bin=reg2bin(p, p + s), mapped=True) for r, p, s in spec]
    records += [dict(raw=bytes(150), ref_id=-1, pos=-1, span=0, bin=4680, mapped=False) for _ in range(3)]
    first = 321
    starts = np.concatenate([[first], first + np.cumsum([len(r["raw"]) for r in records])])
    # blocks: the header alone; up to the middle of record 2; up to exactly the end of record 6; the rest; the end-of-file member
    block_u = [0, first, int(starts[2]) + 57, int(starts[7]), int(starts[-1])]
    block_c = [0, 150, 150 + 400, 150 + 400 + 777, 150 + 400 + 777 + 901]
    return records, first, [int(x) for x in starts], block_u, block_c


def trial_index(L, records, starts, seq_len, call_end, block_u, block_c, n_no_coor):
    mapped = [r for r in records if r["mapped"]]
    keys = np.array([key(r["ref_id"], r["pos"]) for r in mapped], np.uint64)
    span = np.array([r["span"] for r in mapped], np.uint32)
    at = np.array(starts[:len(mapped) + 1], np.uint64)
    ends, lens = np.array(call_end, np.uint64), np.array(seq_len, np.uint32)
    u, c = np.array(block_u, np.uint64), np.array(block_c, np.uint64)
    buf = C.create_string_buffer(1 << 16)
    need = L.bam_sort_trial_index(len(seq_len), lens.ctypes.data, len(mapped), keys.ctypes.data, span.ctypes.data, at.ctypes.data, ends.ctypes.data, len(call_end), u.ctypes.data,
                                  c.ctypes.data, len(u), n_no_coor, buf, len(buf))
    assert need <= len(buf)
    return buf.raw[:need]


@pytest.mark.parametrize("calls", [[13], [1, 2, 5, 8, 9, 13], list(range(1, 14)), [0, 4, 4, 13]])
def test_the_index_equals_the_python_builder(trial, calls):
    """whatever the calls the records left in: runs that touch across two calls are one chunk"""
    records, first, starts, block_u, block_c = crafted_file()
    seq_len = [262144, 40000, 140000]
    assert {r["bin"] for r in records if r["mapped"]} >= {reg2bin(100, 150), reg2bin(16380, 16390), reg2bin(131070, 131080)}
    assert reg2bin(16380, 16390) == 585 and reg2bin(131070, 131080) == 73 and reg2bin(100, 150) == 4681      # across 16384, across 131072, a level-5 bin
    assert starts[2] < block_u[2] < starts[3] and block_u[3] == starts[7]                                   # one record straddles a block's end, one ends exactly at one
    want = build_bai(records, first, 3, block_u, block_c, 3)
    got = trial_index(trial, records, starts, seq_len, calls, block_u, block_c, 3)
    assert got == want
    index = parse_bai(got)
    assert index[1] == 3 and index[0][1] == ({}, [])               # a sequence without records: n_bin = 0, n_intv = 0
    assert len(index[0][0][1]) == (200000 + 149 >> 14) + 1 and len(index[0][2][1]) == (130000 + 1999 >> 14) + 1
    # the record that ends exactly at a block's end: its chunk ends at that block's successor, offset 0
    bin_of_6 = index[0][0][0][records[6]["bin"]]
    assert bin_of_6[-1][1] == block_c[3] << 16
    # an empty window between two populated ones takes the next one's value
    linear = index[0][2][1]
    assert linear[1] == linear[2] == virtual_offset(starts[10], block_u, block_c) and linear[0] == virtual_offset(starts[9], block_u, block_c)


def test_region_queries_through_the_index(trial):
    records, first, starts, block_u, block_c = crafted_file()
    index = parse_bai(trial_index(trial, records, starts, [262144, 40000, 140000], [5, 13], block_u, block_c, 3))
    by_voffset = {virtual_offset(starts[i], block_u, block_c): r for i, r in enumerate(records)}
    regions = [(0, 16000, 16500), (0, 130900, 131100), (0, 16390, 16395), (0, 0, 262144), (0, 120, 121), (0, 150, 16380), (0, 131077, 131078),
               (2, 20000, 40000), (2, 16384, 32768), (2, 0, 140000), (2, 131999, 132000), (1, 0, 40000), (0, 250000, 262144)]
    for ref, beg, end in regions:
        got = records_through_index(index, ref, beg, end, by_voffset)
        want = overlapping(records, ref, beg, end)
        assert [id(r) for r in got] == [id(r) for r in want], (ref, beg, end)
    assert overlapping(records, 0, 16000, 16500) and overlapping(records, 0, 130900, 131100) and not overlapping(records, 2, 20000, 40000) and not overlapping(records, 1, 0, 40000)


# ------------------------------------------------------------------------------------------------ the header and the symbols
def test_header_of_the_golden_reference():
    ref = api.Reference(os.path.join(GOLDEN, "reference-test.fa"))
    try:
        assert ref.bam_header_so(0) == ref.bam_header()
        plain, coordinate = decode_bam_header(ref.bam_header()), decode_bam_header(ref.bam_header_so(1))
        assert coordinate[1] == plain[1]                           # the sequences' names and lengths
        a, b = plain[0].split(b"\n"), coordinate[0].split(b"\n")
        assert a[0] == b"@HD\tVN:1.6\tSO:unsorted\tGO:query" and b[0] == b"@HD\tVN:1.6\tSO:coordinate" and a[1:] == b[1:]
        want = ref.bam_header_so(1)
        need = C.c_size_t(0)
        small = C.create_string_buffer(b"#" * (len(want) - 1), len(want) - 1)
        assert api.lib().rsq_ref_bam_header_so(ref.h, 1, small, len(want) - 1, C.byref(need)) == api.RSQ_ENOSPC
        assert need.value == len(want) and small.raw == b"#" * (len(want) - 1)
    finally:
        ref.close()


def test_abi_symbols():
    header = open(os.path.join(os.path.dirname(HERE), "include", "reseq_amd.h")).read()
    for name in ("rsq_ref_bam_header_so", "rsq_sim_bam_sorted_begin", "rsq_sim_pairs_bam_sorted", "rsq_sim_bam_sorted_flush", "rsq_sim_bam_sorted_index"):
        assert ("int %s(" % name) in header
        assert getattr(api.lib(), name).argtypes is not None
    for method in ("bam_sorted_begin", "pairs_bam_sorted", "pairs_bam_sorted_device", "bam_sorted_flush", "bam_sorted_flush_device", "bam_sorted_index"):
        assert callable(getattr(api.Simulator, method))
    assert callable(api.Reference.bam_header_so)
