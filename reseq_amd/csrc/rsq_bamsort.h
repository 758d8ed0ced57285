// rsq_bamsort.h -- the truth BAM sorted by coordinate on the device, and its .bai index (SAM specification 5.2).  The records are rsq_bam.h's, byte for byte:
// sorting permutes whole records.  The sorted stream is the mapped records stably sorted by (refID, pos), then the unmapped ones in their original order.
//
// Why a call can hand out part of the order before the run ends: block b of sequence i covers the start positions [(b - first_block[i]) * kBlockSize, + kBlockSize),
// a forward mate lies at start + dL, a reverse mate at start + len - t + dL with t <= len (the template part of a read is not longer than its fragment), so every
// record of a call over [block_lo, block_hi) and of every later call has a key >= cut(block_lo) = (block_seq[block_lo], (block_lo - first_block) * kBlockSize).
// The same holds for a reference with variants (BamVarFormat, reference coordinates): every base of a fragment's allele stretch stands at or behind the start
// position, and a position the allele deleted inside the stretch lies behind the base in front of it, so POS - 1 >= start for both mates.
// After sorting, what lies below cut(block_hi) is FINAL and goes to the caller; the rest is HELD for the next call -- the longest fragment times the coverage.
// k_bam_sort_keys counts records below the cut of the call before (and positions the sort's digits do not cover): such a call fails instead of writing a file
// that is silently unsorted.
//
// A call: k_truth_write<BamFormat> (or <BamVarFormat>) writes into a staging buffer [held records | this call's records in pair order]; k_bam_sort_keys appends a
// directory entry per record (key, staging offset, size, reference bases) from the side entries and sam_align (with variants: from the entries alone) -- no record is read again; held records keep
// theirs, in front, so that ties fall in the order of the unsorted stream.  The sort is an LSD radix sort of (key, index) pairs over the significant bits only
// (bits(n_seqs) + bits(longest sequence)), 8 bits a pass: k_bam_sort_hist (per-workgroup digit counts, digit-major), the library's exclusive scan, k_bam_sort_scatter
// (stable rank inside the workgroup from wave ballots and per-wave counters: no place is ever taken from the arrival order of an atomic).  k_bam_cut finds the final
// range, k_bam_gather -- the kernel that moves all the bytes -- copies every final record to its place in the caller's buffer and every held one to the front of
// the other staging buffer, k_bam_index_flags / k_bam_index_runs leave the index material: where (refID, bin) changes, and the smallest offset per 16 kb window.
//
// Host and device alike (tests/hostemu/bam_sort_trial.cpp runs them on the CPU): bam_sort_key, bam_sort_plan, bam_sort_digit, bam_dir_entry, bam_lower_bound,
// bam_sort_pass_host (a pass's tile / digit / rank arithmetic as a loop), BamIndexState and bam_bai_bytes (plain host code).
// tests/hostemu/kernel_trial.cpp runs the sort's passes (bam_sort_passes), the cut, the gather and the index kernels alone on crafted keys, entries and
// records (tests/test_kernel_trial_gpu.py): the ballot ranking and the byte funnel have no host form.
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "rsq_md.h"

namespace rsq {

struct BamDirEntry {
    uint64_t key;              // refID << 32 | pos; an unmapped record: n_seqs << 32
    uint64_t off;              // of the record in the staging buffer
    uint32_t size;             // its bytes, block_size field included
    uint32_t span;             // max(reference bases, 1): [pos, pos + span) is the interval bam_fixed takes the bin from; 0: unmapped
};
static_assert(sizeof(BamDirEntry) == 24, "the directory's entry");

constexpr uint32_t kBamSortBlock = 256, kBamSortWaves = 4, kBamSortRounds = 4, kBamSortTile = kBamSortBlock * kBamSortRounds, kBamSortBins = 256;
constexpr uint32_t kBamWindowShift = 14;                                 // the linear index: 16 kb windows
constexpr uint64_t kBamCutAll = ~0ull;                                   // the flush: everything is final
constexpr uint64_t kBamNoOffset = ~0ull;

RSQ_HD uint64_t bam_sort_key(uint32_t ref_id, uint32_t pos) { return ((uint64_t)ref_id << 32) | pos; }
RSQ_HD uint64_t bam_unmapped_key(uint32_t n_seqs) { return (uint64_t)n_seqs << 32; }      // above every mapped key
RSQ_HD uint32_t bam_bits(uint64_t v) {
    uint32_t n = 0;
    for (; v; v >>= 1) ++n;
    return n;
}
// the bits a run's keys differ in: the position's (values 0 .. longest) below the sequence's (values 0 .. n_seqs, the last the unmapped records')
struct BamSortPlan {
    uint32_t pos_bits, bits, passes;
};
RSQ_HD BamSortPlan bam_sort_plan(uint32_t n_seqs, uint32_t longest) {
    BamSortPlan p;
    p.pos_bits = bam_bits(longest);
    p.bits = p.pos_bits + bam_bits(n_seqs);
    p.passes = (p.bits + 7u) >> 3;
    return p;
}
RSQ_HD uint32_t bam_sort_digit(uint64_t key, uint32_t pass, uint32_t pos_bits) {
    const uint64_t packed = ((key >> 32) << pos_bits) | (key & 0xFFFFFFFFull);
    return (uint32_t)(packed >> (8u * pass)) & 0xFFu;
}
// the cut of a call that ends in front of `block`: blocks are 1-based, the block behind the last one has no start positions -- every mapped record is final
RSQ_HD uint64_t bam_cut_key(uint32_t block, uint32_t total_blocks, uint32_t n_seqs, const uint32_t *block_seq, const uint32_t *first_block, uint32_t block_size) {
    if (block > total_blocks) return bam_unmapped_key(n_seqs);
    const uint32_t seq = block_seq[block];
    return bam_sort_key(seq, (block - first_block[seq]) * block_size);
}
// a mate's directory entry from the fragment and both mates' side entries
RSQ_HD BamDirEntry bam_dir_entry(const Fragment &f, uint32_t seg, const BamPair &p, uint64_t pair_off, uint32_t n_seqs) {
    const SamAlign a = sam_align(true, f, seg, p.mate[0].w, p.mate[1].w);
    const BamMate &m = p.mate[seg];
    BamDirEntry e;
    const uint32_t span = (uint32_t)m.w.t - m.w.lead - m.w.trail;
    e.key = a.mapped ? bam_sort_key(f.seq, a.pos - 1u) : bam_unmapped_key(n_seqs);
    e.off = pair_off + (seg ? p.mate[0].w.bytes : 0u);
    e.size = m.w.bytes;
    e.span = a.mapped ? (span ? span : 1u) : 0u;
    return e;
}
// ... of a reference with variants (BamVarFormat): POS and the reference bases are the entry's
RSQ_HD BamDirEntry bam_dir_entry(const Fragment &f, uint32_t seg, const BamVarPair &p, uint64_t pair_off, uint32_t n_seqs) {
    const bool mapped = f.len != 0u;
    const SamVarMate &m = p.mate[seg].v;
    BamDirEntry e;
    e.key = mapped ? bam_sort_key(f.seq, m.pos) : bam_unmapped_key(n_seqs);
    e.off = pair_off + (seg ? p.mate[0].v.w.bytes : 0u);
    e.size = m.w.bytes;
    e.span = mapped ? (m.ref_bases ? m.ref_bases : 1u) : 0u;
    return e;
}
// ... of the formats with NM and MD (rsq_md.h): the entry's own part says it all, the record's bytes with the tags included
RSQ_HD BamDirEntry bam_dir_entry(const Fragment &f, uint32_t seg, const MdPair<BamMate> &p, uint64_t pair_off, uint32_t n_seqs) {
    return bam_dir_entry(f, seg, BamPair{{p.mate[0].b, p.mate[1].b}}, pair_off, n_seqs);
}
RSQ_HD BamDirEntry bam_dir_entry(const Fragment &f, uint32_t seg, const MdPair<BamVarMate> &p, uint64_t pair_off, uint32_t n_seqs) {
    return bam_dir_entry(f, seg, BamVarPair{{p.mate[0].b, p.mate[1].b}}, pair_off, n_seqs);
}
// what k_bam_sort_keys counts: a mapped record below the cut of the call before, or at a position the digits do not cover
RSQ_HD bool bam_key_out_of_order(uint64_t key, uint64_t prev_cut, uint32_t n_seqs, uint32_t pos_bits) {
    if (key >= bam_unmapped_key(n_seqs)) return false;
    return key < prev_cut || ((key & 0xFFFFFFFFull) >> pos_bits) != 0u;
}
// the first index whose key is >= cut: records with key == cut are held
RSQ_HD uint64_t bam_lower_bound(const uint64_t *keys, uint64_t n, uint64_t cut) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < cut) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
RSQ_HD uint32_t bam_first_window(const BamDirEntry &e) { return (uint32_t)(e.key & 0xFFFFFFFFull) >> kBamWindowShift; }
RSQ_HD uint32_t bam_last_window(const BamDirEntry &e) { return ((uint32_t)(e.key & 0xFFFFFFFFull) + e.span - 1u) >> kBamWindowShift; }
RSQ_HD uint32_t bam_entry_bin(const BamDirEntry &e) {
    const uint32_t pos = (uint32_t)(e.key & 0xFFFFFFFFull);
    return bam_reg2bin(pos, pos + e.span);
}

// One pass as the kernels run it, as a loop: per tile of kBamSortTile items the digits' counts (hist[digit * tiles + tile]), their exclusive scan in that order,
// and every item to scan[digit, tile] + its rank among the tile's earlier items of the same digit.  idx_in nullptr: the identity.
inline void bam_sort_pass_host(const uint64_t *keys_in, const uint32_t *idx_in, uint64_t n, uint32_t pass, uint32_t pos_bits, uint64_t *keys_out, uint32_t *idx_out) {
    const uint64_t tiles = (n + kBamSortTile - 1u) / kBamSortTile;
    std::vector<uint64_t> at(kBamSortBins * tiles + 1u, 0u);
    for (uint64_t i = 0; i < n; ++i) ++at[(uint64_t)bam_sort_digit(keys_in[i], pass, pos_bits) * tiles + i / kBamSortTile + 1u];
    for (uint64_t k = 1; k < at.size(); ++k) at[k] += at[k - 1u];
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t &place = at[(uint64_t)bam_sort_digit(keys_in[i], pass, pos_bits) * tiles + i / kBamSortTile];
        keys_out[place] = keys_in[i];
        idx_out[place] = idx_in ? idx_in[i] : (uint32_t)i;
        ++place;
    }
}
// the whole sort: order[k] = the index of the k-th record of the sorted stream; returns the sorted keys
inline std::vector<uint64_t> bam_sort_host(const uint64_t *keys, uint64_t n, const BamSortPlan &plan, std::vector<uint32_t> &order) {
    std::vector<uint64_t> a(keys, keys + n), b(n);
    std::vector<uint32_t> ia(n), ib(n);
    for (uint64_t i = 0; i < n; ++i) ia[i] = (uint32_t)i;
    for (uint32_t pass = 0; pass < plan.passes; ++pass) {
        bam_sort_pass_host(a.data(), ia.data(), n, pass, plan.pos_bits, b.data(), ib.data());
        a.swap(b);
        ia.swap(ib);
    }
    order = ia;
    return a;
}

// ------------------------------------------------------------------------------------------------ the index (host)
// A chunk run: records of one (refID, bin) that are consecutive in the file, [begin, end) in the uncompressed stream
struct BamRun {
    uint32_t ref_id, bin;
    uint64_t begin, end;
};
struct BamRunStart {                                                     // what the device leaves of a run: it ends where the next one begins
    uint32_t ref_id, bin;
    uint64_t begin;
};
struct BamIndexState {
    std::vector<BamRun> runs;                                            // in file order
    std::vector<uint64_t> window_first;                                  // [n_seqs + 1]: a sequence's first window in `windows`
    std::vector<uint64_t> windows;                                       // the smallest record offset per window (kBamNoOffset: none)
    void begin(const std::vector<uint32_t> &seq_len) {
        runs.clear();
        window_first.assign(1, 0);
        for (const uint32_t l : seq_len) window_first.push_back(window_first.back() + (l >> kBamWindowShift) + 1u);
        windows.assign(window_first.back(), kBamNoOffset);
    }
    // a call's runs; `end`: where its last one ends.  Runs that touch across two calls are one chunk.
    void add_runs(const BamRunStart *starts, size_t n, uint64_t end) {
        for (size_t k = 0; k < n; ++k) {
            const uint64_t run_end = k + 1u < n ? starts[k + 1u].begin : end;
            if (!runs.empty() && runs.back().ref_id == starts[k].ref_id && runs.back().bin == starts[k].bin && runs.back().end == starts[k].begin) runs.back().end = run_end;
            else runs.push_back(BamRun{starts[k].ref_id, starts[k].bin, starts[k].begin, run_end});
        }
    }
    void add_window(uint32_t ref_id, uint32_t window, uint64_t offset) {
        uint64_t &w = windows[window_first[ref_id] + window];
        if (offset < w) w = offset;
    }
};
// The file's BGZF block table: block k holds the uncompressed bytes [block_u[k], block_u[k + 1]) and begins at byte block_c[k] of the file; the end-of-file member
// is the last entry.  An offset at a block's first byte belongs to that block (what bgzf_tell says behind the last byte of the block in front of it).
// rsq_sim_bam_sorted_index has checked the table: it begins at 0, rises, no block holds more than 64 KiB, its last entry lies at or behind every offset.
inline uint64_t bam_virtual_offset(uint64_t u, const uint64_t *block_u, const uint64_t *block_c, size_t n_blocks) {
    const size_t k = (size_t)(std::upper_bound(block_u, block_u + n_blocks, u) - block_u) - 1u;
    return (block_c[k] << 16) | (u - block_u[k]);
}
// the bytes of the .bai: magic, n_ref; per sequence the bins (ascending; the metadata pseudo-bin 37450 is left out) with their chunks, n_intv and the linear index
// (a window no record overlaps takes the value of the next overlapped one); n_no_coor
inline std::string bam_bai_bytes(const BamIndexState &x, const uint64_t *block_u, const uint64_t *block_c, size_t n_blocks, uint64_t n_no_coor) {
    std::string out = "BAI\1";
    auto put32 = [&](uint32_t v) {
        for (int k = 0; k < 4; ++k) out += (char)((v >> (8 * k)) & 0xFFu);
    };
    auto put64 = [&](uint64_t v) {
        for (int k = 0; k < 8; ++k) out += (char)((v >> (8 * k)) & 0xFFu);
    };
    const uint32_t n_ref = (uint32_t)x.window_first.size() - 1u;
    std::vector<std::map<uint32_t, std::vector<const BamRun *>>> bins(n_ref);
    for (const BamRun &r : x.runs) bins[r.ref_id][r.bin].push_back(&r);
    put32(n_ref);
    for (uint32_t ref = 0; ref < n_ref; ++ref) {
        put32((uint32_t)bins[ref].size());
        for (const auto &b : bins[ref]) {
            put32(b.first);
            put32((uint32_t)b.second.size());
            for (const BamRun *r : b.second) {
                put64(bam_virtual_offset(r->begin, block_u, block_c, n_blocks));
                put64(bam_virtual_offset(r->end, block_u, block_c, n_blocks));
            }
        }
        const uint64_t *w = x.windows.data() + x.window_first[ref];
        uint32_t n_intv = (uint32_t)(x.window_first[ref + 1u] - x.window_first[ref]);
        while (n_intv && w[n_intv - 1u] == kBamNoOffset) --n_intv;
        put32(n_intv);
        std::vector<uint64_t> filled(w, w + n_intv);
        for (uint32_t k = n_intv; k-- > 0u;)
            if (filled[k] == kBamNoOffset) filled[k] = filled[k + 1u];
        for (const uint64_t v : filled) put64(bam_virtual_offset(v, block_u, block_c, n_blocks));
    }
    put64(n_no_coor);
    return out;
}

#if RSQ_DEVICE_BUILD
// One lane per raw row pair: both mates' directory entries, at dir[2 * pair + segment] (pair order, whatever the rows' order); counts what is out of order
template <class Pair>
__global__ void __launch_bounds__(256) k_bam_sort_keys(const Fragment *frags, uint64_t n_pairs, const uint32_t *perm, const Pair *side, const uint64_t *offsets, uint64_t stage_base,
                                                       BamDirEntry *dir, uint32_t n_seqs, uint64_t prev_cut, uint32_t pos_bits, uint32_t *out_of_order) {
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_pairs) return;
    const uint64_t pair = perm ? perm[row] : row;
    const Fragment f = frags[pair];
    const Pair p = side[row];
    const uint64_t at = stage_base + offsets[pair];
    uint32_t bad = 0;
    for (uint32_t seg = 0; seg < 2u; ++seg) {
        const BamDirEntry e = bam_dir_entry(f, seg, p, at, n_seqs);
        dir[2u * pair + seg] = e;
        bad += bam_key_out_of_order(e.key, prev_cut, n_seqs, pos_bits) ? 1u : 0u;
    }
    if (bad) atomicAdd(out_of_order, bad);                               // (a count: no order is taken from it)
}

__global__ void __launch_bounds__(256) k_bam_sort_init(const BamDirEntry *dir, uint64_t n, uint64_t *keys, uint32_t *idx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = dir[i].key;
    idx[i] = (uint32_t)i;
}
// a workgroup per tile: its digits' counts to hist[digit * tiles + tile]
__global__ void __launch_bounds__(kBamSortBlock) k_bam_sort_hist(const uint64_t *keys, uint64_t n, uint32_t pass, uint32_t pos_bits, uint32_t *hist) {
    __shared__ uint32_t s_count[kBamSortBins];
    s_count[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * kBamSortTile;
    for (uint32_t r = 0; r < kBamSortRounds; ++r) {
        const uint64_t i = first + r * kBamSortBlock + threadIdx.x;
        if (i < n) atomicAdd(&s_count[bam_sort_digit(keys[i], pass, pos_bits)], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = s_count[threadIdx.x];
}
// a workgroup per tile; wave w holds the tile's items [256 w, 256 w + 256), 64 a round.  An item's rank among the tile's earlier items of its digit = those of
// the waves in front (s_count rows, complete after the barrier) + those of its own wave's earlier rounds (the row's count when the round begins) + those of
// the lanes in front of it in its round (the ballot of the lanes with the same digit).
__global__ void __launch_bounds__(kBamSortBlock) k_bam_sort_scatter(const uint64_t *keys, const uint32_t *idx, uint64_t n, uint32_t pass, uint32_t pos_bits, const uint64_t *hist_at,
                                                                    uint64_t *keys_out, uint32_t *idx_out) {
    __shared__ uint32_t s_count[kBamSortWaves][kBamSortBins];
    for (uint32_t w = 0; w < kBamSortWaves; ++w) s_count[w][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t first = (uint64_t)blockIdx.x * kBamSortTile + wave * (kBamSortRounds * 64u);
    uint64_t key[kBamSortRounds];
    uint32_t digit[kBamSortRounds], rank[kBamSortRounds];
#pragma unroll
    for (uint32_t r = 0; r < kBamSortRounds; ++r) {
        const uint64_t i = first + r * 64u + lane;
        const bool valid = i < n;
        key[r] = valid ? keys[i] : 0u;
        digit[r] = bam_sort_digit(key[r], pass, pos_bits);
        uint64_t same = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8u; ++b) {
            const bool bit = (digit[r] >> b) & 1u;
            const uint64_t set = __ballot(valid && bit);
            same &= bit ? set : ~set;
        }
        const uint32_t in_front = __popcll(same & ((1ull << lane) - 1ull));
        const uint32_t before = valid ? s_count[wave][digit[r]] : 0u;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");           // every lane has read the row before the digit's first lane moves it on ...
        __builtin_amdgcn_wave_barrier();
        if (valid && in_front == 0u) s_count[wave][digit[r]] = before + (uint32_t)__popcll(same);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");           // ... and the next round reads what it wrote
        __builtin_amdgcn_wave_barrier();
        rank[r] = before + in_front;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kBamSortRounds; ++r) {
        const uint64_t i = first + r * 64u + lane;
        if (i >= n) continue;
        uint32_t in_tile = rank[r];
        for (uint32_t w = 0; w < wave; ++w) in_tile += s_count[w][digit[r]];
        const uint64_t place = hist_at[(uint64_t)digit[r] * gridDim.x + blockIdx.x] + in_tile;
        keys_out[place] = key[r];
        idx_out[place] = idx[i];
    }
}
// The passes of the sort: per pass the tiles' digit counts, their exclusive scan (scan(hist, tiles * kBamSortBins, hist_at): the library's, on the same stream) and
// the scatter into the other pair of buffers.  keys[0] / idx[0] hold the input, hist has tiles * kBamSortBins words and hist_at one more, with
// tiles = ceil(n / kBamSortTile); n >= 1.  Returns which pair of buffers the sorted items lie in.
template <class Scan>
inline int bam_sort_passes(uint64_t *const keys[2], uint32_t *const idx[2], uint64_t n, const BamSortPlan &plan, uint32_t *hist, uint64_t *hist_at, Scan &&scan, hipStream_t st) {
    const uint32_t tiles = (uint32_t)((n + kBamSortTile - 1u) / kBamSortTile);
    int from = 0;
    for (uint32_t pass = 0; pass < plan.passes; ++pass, from ^= 1) {
        hipLaunchKernelGGL(k_bam_sort_hist, dim3(tiles), dim3(kBamSortBlock), 0, st, (const uint64_t *)keys[from], n, pass, plan.pos_bits, hist);
        scan((const uint32_t *)hist, (uint64_t)tiles * kBamSortBins, hist_at);
        hipLaunchKernelGGL(k_bam_sort_scatter, dim3(tiles), dim3(kBamSortBlock), 0, st, (const uint64_t *)keys[from], (const uint32_t *)idx[from], n, pass, plan.pos_bits,
                           (const uint64_t *)hist_at, keys[from ^ 1], idx[from ^ 1]);
    }
    return from;
}
// the records' sizes in sorted order (their scan gives every record its place)
__global__ void __launch_bounds__(256) k_bam_sorted_sizes(const BamDirEntry *dir, const uint32_t *idx, uint64_t n, uint32_t *sizes) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sizes[i] = dir[idx[i]].size;
}
// result: {final records, the mapped among them, bytes of the final records, bytes of the mapped among them, bytes of all, records out of order}
__global__ void k_bam_cut(const uint64_t *keys, uint64_t n, uint64_t cut, uint64_t unmapped_key, const uint64_t *at, const uint32_t *out_of_order, uint64_t *result) {
    const uint64_t n_final = cut == kBamCutAll ? n : bam_lower_bound(keys, n, cut), n_mapped = bam_lower_bound(keys, n_final, unmapped_key);
    result[0] = n_final;
    result[1] = n_mapped;
    result[2] = at[n_final];
    result[3] = at[n_mapped];
    result[4] = at[n];
    result[5] = *out_of_order;
}

// The kernel that moves the bytes.  Sixteen lanes a record (100 - 400 bytes, any alignment at both ends): a lane stores aligned 16-byte words of the destination,
// each fed from the two neighbouring aligned 16-byte words of the source through the byte funnel (align_bytes: v_alignbyte_b32); the ragged bytes in front of
// the first and behind the last aligned word are written one a lane.  Every byte of the destination is written by exactly one lane.  The source's second word
// may lie behind the record: the staging buffers end with 32 spare bytes.
__device__ __forceinline__ void bam_copy_record(char *dst, const char *src, uint32_t size, uint32_t lane) {
    const uintptr_t b = (uintptr_t)dst, end = b + size;
    uintptr_t head_end = (b + 15u) & ~(uintptr_t)15u;
    if (head_end > end) head_end = end;
    uintptr_t tail_at = end & ~(uintptr_t)15u;
    if (tail_at < head_end) tail_at = head_end;
    if (b + lane < head_end) dst[lane] = src[lane];
    if (tail_at + lane < end) dst[tail_at - b + lane] = src[tail_at - b + lane];
    for (uintptr_t a = head_end + 16u * lane; a < tail_at; a += 256u) {
        const uintptr_t s = (uintptr_t)src + (a - b);
        const uint4 *w = reinterpret_cast<const uint4 *>(s & ~(uintptr_t)15u);
        const uint4 lo = w[0], hi = w[1];
        const uint32_t q = (uint32_t)(s & 15u) >> 2, r = (uint32_t)s & 3u;
        const uint32_t e0 = q == 0u ? lo.x : q == 1u ? lo.y : q == 2u ? lo.z : lo.w, e1 = q == 0u ? lo.y : q == 1u ? lo.z : q == 2u ? lo.w : hi.x,
                       e2 = q == 0u ? lo.z : q == 1u ? lo.w : q == 2u ? hi.x : hi.y, e3 = q == 0u ? lo.w : q == 1u ? hi.x : q == 2u ? hi.y : hi.z,
                       e4 = q == 0u ? hi.x : q == 1u ? hi.y : q == 2u ? hi.z : hi.w;
        uint4 o;
        o.x = align_bytes(e1, e0, r);
        o.y = align_bytes(e2, e1, r);
        o.z = align_bytes(e3, e2, r);
        o.w = align_bytes(e4, e3, r);
        *reinterpret_cast<uint4 *>(a) = o;
    }
}
// record i of the sorted order: final (i < n_final) to out + at[i], held to the front of the other staging buffer, with its directory entry for the next call
__global__ void __launch_bounds__(256) k_bam_gather(const BamDirEntry *dir, const uint32_t *idx, const uint64_t *at, uint64_t n, uint64_t n_final, const char *stage, char *out, char *held,
                                                    BamDirEntry *held_dir) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t lane = threadIdx.x & 15u;
    if (i >= n) return;
    const BamDirEntry e = dir[idx[i]];
    const bool final = i < n_final;
    const uint64_t to = final ? at[i] : at[i] - at[n_final];
    if (!final && lane == 0u) held_dir[i - n_final] = BamDirEntry{e.key, to, e.size, e.span};
    bam_copy_record((final ? out : held) + to, stage + e.off, e.size, lane);
}

// index material over the mapped final records in sorted order: flags[i] = record i begins a run of its (refID, bin); the smallest offset per window it overlaps
// (a minimum: the same whatever the order of the atomics)
__global__ void __launch_bounds__(256) k_bam_index_flags(const BamDirEntry *dir, const uint32_t *idx, const uint64_t *at, uint64_t n_mapped, uint64_t stream_at, const uint64_t *window_first,
                                                         unsigned long long *windows, uint32_t *flags) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_mapped) return;
    const BamDirEntry e = dir[idx[i]];
    // Positions rise with i inside a sequence, so the first record that overlaps a window is the first whose last window reaches it: a record need only offer
    // itself to the windows behind its predecessor's last one -- a handful of atomics per window instead of one per record
    uint32_t flag = 1u, from = bam_first_window(e);
    if (i) {
        const BamDirEntry p = dir[idx[i - 1u]];
        const bool same_seq = (p.key >> 32) == (e.key >> 32);
        flag = !same_seq || bam_entry_bin(p) != bam_entry_bin(e) ? 1u : 0u;
        if (same_seq && bam_last_window(p) + 1u > from) from = bam_last_window(p) + 1u;
    }
    flags[i] = flag;
    const uint64_t offset = stream_at + at[i], first = window_first[e.key >> 32];
    const uint64_t n_windows = window_first[(e.key >> 32) + 1u] - first;
    for (uint32_t w = from; w <= bam_last_window(e) && w < n_windows; ++w) atomicMin(&windows[first + w], (unsigned long long)offset);
}
__global__ void __launch_bounds__(256) k_bam_index_runs(const BamDirEntry *dir, const uint32_t *idx, const uint64_t *at, uint64_t n_mapped, uint64_t stream_at, const uint32_t *flags,
                                                        const uint64_t *run_of, BamRunStart *runs) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_mapped || !flags[i]) return;
    const BamDirEntry e = dir[idx[i]];
    runs[run_of[i]] = BamRunStart{(uint32_t)(e.key >> 32), bam_entry_bin(e), stream_at + at[i]};
}
#endif

}  // namespace rsq
