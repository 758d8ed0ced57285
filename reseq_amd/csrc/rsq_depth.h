// rsq_depth.h -- truth depth: the per-base coverage of the simulated reads, accumulated on the device from the arrays the truth alignments are written from, and its
// bedGraph text (include/reseq_amd.h rsq_sim_depth_*; DESIGN.md 4.8 "Truth depth").
//
// The rule: depth[seq][p] = the number of MAPPED truth records (rsq_sam.h: the records rsq_sim_pairs_sam writes for the same pairs, in reference coordinates with
// variants) whose CIGAR has an M column on reference position p of sequence seq.  D, I, S and the D runs dropped at either end do not count (samtools depth's
// default); both mates of a pair count, overlapping mates add; unmapped records add nothing.  A depth sink is one more consumer of sam_cigar / sam_var_cigar: no
// alignment rule lives here.
//
// A run owns ONE array of uint32 DIFFERENCES, a word per reference base and one more per sequence: sequence s begins at word seq_base_off[s] + s, so the -1 behind a
// sequence's last base has a word of its own and never lands in the next sequence.  An M element at r of n bases adds +1 at r and -1 at r + n (modulo 2^32,
// counter_add of rsq_portable.h: an atomic without a result on the device).  Every sequence's differences sum to zero, so ONE inclusive prefix sum modulo 2^32 over
// the flat array, with no segment logic, turns it into depths in place; a sequence's extra word ends as 0.  The sums are integers: the result does not depend on
// the order of the additions, on how blocks are cut into calls or on any option.
//
//   depth_mate<VARIANTS>                                 per lane, host and device (tests/hostemu/depth_trial.cpp runs it on the CPU): one mate's M elements into the array
//   k_depth_add<VARIANTS>                                one lane per mate of a part, behind reads_stage
//   k_depth_tile_sums, k_depth_tiles, k_depth_apply      the prefix sum in the three-launch form of rsq_scan.h (tiles of 4096, 16-byte loads, shuffles inside a wave)
//   k_depth_ends, k_depth_run_ends, k_depth_line_sizes   a piece of bedGraph text: the runs that end in it, their line sizes
//   depth_line, k_depth_text                             the lines, through the wave's image (WaveImage, ImageSink: rsq_format.h)
#pragma once
#include "rsq_sam.h"

namespace rsq {

// What a mate's CIGAR elements come to in the array of differences.  element() gets them in ascending reference order from r = POS - 1 on (a reverse mate's CIGAR
// is replayed from its last op down: the same order).  An element outside the sequence -- the record's rules exclude it -- is counted in `bad`, never written.
struct DepthSink {
    uint32_t *diff;            // word 0 of the mate's sequence
    uint32_t r, len;           // the reference position of the next M or D element; the sequence's length
    uint32_t bad;
    RSQ_HD void element(char op, uint32_t n) {
        if (op == 'M') {
            if (r <= len && n <= len - r) {
                counter_add(diff + r, 1u);
                counter_add(diff + r + n, 0xFFFFFFFFu);
            } else ++bad;
        }
        if (op == 'M' || op == 'D') r += n;
    }
    RSQ_HD void ch(char) {}                                             // ("*": a mate without an element)
};

// One mate of a pair with a fragment.  VARIANTS: the record of rsq_sim_truth_variants (sam_var_walk places the mate and walks the columns only where a
// coordinate-moving entry is in reach: pad), else the plain one.  A plain mate (ReadMeta::plain, no such entry in reach) is one M element: two additions.
// Returns the elements that fell outside the sequence (0).
template <bool VARIANTS>
RSQ_HD uint32_t depth_mate(const DevSim &S, const Fragment &f, bool has_fv, const FragmentVar &fv, uint32_t seg, const WordColumn &ops, const ReadMeta &m, uint32_t *diff) {
    if (!f.len) return 0u;                                              // unmapped (flags 77 / 141)
    if (f.seq >= S.n_seqs) return 1u;
    DepthSink t{diff + S.seq_base_off[f.seq] + f.seq, 0u, S.seq_len[f.seq], 0u};
    const bool rev = seg != f.strand;
    if constexpr (VARIANTS) {
        uint32_t n_cigar;
        const SamVarMate e = sam_var_walk(S, true, f, has_fv, fv, seg, ops, m, n_cigar);
        t.r = e.pos;
        sam_var_cigar(S, f, ops, m, e, rev, t);
    } else {
        const SamMate w = sam_walk(ops, m);
        t.r = sam_mate_pos(f, seg, w);
        sam_cigar(ops, m, w, rev, t);
    }
    return t.bad;
}

// words of a run's array: a word per base, one per sequence, whole scan tiles (the prefix sum's kernels then have no edge)
constexpr uint32_t kDepthTile = 4096;
RSQ_HD uint64_t depth_words(uint64_t total_bases, uint32_t n_seqs) { return (total_bases + n_seqs + kDepthTile - 1u) / kDepthTile * kDepthTile; }

// "<name>\t<start>\t<end>\t<depth>\n": a bedGraph line, 0-based and half-open
template <class Sink>
RSQ_HD void depth_line(const NameTable &names, uint32_t seq, uint32_t start, uint32_t end, uint32_t depth, Sink &t) {
    t.str(names.names + names.name_ptr[seq], names.name_ptr[seq + 1] - names.name_ptr[seq]);
    t.ch('\t');
    t.num(start);
    t.ch('\t');
    t.num(end);
    t.ch('\t');
    t.num(depth);
    t.ch('\n');
}
RSQ_HD uint32_t depth_line_size(uint32_t name_len, uint32_t start, uint32_t end, uint32_t depth) { return name_len + 4u + digits_u32(start) + digits_u32(end) + digits_u32(depth); }
// the image of k_depth_text: 64 lines of a name and three numbers at their widest, whole 128 bytes, at most 32 KiB (longer lines go straight to memory)
constexpr uint32_t kDepthLines = 64, kDepthLdsMax = 32u * 1024u;
RSQ_HD uint32_t depth_lds_bytes(uint32_t name_len) {
    const uint64_t want = ((uint64_t)kDepthLines * (name_len + 34u) + 16u + 127u) & ~(uint64_t)127u;
    return (uint32_t)(want > kDepthLdsMax ? kDepthLdsMax : want);
}

#if RSQ_DEVICE_BUILD
// One lane per mate of a part: lane i < n_pairs is the mate of segment 0 in raw row i, lane n_pairs + i the other (the raw arrays' own order); perm: the rows
// are binned (row_order).  fvars: with variants of any kind.  bad: counts what fell outside its sequence.
template <bool VARIANTS>
__global__ void __launch_bounds__(256) k_depth_add(DevSim S, const Fragment *frags, const FragmentVar *fvars, uint64_t n_pairs, RawLayout raw, const uint32_t *perm, uint32_t *diff,
                                                   uint32_t *bad) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 2u * n_pairs) return;
    const uint32_t seg = r >= n_pairs ? 1u : 0u;
    const uint64_t row = r - seg * n_pairs, pair = perm ? perm[row] : row;
    const Fragment f = frags[pair];
    FragmentVar fv{};
    if (fvars) fv = fvars[pair];
    const uint32_t out = depth_mate<VARIANTS>(S, f, fvars != nullptr, fv, seg, raw.ops_of(r), raw.meta[r], diff);
    if (out) atomicAdd(bad, out);
}

// ------------------------------------------------------------------------------------------------ differences -> depths
// The inclusive prefix sum modulo 2^32 of the whole array in place, n_tiles whole tiles of kDepthTile words: a tile is a workgroup of 256, a wave's quarter of it
// four rounds of 256 words, in round k lane l holds the four words from 256 k + 4 l on (one 16-byte load and store).  Three launches, no workgroup waits for another.
constexpr uint32_t kDepthBlock = 256, kDepthRounds = kDepthTile / kDepthBlock / 4u, kDepthWaves = kDepthBlock / 64u, kDepthWaveSpan = kDepthTile / kDepthWaves;
__global__ void __launch_bounds__(kDepthBlock) k_depth_tile_sums(const uint32_t *a, uint32_t *tile_sums) {
    __shared__ uint32_t s_sum[kDepthWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kDepthTile + (uint64_t)wave * kDepthWaveSpan + 4u * lane;
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < kDepthRounds; ++k) {
        const uint4 v = *reinterpret_cast<const uint4 *>(a + base + 256u * k);
        acc += v.x + v.y + v.z + v.w;
    }
    for (uint32_t d = 32; d; d >>= 1) acc += (uint32_t)__shfl_xor((int)acc, (int)d, 64);
    if (0u == lane) s_sum[wave] = acc;
    __syncthreads();
    if (0u == threadIdx.x) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kDepthWaves; ++w) sum += s_sum[w];
        tile_sums[blockIdx.x] = sum;
    }
}
// one workgroup: every thread adds up a stretch of tiles, the stretches' sums are scanned in LDS, then every thread turns its stretch into exclusive prefixes
constexpr uint32_t kDepthTilesBlock = 1024;
__global__ void __launch_bounds__(kDepthTilesBlock) k_depth_tiles(uint32_t *tile_sums, uint32_t n_tiles) {
    __shared__ uint32_t s[kDepthTilesBlock];
    const uint32_t per = (n_tiles + kDepthTilesBlock - 1u) / kDepthTilesBlock, lo = min(threadIdx.x * per, n_tiles), hi = lo + per < n_tiles ? lo + per : n_tiles;
    uint32_t acc = 0;
    for (uint32_t i = lo; i < hi; ++i) acc += tile_sums[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t d = 1; d < kDepthTilesBlock; d <<= 1) {
        const uint32_t v = threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = s[threadIdx.x] - acc;                                // what lies in front of this thread's stretch
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t v = tile_sums[i];
        tile_sums[i] = run;
        run += v;
    }
}
__global__ void __launch_bounds__(kDepthBlock) k_depth_apply(uint32_t *a, const uint32_t *tile_sums) {
    __shared__ uint32_t s_wave[kDepthWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kDepthTile + (uint64_t)wave * kDepthWaveSpan + 4u * lane;
    uint4 v[kDepthRounds];
    uint32_t before[kDepthRounds], run = 0;                             // of the wave's span: what lies in front of this lane's four words of round k; the rounds before
#pragma unroll
    for (uint32_t k = 0; k < kDepthRounds; ++k) v[k] = *reinterpret_cast<const uint4 *>(a + base + 256u * k);
#pragma unroll
    for (uint32_t k = 0; k < kDepthRounds; ++k) {
        const uint32_t mine = v[k].x + v[k].y + v[k].z + v[k].w;
        uint32_t incl = mine;                                           // inclusive scan over the lanes
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += t;
        }
        before[k] = run + incl - mine;
        run += (uint32_t)__shfl((int)incl, 63, 64);                     // the round's sum, from the last lane
    }
    if (0u == lane) s_wave[wave] = run;
    __syncthreads();
    uint32_t front = tile_sums[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) front += s_wave[w];
#pragma unroll
    for (uint32_t k = 0; k < kDepthRounds; ++k) {
        uint4 o;
        o.x = front + before[k] + v[k].x;
        o.y = o.x + v[k].y;
        o.z = o.y + v[k].z;
        o.w = o.z + v[k].w;
        *reinterpret_cast<uint4 *>(a + base + 256u * k) = o;
    }
}

// ------------------------------------------------------------------------------------------------ bedGraph text of a piece [lo, lo + n) of one sequence
// d: word 0 of the sequence's depths.  A run ends at b when b is the sequence's length or d[b] != d[b - 1]; the piece holds the runs that end in (lo, lo + n]:
// flags[i] = 1 if one ends at lo + 1 + i (d[lo + n] is read from the array -- the sequence's extra word lies behind its last base --, so ends need no carry).
__global__ void __launch_bounds__(256) k_depth_ends(const uint32_t *d, uint32_t len, uint32_t lo, uint64_t n, uint32_t *flags) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = lo + 1u + (uint32_t)i;
    flags[i] = b == len || d[b] != d[b - 1u] ? 1u : 0u;
}
// ... compacted: ends[k] = where the piece's k-th run ends (rank: the exclusive scan of the flags)
__global__ void __launch_bounds__(256) k_depth_run_ends(const uint32_t *flags, const uint64_t *rank, uint32_t lo, uint64_t n, uint32_t *ends) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flags[i]) return;
    ends[rank[i]] = lo + 1u + (uint32_t)i;
}
// ... and their lines' sizes: run k begins where run k - 1 ends, the first at `carry` (the start of the run that was open at lo)
__global__ void __launch_bounds__(256) k_depth_line_sizes(const uint32_t *d, const uint32_t *ends, uint64_t n_lines, uint32_t carry, uint32_t name_len, uint32_t *sizes) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_lines) return;
    const uint32_t end = ends[k];
    sizes[k] = depth_line_size(name_len, k ? ends[k - 1u] : carry, end, d[end - 1u]);
}
// One wave per 64 consecutive lines, a lane a line, through the wave's image; offsets: the exclusive scan of the sizes.  The host has checked the capacity.
__global__ void __launch_bounds__(64) k_depth_text(NameTable names, uint32_t seq, const uint32_t *d, const uint32_t *ends, uint32_t carry, uint64_t n_lines, const uint64_t *offsets,
                                                  char *dst, uint32_t lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) char s_depth[];
    using Image = WaveImage<false, kDepthLines>;
    if (Image::first() >= n_lines) return;
    const Image im(offsets, n_lines, dst, lds_bytes, nullptr, threadIdx.x);
    uint32_t start = 0, end = 1, depth = 0;
    if (im.active) {
        end = ends[im.item];
        start = im.item ? ends[im.item - 1u] : carry;
        depth = d[end - 1u];
    }
    if (!im.through_lds) {                                              // names too long for the image: a lane writes its line straight to memory
        if (im.active) {
            WordSinkT<char *> t(dst + offsets[im.item]);
            depth_line(names, seq, start, end, depth, t);
            t.finish();
        }
        return;
    }
    im.clear(s_depth, lds_bytes);
    if (im.active) {
        ImageSink t(im.item_text(s_depth));
        depth_line(names, seq, start, end, depth, t);
        t.finish();
    }
    im.store_out(s_depth);
}
#endif

}  // namespace rsq
