// rsq_stats.h -- the simulation report: exact integer histograms of what a run of pairs calls simulated, accumulated on the device from the arrays the FASTQ text
// and the truth alignments are written from (include/reseq_amd.h rsq_sim_stats_*; DESIGN.md 4.9 "Simulation report").  A second consumer of a call's kept part
// beside rsq_depth.h: one pass over the raw rows (k_stats_rows), one lane per mate for everything else (k_stats_mates).
//
// The tables (StatsLayout; all uint64, segment s = template segment = file s + 1, a cycle = the 0-based position in the read as the FASTQ line has it):
//   per run      pairs[2] (with a fragment, adapter-only), strand[2], tile[T], fragment_length[F + 1] (the last three over pairs with a fragment)
//   per segment  read_length[L + 1], errors_per_read[L + 1] (min(num_errors, L_s)), base_quality[L][Q], base_call[L][5],
//                insertion[L], deletion[L], adapter[L], tail[L] (the id's own CIGAR, StatsCigar), mismatch[L] (MD's rule, StatsMismatch)
//   bad          a quality outside [0, Q), a base code outside the five, an element outside its sequence: counted here, never filed anywhere else
// L = the larger of the two segments' longest read length (a segment's own L_s bounds what is counted for it), F = insert_to, Q = one more than the largest
// quality value of the profile's quality tables, T = n_tiles.
//
// Every count is a sum of ones (deletion: of lengths), so the result does not depend on the order of the additions, on how blocks are cut into calls or on any
// option.  Counting goes through 32-bit histograms in LDS that a workgroup adds to the run's array once, at its end, with 64-bit atomics whose result nobody reads:
// no lane ever issues a global atomic on a counter most lanes share.
//
//   stats_row_word, stats_row_lane     per lane, host and device (tests/hostemu/stats_trial.cpp loops them on the CPU): a read's words of one chunk of positions
//   StatsCigar, StatsMismatch          the sinks of cigar_replay and of MD's column walkers
//   stats_mate<VARIANTS>               per lane, host and device: everything one mate adds but its bases and qualities
//   k_stats_rows<SKEW>, k_stats_mates<VARIANTS>
#pragma once
#include "rsq_md.h"

namespace rsq {

// the table ids: RSQ_STATS_* of include/reseq_amd.h (rsq_sim.hip asserts that the two agree)
enum StatsTable : uint32_t {
    kStPairs, kStStrand, kStTile, kStFragmentLength, kStReadLength, kStErrorsPerRead, kStBaseQuality, kStBaseCall, kStInsertion, kStDeletion, kStAdapter, kStTail,
    kStMismatch, kStBad, kStTables
};

// Where the tables lie in the run's array of counters, in words.  The tables of k_stats_mates come first -- words [0, image_words) ARE its LDS image, index for
// index --: fragment_length is the last of them and part of the image only when all of it fits the budget (frag_in_image), else its counts go to memory one atomic
// each (fragment lengths spread over hundreds of values: no counter is shared by most lanes).  base_quality and base_call, k_stats_rows' own, lie behind.
struct StatsLayout {
    uint32_t len[2], lmax, F, Q, T, phred;
    uint32_t off[kStTables];
    uint32_t image_words, frag_in_image, words;
    RSQ_HD uint32_t segments(uint32_t t) const { return t >= kStReadLength && t <= kStMismatch ? 2u : 1u; }
    RSQ_HD uint32_t dim0(uint32_t t) const {
        return t == kStPairs || t == kStStrand ? 2u : t == kStTile ? T : t == kStFragmentLength ? F + 1u : t == kStReadLength || t == kStErrorsPerRead ? lmax + 1u : t == kStBad ? 1u : lmax;
    }
    RSQ_HD uint32_t dim1(uint32_t t) const { return t == kStBaseQuality ? Q : t == kStBaseCall ? 5u : 1u; }
    RSQ_HD uint32_t table_words(uint32_t t) const { return segments(t) * dim0(t) * dim1(t); }
    RSQ_HD uint32_t at(uint32_t t, uint32_t seg, uint32_t i) const { return off[t] + seg * dim0(t) + i; }      // a table of one dimension
};
constexpr uint32_t kStatsMatesLds = 48u * 1024u;                        // the most LDS k_stats_mates' image may take
RSQ_HD StatsLayout stats_layout(uint32_t len0, uint32_t len1, uint32_t F, uint32_t Q, uint32_t T, uint32_t phred, uint32_t mates_lds_bytes = kStatsMatesLds) {
    StatsLayout y{};
    y.len[0] = len0;
    y.len[1] = len1;
    y.lmax = len0 > len1 ? len0 : len1;
    y.F = F;
    y.Q = Q;
    y.T = T;
    y.phred = phred;
    const uint32_t order[kStTables] = {kStPairs, kStStrand, kStTile, kStReadLength, kStErrorsPerRead, kStInsertion, kStDeletion, kStAdapter, kStTail, kStMismatch, kStBad,
                                       kStFragmentLength, kStBaseQuality, kStBaseCall};
    uint32_t at = 0;
    for (uint32_t k = 0; k < kStTables; ++k) {
        const uint32_t t = order[k];
        if (t == kStFragmentLength) {
            y.frag_in_image = (uint64_t)(at + y.table_words(t)) * 4u <= mates_lds_bytes ? 1u : 0u;
            if (!y.frag_in_image) y.image_words = at;
        }
        y.off[t] = at;
        at += y.table_words(t);
        if (t == kStFragmentLength && y.frag_in_image) y.image_words = at;
    }
    y.words = at;
    return y;
}

// ------------------------------------------------------------------------------------------------ the rows: base_quality and base_call
// k_stats_rows' LDS image of a chunk of positions: [position of the chunk][row_stride] 32-bit counters, a position's Q quality counters and its five base-call
// counters behind them.  The stride is odd: the rows of neighbouring positions -- what the lanes of a wave add to at once, see the kernel -- start in different banks.
RSQ_HD uint32_t stats_row_stride(uint32_t Q) { return (Q + 5u) | 1u; }

// One word of a read's seq row and the same word of its qual row: the first n (1..4) of its four bytes are the read's, `row` is the image index of the first
// byte's position.  add(i) adds one to counter i of the image.  Returns what was out of range (nothing is added for it).
template <class Add>
RSQ_HD uint32_t stats_row_word(uint32_t seq_w, uint32_t qual_w, uint32_t row, uint32_t n, uint32_t Q, uint32_t stride, uint32_t phred, Add &add) {
    uint32_t bad = 0;
    RSQ_UNROLL
    for (uint32_t b = 0; b < 4u; ++b) {
        if (b >= n) break;
        const uint32_t q = ((qual_w >> (8u * b)) & 0xFFu) - phred, c = (seq_w >> (8u * b)) & 0xFFu;       // (a character below the offset wraps to a huge value)
        if (q < Q) add(row + b * stride + q);
        else ++bad;
        if (c < 5u) add(row + b * stride + Q + c);
        else ++bad;
    }
    return bad;
}
// One read's part in a chunk: the chunk holds the positions of the row words [w_lo, w_lo + w_n); src.seq(j) / src.qual(j) are word w_lo + j of the read's rows
// (asked for only where 4 (w_lo + j) < read_len: what lies in the words behind a read's last base is whatever the read kernel left).  The words are taken in the
// order skew, skew + 1, ... modulo w_n (skew < w_n): the lanes of a wave, each with another skew, then add to different positions' rows at any one time.
template <class Src, class Add>
RSQ_HD uint32_t stats_row_lane(const Src &src, uint32_t read_len, uint32_t w_lo, uint32_t w_n, uint32_t skew, uint32_t Q, uint32_t stride, uint32_t phred, Add &add) {
    uint32_t bad = 0;
    for (uint32_t k = 0, j = skew; k < w_n; ++k, j = j + 1u == w_n ? 0u : j + 1u) {
        const uint32_t p = 4u * (w_lo + j);
        if (p >= read_len) continue;
        const uint32_t left = read_len - p;
        bad += stats_row_word(src.seq(j), src.qual(j), 4u * j * stride, left < 4u ? left : 4u, Q, stride, phred, add);
    }
    return bad;
}
// the chunks of a segment's positions: `chunk` (a multiple of four) positions each, the last one what is left
RSQ_HD uint32_t stats_chunks(uint32_t len, uint32_t chunk) { return (len + chunk - 1u) / chunk; }

// ------------------------------------------------------------------------------------------------ the mates: everything else
// A: the counters of k_stats_mates -- add(i, v) adds v to counter i of the run's array (through the workgroup's image where i lies in it), shared(i, on) adds one
// where `on` holds and is called by all lanes of a wave together: for the counters most lanes share, the device adds a wave's equal indices once.

// The id's own CIGAR (cigar_replay; the XC tag) in read orientation, all parts: M moves on, I, S and H mark their cycles, D adds its length at the cycle it
// stands in front of (the read's last where nothing follows).
template <class A>
struct StatsCigar {
    A &a;
    const StatsLayout &y;
    uint32_t seg, L;
    uint32_t q = 0, bad = 0;
    RSQ_HD void span(uint32_t table, uint32_t n) {
        if (q <= L && n <= L - q) {
            for (uint32_t i = 0; i < n; ++i) a.add(y.at(table, seg, q + i), 1u);
        } else ++bad;
        q += n;
    }
    RSQ_HD void element(char op, uint32_t n) {
        if (op == 'M') q += n;
        else if (op == 'I') span(kStInsertion, n);
        else if (op == 'S') span(kStAdapter, n);
        else if (op == 'H') span(kStTail, n);
        else if (op == 'D' && n) {
            if (L) a.add(y.at(kStDeletion, seg, q < L ? q : L - 1u), n);
            else ++bad;
        }
    }
};
// The sink of MdCols (rsq_md.h) that takes no text: mismatch(q) is called with the place in SEQ as written of every M column whose base differs from the reference
template <class A>
struct StatsMismatch {
    A &a;
    const StatsLayout &y;
    uint32_t seg, L, read_len;
    bool reverse;
    uint32_t bad = 0;
    RSQ_HD void mismatch(uint32_t q) {
        const uint32_t cycle = reverse ? read_len - 1u - q : q;
        if (q < read_len && cycle < L) a.add(y.at(kStMismatch, seg, cycle), 1u);
        else ++bad;
    }
    RSQ_HD void num(uint32_t) {}
    RSQ_HD void ch(char) {}
    RSQ_HD void bytes(uint32_t, uint32_t) {}
    RSQ_HD void element(char, uint32_t) {}
};

// One mate (live: the lane has one).  The per-pair tables are counted by the mate of segment 0.  VARIANTS: the mapped record's columns are those of
// rsq_sim_truth_variants (reference coordinates, whatever coordinates the truth calls write), else the plain ones.  Returns what was out of range.
template <bool VARIANTS, class A>
RSQ_HD uint32_t stats_mate(const DevSim &S, const StatsLayout &y, bool live, const Fragment &f, bool has_fv, const FragmentVar &fv, uint32_t seg, const WordColumn &seq,
                           const WordColumn &ops, const ReadMeta &m, A &a) {
    const uint32_t L = y.len[seg];
    const bool first = live && seg == 0u, mapped = live && f.len != 0u;
    uint32_t bad = 0;
    a.shared(y.at(kStPairs, 0u, f.len ? 0u : 1u), first);
    a.shared(y.at(kStStrand, 0u, f.strand ? 1u : 0u), first && mapped);
    a.shared(y.at(kStTile, 0u, m.tile_id), first && mapped && m.tile_id < y.T);
    a.shared(y.at(kStReadLength, seg, m.read_len), live && m.read_len <= L);
    a.shared(y.at(kStErrorsPerRead, seg, m.num_errors < L ? m.num_errors : L), live);
    if (!live) return 0u;
    bad += m.read_len > L;
    if (first && mapped) {
        bad += m.tile_id >= y.T;
        if (f.len <= y.F) a.add(y.at(kStFragmentLength, 0u, f.len), 1u);
        else ++bad;
    }
    StatsCigar<A> c{a, y, seg, L};
    cigar_replay(ops, m, c);
    bad += c.bad;
    if (mapped && f.seq < S.n_seqs) {
        SamAlign al{};
        al.mapped = 1u;
        al.reverse = seg != f.strand ? 1u : 0u;
        StatsMismatch<A> o{a, y, seg, L, m.read_len, al.reverse != 0u};
        if constexpr (VARIANTS) {
            uint32_t n_cigar;
            const SamVarMate e = sam_var_walk(S, true, f, has_fv, fv, seg, ops, m, n_cigar);
            al.pos = e.pos + 1u;
            md_walk(S, f, m, seq, ops, e.w, &e, al, o);
        } else {
            const SamMate w = sam_walk(ops, m);
            al.pos = sam_mate_pos(f, seg, w) + 1u;
            md_walk(S, f, m, seq, ops, w, nullptr, al, o);
        }
        bad += o.bad;
    } else if (mapped) ++bad;
    return bad;
}

// What a workgroup of k_stats_rows is given.  A unit is (segment, chunk of positions): the units of segment 0, then those of segment 1.  Workgroup g of G takes
// unit g % n_units and, of its slabs of `slab` reads, every K-th from g / n_units on -- K the workgroups that share the unit --; with fewer workgroups than units
// it goes on with unit g + G, g + 2 G, ... and all their slabs.  The image is flushed whenever the unit changes and at the end.
struct StatsRowsPlan {
    uint32_t chunk, slab, units[2];     // positions per chunk (a multiple of 4); reads per slab; chunks per segment
    uint32_t row_words;                 // words of a raw row: no read is longer than 4 row_words bases
};
constexpr uint32_t kStatsRowsBlock = 256, kStatsRowsWaves = kStatsRowsBlock / 64u;
// LDS of k_stats_rows: the image, then per wave the staged words [seq | qual][word of the chunk][lane] (SKEW)
RSQ_HD uint32_t stats_rows_lds_bytes(uint32_t chunk, uint32_t Q, bool skew) {
    return (chunk * stats_row_stride(Q) + (skew ? kStatsRowsWaves * 2u * (chunk / 4u) * 64u : 0u)) * 4u;
}
// The rows kernel's geometry for a call of n_pairs pairs on n_cu compute units: the chunk is the largest multiple of four positions, 64 at the most, whose image
// and staged words fit 48 KB of LDS -- four workgroups a CU --, evened out over the longer segment's chunks (150 cycles: three chunks of 52, not 64 + 64 + 22);
// the grid is persistent, four workgroups a CU and never fewer than there are units while that many are resident, and no workgroup without a slab.  The options
// (> 0) replace the three: opt_chunk (rounded up to a multiple of four), opt_slab, opt_groups.  lds: what the launch asks for (the caller refuses more than the
// device has).  tests/hostemu/stats_trial.cpp exports it, tests/hostemu/kernel_trial.cpp launches by it.
constexpr uint32_t kStatsRowsLds = 48u * 1024u;
struct StatsRowsGeometry {
    StatsRowsPlan plan;
    uint32_t lds, groups;
};
RSQ_HD StatsRowsGeometry stats_rows_geometry(uint32_t lmax, uint32_t len0, uint32_t len1, uint32_t Q, bool skew, uint32_t row_words, uint32_t n_cu, uint64_t n_pairs, int64_t opt_chunk,
                                             int64_t opt_slab, int64_t opt_groups) {
    uint32_t chunk = 64u;
    if (opt_chunk > 0) {
        const int64_t c = (opt_chunk + 3) / 4 * 4;
        chunk = (uint32_t)(c < 1024 ? c : 1024);
    } else {
        while (chunk > 4u && stats_rows_lds_bytes(chunk, Q, skew) > kStatsRowsLds) chunk -= 4u;
        const uint32_t n = lmax ? stats_chunks(lmax, chunk) : 1u, even =((lmax + n - 1u) / n + 3u) / 4u * 4u;
        if (even && even < chunk) chunk = even;                          // (lmax 0: no unit, the chunk is never used)
    }
    StatsRowsGeometry g{};
    g.lds = stats_rows_lds_bytes(chunk, Q, skew);
    g.plan = StatsRowsPlan{chunk, opt_slab > 0 ? (uint32_t)(opt_slab < (1 << 30) ? opt_slab : (1 << 30)) : 1024u, {stats_chunks(len0, chunk), stats_chunks(len1, chunk)}, row_words};
    const uint32_t units = g.plan.units[0] + g.plan.units[1];
    if (opt_groups > 0) g.groups = (uint32_t)(opt_groups < (1 << 16) ? opt_groups : (1 << 16));
    else {
        const uint32_t few = units < 8u * n_cu ? units : 8u * n_cu;
        g.groups = 4u * n_cu > few ? 4u * n_cu : few;
        const uint64_t slabs = (n_pairs + g.plan.slab - 1u) / g.plan.slab, most = (uint64_t)units * (slabs > 1u ? slabs : 1u);
        if (g.groups > most) g.groups = (uint32_t)most;
    }
    return g;
}

#if RSQ_DEVICE_BUILD
// a 64-bit counter of the run's array: an atomic without a result
__device__ __forceinline__ void stats_flush_add(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
struct StatsLdsAdd {                                                    // k_stats_rows' image
    uint32_t *image;
    __device__ __forceinline__ void operator()(uint32_t i) const { (void)__hip_atomic_fetch_add(image + i, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

// where stats_row_lane finds a read's words: staged by the wave ([seq | qual][word of the chunk][lane]), or in the rows themselves
struct StatsTileSrc {
    const uint32_t *t;
    uint32_t w_n, lane;
    __device__ __forceinline__ uint32_t seq(uint32_t j) const { return t[j * 64u + lane]; }
    __device__ __forceinline__ uint32_t qual(uint32_t j) const { return t[(w_n + j) * 64u + lane]; }
};
struct StatsRowSrc {
    const uint32_t *s, *q;             // word w_lo of the read
    uint64_t pitch;
    __device__ __forceinline__ uint32_t seq(uint32_t j) const { return s[(uint64_t)j * pitch]; }
    __device__ __forceinline__ uint32_t qual(uint32_t j) const { return q[(uint64_t)j * pitch]; }
};

// The rows.  A wave takes 64 consecutive reads of its slab, a lane a read: word w of the 64 rows is one coalesced 256-byte load.  With all lanes at the same word
// the wave's 64 additions fall into ONE row of the image -- one position's handful of quality values --, and same-address LDS atomics take turns.  SKEW: the wave
// first stages the chunk's words of its 64 reads in LDS (a lane reads back only what it wrote: no barrier), then lane l starts at word l % w_n of its own read, so
// that at any one time the lanes stand on w_n different words: 4 w_n rows of the image.  SKEW false is the direct form, kept for the measurement (option stats_form).
// Masked: rows outside the segment's n_pairs reads, bytes at cycles >= read_len, the last partial chunk and slab.
template <bool SKEW>
__global__ void __launch_bounds__(kStatsRowsBlock) k_stats_rows(const uint32_t *seq, const uint32_t *qual, const ReadMeta *meta, uint64_t pitch, uint64_t n_pairs, StatsLayout y,
                                                                StatsRowsPlan plan, uint64_t *counts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_stats[];
    const uint32_t stride = stats_row_stride(y.Q), image_words = plan.chunk * stride, n_units = plan.units[0] + plan.units[1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, G = gridDim.x, g = blockIdx.x;
    const uint32_t k = g / n_units, K = (G - 1u - g % n_units) / n_units + 1u;
    const uint64_t n_slabs = (n_pairs + plan.slab - 1u) / plan.slab;
    uint32_t *tile = s_stats + image_words + wave * 2u * (plan.chunk / 4u) * 64u;
    StatsLdsAdd add{s_stats};
    uint32_t bad = 0;
    for (uint32_t unit = g % n_units; unit < n_units; unit += G) {
        const uint32_t seg = unit >= plan.units[0] ? 1u : 0u, p0 = (unit - seg * plan.units[0]) * plan.chunk, L = y.len[seg];
        const uint32_t positions = L - p0 < plan.chunk ? L - p0 : plan.chunk, w_lo = p0 / 4u, w_n = (positions + 3u) / 4u;
        for (uint32_t i = threadIdx.x; i < image_words; i += kStatsRowsBlock) s_stats[i] = 0u;
        __syncthreads();
        for (uint64_t sl = k; sl < n_slabs; sl += K) {
            const uint64_t lo = sl * plan.slab, hi = lo + plan.slab < n_pairs ? lo + plan.slab : n_pairs;
            for (uint64_t base = lo + wave * 64u; base < hi; base += kStatsRowsBlock) {
                const uint64_t i = base + lane, r = seg * n_pairs + i;
                uint32_t read_len = 0;
                if (i < hi) {
                    read_len = meta[r].read_len;
                    if (read_len > L) read_len = L;                     // (k_stats_mates counts such a read in bad)
                    if (read_len > 4u * plan.row_words) read_len = 4u * plan.row_words;
                }
                if constexpr (SKEW) {
                    for (uint32_t j = 0; j < w_n; ++j) {
                        const bool in = 4u * (w_lo + j) < read_len;
                        tile[j * 64u + lane] = in ? seq[(uint64_t)(w_lo + j) * pitch + r] : 0u;
                        tile[(w_n + j) * 64u + lane] = in ? qual[(uint64_t)(w_lo + j) * pitch + r] : 0u;
                    }
                    const StatsTileSrc src{tile, w_n, lane};
                    bad += stats_row_lane(src, read_len, w_lo, w_n, lane % w_n, y.Q, stride, y.phred, add);
                } else {
                    const StatsRowSrc src{seq + (uint64_t)w_lo * pitch + r, qual + (uint64_t)w_lo * pitch + r, pitch};
                    bad += stats_row_lane(src, read_len, w_lo, w_n, 0u, y.Q, stride, y.phred, add);
                }
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < positions * stride; i += kStatsRowsBlock) {
            const uint32_t v = s_stats[i];
            if (!v) continue;
            const uint32_t p = i / stride, c = i - p * stride;
            if (c < y.Q) stats_flush_add(counts + y.off[kStBaseQuality] + ((uint64_t)seg * y.lmax + p0 + p) * y.Q + c, v);
            else if (c < y.Q + 5u) stats_flush_add(counts + y.off[kStBaseCall] + ((uint64_t)seg * y.lmax + p0 + p) * 5u + (c - y.Q), v);
        }
        __syncthreads();
    }
    if (bad) stats_flush_add(counts + y.off[kStBad], bad);
}

// k_stats_mates' counters: the workgroup's image of words [0, image_words) of the run's array, memory behind it
struct StatsMatesAdd {
    uint32_t *image;
    uint64_t *counts;
    uint32_t image_words;
    __device__ __forceinline__ void add(uint32_t i, uint32_t v) const {
        if (i < image_words) (void)__hip_atomic_fetch_add(image + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else stats_flush_add(counts + i, v);
    }
    // one addition per distinct index of the wave: the lane that finds itself first among the lanes still waiting adds the count of those with its index
    __device__ __forceinline__ void shared(uint32_t i, bool on) const {
        uint64_t waiting = __builtin_amdgcn_ballot_w64(on);
        while (waiting) {
            const uint32_t leader = lowest_set_bit64(waiting), mine = (uint32_t)__builtin_amdgcn_readlane((int)i, (int)leader);
            const uint64_t same = __builtin_amdgcn_ballot_w64(on && i == mine);
            if ((threadIdx.x & 63u) == leader) add(mine, popcount64(same));
            waiting &= ~same;
        }
    }
};
constexpr uint32_t kStatsMatesBlock = 256;
// One lane per mate of a part, as k_depth_add: lane r < n_pairs is the mate of segment 0 in raw row r, lane n_pairs + r the other; perm: the rows are binned
// (row_order) -- which pair a row holds, never which segment it is.  A persistent grid: a workgroup loops over stretches of 256 mates and flushes its image once.
template <bool VARIANTS>
__global__ void __launch_bounds__(kStatsMatesBlock) k_stats_mates(DevSim S, const Fragment *frags, const FragmentVar *fvars, uint64_t n_pairs, RawLayout raw, const uint32_t *perm,
                                                                  StatsLayout y, uint64_t *counts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_stats[];
    for (uint32_t i = threadIdx.x; i < y.image_words; i += kStatsMatesBlock) s_stats[i] = 0u;
    __syncthreads();
    const StatsMatesAdd a{s_stats, counts, y.image_words};
    uint32_t bad = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * kStatsMatesBlock; base < 2u * n_pairs; base += (uint64_t)gridDim.x * kStatsMatesBlock) {
        const uint64_t r = base + threadIdx.x;
        const bool live = r < 2u * n_pairs;
        const uint64_t rr = live ? r : 0u;
        const uint32_t seg = rr >= n_pairs ? 1u : 0u;
        const uint64_t row = rr - seg * n_pairs, pair = perm ? perm[row] : row;
        const Fragment f = frags[pair];
        FragmentVar fv{};
        if (fvars) fv = fvars[pair];
        bad += stats_mate<VARIANTS>(S, y, live, f, fvars != nullptr, fv, seg, raw.seq_of(rr), raw.ops_of(rr), raw.meta[rr], a);
    }
    if (bad) a.add(y.off[kStBad], bad);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < y.image_words; i += kStatsMatesBlock)
        if (const uint32_t v = s_stats[i]) stats_flush_add(counts + i, v);
}
#endif

}  // namespace rsq
