// rsq_chains.h -- the systematic-error chains and the bias normalisation (library only; the host emulation runs the per-lane parts):
//   k_sys_chain_select, k_sys_chain   one lane per chunk of a systematic-error chain   (Simulator.h:337-382, a13)
//   k_variant_chain_states            one lane per variant and strand: the chain state in front of it
//   k_surrounding_bias_tracks         one lane per reference position
//   k_sum_bias                        one lane per run of fragment start positions      (Reference.cpp:622-659, a14)
// All arithmetic lives in rsq_core.h; this file only maps work to lanes and moves bytes.
#pragma once
#include "rsq_core.h"

namespace rsq {

// ------------------------------------------------------------------------------------ systematic errors
struct Chain {
    uint32_t kind;         // 0 reference forward, 1 reference reverse complement, 2 adapter
    uint32_t id;           // sequence id or adapter id
    uint32_t seg;          // adapter: template segment
    uint32_t len;
    uint32_t c1, c2;       // Philox counter words identifying the chain
    uint32_t first_chunk;
    uint32_t initial_dom;  // DominantBase::dom_base_ left behind by the previous chain (Clear() keeps it)
    uint16_t *out;
    // a rank of a sharded job runs only the chunks its reads can touch: chunks [chunk_lo, chunk_lo + its number of chunks) of the chain,
    // entered with in_state (dist | start_rate << 24), the outgoing state of chunk chunk_lo - 1 on the neighbouring rank (0 at a chain's start)
    uint32_t chunk_lo = 0, in_state = 0;
};

struct ChainAcc {
    const uint64_t *words;
    uint32_t kind, len;
    uint64_t word_off;
    const uint8_t *codes;
    RSQ_HD uint32_t operator()(uint32_t pos) const {
        if (kind == 0) return ref_base(words, word_off, pos);
        if (kind == 1) return 3u - ref_base(words, word_off, len - 1u - pos);
        return codes[pos];
    }
};

template <class Acc>
RSQ_HD uint32_t find_dominant(const Acc &acc, const uint32_t (&cnt)[4], uint32_t cur_pos) {     // utilities.hpp:238-262 (N-free sequence)
    uint32_t mx = cnt[0];
    for (int i = 1; i < 4; ++i) mx = cnt[i] > mx ? cnt[i] : mx;
    uint32_t pos = cur_pos;
    uint32_t b;
    do { b = acc(--pos); } while (cnt[b] != mx);
    return b;
}

// CoverageStats.cpp:379-396
RSQ_HD void update_distances(uint32_t reset_distance, uint32_t &dist, uint32_t &start_rate, uint32_t error_rate) {
    if (dist) {
        if (start_rate < error_rate) {
            dist = 0;
            start_rate = error_rate;
        } else if (++dist >= reset_distance) {
            dist = 0;
            start_rate = 0;
        }
    } else if (error_rate) {
        dist = 1;
        start_rate = error_rate;
    }
}

// One of the chain's two draws, screened (rsq_core.h draw_screened: single precision with a proof that the column is the double-precision
// one); undecided draws and tables outside the screen's preconditions are repeated in double precision.  Q quads per row of the table's
// float copy.  Returns the outcome value; `none`: what an all-zero row gives (prob_sum == 0 in the reference's recipe).
template <int Q>
RSQ_HD uint32_t chain_draw(const DevSim &S, const DevTable &t, const uint32_t (&idx)[3], uint32_t word, uint32_t none) {
    if (S.chain_quads && t.k && t.f32_ok) {
        const float *g = S.pool32 + t.off32;
        const uint32_t slot = 4u * (uint32_t)Q;
        const GlobalRow32 m0{g + clamp_row(t, 0, idx[0]) * slot}, m1{g + (t.rows[0] + clamp_row(t, 1, idx[1])) * slot},
            m2{g + (t.rows[0] + t.rows[1] + clamp_row(t, 2, idx[2])) * slot};
        uint32_t col = 0;
        if (draw_screened<Q>(word, col, m0, m1, m2)) return S.par0[t.par0_off + col];
    }
    double ps;
    const uint32_t value = draw<3>(t, S.pool, S.par0, idx, u32_to_unit(word), ps);
    return 0.0 == ps ? none : value;
}
RSQ_HD uint32_t chain_draw_rate_rows(const DevSim &S, const DevTable &t, const uint32_t (&idx)[3], uint32_t word) {
    switch (S.chain_quads) {
        case 8: return chain_draw<8>(S, t, idx, word, 0u);
        case 16: return chain_draw<16>(S, t, idx, word, 0u);
        default: return chain_draw<26>(S, t, idx, word, 0u);           // also 0: chain_draw goes straight to double precision
    }
}
// the word alone says "rate 0" for the lane's rows of margins 0 and 2 (rsq_pack.h): no row is read
RSQ_HD bool chain_rate_is_zero(const DevSim &S, const DevTable &t, const uint32_t (&idx)[3], uint32_t word) {
    if (!t.sure_range) return false;
    const uint32_t range = S.chain_sure[t.sure_range + clamp_row(t, 0, idx[0]) * t.rows[2] + clamp_row(t, 2, idx[2])], lo16 = range & 0xFFFFu;
    return (word >> 16) - lo16 < (range >> 16) - lo16;
}
RSQ_HD uint32_t chain_draw_rate(const DevSim &S, const DevTable &t, const uint32_t (&idx)[3], uint32_t word) {
    if (chain_rate_is_zero(S, t, idx, word)) return 0u;
    return chain_draw_rate_rows(S, t, idx, word);
}

// Positions [lo,hi) of one chain.  Everything except (dist,start_rate) is a pure function of the sequence and is
// rebuilt at `lo`, so a chunk can start anywhere given the incoming (dist,start_rate).  keep_from > lo: the positions in front of keep_from are a run-up
// (nothing is written for them) and *kept_state receives the state in front of keep_from.
template <class Acc>
RSQ_HD void sys_chain_chunk(const DevSim &S, const Acc &acc, uint32_t c1, uint32_t c2, uint32_t lo, uint32_t hi, uint32_t initial_dom, uint32_t &dist,
                            uint32_t &start_rate, uint16_t *out, uint32_t keep_from = 0, uint32_t *kept_state = nullptr) {
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t p = lo > 5 ? lo - 5 : 0; p < lo; ++p) ++cnt[acc(p)];
    uint32_t last_base = lo ? acc(lo - 1) : 4u;
    uint32_t dom = lo ? find_dominant(acc, cnt, lo) : initial_dom;
    const uint32_t range = S.sys_gc_range;
    uint32_t gc_bases = lo < range ? lo : range, gc = 0;
    for (uint32_t p = lo - gc_bases; p < lo; ++p) gc += is_gc(acc(p));
    for (uint32_t pos = lo; pos < hi; ++pos) {
        if (pos == keep_from && kept_state) *kept_state = dist | (start_rate << 24);
        const uint32_t b = acc(pos);
        const Words w = philox(S.seed, pos, c1, c2, kDomSysErr << 28);
        const uint32_t idx[3] = {transform_distance(dist), safe_percent_u16(gc, gc_bases), start_rate};
        const uint32_t dom_error = chain_draw<(int)kQuadsSmall>(S, S.dom_error[(b * 5u + last_base) * 5u + dom], idx, w.w0, 4u);
        const uint32_t rate = chain_draw_rate(S, S.error_rate[b * 5u + dom_error], idx, w.w1);
        if (pos >= keep_from) out[pos] = (uint16_t)(dom_error | (rate << 8));
        last_base = b;
        ++cnt[b];
        if (pos >= 5) --cnt[acc(pos - 5)];
        dom = find_dominant(acc, cnt, pos + 1);
        update_distances(S.reset_distance, dist, start_rate, rate);
        if (is_gc(b)) ++gc;                                         // Simulator.h:354-366 UpdateGC
        if (gc_bases < range) ++gc_bases;
        else if (is_gc(acc(pos - gc_bases))) --gc;
    }
}

// What the lane of a chunk settles before it walks the chunk (k_sys_chain below, "Speculative chunking"; the host emulation's loop over the chunks): the state the
// chunk is entered with -- the outgoing state of its left neighbour in the pass before, the chain's own entering state for its first chunk -- the chunk's
// positions [lo, hi), and where the walk begins: in pass 0 a run-up of `warmup` positions in front of lo, whose end is the guess of the chunk's incoming state.
RSQ_HD uint32_t chain_incoming(const Chain &ch, uint32_t c, const uint32_t *out_prev, int pass) {
    const uint32_t local = c - ch.first_chunk;
    if (local == 0) return ch.in_state;
    return pass > 0 ? out_prev[c - 1] : 0u;                          // pass 0: the guess (0, 0)
}
struct ChunkEntry {
    uint32_t want, lo, hi, from;
    ChainAcc acc;
};
RSQ_HD ChunkEntry chain_chunk_entry(const DevSim &S, const Chain &ch, uint32_t c, const uint32_t *out_prev, int pass, uint32_t chunk_len, uint32_t warmup) {
    const uint32_t local = c - ch.first_chunk;
    ChunkEntry e;
    e.want = chain_incoming(ch, c, out_prev, pass);
    e.acc = ChainAcc{S.ref_words, ch.kind, ch.len, ch.kind < 2 ? S.seq_word_off[ch.id] : 0, ch.kind == 2 ? S.adapters[ch.seg].seqs + S.adapters[ch.seg].seq_ptr[ch.id] : nullptr};
    e.lo = (ch.chunk_lo + local) * chunk_len;
    e.hi = e.lo + chunk_len < ch.len ? e.lo + chunk_len : ch.len;
    e.from = pass == 0 && local ? e.lo - (warmup < e.lo ? warmup : e.lo) : e.lo;      // pass 0: the guess is the end of a run-up from (0,0)
    return e;
}

#if RSQ_DEVICE_BUILD
// The same positions for the 64 chunks of a wave, with the expensive part of a position -- an error-rate draw that has to read its rows, about one position in
// thirty -- done for several lanes at once: a lane whose draw the random word does not decide waits (its chunk is its own: nothing orders the lanes of a wave)
// until kChainBatch lanes wait or no lane can go on, and the rows are read and multiplied by a wave most of whose lanes take part instead of two of them.
// Position by position a lane does what sys_chain_chunk does; only when it does it differs.
constexpr uint32_t kChainBatch = 16;        // human-sized chains: 8 -> 0.159 s, 16 -> 0.150, 32 -> 0.178, 48 -> 0.20 at a quarter of the size (0.185 one lane at a time)
template <class Acc>
__device__ void sys_chain_chunk_batched(const DevSim &S, const Acc &acc, uint32_t c1, uint32_t c2, uint32_t lo, uint32_t hi, uint32_t initial_dom, uint32_t &dist,
                                        uint32_t &start_rate, uint16_t *out, uint32_t keep_from, uint32_t *kept_state) {
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t p = lo > 5 ? lo - 5 : 0; p < lo; ++p) ++cnt[acc(p)];
    uint32_t last_base = lo ? acc(lo - 1) : 4u;
    uint32_t dom = lo ? find_dominant(acc, cnt, lo) : initial_dom;
    const uint32_t range = S.sys_gc_range;
    uint32_t gc_bases = lo < range ? lo : range, gc = 0;
    for (uint32_t p = lo - gc_bases; p < lo; ++p) gc += is_gc(acc(p));
    uint32_t pos = lo, b = 0, dom_error = 0, word1 = 0;
    bool waiting = false;
    for (;;) {
        const bool left = pos < hi;
        if (!__any(left)) break;
        uint32_t rate = 0;
        bool have_rate = false;
        if (left && !waiting) {
            if (pos == keep_from && kept_state) *kept_state = dist | (start_rate << 24);
            b = acc(pos);
            const Words w = philox(S.seed, pos, c1, c2, kDomSysErr << 28);
            const uint32_t idx[3] = {transform_distance(dist), safe_percent_u16(gc, gc_bases), start_rate};
            dom_error = chain_draw<(int)kQuadsSmall>(S, S.dom_error[(b * 5u + last_base) * 5u + dom], idx, w.w0, 4u);
            word1 = w.w1;
            have_rate = chain_rate_is_zero(S, S.error_rate[b * 5u + dom_error], idx, word1);
            waiting = !have_rate;
        }
        const uint32_t n_wait = (uint32_t)__popcll(__ballot(waiting)), n_go = (uint32_t)__popcll(__ballot(left && !waiting));
        if (n_wait >= kChainBatch || (n_wait && !n_go)) {
            if (waiting) {
                const uint32_t idx[3] = {transform_distance(dist), safe_percent_u16(gc, gc_bases), start_rate};      // the lane's state has not moved while it waited
                rate = chain_draw_rate_rows(S, S.error_rate[b * 5u + dom_error], idx, word1);
                have_rate = true;
                waiting = false;
            }
        }
        if (have_rate) {
            if (pos >= keep_from) out[pos] = (uint16_t)(dom_error | (rate << 8));
            last_base = b;
            ++cnt[b];
            if (pos >= 5) --cnt[acc(pos - 5)];
            dom = find_dominant(acc, cnt, pos + 1);
            update_distances(S.reset_distance, dist, start_rate, rate);
            if (is_gc(b)) ++gc;                                     // Simulator.h:354-366 UpdateGC
            if (gc_bases < range) ++gc_bases;
            else if (is_gc(acc(pos - gc_bases))) --gc;
            ++pos;
        }
    }
}
#endif

struct BiasParam {
    uint32_t seq, len;
    double general_bias;       // ref_seq_bias * insert_lengths_bias[len]
};
constexpr uint32_t kBiasRun = 32;          // start positions per lane
constexpr uint32_t kBiasBlock = 256;

// Reference::Bias of the fragment [start, start+len) (Reference.cpp:634-637,650-653 inside SumBias)
RSQ_HD double site_bias(const DevSim &S, uint64_t word_off, uint32_t L, uint32_t start, uint32_t len, uint32_t gc_count, double general_bias) {
    uint32_t ss[3], se[3];
    surrounding_forward(S.ref_words, word_off, L, start, ss);
    surrounding_reverse(S.ref_words, word_off, L, start + len - 1, se);
    return general_bias * S.gc_bias[percent_u32(gc_count, len)] * surrounding_bias(S.sur_bias, ss) * surrounding_bias(S.sur_bias, se);
}

#if RSQ_DEVICE_BUILD

// Speculative chunking: pass 0 runs every chunk from a guess of its incoming (dist,start_rate); later passes re-run exactly the
// chunks whose true incoming state (the outgoing state of their left neighbour) differs from the one they used.
// The fixed point is the sequential chain, bit for bit, for any seed and any guess.
// The guess: the chain run from (0,0) over the `warmup` positions in front of the chunk.  Two runs of the chain over the same positions draw from the same
// random numbers whatever their states, and meet for good as soon as both have left their error regions (measured on a human-sized reference with (0,0) as
// the guess at the chunk's own first position: 97 % of the chunks were run a second time, 12 % a third time after 256 more positions, 1.3 % a fourth: the states
// of two runs meet within about 120 positions).  Long chunks with a short run-up keep the second pass small: see chain_chunk_len.
//   k_sys_chain_select (passes > 0): one lane per chunk compares; chunks to run again are appended to `list` (their order does not
//       matter: chunks of one pass are independent), the others keep their outgoing state.  A wave of the run kernel then holds 64 chunks
//       that all have work, whatever share of the chunks changed.
//   k_sys_chain: one lane per listed chunk (pass 0: every chunk, list == nullptr).
__global__ void __launch_bounds__(256) k_sys_chain_select(const Chain *chains, const uint32_t *chunk_chain, uint32_t n_chunks, const uint32_t *used_state, const uint32_t *out_prev,
                                                         uint32_t *out_new, uint32_t *list, uint32_t *n_listed, int pass) {
    // places in the list are reserved once per workgroup (ranks in LDS): one global atomic per wave queues at one L2 channel (see k_sieve_finish)
    __shared__ uint32_t s_n, s_base;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    bool again = false;
    if (c < n_chunks) {
        again = chain_incoming(chains[chunk_chain[c]], c, out_prev, pass) != used_state[c];
        if (!again) out_new[c] = out_prev[c];
    }
    const uint32_t rank = again ? atomicAdd(&s_n, 1u) : 0u;
    __syncthreads();
    if (threadIdx.x == 0 && s_n) s_base = atomicAdd(n_listed, s_n);
    __syncthreads();
    if (again) list[s_base + rank] = c;
}
__global__ void __launch_bounds__(64) k_sys_chain(DevSim S, const Chain *chains, const uint32_t *chunk_chain, const uint32_t *list, uint32_t n_run, uint32_t chunk_len,
                                                 uint32_t warmup, uint32_t *used_state, const uint32_t *out_prev, uint32_t *out_new, int pass) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_run) return;
    const uint32_t c = list ? list[i] : i;
    const Chain ch = chains[chunk_chain[c]];
    const ChunkEntry e = chain_chunk_entry(S, ch, c, out_prev, pass, chunk_len, warmup);
    uint32_t dist = e.want & 0xFFFFFFu, start_rate = e.want >> 24;
    uint32_t used = e.want;
    sys_chain_chunk_batched(S, e.acc, ch.c1, ch.c2, e.from, e.hi, ch.initial_dom, dist, start_rate, ch.out, e.lo, &used);
    used_state[c] = used;
    out_new[c] = dist | (start_rate << 24);
}

// -V: the chain state in front of every variant's position, per strand (blockIdx.y): the entering state of the position's chunk at the fixed point (used_state),
// folded over the chunk's track up to the position (at most chunk_len - 1 steps).  The host pass over the variants' own bases (variant_sys_errors_strand) needs
// nothing else of the tracks, which therefore stay on the device (12 GB for a human-sized reference).  span: per (sequence, strand) the chain and how many of its
// chunks were run (a rank of a sharded job runs a part); variants outside get state 0, which nobody reads.
struct ChainSpan {
    int32_t chain;
    uint32_t chunks;
};
__global__ void __launch_bounds__(256) k_variant_chain_states(DevSim S, const Chain *chains, const ChainSpan *span, const uint32_t *used_state, uint32_t chunk_len,
                                                             uint32_t n_variants, uint32_t *states /* [2][n_variants] */) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, strand = blockIdx.y;
    if (i >= n_variants) return;
    uint32_t seq = 0;                                               // the last sequence whose variants begin at or before i
    for (uint32_t lo = 0, hi = S.n_seqs; lo < hi;) {
        const uint32_t mid = (lo + hi) >> 1;
        if (S.var_ptr[mid] <= i) seq = mid, lo = mid + 1u;
        else hi = mid;
    }
    const ChainSpan sp = span[seq * 2u + strand];
    uint32_t state = 0;
    if (sp.chain >= 0) {
        const Chain ch = chains[sp.chain];
        const uint32_t L = S.seq_len[seq], pos = strand ? L - 1u - S.variants[i].pos : S.variants[i].pos, chunk = pos / chunk_len;
        if (chunk >= ch.chunk_lo && chunk - ch.chunk_lo < sp.chunks) {
            state = used_state[ch.first_chunk + (chunk - ch.chunk_lo)];
            uint32_t dist = state & 0xFFFFFFu, start_rate = state >> 24;
            for (uint32_t p = chunk * chunk_len; p < pos; ++p) update_distances(S.reset_distance, dist, start_rate, (uint32_t)ch.out[p] >> 8);
            state = dist | (start_rate << 24);
        }
    }
    states[(size_t)strand * n_variants + i] = state;
}

// ------------------------------------------------------------------------------------ bias normalisation

// The surrounding factors of Reference::Bias depend on one position each (the start, or the end, of the fragment) and are shared by
// every sampled fragment length: computed once per position (3 table lookups in the 24 MB sur_bias table and an exp each), they turn
// k_sum_bias from a random-access kernel into a streaming one.  Same function, same values, same product order.
// [w_lo, w_hi): the part of the concatenated sequences that is needed (a sharded job computes its share); the tracks begin at w_lo
__global__ void __launch_bounds__(256) k_surrounding_bias_tracks(DevSim S, double *start_bias, double *end_bias, uint64_t w_lo, uint64_t w_hi) {
    const uint64_t at = w_lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= w_hi) return;
    uint32_t seq = 0;                                               // the last sequence that begins at or before `at` (empty sequences share their begin)
    for (uint32_t lo = 0, hi = S.n_seqs; lo < hi;) {
        const uint32_t mid = (lo + hi) >> 1;
        if (S.seq_base_off[mid] <= at) seq = mid, lo = mid + 1u;
        else hi = mid;
    }
    const uint32_t L = S.seq_len[seq], pos = (uint32_t)(at - S.seq_base_off[seq]);
    if (pos >= L) return;
    const uint64_t wo = S.seq_word_off[seq];
    uint32_t sur[3];
    surrounding_forward(S.ref_words, wo, L, pos, sur);
    start_bias[at - w_lo] = surrounding_bias(S.sur_bias, sur);
    surrounding_reverse(S.ref_words, wo, L, pos, sur);
    end_bias[at - w_lo] = surrounding_bias(S.sur_bias, sur);
}

// One workgroup = one chunk of kBiasBlock * kBiasRun start positions of one (sequence, sampled length).  A chunk belongs to the share
// [g_lo, g_hi) of the concatenated sequences its first start position lies in; the other chunks' partial results stay zero (the
// ranks of a sharded job add their arrays up: every entry is non-zero on one rank, so the sum is exact whatever the order).
__global__ void __launch_bounds__(256) k_sum_bias(DevSim S, const BiasParam *params, const uint32_t *chunk_param, const uint32_t *chunk_ptr, const double *start_bias,
                                                 const double *end_bias, uint64_t track_base, double *partial_sum, double *partial_max, uint64_t g_lo, uint64_t g_hi) {
    __shared__ double s_sum[kBiasBlock];
    __shared__ double s_max[kBiasBlock];
    const uint32_t param = chunk_param[blockIdx.x], chunk = blockIdx.x - chunk_ptr[param];
    const BiasParam p = params[param];
    const uint32_t L = S.seq_len[p.seq];
    const uint64_t wo = S.seq_word_off[p.seq];
    const uint32_t n_starts = L - p.len + 1;                       // start positions 0 .. L-len (Reference.cpp:645)
    const uint64_t chunk_at = S.seq_base_off[p.seq] + (uint64_t)chunk * kBiasBlock * kBiasRun;
    if (chunk_at < g_lo || chunk_at >= g_hi) return;
    const uint64_t bo = S.seq_base_off[p.seq] - track_base;        // the tracks begin at track_base of the concatenated sequences
    // lane t takes the chunk's start positions t, t + kBiasBlock, ...: neighbouring lanes read neighbouring track entries (coalesced), the
    // G/C count of a fragment comes from the prefix sums.  A lane adds its kBiasRun terms in this order, the tree below adds the lanes.
    const uint32_t chunk_first = chunk * kBiasBlock * kBiasRun;
    double sum = 0.0, mx = 0.0;
    for (uint32_t j = 0; j < kBiasRun; ++j) {
        const uint32_t start = chunk_first + j * kBiasBlock + threadIdx.x;
        if (start >= n_starts) break;
        const uint32_t gc = ref_gc_count_prefix(S.ref_words, S.gc_prefix, wo, start, start + p.len);
        const double bias = start_bias ? p.general_bias * S.gc_bias[percent_u32(gc, p.len)] * start_bias[bo + start] * end_bias[bo + start + p.len - 1u]
                                       : site_bias(S, wo, L, start, p.len, gc, p.general_bias);
        sum += bias;
        mx = bias > mx ? bias : mx;
    }
    s_sum[threadIdx.x] = sum;
    s_max[threadIdx.x] = mx;
    __syncthreads();
    for (uint32_t s = kBiasBlock / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
            s_max[threadIdx.x] = s_max[threadIdx.x + s] > s_max[threadIdx.x] ? s_max[threadIdx.x + s] : s_max[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial_sum[blockIdx.x] = s_sum[0];
        partial_max[blockIdx.x] = s_max[0];
    }
}

#endif

}  // namespace rsq
