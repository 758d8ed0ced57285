// rsq_pileup.h -- truth pileup: per reference position the depth, the called bases A/C/G/T/N, the deleted columns and the insertions of the simulated reads, optionally
// per strand, accumulated on the device from the arrays the truth alignments are written from, and its TSV text (include/reseq_amd.h rsq_sim_pileup_*; DESIGN.md 4.8
// "Truth pileup" states the rule).
//
// The rule, over the MAPPED truth records in reference coordinates (r = POS - 1, q = 0, the CIGAR as written): nM: per column depth[r] += 1 and base[SEQ[q]][r] += 1;
// nD: del[r, r + n) += 1; nI: ins[max(r, 1) - 1] += 1, once per element; nS: q += n.  A record's strand is its FLAG 0x10.  No alignment rule lives here: the columns
// come from the walkers MD's come from (md_plain_columns, sam_var_columns), merged and compared by MdCols, whose sink PileupSink is.
//
// A run owns kPileupPlanes planes of uint32 per strand set (one set, or forward then reverse), each in the depth array's layout (rsq_depth.h: sequence s begins at
// word seq_base_off[s] + s, depth_words() words a plane):
//   plane 0      the depth as differences, +1 at an M run's start and -1 behind it (DepthSink's rule); rsq_sim_pileup_finish runs rsq_depth.h's prefix sum over it
//   planes 1-5   the calls that differ from the reference: to A, C, G, T, and a read base N.  The reference letter's own count is never stored: it is the depth
//                less the five, formed when rows are read out -- a mate without a mismatch costs two atomics
//   plane 6, 7   del, one add per deleted column; ins, one add per I element
//
//   pileup_mate<VARIANTS>                    per lane, host and device (tests/hostemu/pileup_trial.cpp runs it on the CPU)
//   k_pileup_add<VARIANTS>                   one lane per mate of the kept part, k_depth_add's indexing
//   pileup_row, k_pileup_rows                the full counts [pos][S][8] of a window
//   k_pileup_lines, k_pileup_place           a piece of text: the rows kept under the predicate and their lines' sizes; after the scan, the lines' positions and places
//   pileup_line, k_pileup_text               the lines, through the wave's image (WaveImage, ImageSink: rsq_format.h)
#pragma once
#include "rsq_depth.h"
#include "rsq_md.h"

namespace rsq {

constexpr uint32_t kPileupPlanes = 8, kPileupDel = 6, kPileupIns = 7;

// MdCols' sink: takes no text; column_run and mismatch_base (rsq_md.h md_note_run, md_note_base) are what it is for.  An element outside the sequence -- the
// record's rules exclude it -- is counted in `bad`, never written.
struct PileupSink {
    uint32_t *plane0;          // word 0 of the mate's sequence in plane 0 of its strand set
    uint64_t words;            // of a plane
    uint32_t r, len;           // the reference position of the next M or D column (POS - 1 at first); the sequence's length
    uint32_t bad = 0;
    bool ok = true;            // the M run being compared lies inside the sequence
    RSQ_HD void column_run(uint32_t op, uint32_t p, uint32_t n) {
        if (op == 2u) {                                                 // the base in front of the insertion, position 0 where there is none
            const uint32_t a = (r > 1u ? r : 1u) - 1u;
            if (a < len) counter_add(plane0 + kPileupIns * words + a, 1u);
            else ++bad;
            return;
        }
        const bool inside = p <= len && n <= len - p;
        if (op == 0u) {
            ok = inside;
            if (inside) {
                counter_add(plane0 + p, 1u);
                counter_add(plane0 + p + n, 0xFFFFFFFFu);
            } else ++bad;
        } else if (op == 1u) {
            if (inside) {
                for (uint32_t i = 0; i < n; ++i) counter_add(plane0 + kPileupDel * words + p + i, 1u);
            } else ++bad;
        }
        r = p + n;                                                      // (a dropped D run moves the cursor too: an I behind it stands at POS - 1)
    }
    RSQ_HD void mismatch_base(uint32_t p, uint32_t code) {
        if (ok && p < len) counter_add(plane0 + (1u + code) * words + p, 1u);
    }
    RSQ_HD void num(uint32_t) {}
    RSQ_HD void ch(char) {}
    RSQ_HD void bytes(uint32_t, uint32_t) {}
    RSQ_HD void element(char, uint32_t) {}
};

// One mate of a pair with a fragment, as depth_mate: one walk of its columns.  planes: the run's array; strands: the run keeps two strand sets, a reverse record
// (FLAG 0x10) goes to the second.  Returns the elements that fell outside the sequence (0).
template <bool VARIANTS>
RSQ_HD uint32_t pileup_mate(const DevSim &S, const Fragment &f, bool has_fv, const FragmentVar &fv, uint32_t seg, const WordColumn &seq, const WordColumn &ops, const ReadMeta &m,
                            uint32_t *planes, uint64_t words, bool strands) {
    if (!f.len) return 0u;                                              // unmapped (flags 77 / 141)
    if (f.seq >= S.n_seqs) return 1u;
    SamAlign al{};
    al.mapped = 1u;
    al.reverse = seg != f.strand ? 1u : 0u;
    PileupSink o{planes + (strands && al.reverse ? kPileupPlanes * words : 0u) + S.seq_base_off[f.seq] + f.seq, words, 0u, S.seq_len[f.seq]};
    if constexpr (VARIANTS) {
        uint32_t n_cigar;
        const SamVarMate e = sam_var_walk(S, true, f, has_fv, fv, seg, ops, m, n_cigar);
        al.pos = e.pos + 1u;
        o.r = e.pos;
        md_walk(S, f, m, seq, ops, e.w, &e, al, o);
    } else {
        const SamMate w = sam_walk(ops, m);
        o.r = sam_mate_pos(f, seg, w);
        al.pos = o.r + 1u;
        md_walk(S, f, m, seq, ops, w, nullptr, al, o);
    }
    return o.bad;
}

// The full counts of one position of one strand set: v = { depth, A, C, G, T, N, del, ins }; in: the eight planes' words, ref: the reference base's code.
RSQ_HD void pileup_row(const uint32_t *in, uint32_t ref, uint32_t *v) {
    const uint32_t own = in[0] - (in[1] + in[2] + in[3] + in[4] + in[5]);      // (the plane of the reference's own letter holds 0)
    for (uint32_t k = 0; k < kPileupPlanes; ++k) v[k] = k == 1u + ref ? own : in[k];
}
// sites: any value but the depth and the reference letter's own count; all: any value at all
RSQ_HD bool pileup_keep(const uint32_t *v, uint32_t sets, uint32_t ref, bool all) {
    uint32_t any = 0;
    for (uint32_t s = 0; s < sets; ++s)
        for (uint32_t k = all ? 0u : 1u; k < kPileupPlanes; ++k)
            if (all || k != 1u + ref) any |= v[s * kPileupPlanes + k];
    return any != 0u;
}
// "<name>\t<pos, 1-based>\t<ref letter>" and per strand set "\t<depth>\t<A>\t<C>\t<G>\t<T>\t<N>\t<del>\t<ins>", "\n"
template <class Sink>
RSQ_HD void pileup_line(const NameTable &names, uint32_t seq, uint32_t pos, uint32_t ref, const uint32_t *v, uint32_t sets, Sink &t) {
    t.str(names.names + names.name_ptr[seq], names.name_ptr[seq + 1] - names.name_ptr[seq]);
    t.ch('\t');
    t.num(pos + 1u);
    t.ch('\t');
    t.ch((char)md_ref_letter(ref));
    for (uint32_t k = 0; k < sets * kPileupPlanes; ++k) {
        t.ch('\t');
        t.num(v[k]);
    }
    t.ch('\n');
}
RSQ_HD uint32_t pileup_line_size(uint32_t name_len, uint32_t pos, const uint32_t *v, uint32_t sets) {
    uint32_t n = name_len + 1u + digits_u32(pos + 1u) + 2u + 1u;
    for (uint32_t k = 0; k < sets * kPileupPlanes; ++k) n += 1u + digits_u32(v[k]);
    return n;
}
// the image of k_pileup_text: 64 lines at their widest, whole 128 bytes, at most 32 KiB (longer lines go straight to memory)
constexpr uint32_t kPileupLines = 64, kPileupLdsMax = 32u * 1024u;
RSQ_HD uint32_t pileup_lds_bytes(uint32_t name_len, uint32_t sets) {
    const uint64_t want = ((uint64_t)kPileupLines * (name_len + 14u + 11u * kPileupPlanes * sets) + 16u + 127u) & ~(uint64_t)127u;
    return (uint32_t)(want > kPileupLdsMax ? kPileupLdsMax : want);
}

#if RSQ_DEVICE_BUILD
// One lane per mate of a part, indexed as k_depth_add.  strands: 0 or 1, the run's choice; the lane's plane offset follows from it and the mate's strand.
template <bool VARIANTS>
__global__ void __launch_bounds__(256) k_pileup_add(DevSim S, const Fragment *frags, const FragmentVar *fvars, uint64_t n_pairs, RawLayout raw, const uint32_t *perm, uint32_t *planes,
                                                    uint64_t words, uint32_t strands, uint32_t *bad) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 2u * n_pairs) return;
    const uint32_t seg = r >= n_pairs ? 1u : 0u;
    const uint64_t row = r - seg * n_pairs, pair = perm ? perm[row] : row;
    const Fragment f = frags[pair];
    FragmentVar fv{};
    if (fvars) fv = fvars[pair];
    const uint32_t out = pileup_mate<VARIANTS>(S, f, fvars != nullptr, fv, seg, raw.seq_of(r), raw.ops_of(r), raw.meta[r], planes, words, strands != 0u);
    if (out) atomicAdd(bad, out);
}

// the reference base of position p of a sequence whose packed words begin at w
__device__ __forceinline__ uint32_t pileup_ref_code(const uint64_t *w, uint32_t p) { return (uint32_t)(w[p >> 5] >> (2u * (p & 31u))) & 3u; }
// the full counts of position p, all strand sets, from the planes (at: word 0 of the sequence in plane 0 of set 0): a wave's loads of one plane lie side by side
__device__ __forceinline__ void pileup_load_row(const uint32_t *at, uint64_t words, uint32_t sets, uint32_t p, uint32_t ref, uint32_t *v) {
    for (uint32_t s = 0; s < sets; ++s) {
        uint32_t in[kPileupPlanes];
#pragma unroll
        for (uint32_t k = 0; k < kPileupPlanes; ++k) in[k] = at[(s * kPileupPlanes + k) * words + p];
        pileup_row(in, ref, v + s * kPileupPlanes);
    }
}

// rows[i][s][8], i the position lo + i of the sequence: two 16-byte stores a strand set (the caller's array is 16-byte aligned, or the words go one by one)
__global__ void __launch_bounds__(256) k_pileup_rows(const uint32_t *at, uint64_t words, uint32_t sets, const uint64_t *ref_words, uint32_t lo, uint64_t n, uint32_t *rows) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = lo + (uint32_t)i;
    uint32_t v[2u * kPileupPlanes];
    pileup_load_row(at, words, sets, p, pileup_ref_code(ref_words, p), v);
    uint32_t *out = rows + i * sets * kPileupPlanes;
    if (0u == (reinterpret_cast<uintptr_t>(rows) & 15u)) {
        for (uint32_t k = 0; k < sets * kPileupPlanes; k += 4u) *reinterpret_cast<uint4 *>(out + k) = uint4{v[k], v[k + 1u], v[k + 2u], v[k + 3u]};
    } else {
        for (uint32_t k = 0; k < sets * kPileupPlanes; ++k) out[k] = v[k];
    }
}

// ------------------------------------------------------------------------------------------------ TSV text of a piece [lo, lo + n) of one sequence
// flags[i] = 1 where position lo + i has a line under the predicate, sizes[i] = that line's bytes (0 without one).  Rows are independent: a piece needs no carry.
__global__ void __launch_bounds__(256) k_pileup_lines(const uint32_t *at, uint64_t words, uint32_t sets, const uint64_t *ref_words, uint32_t lo, uint64_t n, uint32_t all,
                                                      uint32_t name_len, uint32_t *flags, uint32_t *sizes) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = lo + (uint32_t)i, ref = pileup_ref_code(ref_words, p);
    uint32_t v[2u * kPileupPlanes];
    pileup_load_row(at, words, sets, p, ref, v);
    const bool keep = pileup_keep(v, sets, ref, all != 0u);
    flags[i] = keep ? 1u : 0u;
    sizes[i] = keep ? pileup_line_size(name_len, p, v, sets) : 0u;
}
// ... compacted: line k = rank[i] stands on position lo + i and begins at byte at_pos[i] of the piece's text (rank, at_pos: the exclusive scans of flags and
// sizes, n + 1 entries each); offsets gets one entry more, the text's length
__global__ void __launch_bounds__(256) k_pileup_place(const uint32_t *flags, const uint64_t *rank, const uint64_t *at_pos, uint32_t lo, uint64_t n, uint32_t *line_pos, uint64_t *offsets) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        offsets[rank[n]] = at_pos[n];
        return;
    }
    if (!flags[i]) return;
    line_pos[rank[i]] = lo + (uint32_t)i;
    offsets[rank[i]] = at_pos[i];
}
// One wave per 64 consecutive lines, a lane a line, through the wave's image.  The host has checked the capacity.
__global__ void __launch_bounds__(64) k_pileup_text(NameTable names, uint32_t seq, const uint32_t *at, uint64_t words, uint32_t sets, const uint64_t *ref_words, const uint32_t *line_pos,
                                                   uint64_t n_lines, const uint64_t *offsets, char *dst, uint32_t lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) char s_pileup[];
    using Image = WaveImage<false, kPileupLines>;
    if (Image::first() >= n_lines) return;
    const Image im(offsets, n_lines, dst, lds_bytes, nullptr, threadIdx.x);
    uint32_t p = 0, ref = 0, v[2u * kPileupPlanes];
    for (uint32_t k = 0; k < 2u * kPileupPlanes; ++k) v[k] = 0u;
    if (im.active) {
        p = line_pos[im.item];
        ref = pileup_ref_code(ref_words, p);
        pileup_load_row(at, words, sets, p, ref, v);
    }
    if (!im.through_lds) {                                              // names too long for the image: a lane writes its line straight to memory
        if (im.active) {
            WordSinkT<char *> t(dst + offsets[im.item]);
            pileup_line(names, seq, p, ref, v, sets, t);
            t.finish();
        }
        return;
    }
    im.clear(s_pileup, lds_bytes);
    if (im.active) {
        ImageSink t(im.item_text(s_pileup));
        pileup_line(names, seq, p, ref, v, sets, t);
        t.finish();
    }
    im.store_out(s_pileup);
}
#endif

}  // namespace rsq
