// rsq_sieve.h -- the sieve: which (start position, fragment length) cells have fragments, and how many (library only; the host emulation runs the per-lane parts):
//   k_slot_table     variants of any kind: one workgroup per block of start positions
//   k_sieve_gaps     one lane per start position slot                                  (Simulator.cpp:2249-2357, a6)
//   k_sieve_gaps_lds the same with the coverage group's gap tables staged in LDS
//   k_sieve_finish   one lane per cell that passed the zero threshold
//   k_sieve_emit     one lane per cell with fragments writes its Fragment records
// The scans between them are rsq_scan.h's.
#pragma once
#include "rsq_core.h"
#include "rsq_variants.h"

namespace rsq {

// --------------------------------------------------------------------------------------------- the sieve
// One cell = one (start, fragment length) pair of SimulateFromGivenBlock's double loop (Simulator.cpp:2290-2350), one
// allele, no variants.  Returns the number of pairs; cnt[j] / strand_of[j] describe the chosen strands in draw order.
struct SieveSite {
    uint32_t seq, start, L;
    uint64_t word_off;
    const double *thr;                 // thresholds of the sequence's coverage group: [insert_to][2]
    uint32_t group;                    // the coverage group
    uint32_t sur_start[3];
    bool have_start;
    uint32_t sub;                      // variants of any kind: pass at this start position and what the pass starts from
    VarStart st;
};

RSQ_HD uint32_t site_c1(const SieveSite &site) { return site.seq | (site.sub << 22); }

// Which cells of a start position pass the zero threshold (Simulator.cpp:2304-2306, Simulator.h:415-420).  The reference draws
// probability_chosen ~ U[0,1) for every (start, fragment length) and goes on iff it is >= thr1[length]: the cells are independent, one
// passes with probability 1 - thr1, and given that it passes probability_chosen ~ U[thr1, 1).  The same process drawn directly
// (hard part 3): with q[len] = product of thr1 over the lengths up to len (DevSim::gap_q), the first passing length
// behind cur-1 is the first one with q[len] <= u * q[cur-1] for one uniform u, found by bisection, and its probability_chosen is
// thr1 + v * (1 - thr1) for a second one -- 1 + passes Philox blocks per start position instead of one per four cells.
// Draw k of a start position: block (start, c1, k, 1<<28), u = u53(w0, w1), v = u53(w2, w3).  on_pass(length, probability_chosen).
// The walk reads three tables of the sequence's coverage group through `tab`: q(len), seg_end(len) and thr1(len) for insert_from <= len < insert_to.
// GapTables reads them where the pre-pass put them (the host emulation, the oracle port, the device's fallback); k_sieve_gaps_lds hands in its LDS copies.
struct GapTables {
    const double *q_;                  // DevSim::gap_q of the group
    const uint32_t *seg_end_;          // DevSim::gap_seg_end of the group
    const double *thr_;                // the group's thresholds, [insert_to][2]
    RSQ_HD double q(uint32_t len) const { return q_[len]; }
    RSQ_HD uint32_t seg_end(uint32_t len) const { return seg_end_[len]; }
    RSQ_HD double thr1(uint32_t len) const { return thr_[2u * len + 1u]; }
};
RSQ_HD GapTables gap_tables(const DevSim &S, const SieveSite &site) {
    return GapTables{S.gap_q + (size_t)site.group * S.insert_to, S.gap_seg_end + (size_t)site.group * S.insert_to, site.thr};
}
template <class T, class F>
RSQ_HD uint32_t sieve_gaps_in(const DevSim &S, const SieveSite &site, const T &tab, F &&on_pass) {
    const uint32_t c1 = site_c1(site);
    uint32_t cur = S.insert_from, k = 0, n = 0;
    while (cur < S.insert_to) {
        const Words w = philox(S.seed, site.start, c1, k++, kDomSieve << 28);
        const uint32_t e = tab.seg_end(cur);
        const double base = (cur == S.insert_from || tab.seg_end(cur - 1u) == cur) ? 1.0 : tab.q(cur - 1u);      // a segment starts from 1
        const double target = u53_to_unit(w.w0, w.w1) * base;
        uint32_t lo = cur, hi = e;                                  // q does not increase inside a segment
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tab.q(mid) <= target) hi = mid;
            else lo = mid + 1u;
        }
        if (lo < e) {
            const double thr1 = tab.thr1(lo);
            on_pass(lo, thr1 + u53_to_unit(w.w2, w.w3) * (1 - thr1));
            ++n;
            cur = lo + 1u;
        } else cur = e;                                             // nothing passes in this segment: the next one gets a fresh draw
    }
    return n;
}
template <class F>
RSQ_HD uint32_t sieve_gaps(const DevSim &S, const SieveSite &site, F &&on_pass) {
    return sieve_gaps_in(S, site, gap_tables(S, site), on_pass);
}

// the two surrounding factors of a cell from the reference: the start's surrounding is found once per site
RSQ_HD void surrounding_factors(const DevSim &S, SieveSite &site, uint32_t end, double &start_factor, double &end_factor) {
    if (!site.have_start) {
        surrounding_forward(S.ref_words, site.word_off, site.L, site.start, site.sur_start);
        site.have_start = true;
    }
    uint32_t sur_end[3];
    surrounding_reverse(S.ref_words, site.word_off, site.L, end - 1u, sur_end);     // :1820-1832
    start_factor = surrounding_bias(S.sur_bias, site.sur_start);
    end_factor = surrounding_bias(S.sur_bias, sur_end);
}
// factors(site, end, start_factor, end_factor): where the cell's surrounding factors come from
template <class Factors>
RSQ_HD uint32_t sieve_cell_with(const DevSim &S, SieveSite &site, uint32_t len, double probability_chosen, uint32_t (&cnt)[2], uint32_t (&strand_of)[2], Factors &&factors) {
    cnt[0] = cnt[1] = 0;
    strand_of[0] = strand_of[1] = 0;
    const double thr0 = site.thr[2u * len], thr1 = site.thr[2u * len + 1u];
    if (!(probability_chosen >= thr1)) return 0;                                    // Simulator.h:418-420
    const uint32_t non_zero_strands = binomial(2u, 1 - thr0, probability_chosen);   // Simulator.cpp:2307
    const uint32_t end = site.start + len;
    if (!non_zero_strands || !(end < site.L)) return 0;                             // :2308,:2318
    const Words w2 = philox(S.seed, site.start, site.seq, len, (kDomSieve << 28) | 1u);
    uint32_t n_chosen;
    if (non_zero_strands <= 1u) {                                                   // :1387-1391 DrawNAlleles(1) -> SelectAllele
        strand_of[0] = (uint32_t)(u32_to_unit(w2.w2) * 2.0) & 1u;
        n_chosen = 1;
    } else {                                                                        // :1392-1396 complement of the empty draw
        strand_of[0] = 0;
        strand_of[1] = 1;
        n_chosen = 2;
    }
    double start_factor, end_factor;
    factors(site, end, start_factor, end_factor);
    const uint32_t gc = percent_u32(ref_gc_count_prefix(S.ref_words, S.gc_prefix, site.word_off, site.start, end), len);   // :1858-1873
    uint32_t n_here = 0;
    for (uint32_t j = 0; j < n_chosen; ++j) {
        const double u = j ? u53_to_unit(w2.w2, w2.w3) : u53_to_unit(w2.w0, w2.w1);
        const double adjusted_random = thr0 + u * (1 - thr0);                       // :2322
        cnt[j] = fragment_counts_from(S, site.seq, len, gc, start_factor, end_factor, adjusted_random);
        n_here += cnt[j];
    }
    return n_here;
}
RSQ_HD uint32_t sieve_cell(const DevSim &S, SieveSite &site, uint32_t len, double probability_chosen, uint32_t (&cnt)[2], uint32_t (&strand_of)[2]) {
    return sieve_cell_with(S, site, len, probability_chosen, cnt, strand_of,
                           [&S](SieveSite &st, uint32_t end, double &start_factor, double &end_factor) { surrounding_factors(S, st, end, start_factor, end_factor); });
}

// ---- the cell with variants (substitutions only): every allele is a copy of the packed reference with its substitutions applied, so
// the per-allele GC modification and the surrounding edits of Simulator.cpp:1404-1896 are plain reads of that copy -- what the
// reference's own test demands of them (SimulatorTest.cpp:116-195 compares with the sequence that has the variants applied).
constexpr uint32_t kMaxDevAlleles = 128;           // Reference::Variant::kMaxAlleles: 2 * alleles (allele, strand) slots per cell, in scratch memory
template <uint32_t CAP>                            // CAP alleles at most: small sets keep the cell in registers (k_sieve_finish<VM, 8>)
struct VarCellT {
    uint32_t n;                                    // chosen (allele, strand) slots with pairs, in draw order
    uint16_t cnt[2 * CAP];
    uint8_t id[2 * CAP];                           // allele * 2 + strand
};
using VarCell = VarCellT<kMaxDevAlleles>;
// SelectAllele (Simulator.cpp:1341-1361); reverse_selection as a bit mask over the 2 * alleles slots
template <uint32_t CAP>
struct SlotMaskT {
    static constexpr uint32_t kWords = (2 * CAP + 31) / 32;
    uint32_t w[kWords];
    RSQ_HD void set_first(uint32_t n) {
        for (uint32_t i = 0; i < kWords; ++i) w[i] = n >= 32u * (i + 1u) ? 0xFFFFFFFFu : (n > 32u * i ? (1u << (n - 32u * i)) - 1u : 0u);
    }
    RSQ_HD bool test(uint32_t id) const { return (w[id >> 5] >> (id & 31u)) & 1u; }
    RSQ_HD void clear(uint32_t id) { w[id >> 5] &= ~(1u << (id & 31u)); }
};
template <class Mask>
RSQ_HD void select_allele(uint8_t *chosen, uint32_t &n_chosen, Mask &selectable, uint32_t possible_strands, double random_value) {
    uint32_t chosen_id = (uint32_t)(uint16_t)(random_value * (possible_strands - n_chosen));
    uint32_t replacement_correction = 0;
    for (uint32_t i = 0; i < n_chosen; ++i)
        if (chosen[i] <= chosen_id) ++replacement_correction;
    while (replacement_correction)
        if (selectable.test(++chosen_id)) --replacement_correction;
    chosen[n_chosen++] = (uint8_t)chosen_id;
    selectable.clear(chosen_id);
}
RSQ_HD uint32_t word_of(const Words &w, uint32_t k) { return k == 0u ? w.w0 : (k == 1u ? w.w1 : (k == 2u ? w.w2 : w.w3)); }
// Streams (DESIGN.md "Random streams", rows "with variants"): SelectAllele's j-th value = word j&3 of block (start, seq, length,
// 1<<28 | 2 + (j>>2)); the count uniform of the j-th chosen slot = u53 of words 2(j&1), 2(j&1)+1 of block (.., 1<<28 | 128 + (j>>1)).
template <uint32_t CAP>
RSQ_HD uint32_t sieve_cell_var(const DevSim &S, const SieveSite &site, uint32_t len, double probability_chosen, VarCellT<CAP> &cell) {
    cell.n = 0;
    const double thr0 = site.thr[2u * len], thr1 = site.thr[2u * len + 1u];
    if (!(probability_chosen >= thr1)) return 0;                                    // Simulator.h:418-420
    const uint32_t possible_strands = 2u * S.num_alleles;                           // no deletions: every allele is possible (:1330-1340)
    const uint32_t non_zero_strands = binomial(possible_strands, 1 - thr0, probability_chosen);
    const uint32_t end = site.start + len;                                          // end_pos_shift_ is 0 without insertions and deletions
    if (!non_zero_strands || !(end < site.L)) return 0;
    uint8_t chosen[2 * CAP];
    uint32_t n_chosen = 0, n_draws = 0;
    SlotMaskT<CAP> selectable;
    selectable.set_first(possible_strands);
    const bool direct = non_zero_strands <= possible_strands / 2u;                  // ChooseAlleles :1387-1397
    const uint32_t to_draw = direct ? non_zero_strands : possible_strands - non_zero_strands;
    Words ws{0, 0, 0, 0};
    while (n_chosen < to_draw) {
        if (0u == (n_draws & 3u)) ws = philox(S.seed, site.start, site.seq, len, (kDomSieve << 28) | (2u + (n_draws >> 2)));
        select_allele(chosen, n_chosen, selectable, possible_strands, u32_to_unit(word_of(ws, n_draws & 3u)));
        ++n_draws;
    }
    if (!direct) {                                                                  // ReverseSelection :1373-1385
        n_chosen = 0;
        for (uint32_t id = 0; id < possible_strands; ++id)
            if (selectable.test(id)) chosen[n_chosen++] = (uint8_t)id;
    }
    uint32_t n_here = 0;
    Words wc{0, 0, 0, 0};
#pragma unroll 1                                                                   // unrolled over the 16 slots the loop body's gathers and the count draw took 361 vector registers
    for (uint32_t j = 0; j < n_chosen; ++j) {
        const uint32_t allele = chosen[j] >> 1;
        const uint64_t *words = hap_words(S, allele);
        uint32_t sur_start[3], sur_end[3];
        surrounding_forward(words, site.word_off, site.L, site.start, sur_start, S.ref_words);       // bias_mod.surrounding_start_.at(allele)
        surrounding_reverse(words, site.word_off, site.L, end - 1u, sur_end, S.ref_words);           // bias_mod.surrounding_end_.at(allele)
        const uint32_t gc = percent_u32(ref_gc_count_prefix(words, hap_gc_prefix(S, allele), site.word_off, site.start, end), len);   // GetGCPercent with gc_mod_
        if (0u == (j & 1u)) wc = philox(S.seed, site.start, site.seq, len, (kDomSieve << 28) | (128u + (j >> 1)));
        const double u = (j & 1u) ? u53_to_unit(wc.w2, wc.w3) : u53_to_unit(wc.w0, wc.w1);
        const double adjusted_random = thr0 + u * (1 - thr0);                       // :2322
        const uint32_t c = fragment_counts(S, site.seq, len, gc, sur_start, sur_end, adjusted_random);
        if (c) {
            cell.id[cell.n] = chosen[j];
            cell.cnt[cell.n] = (uint16_t)c;
            ++cell.n;
            n_here += c;
        }
    }
    return n_here;
}

// the cell with variants of any kind: possible alleles, ChooseAlleles, and per chosen (allele, strand) the allele's own stretch (rsq_variants.h)
template <uint32_t CAP>
RSQ_HD uint32_t sieve_cell_general(const DevSim &S, const SieveSite &site, uint32_t len, double probability_chosen, VarCellT<CAP> &cell) {
    cell.n = 0;
    const double thr0 = site.thr[2u * len], thr1 = site.thr[2u * len + 1u];
    if (!(probability_chosen >= thr1)) return 0;
    const VarView r = var_view(S, site.seq);
    uint8_t possible[CAP];
    uint32_t n_possible = 0;
    for (uint32_t allele = 0; allele < S.num_alleles; ++allele)                     // GetPossibleAlleles :1330-1340
        if (allele_starts_here(r, site.st, allele, site.start)) possible[n_possible++] = (uint8_t)allele;
    const uint32_t possible_strands = 2u * n_possible;
    const uint32_t non_zero_strands = binomial(possible_strands, 1 - thr0, probability_chosen);
    if (!non_zero_strands) return 0;
    const uint32_t c1 = site_c1(site);
    uint8_t chosen[2 * CAP];
    uint32_t n_chosen = 0, n_draws = 0;
    SlotMaskT<CAP> selectable;
    selectable.set_first(possible_strands);
    const bool direct = non_zero_strands <= possible_strands / 2u;
    const uint32_t to_draw = direct ? non_zero_strands : possible_strands - non_zero_strands;
    Words ws{0, 0, 0, 0};
    while (n_chosen < to_draw) {
        if (0u == (n_draws & 3u)) ws = philox(S.seed, site.start, c1, len, (kDomSieve << 28) | (2u + (n_draws >> 2)));
        select_allele(chosen, n_chosen, selectable, possible_strands, u32_to_unit(word_of(ws, n_draws & 3u)));
        ++n_draws;
    }
    if (!direct) {
        n_chosen = 0;
        for (uint32_t id = 0; id < possible_strands; ++id)
            if (selectable.test(id)) chosen[n_chosen++] = (uint8_t)id;
    }
    uint32_t n_here = 0;
    Words wc{0, 0, 0, 0};
    for (uint32_t j = 0; j < n_chosen; ++j) {
        const uint32_t allele = possible[chosen[j] >> 1], strand = chosen[j] & 1u;
        if (0u == (j & 1u)) wc = philox(S.seed, site.start, c1, len, (kDomSieve << 28) | (128u + (j >> 1)));
        const AlleleView a = allele_view(S, site.seq, allele);
        const AlleleCell ac = allele_cell(a, site.st, site.start, len);
        if (!ac.inside) continue;                                                   // :2318
        uint32_t sur_start[3], sur_end[3];
        allele_surrounding_forward(a, ac.hs, sur_start, ac.first_entries);          // bias_mod.surrounding_start_.at(allele)
        allele_surrounding_reverse(a, ac.he - 1, sur_end, ac.last_entries);         // bias_mod.surrounding_end_.at(allele)
        const double u = (j & 1u) ? u53_to_unit(wc.w2, wc.w3) : u53_to_unit(wc.w0, wc.w1);
        const double adjusted_random = thr0 + u * (1 - thr0);
        const uint32_t c = fragment_counts(S, site.seq, len, ac.gc_percent, sur_start, sur_end, adjusted_random);
        if (c) {
            cell.id[cell.n] = (uint8_t)(allele * 2u + strand);
            cell.cnt[cell.n] = (uint16_t)c;
            ++cell.n;
            n_here += c;
        }
    }
    return n_here;
}

// a cell that passed the zero threshold: (start position slot, fragment length) and its probability_chosen, in loop order
struct SieveCand {
    uint32_t slot, len;
    double probability_chosen;
};
// a cell with fragments, recorded by the sieve pass and expanded into Fragment records after the scan (with variants: one record per
// two chosen (allele, strand) slots of the cell)
struct SieveHit {
    uint32_t slot;         // start position slot of the batch
    uint32_t cand;         // the cell: index in the batch's candidate list
    uint32_t intra;        // pairs of the same cell that come before this record's
    uint16_t len, cnt0, cnt1;
    uint8_t strand0, strand1, allele0, allele1;
};

RSQ_HD Fragment make_fragment(const SieveSite &site, uint32_t len, uint32_t dup, uint32_t strand, uint32_t block_id, uint32_t number, uint32_t allele = 0) {
    Fragment f;
    f.seq = site.seq;
    f.start = site.start;
    f.len = len;
    f.dup = (uint16_t)dup;
    f.strand = (uint8_t)strand;
    f.allele = (uint8_t)allele;
    f.block = block_id;
    f.number = number;
    return f;
}

RSQ_HD void init_site(const DevSim &S, uint32_t block_id, uint32_t offset_in_block, SieveSite &site) {
    site.seq = S.block_seq[block_id];
    site.L = S.seq_len[site.seq];
    site.start = (block_id - S.first_block[site.seq]) * kBlockSize + offset_in_block;
    site.word_off = S.seq_word_off[site.seq];
    site.group = S.coverage_group[site.seq];
    site.thr = S.thresholds + (size_t)site.group * S.insert_to * 2u;
    site.have_start = false;
    site.sub = 0;
    site.st = VarStart{0, 0};
}

// Slots of a batch.  VM 0 / 1 (no variants / substitutions): slot = block * 1000 + offset.  VM 2 (variants of any kind): a block has
// its 1000 start positions plus the extra passes inside inserted bases (DevSim::extra), merged in loop order -- the extra pass j of a
// block (0-based, extras sorted) sits at local index (pos - block start) + j + 1.  Returns the block id; first_slot_of_block = the
// batch slot of the block's first position.
struct SlotInfo {                      // VM 2: what init_site_slot finds for a slot, written once per batch by k_slot_table
    uint32_t block_id, offset_in_block, sub, first_slot;
    int32_t first_variant_id;
    uint32_t start_variant_pos;
};
template <int VM, bool NEED_START = true>                             // NEED_START false: only the position and the pass (what the cell's random stream needs)
RSQ_HD uint32_t init_site_slot(const DevSim &S, uint32_t block_lo, uint32_t block_hi, uint32_t slot, SieveSite &site, uint32_t *first_slot_of_block = nullptr,
                               const SlotInfo *table = nullptr) {
    if (VM == 2 && table) {
        const SlotInfo t = table[slot];
        init_site(S, t.block_id, t.offset_in_block, site);
        site.sub = t.sub;
        site.st = VarStart{t.first_variant_id, t.start_variant_pos};
        if (first_slot_of_block) *first_slot_of_block = t.first_slot;
        return t.block_id;
    }
    if constexpr (VM != 2) {
        const uint32_t block_id = block_lo + slot / kBlockSize;
        init_site(S, block_id, slot % kBlockSize, site);
        if (first_slot_of_block) *first_slot_of_block = slot - slot % kBlockSize;
        return block_id;
    } else {
        const uint32_t base_lo = S.block_extra_ptr[block_lo];
        uint32_t lo = block_lo, hi = block_hi;                      // the last block b with (b - block_lo) * 1000 + extras before b <= slot
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((mid - block_lo) * kBlockSize + (S.block_extra_ptr[mid] - base_lo) <= slot) lo = mid;
            else hi = mid;
        }
        const uint32_t block_id = lo, first = (block_id - block_lo) * kBlockSize + (S.block_extra_ptr[block_id] - base_lo), local = slot - first;
        if (first_slot_of_block) *first_slot_of_block = first;
        const ExtraStart *e = S.extra + S.block_extra_ptr[block_id];
        const uint32_t m = S.block_extra_ptr[block_id + 1] - S.block_extra_ptr[block_id];
        const uint32_t seq = S.block_seq[block_id], bs = (block_id - S.first_block[seq]) * kBlockSize;
        uint32_t a = 0, b = m;                                       // c = extras whose local index is below `local`
        while (a < b) {
            const uint32_t mid = (a + b) >> 1;
            if ((e[mid].pos - bs) + mid + 1u < local) a = mid + 1u;
            else b = mid;
        }
        const uint32_t c = a;
        if (c < m && (e[c].pos - bs) + c + 1u == local) {
            init_site(S, block_id, e[c].pos - bs, site);
            site.sub = e[c].sub;
            site.st = VarStart{e[c].first_variant_id, e[c].start_variant_pos};
        } else {
            init_site(S, block_id, local - c, site);
            if (NEED_START && site.start < site.L) site.st = VarStart{(int32_t)var_view(S, seq).lower_bound(site.start), 0u};      // bias_mod.first_variant_id_ at a plain position
        }
        return block_id;
    }
}

#if RSQ_DEVICE_BUILD
// The sieve.
//   k_sieve_gaps<VM, false>: one lane per start position slot counts the cells that pass the zero threshold (sieve_gaps);
//   exclusive scan of the counts;
//   k_sieve_gaps<VM, true>: the same walk again writes the batch's candidate list, (slot, length, probability_chosen) in loop order;
//   k_sieve_finish: one lane per candidate -- full lanes -- runs the expensive part (strand / allele choice, G/C percent, surroundings,
//            negative binomial counts), records the cells with fragments in `hits` and the pairs of every candidate in pairs_of;
//   exclusive scan of pairs_of: the candidates are in the order of the reference's loops (block, start, pass, length), so the scan is
//            the position of a cell's first Fragment; k_sieve_emit writes the records (chosen strand order, duplicate).  No atomic
//            decides an order, hence deterministic read ids.
constexpr uint32_t kSieveBlock = 256;

// variants of any kind: what init_site_slot<2> finds, once per slot and batch.  One workgroup per block of 1000 start positions: the
// searches over all blocks / all variants happen once per block, the per-slot ones only over the block's own few extra starts and variants.
__global__ void __launch_bounds__(256) k_slot_table(DevSim S, uint32_t block_lo, SlotInfo *out) {
    const uint32_t block_id = block_lo + blockIdx.x, base_lo = S.block_extra_ptr[block_lo];
    const uint32_t first_slot = (block_id - block_lo) * kBlockSize + (S.block_extra_ptr[block_id] - base_lo);
    const ExtraStart *e = S.extra + S.block_extra_ptr[block_id];
    const uint32_t m = S.block_extra_ptr[block_id + 1] - S.block_extra_ptr[block_id];
    const uint32_t seq = S.block_seq[block_id], bs = (block_id - S.first_block[seq]) * kBlockSize, L = S.seq_len[seq];
    const VarView r = var_view(S, seq);
    __shared__ uint32_t s_v[2];
    if (threadIdx.x < 2) s_v[threadIdx.x] = r.lower_bound(bs + threadIdx.x * kBlockSize);
    __syncthreads();
    const uint32_t v0 = s_v[0], v1 = s_v[1];                       // the block's variants
    for (uint32_t local = threadIdx.x; local < kBlockSize + m; local += blockDim.x) {
        uint32_t a = 0, b = m;                                      // extras whose local index is below `local`
        while (a < b) {
            const uint32_t mid = (a + b) >> 1;
            if ((e[mid].pos - bs) + mid + 1u < local) a = mid + 1u;
            else b = mid;
        }
        SlotInfo t;
        t.block_id = block_id;
        t.first_slot = first_slot;
        if (a < m && (e[a].pos - bs) + a + 1u == local) {
            t.offset_in_block = e[a].pos - bs;
            t.sub = e[a].sub;
            t.first_variant_id = e[a].first_variant_id;
            t.start_variant_pos = e[a].start_variant_pos;
        } else {
            t.offset_in_block = local - a;
            t.sub = 0;
            const uint32_t pos = bs + t.offset_in_block;
            uint32_t lo = v0, hi = v1;                              // first variant at or after the position (none of it is used beyond the sequence)
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (r.v[mid].pos < pos) lo = mid + 1u;
                else hi = mid;
            }
            t.first_variant_id = pos < L ? (int32_t)lo : 0;
            t.start_variant_pos = 0;
        }
        out[first_slot + local] = t;
    }
}

// one lane's walk: the count of its start position slot, or its candidates from cand_off[slot] on
template <bool FILL, class T>
__device__ __forceinline__ void sieve_gaps_lane(const DevSim &S, const SieveSite &site, const T &tab, uint32_t slot, uint32_t *counts, const uint64_t *cand_off, SieveCand *cands,
                                                uint64_t cand_cap) {
    if constexpr (FILL) {
        uint64_t at = cand_off[slot];
        sieve_gaps_in(S, site, tab, [&](uint32_t len, double probability_chosen) {
            if (at < cand_cap) cands[at] = SieveCand{slot, len, probability_chosen};
            ++at;
        });
    } else counts[slot] = sieve_gaps_in(S, site, tab, [](uint32_t, double) {});
}

template <int VM, bool FILL>
__global__ void __launch_bounds__(kSieveBlock) k_sieve_gaps(DevSim S, uint32_t block_lo, uint32_t block_hi, uint32_t n_slots, uint32_t *counts, const uint64_t *cand_off,
                                                            SieveCand *cands, uint64_t cand_cap, const SlotInfo *slots) {
    const uint32_t slot = blockIdx.x * kSieveBlock + threadIdx.x;
    if (slot >= n_slots) return;
    SieveSite site;
    init_site_slot<VM, false>(S, block_lo, block_hi, slot, site, nullptr, slots);
    if (!(site.start < site.L)) {                                   // the last block of a sequence is shorter
        if constexpr (!FILL) counts[slot] = 0;
        return;
    }
    sieve_gaps_lane<FILL>(S, site, gap_tables(S, site), slot, counts, cand_off, cands, cand_cap);
}

// The same walk on LDS copies of the group's tables.  A lane's walk is a chain of about fourteen loads per draw, each at the lane's own length: from memory every
// one of them occupies the CU's vector-memory path for a wave-level load, from LDS a few cycles.  A workgroup stages q, thr1 and seg_end of one coverage group over
// [insert_from, insert_to) -- 20 bytes per length, dynamic LDS -- and serves kSieveTilesPerGroup consecutive tiles of 256 slots with them; it stages again where a
// tile begins in a sequence of another group.  Lanes of a tile whose sequence belongs to another group than the tile's first slot (a tile can straddle two
// sequences) walk the tables in memory, as k_sieve_gaps does.  Draws, bisection and candidate order are sieve_gaps_in's in both.
constexpr uint32_t kSieveTilesPerGroup = 4;
constexpr uint32_t kSieveLdsPerLength = 20;
constexpr size_t kSieveLdsLimit = 64u << 10;                     // what a workgroup can have without asking for more
struct GapTablesLds {
    const double *q_, *thr1_;          // [insert_to - insert_from]
    const uint32_t *seg_end_;
    uint32_t from;
    __device__ double q(uint32_t len) const { return q_[len - from]; }
    __device__ uint32_t seg_end(uint32_t len) const { return seg_end_[len - from]; }
    __device__ double thr1(uint32_t len) const { return thr1_[len - from]; }
};
template <int VM, bool FILL>
__global__ void __launch_bounds__(kSieveBlock) k_sieve_gaps_lds(DevSim S, uint32_t block_lo, uint32_t block_hi, uint32_t n_slots, uint32_t *counts, const uint64_t *cand_off,
                                                                SieveCand *cands, uint64_t cand_cap, const SlotInfo *slots) {
    extern __shared__ double s_gap_tables[];                        // q | thr1 | seg_end
    const uint32_t from = S.insert_from, n_len = S.insert_to - from;
    double *s_q = s_gap_tables, *s_thr1 = s_gap_tables + n_len;
    uint32_t *s_seg_end = reinterpret_cast<uint32_t *>(s_gap_tables + 2u * n_len);
    const GapTablesLds lds{s_q, s_thr1, s_seg_end, from};
    const uint32_t n_tiles = (n_slots + kSieveBlock - 1u) / kSieveBlock;
    const uint32_t tile_lo = blockIdx.x * kSieveTilesPerGroup, tile_hi = tile_lo + kSieveTilesPerGroup < n_tiles ? tile_lo + kSieveTilesPerGroup : n_tiles;
    uint32_t staged = 0xFFFFFFFFu;                                  // the group whose tables are in LDS; the same in every lane of the workgroup
    for (uint32_t tile = tile_lo; tile < tile_hi; ++tile) {
        SieveSite first;
        init_site_slot<VM, false>(S, block_lo, block_hi, tile * kSieveBlock, first, nullptr, slots);
        if (first.group != staged) {
            __syncthreads();                                        // the tile before is walked to its end
            const GapTables mem = gap_tables(S, first);
            for (uint32_t i = threadIdx.x; i < n_len; i += kSieveBlock) {
                s_q[i] = mem.q(from + i);
                s_thr1[i] = mem.thr1(from + i);
                s_seg_end[i] = mem.seg_end(from + i);
            }
            staged = first.group;
            __syncthreads();
        }
        const uint32_t slot = tile * kSieveBlock + threadIdx.x;
        if (slot >= n_slots) continue;
        SieveSite site;
        init_site_slot<VM, false>(S, block_lo, block_hi, slot, site, nullptr, slots);
        if (!(site.start < site.L)) {                               // the last block of a sequence is shorter
            if constexpr (!FILL) counts[slot] = 0;
        } else if (site.group == staged) sieve_gaps_lane<FILL>(S, site, lds, slot, counts, cand_off, cands, cand_cap);
        else sieve_gaps_lane<FILL>(S, site, gap_tables(S, site), slot, counts, cand_off, cands, cand_cap);
    }
}

// The surrounding factors of every position of [lo, hi) of the concatenated sequences, kept from the pre-pass (k_surrounding_bias_tracks): surrounding_bias itself of the
// position's start and end surroundings.  Without variants the candidate kernel takes a cell's two factors from them -- two loads that neighbouring lanes make near each
// other in place of six gathers in the 24 MB sur_bias table and two exp -- and computes them where the cell lies outside (lo == hi: no tracks).
struct BiasTracks {
    const double *start_bias, *end_bias;
    uint64_t lo, hi;
};

// The cells with fragments go into the hit list.  Their order in the list is free (k_sieve_emit places fragments by the scan of pairs_of), so places are taken with an
// atomic counter -- ONE reservation per workgroup: a counter bumped once per wave (557 k times per 10 M pairs) is a queue at one L2 channel, about 10 ns per
// atomic, and was what the kernel's 6.5 ms consisted of for two rounds (VALU 13 % busy, TA 54 %: "latency-bound").  Without variants there is no list at all
// (a cell has one record at most: a word per candidate, k_sieve_emit runs over the candidates).
template <int VM, uint32_t CAP = kMaxDevAlleles>
__global__ void __launch_bounds__(kSieveBlock) k_sieve_finish(DevSim S, uint32_t block_lo, uint32_t block_hi, uint32_t n_slots, const uint64_t *cand_off, const SieveCand *cands,
                                                              uint64_t cand_cap, uint32_t *pairs_of, SieveHit *hits, uint32_t hit_cap, uint32_t *hit_count, const SlotInfo *slots,
                                                              uint32_t *cell_info, BiasTracks tracks) {
    __shared__ uint32_t s_records, s_base;
    if (threadIdx.x == 0) s_records = 0;
    __syncthreads();
    const uint64_t c = (uint64_t)blockIdx.x * kSieveBlock + threadIdx.x;
    const bool has_cell = c < cand_cap && c < cand_off[n_slots];
    uint32_t n_here = 0, n_records = 0;                             // pairs of the cell; its records: one per two chosen (allele, strand) slots
    SieveCand cand{};
    VarCellT<VM != 0 ? CAP : 1u> cell;                              // VM 0: the two strands' counts in cnt[0..1], their strands in id[0..1]
    cell.n = 0;
    if (has_cell) {
        cand = cands[c];
        SieveSite site;
        init_site_slot<VM>(S, block_lo, block_hi, cand.slot, site, nullptr, slots);
        if constexpr (VM == 2) n_here = sieve_cell_general(S, site, cand.len, cand.probability_chosen, cell);
        else if constexpr (VM == 1) n_here = sieve_cell_var(S, site, cand.len, cand.probability_chosen, cell);
        else {
            uint32_t cnt[2], strand_of[2];
            n_here = sieve_cell_with(S, site, cand.len, cand.probability_chosen, cnt, strand_of, [&](SieveSite &st, uint32_t end, double &start_factor, double &end_factor) {
                const uint64_t at = S.seq_base_off[st.seq] + st.start, at_end = S.seq_base_off[st.seq] + end - 1u;      // k_sum_bias's indices
                if (at >= tracks.lo && at_end < tracks.hi) {
                    start_factor = tracks.start_bias[at - tracks.lo];
                    end_factor = tracks.end_bias[at_end - tracks.lo];
                } else surrounding_factors(S, st, end, start_factor, end_factor);
            });
            cell.n = n_here ? 2u : 0u;
            for (uint32_t e = 0; e < 2u; ++e) {
                cell.cnt[e] = (uint16_t)cnt[e];
                cell.id[e] = (uint8_t)strand_of[e];                 // allele 0
            }
        }
        n_records = (cell.n + 1u) / 2u;
    }
    if constexpr (VM == 0) {
        // without variants a cell has one record at most: no list -- what k_sieve_emit needs beyond pairs_of goes into a word per candidate (coalesced), and the
        // emit kernel runs over the candidates
        if (c < cand_cap) {
            pairs_of[c] = n_here;
            cell_info[c] = (uint32_t)cell.cnt[0] | ((uint32_t)(cell.id[0] & 1u) << 16) | ((uint32_t)(cell.id[1] & 1u) << 17);
        }
        return;
    }
    const uint32_t rank = n_records ? atomicAdd(&s_records, n_records) : 0u;
    __syncthreads();
    if (threadIdx.x == 0 && s_records) s_base = atomicAdd(hit_count, s_records);
    __syncthreads();
    uint32_t intra = 0;
    for (uint32_t e = 0; e < cell.n; e += 2u) {
        const bool two = e + 1u < cell.n;
        const uint32_t at = s_base + rank + e / 2u;
        SieveHit h;
        h.slot = cand.slot;
        h.cand = (uint32_t)c;
        h.intra = intra;
        h.len = (uint16_t)cand.len;
        h.cnt0 = cell.cnt[e];
        h.cnt1 = two ? cell.cnt[e + 1u] : (uint16_t)0;
        h.strand0 = cell.id[e] & 1u;
        h.allele0 = cell.id[e] >> 1;
        h.strand1 = two ? cell.id[e + 1u] & 1u : 0;
        h.allele1 = two ? cell.id[e + 1u] >> 1 : 0;
        if (at < hit_cap) hits[at] = h;
        intra += (uint32_t)h.cnt0 + h.cnt1;
    }
    if (c < cand_cap) pairs_of[c] = n_here;
}

// one lane per recorded cell: writes its cnt0 + cnt1 Fragment records at pair_off[cell] + intra; a read's number counts the pairs of
// its block (CreateReadId, Simulator.cpp:596-632): the block's first cell is the first candidate of its first slot
// VM 0: one lane per CANDIDATE (n_hits = their number): the cell's record is put together from pairs_of, cell_info and the candidate itself
template <int VM>
__global__ void __launch_bounds__(256) k_sieve_emit(DevSim S, uint32_t block_lo, uint32_t block_hi, const SieveHit *hits, uint32_t n_hits, const uint64_t *cand_off,
                                                   const uint64_t *pair_off, Fragment *frags, FragmentVar *fvars, const SlotInfo *slots, const SieveCand *cands = nullptr,
                                                   const uint32_t *pairs_of = nullptr, const uint32_t *cell_info = nullptr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_hits) return;
    SieveHit h;
    if constexpr (VM == 0) {
        const uint32_t pairs = pairs_of[i];
        if (!pairs) return;
        const SieveCand cand = cands[i];
        const uint32_t info = cell_info[i];
        h.slot = cand.slot;
        h.cand = i;
        h.intra = 0;
        h.len = (uint16_t)cand.len;
        h.cnt0 = (uint16_t)(info & 0xFFFFu);
        h.cnt1 = (uint16_t)(pairs - (info & 0xFFFFu));
        h.strand0 = (uint8_t)((info >> 16) & 1u);
        h.strand1 = (uint8_t)((info >> 17) & 1u);
        h.allele0 = h.allele1 = 0;
    } else h = hits[i];
    SieveSite site;
    uint32_t first_slot;
    const uint32_t block_id = init_site_slot<VM>(S, block_lo, block_hi, h.slot, site, &first_slot, slots);
    const uint64_t base = pair_off[h.cand];
    const uint32_t number_base = (uint32_t)(base - pair_off[cand_off[first_slot]]);
    uint32_t k = h.intra;
    for (uint32_t e = 0; e < 2u; ++e) {
        const uint32_t cnt = e ? h.cnt1 : h.cnt0, strand = e ? h.strand1 : h.strand0, allele = e ? h.allele1 : h.allele0;
        if (!cnt) continue;
        FragmentVar fv{};
        if constexpr (VM == 2) {                                    // what SimulateFromGivenBlock hands to CreateReads (:2334-2337), derived again
            const AlleleCell ac = allele_cell(allele_view(S, site.seq, allele), site.st, site.start, h.len);
            fv.end = ac.end;
            fv.sub = site.sub;
            fv.start_var = site.st.first_variant_id;
            fv.start_var_pos = site.st.start_variant_pos;
            fv.end_var = ac.end_var.first_variant_id;
            fv.end_var_pos = ac.end_var.start_variant_pos;
        }
        for (uint32_t dup = 0; dup < cnt; ++dup, ++k) {
            frags[base + k] = make_fragment(site, h.len, dup, strand, block_id, number_base + k + 1u, allele);
            if constexpr (VM == 2) fvars[base + k] = fv;
        }
    }
}
#endif

}  // namespace rsq
