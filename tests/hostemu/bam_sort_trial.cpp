// bam_sort_trial.cpp -- TEST-ONLY: the host-callable pieces of reseq_amd/csrc/rsq_bamsort.h on inputs the caller crafts (tests/test_truth_bam_sorted.py builds this with
// g++): the key of a mate, the sort as the passes' tile / digit / rank arithmetic run as a loop, the cut, the rules of the chunk runs and of the 16 kb windows
// applied call by call as the device applies them, and the .bai builder.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_bamsort.h"

using namespace rsq;

extern "C" {
struct bam_sort_trial_mate {
    uint32_t q, t, lead, trail, bytes;
};
// both mates' directory entries of a pair whose records begin at `pair_off`: out[seg] = {key, off, size, span}
void bam_sort_trial_entries(uint32_t seq, uint32_t start, uint32_t len, uint32_t strand, const bam_sort_trial_mate *mates, uint64_t pair_off, uint32_t n_seqs, uint64_t *out) {
    Fragment f{};
    f.seq = seq;
    f.start = start;
    f.len = len;
    f.strand = (uint8_t)strand;
    BamPair p{};
    for (uint32_t seg = 0; seg < 2u; ++seg) {
        p.mate[seg].w.q = (uint16_t)mates[seg].q;
        p.mate[seg].w.t = (uint16_t)mates[seg].t;
        p.mate[seg].w.lead = (uint16_t)mates[seg].lead;
        p.mate[seg].w.trail = (uint16_t)mates[seg].trail;
        p.mate[seg].w.bytes = mates[seg].bytes;
    }
    for (uint32_t seg = 0; seg < 2u; ++seg) {
        const BamDirEntry e = bam_dir_entry(f, seg, p, pair_off, n_seqs);
        out[4u * seg] = e.key;
        out[4u * seg + 1u] = e.off;
        out[4u * seg + 2u] = e.size;
        out[4u * seg + 3u] = e.span;
    }
}
uint64_t bam_sort_trial_key(uint32_t ref_id, uint32_t pos) { return bam_sort_key(ref_id, pos); }
uint64_t bam_sort_trial_unmapped_key(uint32_t n_seqs) { return bam_unmapped_key(n_seqs); }
uint32_t bam_sort_trial_tile(void) { return kBamSortTile; }
int bam_sort_trial_out_of_order(uint64_t key, uint64_t prev_cut, uint32_t n_seqs, uint32_t longest) {
    return bam_key_out_of_order(key, prev_cut, n_seqs, bam_sort_plan(n_seqs, longest).pos_bits) ? 1 : 0;
}
// order[k] = the index of the k-th record of the sorted stream, sorted[k] its key; returns the number of 8-bit passes (plan[0..1]: position bits, all bits)
uint32_t bam_sort_trial_sort(const uint64_t *keys, uint64_t n, uint32_t n_seqs, uint32_t longest, uint32_t *order, uint64_t *sorted, uint32_t *plan_out) {
    const BamSortPlan plan = bam_sort_plan(n_seqs, longest);
    std::vector<uint32_t> o;
    const std::vector<uint64_t> k = bam_sort_host(keys, n, plan, o);
    if (n) {
        memcpy(order, o.data(), n * 4u);
        memcpy(sorted, k.data(), n * 8u);
    }
    plan_out[0] = plan.pos_bits;
    plan_out[1] = plan.bits;
    return plan.passes;
}
// the records of sorted[0, n) that are final for a call that ends in front of `block`; *cut: the key they lie below
uint64_t bam_sort_trial_cut(const uint64_t *sorted, uint64_t n, uint32_t block, uint32_t total_blocks, uint32_t n_seqs, const uint32_t *block_seq, const uint32_t *first_block,
                            uint32_t block_size, uint64_t *cut) {
    *cut = bam_cut_key(block, total_blocks, n_seqs, block_seq, first_block, block_size);
    return bam_lower_bound(sorted, n, *cut);
}
// The .bai of a file whose mapped records -- in file order: keys[i], span[i], at the uncompressed offset at[i]; the last ends at at[n] -- left in calls of
// call_end[c] records so far (rising, the last = n).  Per call what k_bam_index_flags / k_bam_index_runs leave, merged as the library merges it.
// Returns the bytes needed; writes them if they fit.
uint64_t bam_sort_trial_index(uint32_t n_ref, const uint32_t *seq_len, uint64_t n, const uint64_t *keys, const uint32_t *span, const uint64_t *at, const uint64_t *call_end, uint32_t n_calls,
                              const uint64_t *block_u, const uint64_t *block_c, uint64_t n_blocks, uint64_t n_no_coor, char *out, uint64_t cap) {
    BamIndexState x;
    x.begin(std::vector<uint32_t>(seq_len, seq_len + n_ref));
    uint64_t first = 0;
    for (uint32_t c = 0; c < n_calls; ++c) {
        std::vector<BamRunStart> starts;
        for (uint64_t i = first; i < call_end[c]; ++i) {
            const BamDirEntry e{keys[i], 0, 0, span[i]};
            bool flag = i == first;
            if (!flag) {
                const BamDirEntry p{keys[i - 1u], 0, 0, span[i - 1u]};
                flag = (p.key >> 32) != (e.key >> 32) || bam_entry_bin(p) != bam_entry_bin(e);
            }
            if (flag) starts.push_back(BamRunStart{(uint32_t)(e.key >> 32), bam_entry_bin(e), at[i]});
            for (uint32_t w = bam_first_window(e); w <= bam_last_window(e); ++w) x.add_window((uint32_t)(e.key >> 32), w, at[i]);
        }
        x.add_runs(starts.data(), starts.size(), at[call_end[c]]);
        first = call_end[c];
    }
    const std::string bytes = bam_bai_bytes(x, block_u, block_c, (size_t)n_blocks, n_no_coor);
    if (bytes.size() <= cap) memcpy(out, bytes.data(), bytes.size());
    return bytes.size();
}
}
