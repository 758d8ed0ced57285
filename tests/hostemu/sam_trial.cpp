// sam_trial.cpp -- TEST-ONLY: the per-lane functions of the truth alignments (rsq_sam.h: sam_walk, sam_align, sam_record_size, sam_record) on rows the caller
// crafts, on the CPU, beside the FASTQ records the same rows give (rsq_text.h format_record).  tests/test_truth_sam.py compiles it with g++ and compares the
// SAM text with a Python statement of the record's rules applied to that FASTQ text.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_sam.h"

using namespace rsq;

extern "C" {

struct sam_trial_mate {
    uint32_t read_len, n_iter_m, n_iter_s, hard_clip, num_errors;
    const uint8_t *seq;       // read_len base codes 0..4
    const uint8_t *qual;      // read_len characters, the profile's offset included
    const uint8_t *ops;       // n_iter_m + n_iter_s codes: 0 the part's own op (M / S), 1 D, 2 I
};
struct sam_trial_pair {
    int32_t has_fragment;     // 0: an adapter-only pair with number `adapter_only_number`
    uint32_t seq, start, len, strand, block, number;
    uint64_t adapter_only_number;
    uint32_t phred_offset, tile;
    const char *base_identifier;
    const char *names;        // the reference ids' first parts, one after the other
    const uint32_t *name_ptr; // their offsets (one more than there are names)
    sam_trial_mate mate[2];
};

// fastq[seg] / sam receive the texts (both SAM records, segment 0 first); sizes: {fastq 0, fastq 1, sam record 0, sam record 1} as written, then the two
// sam_record_size values.  -1: a buffer is too small.
int sam_trial(const sam_trial_pair *in, char *fastq0, char *fastq1, char *sam, uint32_t cap, uint32_t *sizes) {
    DevSim S{};
    const uint16_t tiles[1] = {(uint16_t)in->tile};
    S.tiles = tiles;
    S.phred_offset = (uint8_t)in->phred_offset;
    S.num_alleles = 1;
    NameTable names{};
    names.names = in->names;
    names.name_ptr = in->name_ptr;
    names.base_len = (uint32_t)strlen(in->base_identifier);
    if (names.base_len > sizeof names.base_identifier) return -1;
    memcpy(names.base_identifier, in->base_identifier, names.base_len);
    Fragment f{};
    f.seq = in->seq;
    f.start = in->start;
    f.len = in->len;
    f.strand = (uint8_t)in->strand;
    f.block = in->block;
    f.number = in->number;
    const bool has_f = in->has_fragment != 0;

    std::vector<uint32_t> seq[2], qual[2], ops[2];
    ReadMeta meta[2];
    SamMate walk[2];
    for (int seg = 0; seg < 2; ++seg) {
        const sam_trial_mate &r = in->mate[seg];
        const uint32_t words = (r.read_len + 3u) / 4u, n_ops = r.n_iter_m + r.n_iter_s;
        seq[seg].assign(words + 1u, 0xA5A5A5A5u);                    // what lies behind a row's last character must not matter
        qual[seg].assign(words + 1u, 0xA5A5A5A5u);
        ops[seg].assign(n_ops / 16u + 2u, 0u);
        for (uint32_t i = 0; i < r.read_len; ++i) {
            seq[seg][i / 4u] = (seq[seg][i / 4u] & ~(0xFFu << (8u * (i & 3u)))) | ((uint32_t)r.seq[i] << (8u * (i & 3u)));
            qual[seg][i / 4u] = (qual[seg][i / 4u] & ~(0xFFu << (8u * (i & 3u)))) | ((uint32_t)r.qual[i] << (8u * (i & 3u)));
        }
        bool plain = true;
        for (uint32_t i = 0; i < n_ops; ++i) {
            ops[seg][i / 16u] |= (uint32_t)(r.ops[i] & 3u) << (2u * (i & 15u));
            plain = plain && !r.ops[i];
        }
        ReadMeta &m = meta[seg];
        m = ReadMeta{};
        m.read_len = (uint16_t)r.read_len;
        m.num_errors = (uint16_t)r.num_errors;
        m.n_iter_m = (uint16_t)r.n_iter_m;
        m.n_iter_s = (uint16_t)r.n_iter_s;
        m.hard_clip = (uint16_t)r.hard_clip;
        m.tile_id = 0;
        m.plain = plain ? 1 : 0;
        char cigar[4096];
        TextSink count(cigar, 0);
        cigar_replay(WordColumn{ops[seg].data(), 1}, m, count);
        m.cigar_chars = (uint16_t)count.n;
        walk[seg] = sam_walk(WordColumn{ops[seg].data(), 1}, m);
    }
    uint32_t sam_at = 0;
    for (int seg = 0; seg < 2; ++seg) {
        const ReadMeta &m = meta[seg];
        const WordColumn s{seq[seg].data(), 1}, q{qual[seg].data(), 1}, o{ops[seg].data(), 1};
        const Fragment *fp = has_f ? &f : nullptr;
        if (record_size(S, names, fp, in->adapter_only_number, m) > cap) return -1;
        sizes[seg] = format_record(S, names, fp, in->adapter_only_number, m, s, q, o, seg ? fastq1 : fastq0);
        const SamAlign a = sam_align(has_f, f, (uint32_t)seg, walk[0], walk[1]);
        sizes[4 + seg] = sam_record_size(S, names, has_f, f, in->adapter_only_number, m, walk[seg], a);
        if (sam_at + sizes[4 + seg] > cap) return -1;
        sizes[2 + seg] = sam_record(S, names, has_f, f, in->adapter_only_number, m, s, q, o, walk[seg], a, sam + sam_at);
        sam_at += sizes[2 + seg];
    }
    return 0;
}
}
