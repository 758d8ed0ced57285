// bam_trial.cpp -- TEST-ONLY: the per-lane functions of the truth alignments as BAM (rsq_bam.h: bam_mate, bam_record_size, bam_record, on top of rsq_sam.h's
// sam_walk and sam_align) on rows the caller crafts, on the CPU, beside the FASTQ records the same rows give (rsq_text.h format_record).  tests/test_truth_bam.py
// compiles it with g++, decodes the records back to SAM lines and compares them with its statement of the SAM record applied to that FASTQ text.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_bam.h"

using namespace rsq;

extern "C" {

struct bam_trial_mate {
    uint32_t read_len, n_iter_m, n_iter_s, hard_clip, num_errors;
    const uint8_t *seq;       // read_len base codes 0..4
    const uint8_t *qual;      // read_len characters, the profile's offset included
    const uint8_t *ops;       // n_iter_m + n_iter_s codes: 0 the part's own op (M / S), 1 D, 2 I
};
struct bam_trial_pair {
    int32_t has_fragment;     // 0: an adapter-only pair with number `adapter_only_number`
    uint32_t seq, start, len, strand, block, number;
    uint64_t adapter_only_number;
    uint32_t phred_offset, tile;
    const char *base_identifier;
    const char *names;        // the reference ids' first parts, one after the other
    const uint32_t *name_ptr; // their offsets (one more than there are names)
    bam_trial_mate mate[2];
};

// fastq[seg] / bam receive the texts and the records (segment 0 first, at bam + at); sizes: {fastq 0, fastq 1, bam record 0, bam record 1} as written, then the two
// bam_record_size values.  -1: a buffer is too small.  -2: the same records written as k_bam_write's lanes write them -- two ImageSinks a mate ORing into a zeroed
// image, the second starting at QUAL -- differ from bam_record's bytes.
int bam_trial(const bam_trial_pair *in, char *fastq0, char *fastq1, char *bam, uint32_t at, uint32_t cap, uint32_t *sizes) {
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
        const bam_trial_mate &r = in->mate[seg];
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
    uint32_t bam_at = at;
    for (int seg = 0; seg < 2; ++seg) {
        const ReadMeta &m = meta[seg];
        const WordColumn s{seq[seg].data(), 1}, q{qual[seg].data(), 1}, o{ops[seg].data(), 1};
        const Fragment *fp = has_f ? &f : nullptr;
        if (record_size(S, names, fp, in->adapter_only_number, m) > cap) return -1;
        sizes[seg] = format_record(S, names, fp, in->adapter_only_number, m, s, q, o, seg ? fastq1 : fastq0);
        const SamAlign a = sam_align(has_f, f, (uint32_t)seg, walk[0], walk[1]);
        const BamMate b = bam_mate(S, names, has_f, f, in->adapter_only_number, m, o, walk[seg], a);
        sizes[4 + seg] = bam_record_size(m, b.l_read_name, b.n_cigar);
        if (b.w.bytes != sizes[4 + seg] || bam_at + sizes[4 + seg] > cap) return -1;
        sizes[2 + seg] = bam_record(S, names, has_f, f, in->adapter_only_number, m, s, q, o, b, a, bam + bam_at);
        // the writer's lane roles on the host: half 0 up to and with SEQ, half 1 QUAL and tags, at the same unaligned place of a zeroed image
        std::vector<uint32_t> image((bam_at + sizes[2 + seg]) / 4u + 2u, 0u);
        RSQ_LDS char *text = reinterpret_cast<RSQ_LDS char *>(image.data()) + bam_at;
        ImageSink head(text);
        bam_head(S, names, has_f, f, in->adapter_only_number, m, s, o, b, a, head);
        head.finish();
        ImageSink tail(text + (b.w.bytes - bam_tags_size(m) - m.read_len));
        bam_qual(q, m.read_len, a.reverse != 0u, S.phred_offset, tail);
        bam_tags(m, o, tail);
        tail.finish();
        if (head.n + tail.n != sizes[2 + seg] || memcmp(text, bam + bam_at, sizes[2 + seg]) != 0) return -2;
        for (uint32_t i = 0; i < 4u * image.size(); ++i)
            if ((i < bam_at || i >= bam_at + sizes[2 + seg]) && reinterpret_cast<const char *>(image.data())[i]) return -2;
        bam_at += sizes[2 + seg];
    }
    return 0;
}
}
