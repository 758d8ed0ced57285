// truth_trial.h -- TEST-ONLY: the per-lane functions of the truth alignments in a format (rsq_sam.h SamFormat, rsq_bam.h BamFormat, on top of sam_walk and
// sam_align) on rows the caller crafts, on the CPU, beside the FASTQ records the same rows give (rsq_text.h format_record).  One trial over the format; sam_trial.cpp
// and bam_trial.cpp export it for theirs: tests/test_truth_sam.py builds the first with g++ and compares the SAM text with a Python statement of the record's rules
// applied to that FASTQ text, tests/test_truth_bam.py builds the second, decodes the BAM records back to SAM lines and compares them with the same statement.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_bam.h"

using namespace rsq;

extern "C" {
struct truth_trial_mate {
    uint32_t read_len, n_iter_m, n_iter_s, hard_clip, num_errors;
    const uint8_t *seq;       // read_len base codes 0..4
    const uint8_t *qual;      // read_len characters, the profile's offset included
    const uint8_t *ops;       // n_iter_m + n_iter_s codes: 0 the part's own op (M / S), 1 D, 2 I
};
struct truth_trial_pair {
    int32_t has_fragment;     // 0: an adapter-only pair with number `adapter_only_number`
    uint32_t seq, start, len, strand, block, number;
    uint64_t adapter_only_number;
    uint32_t phred_offset, tile;
    const char *base_identifier;
    const char *names;        // the reference ids' first parts, one after the other
    const uint32_t *name_ptr; // their offsets (one more than there are names)
    truth_trial_mate mate[2];
};
}

// fastq[seg] / out receive the texts and the records (segment 0 first, at out + at); sizes: {fastq 0, fastq 1, record 0, record 1} as written, then the two sizes
// Format::mate states.  -1: a buffer is too small.  -2: the same records written as k_truth_write's lanes write them -- two ImageSinks a mate ORing into a zeroed
// image, the second starting at Format::tail_at -- differ from Format::record's bytes, or touch what lies around them.
template <class Format>
static int truth_trial(const truth_trial_pair *in, char *fastq0, char *fastq1, char *out, uint32_t at, uint32_t cap, uint32_t *sizes) {
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
        const truth_trial_mate &r = in->mate[seg];
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
    for (int seg = 0; seg < 2; ++seg) {
        const ReadMeta &m = meta[seg];
        const WordColumn s{seq[seg].data(), 1}, q{qual[seg].data(), 1}, o{ops[seg].data(), 1};
        const Fragment *fp = has_f ? &f : nullptr;
        if (record_size(S, names, fp, in->adapter_only_number, m) > cap) return -1;
        sizes[seg] = format_record(S, names, fp, in->adapter_only_number, m, s, q, o, seg ? fastq1 : fastq0);
        const SamAlign a = sam_align(has_f, f, (uint32_t)seg, walk[0], walk[1]);
        const typename Format::Mate e = Format::mate(S, names, has_f, f, in->adapter_only_number, m, o, walk[seg], a);
        sizes[4 + seg] = Format::bytes(e);
        if (at + sizes[4 + seg] > cap) return -1;
        sizes[2 + seg] = Format::record(S, names, has_f, f, in->adapter_only_number, m, s, q, o, e, a, out + at);
        // the writer's lane roles on the host: half 0 the head, half 1 the tail, at the same unaligned place of a zeroed image
        std::vector<uint32_t> image((at + sizes[2 + seg]) / 4u + 2u, 0u);
        RSQ_LDS char *text = reinterpret_cast<RSQ_LDS char *>(image.data()) + at;
        ImageSink head(text);
        Format::head(S, names, has_f, f, in->adapter_only_number, m, s, o, e, a, head);
        head.finish();
        ImageSink tail(text + Format::tail_at(e, m));
        Format::tail(S, m, q, o, a, tail);
        tail.finish();
        if (head.n + tail.n != sizes[2 + seg] || memcmp(text, out + at, sizes[2 + seg]) != 0) return -2;
        for (uint32_t i = 0; i < 4u * image.size(); ++i)
            if ((i < at || i >= at + sizes[2 + seg]) && reinterpret_cast<const char *>(image.data())[i]) return -2;
        at += sizes[2 + seg];
    }
    return 0;
}
