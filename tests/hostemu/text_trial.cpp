// text_trial.cpp -- TEST-ONLY: the writers of the text kernels' image (rsq_format.h: ImageSink, image_header, image_line_part, image_record_part) on the CPU, where
// the image is a byte buffer, beside format_record (rsq_text.h) on the same rows.  tests/test_text_sink.py compiles it with g++ and compares the two.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_format.h"

using namespace rsq;

extern "C" {

struct text_trial_record {
    int32_t has_fragment;      // 0: an adapter-only pair with number `adapter_only_number`
    uint32_t seq, start, len, strand, block, number, allele, num_alleles;
    int32_t has_end;           // a fragment with variants: its end is `end`, not start + len
    uint32_t end;
    uint64_t adapter_only_number;
    uint32_t tile, read_len, n_iter_m, n_iter_s, hard_clip, num_errors;
    const char *base_identifier;
    const char *names;         // the reference ids' first parts, one after the other, in a buffer that begins on a word boundary and ends on one
    const uint32_t *name_ptr;
    const uint8_t *bases;      // read_len base codes 0..4
    const uint8_t *quals;      // read_len characters
    const uint8_t *ops;        // n_iter_m + n_iter_s codes: 0 the part's own op (M / S), 1 D, 2 I
};

constexpr uint32_t kGuard = 64;
constexpr uint8_t kGuardByte = 0xA7;

// The record three times in a row (a record has neighbours on both sides), the first at byte `align` behind the guard of an image that begins on a 16-byte
// boundary; the twelve parts written in ascending (order 0) or descending (order 1) order, as the four lanes of a record write theirs.  want: format_record's
// bytes of one record.  Returns the record's length, -1: cap is too small, -2: the image differs from three times `want`, -3: a guard byte changed, -4: the
// sink counted another length than format_record.
int text_trial_fastq(const text_trial_record *in, uint32_t align, int order, char *want, uint32_t cap) {
    DevSim S{};
    const uint16_t tiles[1] = {(uint16_t)in->tile};
    S.tiles = tiles;
    S.num_alleles = in->num_alleles;
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
    f.allele = (uint8_t)in->allele;
    FragmentVar fv{};
    fv.end = in->end;
    const bool has_f = in->has_fragment != 0, has_fv = has_f && in->has_end != 0;

    const uint32_t words = (in->read_len + 3u) / 4u, n_ops = in->n_iter_m + in->n_iter_s;
    std::vector<uint32_t> seq(words + 1u, 0xA5A5A5A5u), qual(words + 1u, 0xA5A5A5A5u), ops(n_ops / 16u + 2u, 0u);      // what lies behind a row's last character must not matter
    for (uint32_t i = 0; i < in->read_len; ++i) {
        seq[i / 4u] = (seq[i / 4u] & ~(0xFFu << (8u * (i & 3u)))) | ((uint32_t)in->bases[i] << (8u * (i & 3u)));
        qual[i / 4u] = (qual[i / 4u] & ~(0xFFu << (8u * (i & 3u)))) | ((uint32_t)in->quals[i] << (8u * (i & 3u)));
    }
    bool plain = true;
    for (uint32_t i = 0; i < n_ops; ++i) {
        ops[i / 16u] |= (uint32_t)(in->ops[i] & 3u) << (2u * (i & 15u));
        plain = plain && !in->ops[i];
    }
    ReadMeta m{};
    m.read_len = (uint16_t)in->read_len;
    m.num_errors = (uint16_t)in->num_errors;
    m.n_iter_m = (uint16_t)in->n_iter_m;
    m.n_iter_s = (uint16_t)in->n_iter_s;
    m.hard_clip = (uint16_t)in->hard_clip;
    m.plain = plain ? 1 : 0;
    const WordColumn s{seq.data(), 1}, q{qual.data(), 1}, o{ops.data(), 1};
    char cigar[4096];
    TextSink count(cigar, 0);
    cigar_replay(o, m, count);
    m.cigar_chars = (uint16_t)count.n;

    const uint32_t bytes = record_size(S, names, has_f, f, in->adapter_only_number, m, has_fv, fv);
    if (bytes > cap) return -1;
    if (format_record(S, names, has_f, f, in->adapter_only_number, m, s, q, o, want, has_fv, fv) != bytes) return -4;

    std::vector<uint8_t> buffer(kGuard + 16u + 3u * bytes + kGuard + 16u, kGuardByte);
    uint8_t *image = buffer.data() + ((16u - ((uintptr_t)buffer.data() & 15u)) & 15u) + kGuard - 16u;        // 16-byte aligned, at least kGuard - 16 guard bytes in front
    uint8_t *text = image + 16u + align;
    memset(text, 0, 3u * bytes);                                       // the wave zeroes its image; the guard stays: an OR of a stray bit shows
    const uint32_t header = bytes - 2u * m.read_len - 4u, n_parts = 2u * kFormatLineParts;
    uint32_t counted = 0;
    for (uint32_t k = 0; k < 3u * n_parts; ++k) {
        const uint32_t j = order ? 3u * n_parts - 1u - k : k, record = j / n_parts, part = j % n_parts;
        image_record_part(m, s, q, header, part, (char *)text + record * bytes, [&](ImageSink &t) {
            image_header(S, names, has_f, f, in->adapter_only_number, m, o, t, has_fv, fv);
            counted = t.n;
        });
    }
    if (counted != header) return -4;
    for (uint32_t record = 0; record < 3u; ++record)
        if (memcmp(text + record * bytes, want, bytes)) {
            memcpy(want, text + record * bytes, bytes);                // what the image holds, for the message
            return -2;
        }
    for (uint8_t *p = buffer.data(); p < buffer.data() + buffer.size(); ++p)
        if ((p < text || p >= text + 3u * bytes) && *p != kGuardByte) return -3;
    return (int)bytes;
}

// ImageSink::num against snprintf: every value at every phase of the destination, alone and with a tail of 1 and 4 characters; wide: through num(uint64_t).
// Returns the index of the first value that differs, -1: none.
int64_t text_trial_numbers(const uint64_t *values, uint64_t n, int wide) {
    alignas(16) char image[64];
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t phase = 0; phase < 4u; ++phase)
            for (uint32_t tail_len = 0; tail_len <= 4u; tail_len += tail_len ? 3u : 1u) {
                const uint32_t tail = tail_len == 4u ? chars4(':', '1', '3', '3') : tail_len ? (uint32_t)'_' : 0u;
                char want[40];
                const int len = snprintf(want, sizeof want, "%llu%s", (unsigned long long)values[i], tail_len == 4u ? ":133" : tail_len ? "_" : "");
                memset(image, 0, sizeof image);
                ImageSink t(image + 4u + phase);
                if (wide) t.num(values[i], tail, tail_len);
                else t.num((uint32_t)values[i], tail, tail_len);
                t.finish();
                if ((int)t.n != len || memcmp(image + 4u + phase, want, (size_t)len)) return (int64_t)i;
                for (uint32_t b = 0; b < sizeof image; ++b)
                    if ((b < 4u + phase || b >= 4u + phase + (uint32_t)len) && image[b]) return (int64_t)i;
            }
    return -1;
}

// ImageSink::str: len characters from every alignment of the source, with and without a character in front and behind, at every phase of the destination.
// source: a buffer on a word boundary with at least len + 8 bytes.  Returns 0, or a code of the first case that differs.
int text_trial_strings(const char *source, uint32_t len) {
    alignas(16) char image[256];
    if (len + 16u > sizeof image) return -1;
    for (uint32_t from = 0; from < 4u; ++from)
        for (uint32_t phase = 0; phase < 4u; ++phase)
            for (uint32_t ends = 0; ends < 4u; ++ends) {
                const char head = ends & 1u ? '@' : 0, tail = ends & 2u ? ' ' : 0;
                char want[260];
                uint32_t n = 0;
                if (head) want[n++] = head;
                memcpy(want + n, source + from, len);
                n += len;
                if (tail) want[n++] = tail;
                memset(image, 0, sizeof image);
                ImageSink t(image + 4u + phase);
                t.str(source + from, len, (uint32_t)(uint8_t)head, (uint32_t)(uint8_t)tail);
                t.finish();
                if (t.n != n || memcmp(image + 4u + phase, want, n)) return (int)(1000u * (from + 1u) + 10u * phase + ends);
                for (uint32_t b = 0; b < sizeof image; ++b)
                    if ((b < 4u + phase || b >= 4u + phase + n) && image[b]) return -(int)(1000u * (from + 1u) + 10u * phase + ends);
            }
    return 0;
}
}
