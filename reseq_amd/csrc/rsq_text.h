// rsq_text.h -- what a FASTQ record is made of, per lane (Simulator.cpp:596-632, a5): the word-major rows a read is kept in, the CIGAR replay, the
// character sinks, the id line, the data lines, and the record's size without producing it.  No kernels: the read kernels (rsq_reads.h; also compiled at run
// time for one profile, rsq_spec.h) need the rows and record_size, the formatter (rsq_format.h) and the host emulation the rest.
#pragma once
#include "rsq_core.h"

namespace rsq {

// ---------------------------------------------------------------------------------------------- FASTQ text
// The read kernel's per-read word arrays are stored word-major: word w of read r lives at p[w * pitch + r], so the 64 lanes
// of a wave (64 consecutive reads at the same position) store, and later load, 256 contiguous bytes.  pitch 1 = one read alone.
struct WordColumn {
    uint32_t *p;            // word 0 of this read
    uint64_t pitch;         // reads per word row
    RSQ_HD uint32_t &at(uint32_t w) const { return p[(uint64_t)w * pitch]; }
};

// Replays the CIGAR bookkeeping of FillReadPart over the stored 2-bit ops (see fill_read_part in rsq_core.h).
template <class Sink>
RSQ_HD void cigar_replay(const WordColumn &ops, const ReadMeta &m, Sink &sink) {
    if (m.plain) {                                                  // the common read: no need to touch the ops
        if (m.n_iter_m) sink.element('M', m.n_iter_m);
        if (m.n_iter_s) sink.element('S', m.n_iter_s);
        if (m.hard_clip) sink.element('H', m.hard_clip);
        return;
    }
    uint32_t it = 0;
    for (int part = 0; part < 2; ++part) {
        const char base = part ? 'S' : 'M';
        const uint32_t n = part ? m.n_iter_s : m.n_iter_m;
        char element = base;
        uint32_t length = 0;
        for (uint32_t i = 0; i < n; ++i, ++it) {
            if (!(it & 15u) && i + 16u <= n && element == base && !ops.at(it >> 4)) {      // 16 plain iterations at once
                length += 16u;
                i += 15u;
                it += 15u;
                continue;
            }
            const uint32_t code = (ops.at(it >> 4) >> ((it & 15u) * 2u)) & 3u;
            const char want = code == 0 ? base : (code == 1 ? 'D' : 'I');
            if (want == element) ++length;
            else {
                sink.element(element, length);
                element = want;
                length = 1;
            }
        }
        if (length) sink.element(element, length);
    }
    if (m.hard_clip) sink.element('H', m.hard_clip);
}

template <class Derived>
struct TextOps {                        // what a record is made of, on top of Derived::ch
    RSQ_HD Derived &self() { return *static_cast<Derived *>(this); }
    // four characters per push (the sinks take up to four bytes at once): the id line is mostly fixed text
    RSQ_HD void str(const char *s, uint32_t len) {
        uint32_t i = 0;
        for (; i + 4u <= len; i += 4u)
            self().bytes((uint32_t)(uint8_t)s[i] | ((uint32_t)(uint8_t)s[i + 1u] << 8) | ((uint32_t)(uint8_t)s[i + 2u] << 16) | ((uint32_t)(uint8_t)s[i + 3u] << 24), 4u);
        if (i < len) {
            uint32_t w = 0;
            for (uint32_t k = 0; i + k < len; ++k) w |= (uint32_t)(uint8_t)s[i + k] << (8u * k);
            self().bytes(w, len - i);
        }
    }
    // decimal digits without a buffer: peeled from the least significant end into a register, most significant digit lowest, then handed to the
    // sink four at a time
    RSQ_HD void num(uint32_t v) {              // 32-bit: division by 10 is a multiply and a shift
        uint64_t acc = 0;
        uint32_t n = 0;
        do {
            acc = (acc << 8) | (uint64_t)('0' + v % 10u);
            v /= 10u;
            ++n;
        } while (v && n < 8u);
        if (v) {                               // nine or ten digits: the leading ones first
            uint32_t hi = 0, nh = 0;
            do {
                hi = (hi << 8) | ('0' + v % 10u);
                v /= 10u;
                ++nh;
            } while (v);
            self().bytes(hi, nh);
        }
        self().bytes((uint32_t)acc, n < 4u ? n : 4u);
        if (n > 4u) self().bytes((uint32_t)(acc >> 32), n - 4u);
    }
    RSQ_HD void nine_digits(uint32_t v) {      // v < 10^9 with its leading zeros
        uint32_t low = 0, mid = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            low = (low << 8) | ('0' + v % 10u);
            v /= 10u;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mid = (mid << 8) | ('0' + v % 10u);
            v /= 10u;
        }
        self().ch((char)('0' + v));
        self().bytes(mid, 4u);
        self().bytes(low, 4u);
    }
    RSQ_HD void num(uint64_t v) {              // beyond 32 bits (read numbers of a job of more than 4 G pairs): groups of nine digits, no buffer
        if (v <= 0xFFFFFFFFull) return num((uint32_t)v);
        const uint64_t kE9 = 1000000000ull, upper = v / kE9;
        if (upper >= kE9) {
            num((uint32_t)(upper / kE9));
            nine_digits((uint32_t)(upper % kE9));
        } else num((uint32_t)upper);
        nine_digits((uint32_t)(v % kE9));
    }
    RSQ_HD void element(char op, uint32_t count) {
        num(count);
        self().ch(op);
    }
};
template <class P>
struct TextSinkT : TextOps<TextSinkT<P>> {      // appends characters at p (no null check: LDS offset 0 is a valid destination)
    P p;
    uint32_t n;
    RSQ_HD TextSinkT(P dst, uint32_t at) : p(dst), n(at) {}
    RSQ_HD void ch(char c) {
        p[n] = c;
        ++n;
    }
    RSQ_HD void bytes(uint32_t word, uint32_t count) {        // count <= 4 characters, the first in the low byte
        for (uint32_t i = 0; i < count; ++i) ch((char)(word >> (8u * i)));
    }
};
using TextSink = TextSinkT<char *>;

// The same stream written with aligned 4-byte stores: bytes collect in a register and leave a word at a time; only the
// bytes before the first and after the last aligned word of the destination are stored singly (neighbouring records of
// other lanes share those words).
template <class P>
struct WordPtr {
    using type = uint32_t *;
};
template <>
struct WordPtr<RSQ_LDS char *> {         // (the host: RSQ_LDS is empty and this is the general case again)
    using type = RSQ_LDS uint32_t *;
};
template <class P>
struct WordSinkT : TextOps<WordSinkT<P>> {
    P p;                 // next destination byte not yet stored
    uint64_t acc;        // pending bytes, first in the low byte
    uint32_t pending, lead, n;
    RSQ_HD explicit WordSinkT(P dst) : p(dst), acc(0), pending(0), lead((4u - ((uint32_t)(uintptr_t)dst & 3u)) & 3u), n(0) {}
    RSQ_HD void push(uint32_t bytes, uint32_t count) {       // count <= 4 bytes, first in the low byte, the rest zero
        acc |= (uint64_t)bytes << (8u * pending);
        pending += count;
        n += count;
        while (lead && pending) {
            *p = (char)(acc & 0xFFu);
            p += 1;
            acc >>= 8;
            --pending;
            --lead;
        }
        if (!lead && pending >= 4u) {
            *reinterpret_cast<typename WordPtr<P>::type>(p) = (uint32_t)acc;
            p += 4;
            acc >>= 32;
            pending -= 4u;
        }
    }
    RSQ_HD void ch(char c) { push((uint8_t)c, 1u); }
    RSQ_HD void bytes(uint32_t word, uint32_t count) { push(count < 4u ? word & ((1u << (8u * count)) - 1u) : word, count); }
    RSQ_HD void finish() {
        while (pending) {
            *p = (char)(acc & 0xFFu);
            p += 1;
            acc >>= 8;
            --pending;
        }
    }
};

RSQ_HD uint32_t digits_u32(uint32_t v) {
    uint32_t n = 1;
    while (v >= 10u) {
        v /= 10u;
        ++n;
    }
    return n;
}
RSQ_HD uint32_t digits_u64(uint64_t v) {
    if (v <= 0xFFFFFFFFull) return digits_u32((uint32_t)v);
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        ++n;
    }
    return n;
}


// One FASTQ record "@id\nSEQ\n+\nQUAL\n" with the id of Simulator.cpp:596-632: the id line ...
template <class Sink>
// (the fragment and its variant part by reference and two flags, not by pointers that may be null: a pointer chosen at run time puts the structure into scratch memory)
RSQ_HD void format_header(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &ops, Sink &t,
                          bool has_fv, const FragmentVar &fv) {
    t.ch('@');
    t.str(names.base_identifier, names.base_len);
    if (has_f) {
        const uint32_t end = has_fv ? fv.end : f.start + f.len;                  // end_position_forward of CreateReads
        t.num(f.block);
        t.ch('_');
        t.num(f.number);
        if (1u < S.num_alleles) {                                    // Simulator.cpp:612-614
            t.str("_allele", 7);
            t.num((uint32_t)f.allele);
        }
        t.ch(':');
        t.num(f.strand ? end : f.start + 1u);
        t.ch(':');
        t.str(names.names + names.name_ptr[f.seq], names.name_ptr[f.seq + 1] - names.name_ptr[f.seq]);
        t.ch(':');
        t.num(f.strand ? f.start + 1u : end);
    } else {
        t.ch('0');
        t.ch('_');
        t.num(adapter_only_number);
        t.str(":0:Adapter:0", 12);
    }
    t.ch(':');
    t.num((uint32_t)S.tiles[m.tile_id]);
    t.str(":1337:1337 ", 11);
    cigar_replay(ops, m, t);
    t.str(" E", 2);
    t.num((uint32_t)m.num_errors);
    t.ch('\n');
}
template <class Sink>
RSQ_HD void format_header(const DevSim &S, const NameTable &names, const Fragment *f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &ops, Sink &t,
                          const FragmentVar *fv = nullptr) {
    format_header(S, names, f != nullptr, f ? *f : Fragment{}, adapter_only_number, m, ops, t, fv != nullptr, fv ? *fv : FragmentVar{});
}
// ... and one of its two data lines: the bases ("SEQ\n+\n", is_qual false) or the qualities ("QUAL\n").  The read kernel
// leaves both as bytes in 16-byte aligned rows; four base codes become four letters with one byte permute (base_letters, rsq_portable.h).
// words [first_word, first_word + n_words) of the line, then (with_end) the line end
template <class Sink>
RSQ_HD void format_line_part(const WordColumn &row, uint32_t read_len, bool is_qual, uint32_t first_word, uint32_t n_words, bool with_end, Sink &t) {
    const uint32_t all_words = (read_len + 3u) >> 2, end_word = first_word + n_words < all_words ? first_word + n_words : all_words;
    constexpr uint32_t kAhead = 10u;                                 // loads in flight
    for (uint32_t i = first_word; i < end_word; i += kAhead) {
        uint32_t w[kAhead];
#pragma unroll
        for (uint32_t k = 0; k < kAhead; ++k) w[k] = i + k < end_word ? row.at(i + k) : 0u;
#pragma unroll
        for (uint32_t k = 0; k < kAhead; ++k) {
            const uint32_t at = 4u * (i + k);
            if (i + k >= end_word) break;
            const uint32_t left = read_len - at, text = is_qual ? w[k] : base_letters(w[k]);
            if (left >= 4u) t.push(text, 4u);
            else t.push(text & ((1u << (8u * left)) - 1u), left);
        }
    }
    if (with_end) {
        if (is_qual) t.push('\n', 1u);
        else t.push('\n' | ('+' << 8) | ('\n' << 16), 3u);
    }
}
template <class Sink>
RSQ_HD void format_line(const WordColumn &row, uint32_t read_len, bool is_qual, Sink &t) {
    format_line_part(row, read_len, is_qual, 0u, (read_len + 3u) >> 2, true, t);
}
template <class P>
RSQ_HD uint32_t format_record(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                              const WordColumn &qual, const WordColumn &ops, P dst, bool has_fv, const FragmentVar &fv) {
    WordSinkT<P> t(dst);
    format_header(S, names, has_f, f, adapter_only_number, m, ops, t, has_fv, fv);
    format_line(seq, m.read_len, false, t);
    format_line(qual, m.read_len, true, t);
    t.finish();
    return t.n;
}
template <class P>
RSQ_HD uint32_t format_record(const DevSim &S, const NameTable &names, const Fragment *f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                              const WordColumn &qual, const WordColumn &ops, P dst, const FragmentVar *fv = nullptr) {
    return format_record(S, names, f != nullptr, f ? *f : Fragment{}, adapter_only_number, m, seq, qual, ops, dst, fv != nullptr, fv ? *fv : FragmentVar{});
}

// length of that record without producing it (the read kernel writes it next to the read)
RSQ_HD uint32_t record_size(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, bool has_fv, const FragmentVar &fv) {
    uint32_t n = 1u + names.base_len;
    if (has_f) {
        const uint32_t end = has_fv ? fv.end : f.start + f.len;
        if (1u < S.num_alleles) n += 7u + digits_u64(f.allele);
        n += digits_u64(f.block) + 1u + digits_u64(f.number) + 1u + digits_u64(f.strand ? end : f.start + 1u) + 1u +
             (names.name_ptr[f.seq + 1] - names.name_ptr[f.seq]) + 1u + digits_u64(f.strand ? f.start + 1u : end);
    } else n += 2u + digits_u64(adapter_only_number) + 12u;
    n += 1u + digits_u64(S.tiles[m.tile_id]) + 11u + m.cigar_chars + 2u + digits_u64(m.num_errors) + 1u;
    return n + 2u * m.read_len + 4u;
}
RSQ_HD uint32_t record_size(const DevSim &S, const NameTable &names, const Fragment *f, uint64_t adapter_only_number, const ReadMeta &m, const FragmentVar *fv = nullptr) {
    return record_size(S, names, f != nullptr, f ? *f : Fragment{}, adapter_only_number, m, fv != nullptr, fv ? *fv : FragmentVar{});
}

}  // namespace rsq
