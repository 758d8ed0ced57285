// rsq_sam.h -- truth alignments: one SAM record per simulated read, written on the device from the arrays the FASTQ text is written from (the raw rows of the
// read kernel, rsq_reads.h RawLayout, and the fragment list).  ReSeq keeps a read's origin only in its id ("...:{start}:{ref}:{end}:... {CIGAR} E{n}",
// Simulator.cpp:596-632) -- with a CIGAR that is not SAM's (0M / 0S elements, I and D inside the adapter part, H for bases that are in the read), in read
// orientation and with an end coordinate for the reverse mate; ART, Mason and dwgsim write a truth SAM beside their reads for that reason.
//
// The record (DESIGN.md "Truth alignments" states the rules): two per pair, the mate of template segment 0 first, tab-separated
//   QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL XC:Z:<the id's CIGAR> XE:i:<the id's error count>
// Only the template part of a read (ReadMeta::n_iter_m iterations, ops M / D / I) is alignment: q read bases (M, I) over t template bases (M, D); everything
// behind it -- adapter, tail -- is ONE S element of read_len - q bases.  Elements of equal op merge, D at either end of the template part is dropped (dL at the
// reference's left end moves POS).  A forward mate (segment == strand) covers [start, start + t), a reverse mate [end - t, end): its CIGAR is replayed from the
// last op down, its bases are the reverse complement, its qualities reversed.  Adapter-only pairs are unmapped (flags 77 / 141).
//
// Per lane, host and device (tests/hostemu/truth_trial.h runs them on the CPU): sam_walk, sam_align, sam_cigar, RowRound, sam_line, sam_record_size, sam_record.
// For a reference with variants (rsq_sim_truth_variants; the second half of this file, tests/hostemu/truth_var_trial.cpp): AlleleCursor, sam_var_walk, sam_var_columns,
// sam_var_cigar, sam_var_align -- the record in reference coordinates, SamVarFormat (BamVarFormat in rsq_bam.h).
//
// A truth-record FORMAT is a type of static members (SamFormat below, BamFormat in rsq_bam.h): the side array's entry per mate (Mate; Pair holds a row's two,
// one load), walk(entry) and bytes(entry), mate(...) -- the entry from a walk and an alignment --, head(..., sink) -- everything in front of QUAL --,
// tail(..., sink) -- QUAL and the tags --, tail_at(entry, meta), the offset at which the tail begins, and record(..., dst), the whole record through one sink
// (sam_record, bam_record: the straight-to-HBM fallback).  Everything that is not a record's bytes is written once over a format: the kernels k_truth_sizes<Format> (one lane per pair: both
// mates' entries into the side array, the pair's bytes) and k_truth_write<Format, PERM> (one wave per 16 pairs, four lanes a pair, through the wave's LDS image,
// WaveImage in rsq_format.h).  A format with kVariants has the same members with the FragmentVar's part (SamVarId) among their arguments, and its alignment comes from the
// entries (sam_var_align): the two kernels branch on it at compile time.  A format with kMd (rsq_md.h: MdFormat over each of the four, rsq_sim_truth_md) appends NM:i and MD:Z to a
// mapped record: its mate() and tail() also take the SEQ row, the fragment and the entry -- the second compile-time branch --, and it is built from the members grow (more
// bytes behind a record's own) and tail_open (the tail up to where more tags go) that every format has.  Not part of what hiprtc compiles for a profile (rsq_spec.h): nothing of the read kernel's text includes this file.
#pragma once
#include "rsq_format.h"

namespace rsq {

// what the ops of one mate's template part come to (k_truth_sizes keeps it so that the writer does not walk them again)
struct SamMate {
    uint16_t q, t;             // read bases (M + I) and template bases (M + D) of the template part
    uint16_t lead, trail;      // D iterations at its first and last end in READ order: dropped from the CIGAR
    uint16_t cigar_chars;      // length of the SAM CIGAR
    uint16_t pad;
    uint32_t bytes;            // of the mate's record
};
static_assert(sizeof(SamMate) == 16, "two mates are one 32-byte load");
struct SamPair {
    SamMate mate[2];
};

RSQ_HD uint32_t sam_op_at(const WordColumn &ops, uint32_t it) { return (ops.at(it >> 4) >> ((it & 15u) * 2u)) & 3u; }      // 0 M, 1 D, 2 I (fill_read_part, rsq_core.h)

RSQ_HD SamMate sam_walk(const WordColumn &ops, const ReadMeta &m) {
    SamMate w{};
    const uint32_t n = m.n_iter_m;
    uint32_t chars = 0;
    if (m.plain) {
        w.q = w.t = (uint16_t)n;
        if (n) chars = digits_u32(n) + 1u;
    } else {
        uint32_t q = 0, t = 0, run = 0, cur = 3u, runs = 0;
        auto flush = [&](bool last) {                                   // the run that ends here
            if (!run) return;
            if (cur == 1u && runs == 1u) w.lead = (uint16_t)run;       // (a template part of D alone is all lead)
            else if (cur == 1u && last) w.trail = (uint16_t)run;
            else chars += digits_u32(run) + 1u;
        };
        for (uint32_t it = 0; it < n; ++it) {
            if (!(it & 15u) && it + 16u <= n && !ops.at(it >> 4)) {     // 16 plain iterations at once
                if (cur != 0u) {
                    flush(false);
                    cur = 0u;
                    run = 0;
                    ++runs;
                }
                run += 16u;
                q += 16u;
                t += 16u;
                it += 15u;
                continue;
            }
            const uint32_t c = sam_op_at(ops, it);
            if (c != cur) {
                flush(false);
                cur = c;
                run = 0;
                ++runs;
            }
            ++run;
            q += c != 1u;
            t += c != 2u;
        }
        flush(true);
        w.q = (uint16_t)q;
        w.t = (uint16_t)t;
    }
    const uint32_t clip = (uint32_t)m.read_len - w.q;
    if (clip) chars += digits_u32(clip) + 1u;
    w.cigar_chars = (uint16_t)(chars ? chars : 1u);                     // nothing left: "*"
    return w;
}

// The CIGAR: the template part's elements in read order and the clip behind them, or (reverse) the clip and the elements from the last op down
template <class Sink>
RSQ_HD void sam_cigar(const WordColumn &ops, const ReadMeta &m, const SamMate &w, bool reverse, Sink &t) {
    const uint32_t clip = (uint32_t)m.read_len - w.q;
    bool any = false;
    if (reverse && clip) {
        t.element('S', clip);
        any = true;
    }
    if (m.plain) {
        if (m.n_iter_m) {
            t.element('M', m.n_iter_m);
            any = true;
        }
    } else {
        const uint32_t lo = w.lead, hi = (uint32_t)m.n_iter_m - w.trail;
        uint32_t cur = 3u, run = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t it = reverse ? hi - 1u - (i - lo) : i;
            // 16 plain iterations at once: the word that holds `it` lies inside the range, and the replay stands at its first (reverse: last) op
            if ((reverse ? (it & 15u) == 15u && it >= lo + 15u : !(it & 15u) && it + 16u <= hi) && (cur == 0u || !run) && !ops.at(it >> 4)) {
                cur = 0u;
                run += 16u;
                i += 15u;
                continue;
            }
            const uint32_t c = sam_op_at(ops, it);
            if (c != cur) {
                if (run) t.element(cur == 0u ? 'M' : cur == 1u ? 'D' : 'I', run);
                cur = c;
                run = 0;
            }
            ++run;
        }
        if (run) {
            t.element(cur == 0u ? 'M' : cur == 1u ? 'D' : 'I', run);
            any = true;
        }
    }
    if (!reverse && clip) {
        t.element('S', clip);
        any = true;
    }
    if (!any) t.ch('*');
}

// Where a mate aligns, from the fragment and both mates' walks
struct SamAlign {
    uint32_t flag, pos, pnext;
    int32_t tlen;
    uint32_t mapped, reverse;
};
// ... from both mates' POS and last aligned position (1-based; a mate without reference bases: last = pos - 1)
RSQ_HD SamAlign sam_align_at(bool has_f, const Fragment &f, uint32_t seg, const int32_t (&pos)[2], const int32_t (&last)[2]) {
    SamAlign a{};
    if (!has_f || !f.len) {                                             // adapter-only: unmapped
        a.flag = seg ? 141u : 77u;
        return a;
    }
    const uint32_t o = seg ^ 1u;
    const bool rev = seg != f.strand;
    a.mapped = 1u;
    a.reverse = rev ? 1u : 0u;
    a.flag = 0x1u | 0x2u | (rev ? 0x10u : 0x20u) | (seg ? 0x80u : 0x40u);      // (the mates of a pair read opposite strands)
    a.pos = (uint32_t)pos[seg];
    a.pnext = (uint32_t)pos[o];
    const int32_t span = (last[0] > last[1] ? last[0] : last[1]) - (pos[0] < pos[1] ? pos[0] : pos[1]) + 1;
    const bool leftmost = pos[seg] < pos[o] || (pos[seg] == pos[o] && seg == 0u);
    a.tlen = leftmost ? span : -span;
    return a;
}
// POS - 1 of one mate from its own walk (a mapped pair's): what sam_align makes POS of, and where the depth of rsq_depth.h begins to count the mate
RSQ_HD uint32_t sam_mate_pos(const Fragment &f, uint32_t seg, const SamMate &w) {
    const bool rev = seg != f.strand;                                   // fragment_src (rsq_reads.h): src.reverse = seg != f.strand
    return (rev ? f.start + f.len - w.t : f.start) + (rev ? w.trail : w.lead);
}
RSQ_HD SamAlign sam_align(bool has_f, const Fragment &f, uint32_t seg, const SamMate &w0, const SamMate &w1) {
    int32_t pos[2], last[2];
    for (uint32_t s = 0; s < 2u; ++s) {
        const SamMate &w = s ? w1 : w0;
        pos[s] = (int32_t)(sam_mate_pos(f, s, w) + 1u);
        last[s] = pos[s] + (int32_t)((uint32_t)w.t - w.lead - w.trail) - 1;
    }
    return sam_align_at(has_f, f, seg, pos, last);
}

// QNAME: the id line of format_header (rsq_text.h) without '@', up to its first blank.  `end`: the id's end position; allele: the id carries "_allele<a>" (both
// differ from the fragment's own only for a reference with variants, SamVarFormat below)
template <class Sink>
RSQ_HD void sam_qname_at(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint32_t end, bool allele, uint64_t adapter_only_number, const ReadMeta &m, Sink &t) {
    t.str(names.base_identifier, names.base_len);
    if (has_f) {
        t.num(f.block);
        t.ch('_');
        t.num(f.number);
        if (allele) {
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
    t.str(":1337:1337", 10);
}
RSQ_HD uint32_t sam_qname_size_at(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint32_t end, bool allele, uint64_t adapter_only_number, const ReadMeta &m) {
    uint32_t n = names.base_len + 1u + digits_u32(S.tiles[m.tile_id]) + 10u;
    if (has_f) {
        n += digits_u32(f.block) + 1u + digits_u32(f.number) + 1u + digits_u32(f.start + 1u) + 1u + (names.name_ptr[f.seq + 1] - names.name_ptr[f.seq]) + 1u + digits_u32(end);
        if (allele) n += 7u + digits_u32(f.allele);
    } else n += 2u + digits_u64(adapter_only_number) + 12u;
    return n;
}
template <class Sink>
RSQ_HD void sam_qname(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, Sink &t) {
    sam_qname_at(S, names, has_f, f, f.start + f.len, false, adapter_only_number, m, t);
}
RSQ_HD uint32_t sam_qname_size(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m) {
    return sam_qname_size_at(S, names, has_f, f, f.start + f.len, false, adapter_only_number, m);
}
RSQ_HD uint32_t sam_tlen_chars(int32_t v) { return v < 0 ? 1u + digits_u32((uint32_t)-(int64_t)v) : digits_u32((uint32_t)v); }

// the record's three stretches: everything in front of SEQ (with its tab) -- QNAME, the fields up to the CIGAR, the CIGAR, the fields behind it -- ...
template <class Sink>
RSQ_HD void sam_head_front(const NameTable &names, const Fragment &f, const SamAlign &a, Sink &t) {
    t.ch('\t');
    t.num(a.flag);
    t.ch('\t');
    if (a.mapped) {
        t.str(names.names + names.name_ptr[f.seq], names.name_ptr[f.seq + 1] - names.name_ptr[f.seq]);
        t.ch('\t');
        t.num(a.pos);
        t.str("\t60\t", 4);
    } else t.str("*\t0\t0\t*\t*\t0\t0\t", 14);
}
template <class Sink>
RSQ_HD void sam_head_back(const SamAlign &a, Sink &t) {
    t.str("\t=\t", 3);
    t.num(a.pnext);
    t.ch('\t');
    if (a.tlen < 0) {
        t.ch('-');
        t.num((uint32_t)-(int64_t)a.tlen);
    } else t.num((uint32_t)a.tlen);
    t.ch('\t');
}
template <class Sink>
RSQ_HD void sam_head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &ops, const SamMate &w,
                     const SamAlign &a, Sink &t) {
    sam_qname(S, names, has_f, f, adapter_only_number, m, t);
    sam_head_front(names, f, a, t);
    if (a.mapped) {
        sam_cigar(ops, m, w, a.reverse != 0u, t);
        sam_head_back(a, t);
    }
}
// (without the QNAME's characters)
RSQ_HD uint32_t sam_head_fields_size(const NameTable &names, const Fragment &f, uint32_t cigar_chars, const SamAlign &a) {
    uint32_t n = 1u + digits_u32(a.flag) + 1u;
    if (a.mapped) n += (names.name_ptr[f.seq + 1] - names.name_ptr[f.seq]) + 1u + digits_u32(a.pos) + 4u + cigar_chars + 3u + digits_u32(a.pnext) + 1u + sam_tlen_chars(a.tlen) + 1u;
    else n += 14u;
    return n;
}
RSQ_HD uint32_t sam_head_size(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const SamMate &w, const SamAlign &a) {
    return sam_qname_size(S, names, has_f, f, adapter_only_number, m) + sam_head_fields_size(names, f, w.cigar_chars, a);
}
// ... SEQ or QUAL (no tab, no line end): the row's words as they lie, or from the last one down -- a read length that is no multiple of four takes every output
// word from two neighbours --, bytes reversed; bases as letters (reverse: the complement's), qualities moved from the profile's offset to Phred+33
// (sam_byte_reverse, sam_complement_letters and align_bytes: rsq_portable.h)
// A round of up to kRowAhead of a row's words, loaded together and handed out oriented for output: at(k) is output word i + k -- row word i + k, or (reverse) the
// row from its last word down, funnelled over two neighbours when read_len & 3, byte-reversed.  Words behind the row's last are 0.
constexpr uint32_t kRowAhead = 10u;                                      // loads in flight (even: bam_seq pairs the words of a round)
struct RowRound {
    uint32_t w[kRowAhead + 1u], odd;
    bool reverse;
    RSQ_HD RowRound(const WordColumn &row, uint32_t read_len, bool reverse_, uint32_t i) : odd(read_len & 3u), reverse(reverse_) {
        const uint32_t words = (read_len + 3u) >> 2;
        uint64_t at = (uint64_t)(reverse ? words - 1u - i : i) * row.pitch;      // output word j reads row word j, or (reverse) words - 1 - j and the one below it:
        const uint64_t step = reverse ? 0u - row.pitch : row.pitch;              // a step of the pitch up or down (modulo 2^64) in place of a product per load
#pragma unroll
        for (uint32_t k = 0; k <= kRowAhead; ++k, at += step) w[k] = i + k < words && (k < kRowAhead || (reverse && odd)) ? row.p[at] : 0u;
    }
    RSQ_HD uint32_t at(uint32_t k) const { return reverse ? sam_byte_reverse(odd ? align_bytes(w[k], w[k + 1u], odd) : w[k]) : w[k]; }
};
template <class Sink>
RSQ_HD void sam_line(const WordColumn &row, uint32_t read_len, bool is_qual, bool reverse, uint32_t phred_offset, Sink &t) {
    const uint32_t words = (read_len + 3u) >> 2;
    const uint32_t shift = ((phred_offset - 33u) & 0xFFu) * 0x01010101u;      // one packed subtract: no character is below the offset, so no byte borrows from a character
    for (uint32_t i = 0; i < words; i += kRowAhead) {
        const RowRound round(row, read_len, reverse, i);
#pragma unroll
        for (uint32_t k = 0; k < kRowAhead; ++k) {
            if (i + k >= words) break;
            const uint32_t v = round.at(k);
            const uint32_t text = is_qual ? v - shift : reverse ? sam_complement_letters(v) : base_letters(v), left = read_len - 4u * (i + k);
            t.bytes(text, left < 4u ? left : 4u);
        }
    }
}
// ... and the two tags (sam_tags_open: without the line end, for a format that writes more tags behind them) with the line end
template <class Sink>
RSQ_HD void sam_tags_open(const ReadMeta &m, const WordColumn &ops, Sink &t) {
    t.str("\tXC:Z:", 6);
    cigar_replay(ops, m, t);
    t.str("\tXE:i:", 6);
    t.num((uint32_t)m.num_errors);
}
template <class Sink>
RSQ_HD void sam_tags(const ReadMeta &m, const WordColumn &ops, Sink &t) {
    sam_tags_open(m, ops, t);
    t.ch('\n');
}
RSQ_HD uint32_t sam_tags_size(const ReadMeta &m) { return 6u + m.cigar_chars + 6u + digits_u32(m.num_errors) + 1u; }

// length of a record without producing it
RSQ_HD uint32_t sam_record_size(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const SamMate &w,
                                const SamAlign &a) {
    return sam_head_size(S, names, has_f, f, adapter_only_number, m, w, a) + 2u * m.read_len + 1u + sam_tags_size(m);
}
// the whole record at dst; returns its length
template <class P>
RSQ_HD uint32_t sam_record(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                           const WordColumn &qual, const WordColumn &ops, const SamMate &w, const SamAlign &a, P dst) {
    WordSinkT<P> t(dst);
    sam_head(S, names, has_f, f, adapter_only_number, m, ops, w, a, t);
    sam_line(seq, m.read_len, false, a.reverse != 0u, S.phred_offset, t);
    t.ch('\t');
    sam_line(qual, m.read_len, true, a.reverse != 0u, S.phred_offset, t);
    sam_tags(m, ops, t);
    t.finish();
    return t.n;
}

// SAM text as a format (the header comment states what a format is); an entry is the walk itself, with the record's bytes
struct SamFormat {
    static constexpr bool kVariants = false, kMd = false, kBam = false;
    using Mate = SamMate;
    using Pair = SamPair;
    static RSQ_HD void grow(Mate &e, uint32_t n) { e.bytes += n; }      // more tags behind the record's own (rsq_md.h)
    static RSQ_HD const SamMate &walk(const Mate &e) { return e; }
    static RSQ_HD uint32_t bytes(const Mate &e) { return e.bytes; }
    static RSQ_HD Mate mate(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &, const SamMate &w,
                            const SamAlign &a) {
        Mate e = w;
        e.bytes = sam_record_size(S, names, has_f, f, adapter_only_number, m, w, a);
        return e;
    }
    template <class Sink>
    static RSQ_HD void head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                            const WordColumn &ops, const Mate &e, const SamAlign &a, Sink &t) {
        sam_head(S, names, has_f, f, adapter_only_number, m, ops, e, a, t);
        sam_line(seq, m.read_len, false, a.reverse != 0u, S.phred_offset, t);
        t.ch('\t');
    }
    template <class Sink>
    static RSQ_HD void tail(const DevSim &S, const ReadMeta &m, const WordColumn &qual, const WordColumn &ops, const SamAlign &a, Sink &t) {
        sam_line(qual, m.read_len, true, a.reverse != 0u, S.phred_offset, t);
        sam_tags(m, ops, t);
    }
    template <class Sink>
    static RSQ_HD void tail_open(const DevSim &S, const ReadMeta &m, const WordColumn &qual, const WordColumn &ops, const SamAlign &a, Sink &t) {      // ... up to where more tags go
        sam_line(qual, m.read_len, true, a.reverse != 0u, S.phred_offset, t);
        sam_tags_open(m, ops, t);
    }
    static RSQ_HD uint32_t tail_at(const Mate &e, const ReadMeta &m) { return e.bytes - sam_tags_size(m) - m.read_len; }
    template <class P>
    static RSQ_HD uint32_t record(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                                  const WordColumn &qual, const WordColumn &ops, const Mate &e, const SamAlign &a, P dst) {
        return sam_record(S, names, has_f, f, adapter_only_number, m, seq, qual, ops, e, a, dst);
    }
};

// ------------------------------------------------------------------------------------------------ a reference with variants (rsq_sim_truth_variants)
// The same record in REFERENCE coordinates (DESIGN.md 4.8 states the rules).  A mate's template part is a stretch of its ALLELE's sequence (rsq_variants.h): the
// forward mate's begins at the allele coordinate of (start, start variant), the reverse mate's ends where (end position, EndVariant) points, exactly as
// allele_template places them.  Every allele base either stands at a reference position p (class R) or is base k >= 1 of the replacement at p (class X, inserted).
// Walked in ascending allele order -- the ops in read order, or (reverse) from the last op down -- the columns are: M on R -> M, M on X -> I, D on R -> D, D on X ->
// nothing, I -> I, and in front of an allele base one D per reference position the allele deleted between it and the base before it (deleted positions that touch
// only the outside of the stretch are no part of the alignment).  Equal neighbours merge, D runs at either end are dropped, POS is the first remaining column that
// consumes the reference; a mate without one (wholly inside inserted bases of the variant at p, or without template bases) takes the position its next such column
// would have: POS = p + 2.  The id's "_allele<a>" stays in the QNAME, its end position is the id's (FragmentVar::end), and one tag follows XE:
// XI:i:<FragmentVar::start_var_pos>, the bases of the replacement at the start position that lie in front of the fragment.
//
// AlleleCursor is placed once per mate (one allele_point, hinted by the one bisection that finds the stretch) and then steps base by base, entry by entry.  A mate
// whose stretch no entry with a coordinate effect reaches -- most of them -- is `plain`: today's walk and CIGAR, its position the stretch's first base's.  With
// substitutions only (allele copies, no FragmentVar) every mate is plain and the stretch is the fragment's own.
struct AlleleBase {
    uint32_t p;                // the base's reference position (class X: of its replacement)
    uint32_t gap;              // reference positions the allele deleted between the base before and this one: [p - gap, p)
    bool x;                    // class X
};
struct AlleleCursor {
    AlleleView a;
    uint32_t j;                // the map's next entry
    uint32_t ref;              // the reference position of the next base
    uint32_t k, len;           // k < len: the next base is base k of the replacement at ref
    // at allele coordinate h, `entries` of the map beginning at or before it (what allele_point found there)
    RSQ_HD AlleleCursor(const AlleleView &a_, int64_t h, uint32_t entries) : a(a_), j(entries), k(0u), len(0u) {
        if (j) {
            const int64_t at = h - a.begin_of(j - 1u);
            const uint32_t n = a.var(j - 1u).len;
            if (at < (int64_t)n) {
                ref = a.e[j - 1u].pos;
                k = (uint32_t)at;
                len = n;
                return;
            }
        }
        ref = (uint32_t)(h - a.e[j].shift);
    }
    RSQ_HD bool inserted() const { return k < len && k != 0u; }         // the next base is of class X
    RSQ_HD bool clear(uint32_t n) const { return !(k < len) && a.e[j].pos - ref >= n; }      // the next n bases are no entry's (the sentinel stands at the sequence's length)
    RSQ_HD void skip(uint32_t n) { ref += n; }                          // ... n such bases
    RSQ_HD AlleleBase next() {
        AlleleBase b{ref, 0u, false};
        if (k < len) {
            b.x = k != 0u;
            if (++k == len) {
                ++ref;
                k = len = 0u;
            }
            return b;
        }
        while (j < a.n && a.e[j].pos == ref) {
            const uint32_t n = a.var(j).len;
            ++j;
            if (n) {                                                    // the base standing at ref, with n - 1 inserted ones behind it
                b.p = ref;
                if (n > 1u) {
                    k = 1u;
                    len = n;
                } else ++ref;
                return b;
            }
            ++b.gap;                                                    // deleted
            ++ref;
        }
        b.p = ref++;
        return b;
    }
};

// the side entry of a mate: the walk, and where the record stands
struct SamVarMate {
    SamMate w;                 // q, t, cigar_chars, bytes as ever; pad: 0 plain (lead, trail as ever: sam_cigar writes the CIGAR), 1: the columns are walked with the cursor
    uint32_t pos;              // POS - 1
    uint32_t ref_bases;        // reference bases of the cleaned CIGAR
    uint32_t entry;            // the cursor's start: entries of the map at or before ...
    uint32_t at;               // ... the allele coordinate of the stretch's first base
};
static_assert(sizeof(SamVarMate) == 32, "two mates are one 64-byte load");
struct SamVarPair {
    SamVarMate mate[2];
};
// what the record takes from the FragmentVar beside the stretch
struct SamVarId {
    uint32_t end;              // the id's end position
    uint32_t allele;           // the id names the allele
    uint32_t xi;               // the XI tag
};
RSQ_HD SamVarId sam_var_id(const DevSim &S, const Fragment &f, bool has_fv, const FragmentVar &fv) {
    return SamVarId{has_fv ? fv.end : f.start + f.len, 1u < S.num_alleles ? 1u : 0u, has_fv ? fv.start_var_pos : 0u};
}

// The columns of a template part, merged into elements: col() takes them in ascending allele order, end() closes; element() of the sink gets every run but D
// runs at either end.  Beside the elements: where the first reference-consuming column stands and how many there are, dropped ones included.
template <class Sink>
struct SamVarRuns {
    Sink &t;
    bool reverse;
    uint32_t cur = 3u, run = 0u, runs = 0u;
    uint32_t first_ref = 0u, n_ref = 0u, left = 0u, right = 0u;         // left, right: reference positions of the D runs dropped at the low and the high end
    bool any = false;
    RSQ_HD void put() {
        t.element(cur == 0u ? 'M' : cur == 1u ? 'D' : 'I', run);
        any = true;
    }
    RSQ_HD void col(uint32_t op, uint32_t count, uint32_t p) {         // op: 0 M, 1 D, 2 I; p: the reference position of an M or D column (of the first of `count`)
        if (op != 2u) {
            if (!n_ref) first_ref = p;
            n_ref += count;
        }
        if (op != cur) {
            if (run) {
                if (cur == 1u && runs == 1u) left = run;
                else put();
            }
            cur = op;
            run = 0u;
            ++runs;
        }
        run += count;
    }
    RSQ_HD void end() {
        if (!run) return;
        if (cur != 1u) put();
        else if (runs == 1u && !reverse) left = run;                    // D alone is dropped at the end the read begins at, as sam_walk's lead
        else right = run;
    }
};
template <class V>
RSQ_HD void sam_var_columns(const WordColumn &ops, const ReadMeta &m, AlleleCursor &c, bool reverse, V &v) {
    const uint32_t n = m.n_iter_m;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t it = reverse ? n - 1u - i : i;
        // 16 plain iterations at once, as sam_cigar takes them -- where no entry of the map stands among their 16 bases
        if ((reverse ? (it & 15u) == 15u : !(it & 15u) && it + 16u <= n) && (m.plain || !ops.at(it >> 4)) && c.clear(16u)) {
            v.col(0u, 16u, c.ref);
            c.skip(16u);
            i += 15u;
            continue;
        }
        const uint32_t op = m.plain ? 0u : sam_op_at(ops, it);
        if (op == 2u) {
            v.col(2u, 1u, 0u);
            continue;
        }
        const AlleleBase b = c.next();
        if (b.gap) v.col(1u, b.gap, b.p - b.gap);
        if (!b.x) v.col(op, 1u, b.p);
        else if (op == 0u) v.col(2u, 1u, 0u);
    }
    v.end();
}
// The CIGAR of a mate with an entry in reach (e.w.pad), or sam_cigar: the clip and the merged columns.  Returns what the columns came to.
struct SamVarSpan {
    uint32_t pos, ref_bases;
};
template <class Sink>
RSQ_HD SamVarSpan sam_var_cigar(const DevSim &S, const Fragment &f, const WordColumn &ops, const ReadMeta &m, const SamVarMate &e, bool reverse, Sink &t) {
    if (!e.w.pad) {
        sam_cigar(ops, m, e.w, reverse, t);
        return SamVarSpan{e.pos, e.ref_bases};
    }
    const uint32_t clip = (uint32_t)m.read_len - e.w.q;
    AlleleCursor c(allele_view(S, f.seq, f.allele), (int64_t)e.at, e.entry);
    const uint32_t behind = c.ref + (c.inserted() ? 1u : 0u);           // where a mate without a reference-consuming column stands
    SamVarRuns<Sink> v{t, reverse};
    if (reverse && clip) {
        t.element('S', clip);
        v.any = true;
    }
    sam_var_columns(ops, m, c, reverse, v);
    if (!reverse && clip) {
        t.element('S', clip);
        v.any = true;
    }
    if (!v.any) t.ch('*');
    return SamVarSpan{v.n_ref ? v.first_ref + v.left : behind, v.n_ref - v.left - v.right};
}
struct SamCigarCount {                                                  // a CIGAR's characters and elements
    uint32_t chars = 0, n = 0;
    RSQ_HD void element(char, uint32_t count) {
        chars += digits_u32(count) + 1u;
        ++n;
    }
    RSQ_HD void ch(char) { ++chars; }
};

// A mate's walk: sam_walk, the stretch, and -- only with an entry in reach -- the columns.  n_cigar: the CIGAR's elements where the columns were walked.
RSQ_HD SamVarMate sam_var_walk(const DevSim &S, bool has_f, const Fragment &f, bool has_fv, const FragmentVar &fv, uint32_t seg, const WordColumn &ops, const ReadMeta &m,
                               uint32_t &n_cigar) {
    SamVarMate e{};
    e.w = sam_walk(ops, m);
    n_cigar = 0;
    if (!has_f || !f.len) return e;
    const bool rev = seg != f.strand;
    const uint32_t t = e.w.t, d_left = rev ? e.w.trail : e.w.lead;
    e.ref_bases = t - e.w.lead - e.w.trail;
    if (!has_fv) {                                                      // allele copies: the fragment's own coordinates
        e.pos = (rev ? f.start + f.len - t : f.start) + d_left;
        return e;
    }
    // the stretch's first base, as allele_template finds it
    const AlleleView a = allele_view(S, f.seq, f.allele);
    const uint32_t var_pos = rev ? fv.end_var_pos : fv.start_var_pos, at = var_pos ? a.r.v[rev ? fv.end_var : fv.start_var].pos : rev ? fv.end : f.start;
    const uint32_t near = a.entries_before(at);                         // the mate's one bisection
    int64_t h = (int64_t)at + a.e[near].shift + var_pos - (rev ? t : 0u);
    if (h < 0) h = 0;
    const AllelePoint p = allele_point(a, h, near);
    e.entry = p.j;
    e.at = (uint32_t)h;
    e.pos = p.ref + d_left;
    bool reach = p.inside && (p.k || a.var(p.j - 1u).len != 1u);
    for (uint32_t j = p.j; !reach && j < a.n && a.e[j].pos - p.ref < t; ++j) reach = a.var(j).len != 1u;      // (a substitution moves no coordinate)
    if (reach) {
        e.w.pad = 1u;
        SamCigarCount count;
        const SamVarSpan span = sam_var_cigar(S, f, ops, m, e, rev, count);
        e.w.cigar_chars = (uint16_t)count.chars;
        e.pos = span.pos;
        e.ref_bases = span.ref_bases;
        n_cigar = count.n;
    }
    return e;
}
RSQ_HD SamAlign sam_var_align(bool has_f, const Fragment &f, uint32_t seg, const SamVarMate &e0, const SamVarMate &e1) {
    const int32_t pos[2] = {(int32_t)e0.pos + 1, (int32_t)e1.pos + 1}, last[2] = {pos[0] + (int32_t)e0.ref_bases - 1, pos[1] + (int32_t)e1.ref_bases - 1};
    return sam_align_at(has_f, f, seg, pos, last);
}

template <class Sink>
RSQ_HD void sam_var_head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &ops,
                         const SamVarMate &e, const SamAlign &a, Sink &t) {
    sam_qname_at(S, names, has_f, f, id.end, id.allele != 0u, adapter_only_number, m, t);
    sam_head_front(names, f, a, t);
    if (a.mapped) {
        sam_var_cigar(S, f, ops, m, e, a.reverse != 0u, t);
        sam_head_back(a, t);
    }
}
template <class Sink>
RSQ_HD void sam_var_tags_open(const ReadMeta &m, const WordColumn &ops, const SamVarId &id, Sink &t) {
    sam_tags_open(m, ops, t);
    t.str("\tXI:i:", 6);
    t.num(id.xi);
}
template <class Sink>
RSQ_HD void sam_var_tags(const ReadMeta &m, const WordColumn &ops, const SamVarId &id, Sink &t) {
    sam_var_tags_open(m, ops, id, t);
    t.ch('\n');
}
RSQ_HD uint32_t sam_var_tags_size(const ReadMeta &m, const SamVarId &id) { return sam_tags_size(m) + 6u + digits_u32(id.xi); }

// SAM text of a reference with variants as a format.  What differs from SamFormat's members: the FragmentVar's part (SamVarId) where the QNAME or the tags are
// written, and the alignment comes from the entries (sam_var_align).
struct SamVarFormat {
    static constexpr bool kVariants = true, kMd = false, kBam = false;
    using Mate = SamVarMate;
    using Pair = SamVarPair;
    static RSQ_HD void grow(Mate &e, uint32_t n) { e.w.bytes += n; }
    static RSQ_HD const SamVarMate &var(const Mate &e) { return e; }
    static RSQ_HD uint32_t bytes(const Mate &e) { return e.w.bytes; }
    static RSQ_HD Mate mate(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &,
                            const SamVarMate &w, uint32_t, const SamAlign &a) {
        Mate e = w;
        e.w.bytes = sam_qname_size_at(S, names, has_f, f, id.end, id.allele != 0u, adapter_only_number, m) + sam_head_fields_size(names, f, w.w.cigar_chars, a) + 2u * m.read_len + 1u +
                    sam_var_tags_size(m, id);
        return e;
    }
    template <class Sink>
    static RSQ_HD void head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                            const WordColumn &ops, const Mate &e, const SamAlign &a, Sink &t) {
        sam_var_head(S, names, has_f, f, id, adapter_only_number, m, ops, e, a, t);
        sam_line(seq, m.read_len, false, a.reverse != 0u, S.phred_offset, t);
        t.ch('\t');
    }
    template <class Sink>
    static RSQ_HD void tail(const DevSim &S, const ReadMeta &m, const SamVarId &id, const WordColumn &qual, const WordColumn &ops, const SamAlign &a, Sink &t) {
        sam_line(qual, m.read_len, true, a.reverse != 0u, S.phred_offset, t);
        sam_var_tags(m, ops, id, t);
    }
    template <class Sink>
    static RSQ_HD void tail_open(const DevSim &S, const ReadMeta &m, const SamVarId &id, const WordColumn &qual, const WordColumn &ops, const SamAlign &a, Sink &t) {
        sam_line(qual, m.read_len, true, a.reverse != 0u, S.phred_offset, t);
        sam_var_tags_open(m, ops, id, t);
    }
    static RSQ_HD uint32_t tail_at(const Mate &e, const ReadMeta &m, const SamVarId &id) { return e.w.bytes - sam_var_tags_size(m, id) - m.read_len; }
    template <class P>
    static RSQ_HD uint32_t record(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m,
                                  const WordColumn &seq, const WordColumn &qual, const WordColumn &ops, const Mate &e, const SamAlign &a, P dst) {
        WordSinkT<P> t(dst);
        head(S, names, has_f, f, id, adapter_only_number, m, seq, ops, e, a, t);
        tail(S, m, id, qual, ops, a, t);
        t.finish();
        return t.n;
    }
};

// ------------------------------------------------------------------------------------------------ a reference with variants, in ALLELE coordinates (rsq_sim_truth_alleles)
// The record against the sequence the fragment was drawn from: allele a of its sequence, a record of the alleles' FASTA text (rsq_alleles.h).  There the fragment is
// the stretch [hs, he) of the allele and the alignment is the PLAIN one of SamFormat with start := hs and end := he: no I or D comes from a variant, POS = hs + 1 +
// dL (forward) or he - t + 1 + dL (reverse).  RNAME is "<name>_allele<a>" (always, as the text's records are named); QNAME and the tags are those of the record in
// reference coordinates ("_allele<a>" when the id has it, XC, XE, XI:i -- XI ties the record to the id's reference positions).  hs is the allele coordinate of (start
// position, start variant); he is where allele_template ends the reverse mate's template -- inside inserted bases behind end_var_pos of them, else in front of
// whatever replaces the end position --, hs + len but for allele_cell's fragment inside one insertion.  One placement per pair (the bisection that finds hs; the
// entries up to the end position are walked from there: they lie inside the fragment), kept in the side entry: the writer neither searches nor walks the map.
// A format says so with kAlleles (formats without the member: AlleleCoordinates is false, and k_truth_sizes is the code it was).
template <class Format, class = void>
struct AlleleCoordinates {
    static constexpr bool value = false;
};
template <class Format>
struct AlleleCoordinates<Format, decltype((void)Format::kAlleles)> {
    static constexpr bool value = Format::kAlleles;
};
struct AlleleSpan {
    uint32_t hs, he;
};
RSQ_HD AlleleSpan sam_allele_span(const DevSim &S, bool has_f, const Fragment &f, bool has_fv, const FragmentVar &fv) {
    if (!has_f || !f.len) return AlleleSpan{0u, 0u};
    if (!has_fv) return AlleleSpan{f.start, f.start + f.len};           // allele copies: as long as the sequence
    const AlleleView a = allele_view(S, f.seq, f.allele);
    const uint32_t at = fv.start_var_pos ? a.r.v[fv.start_var].pos : f.start, end = fv.end_var_pos ? a.r.v[fv.end_var].pos : fv.end;
    uint32_t j = a.entries_before(at);                                  // the pair's one bisection
    const int64_t hs = (int64_t)at + a.e[j].shift + fv.start_var_pos;
    while (j < a.n && a.e[j].pos < end) ++j;                            // entries_before(end)
    return AlleleSpan{(uint32_t)hs, (uint32_t)((int64_t)end + a.e[j].shift + fv.end_var_pos)};
}
// a mate's entry: the plain walk (pad 0: sam_cigar writes the CIGAR), placed in the allele
RSQ_HD SamVarMate sam_allele_walk(bool has_f, const Fragment &f, const AlleleSpan &span, uint32_t seg, const WordColumn &ops, const ReadMeta &m) {
    SamVarMate e{};
    e.w = sam_walk(ops, m);
    if (!has_f || !f.len) return e;
    const bool rev = seg != f.strand;
    e.ref_bases = (uint32_t)e.w.t - e.w.lead - e.w.trail;
    e.pos = (rev ? span.he - e.w.t : span.hs) + (rev ? e.w.trail : e.w.lead);
    e.at = span.hs;
    return e;
}
RSQ_HD uint32_t sam_allele_name_size(const Fragment &f, const SamAlign &a) { return a.mapped ? 7u + digits_u32(f.allele) : 0u; }
struct SamAlleleFormat : SamVarFormat {
    static constexpr bool kAlleles = true;
    static RSQ_HD Mate mate(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &ops,
                            const SamVarMate &w, uint32_t n_cigar, const SamAlign &a) {
        Mate e = SamVarFormat::mate(S, names, has_f, f, id, adapter_only_number, m, ops, w, n_cigar, a);
        e.w.bytes += sam_allele_name_size(f, a);
        return e;
    }
    template <class Sink>
    static RSQ_HD void head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                            const WordColumn &ops, const Mate &e, const SamAlign &a, Sink &t) {
        sam_qname_at(S, names, has_f, f, id.end, id.allele != 0u, adapter_only_number, m, t);
        t.ch('\t');
        t.num(a.flag);
        t.ch('\t');
        if (a.mapped) {
            t.str(names.names + names.name_ptr[f.seq], names.name_ptr[f.seq + 1] - names.name_ptr[f.seq]);
            t.str("_allele", 7);
            t.num((uint32_t)f.allele);
            t.ch('\t');
            t.num(a.pos);
            t.str("\t60\t", 4);
            sam_cigar(ops, m, e.w, a.reverse != 0u, t);
            sam_head_back(a, t);
        } else t.str("*\t0\t0\t*\t*\t0\t0\t", 14);
        sam_line(seq, m.read_len, false, a.reverse != 0u, S.phred_offset, t);
        t.ch('\t');
    }
    template <class P>
    static RSQ_HD uint32_t record(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m,
                                  const WordColumn &seq, const WordColumn &qual, const WordColumn &ops, const Mate &e, const SamAlign &a, P dst) {
        WordSinkT<P> t(dst);
        head(S, names, has_f, f, id, adapter_only_number, m, seq, ops, e, a, t);
        tail(S, m, id, qual, ops, a, t);
        t.finish();
        return t.n;
    }
};

#if RSQ_DEVICE_BUILD
// One lane per raw row pair (row i of both segments: the two mates of pair perm[i], or of pair i): both mates' entries into side[row], the pair's bytes into
// sizes[pair].  fvars: read by the formats of a reference with variants only (nullptr: allele copies)
template <class Format>
__global__ void __launch_bounds__(256) k_truth_sizes(DevSim S, NameTable names, const Fragment *frags, uint64_t n_pairs, uint64_t adapter_only_first, RawLayout raw, const uint32_t *perm,
                                                     typename Format::Pair *side, uint32_t *sizes, const FragmentVar *fvars) {
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_pairs) return;
    const uint64_t pair = perm ? perm[row] : row;
    Fragment f{};
    if (frags) f = frags[pair];
    const bool has_f = frags != nullptr;
    const ReadMeta m0 = raw.meta[row], m1 = raw.meta[n_pairs + row];
    const WordColumn ops0 = raw.ops_of(row), ops1 = raw.ops_of(n_pairs + row);
    const uint64_t ao_number = adapter_only_first + pair + 1u;
    typename Format::Pair p;
    if constexpr (Format::kVariants) {
        const bool has_fv = has_f && fvars != nullptr;
        FragmentVar fv{};
        if (has_fv) fv = fvars[pair];
        const SamVarId id = sam_var_id(S, f, has_fv, fv);
        if constexpr (AlleleCoordinates<Format>::value) {               // (allele coordinates: the pair's one placement, two plain walks)
            const AlleleSpan span = sam_allele_span(S, has_f, f, has_fv, fv);
            const SamVarMate w0 = sam_allele_walk(has_f, f, span, 0u, ops0, m0), w1 = sam_allele_walk(has_f, f, span, 1u, ops1, m1);
            p.mate[0] = Format::mate(S, names, has_f, f, id, ao_number, m0, ops0, w0, 0u, sam_var_align(has_f, f, 0u, w0, w1));
            p.mate[1] = Format::mate(S, names, has_f, f, id, ao_number, m1, ops1, w1, 0u, sam_var_align(has_f, f, 1u, w0, w1));
            side[row] = p;
            sizes[pair] = Format::bytes(p.mate[0]) + Format::bytes(p.mate[1]);
            return;
        }
        uint32_t n0, n1;
        const SamVarMate w0 = sam_var_walk(S, has_f, f, has_fv, fv, 0u, ops0, m0, n0), w1 = sam_var_walk(S, has_f, f, has_fv, fv, 1u, ops1, m1, n1);
        if constexpr (Format::kMd) {                                    // (rsq_md.h: the entry also takes what comparing SEQ with the reference comes to)
            p.mate[0] = Format::mate(S, names, has_f, f, id, ao_number, m0, raw.seq_of(row), ops0, w0, n0, sam_var_align(has_f, f, 0u, w0, w1));
            p.mate[1] = Format::mate(S, names, has_f, f, id, ao_number, m1, raw.seq_of(n_pairs + row), ops1, w1, n1, sam_var_align(has_f, f, 1u, w0, w1));
        } else {
            p.mate[0] = Format::mate(S, names, has_f, f, id, ao_number, m0, ops0, w0, n0, sam_var_align(has_f, f, 0u, w0, w1));
            p.mate[1] = Format::mate(S, names, has_f, f, id, ao_number, m1, ops1, w1, n1, sam_var_align(has_f, f, 1u, w0, w1));
        }
    } else {
        const SamMate w0 = sam_walk(ops0, m0), w1 = sam_walk(ops1, m1);
        if constexpr (Format::kMd) {
            p.mate[0] = Format::mate(S, names, has_f, f, ao_number, m0, raw.seq_of(row), ops0, w0, sam_align(has_f, f, 0u, w0, w1));
            p.mate[1] = Format::mate(S, names, has_f, f, ao_number, m1, raw.seq_of(n_pairs + row), ops1, w1, sam_align(has_f, f, 1u, w0, w1));
        } else {
            p.mate[0] = Format::mate(S, names, has_f, f, ao_number, m0, ops0, w0, sam_align(has_f, f, 0u, w0, w1));
            p.mate[1] = Format::mate(S, names, has_f, f, ao_number, m1, ops1, w1, sam_align(has_f, f, 1u, w0, w1));
        }
    }
    side[row] = p;
    sizes[pair] = Format::bytes(p.mate[0]) + Format::bytes(p.mate[1]);
}

// One wave per 16 consecutive raw rows = 16 pairs, four lanes a pair, through the wave's image (WaveImage, rsq_format.h; the wave's 32 records are one
// contiguous byte range of the output, PERM: a slot per pair): lanes 0-15 write the head of mate 0's record (everything in front of QUAL), lanes 16-31 its tail
// (QUAL and the tags), lanes 32-47 and 48-63 the same of mate 1.  Nothing is written when any of the call's three outputs exceeds its capacity so far
// (fastq_end: the FASTQ offsets' last entries).  A wave whose records do not fit the image writes them straight to dst, a lane a record (Format::record).
constexpr uint32_t kSamPairs = 16, kSamLdsMax = 32u * 1024u, kSamLdsMin = 2048u;
RSQ_HD uint32_t sam_lds_bytes(uint64_t pair_bytes, bool slots) {        // the image for pairs of at most pair_bytes; slots: each its own alignment
    const uint64_t want = (kSamPairs * (pair_bytes + (slots ? 16u : 0u)) + 16u + 127u) & ~(uint64_t)127u;
    return (uint32_t)(want < kSamLdsMin ? kSamLdsMin : want > kSamLdsMax ? kSamLdsMax : want);
}
template <class Format, bool PERM>
__global__ void __launch_bounds__(64) k_truth_write(DevSim S, NameTable names, const Fragment *frags, uint64_t n_pairs, uint64_t adapter_only_first, RawLayout raw,
                                                   const typename Format::Pair *side, const uint64_t *offsets, char *dst, uint64_t cap, const uint64_t *fastq_end0,
                                                   const uint64_t *fastq_end1, uint64_t fastq_cap0, uint64_t fastq_cap1, const uint32_t *perm, uint32_t lds_bytes,
                                                   const FragmentVar *fvars) {
    extern __shared__ __attribute__((aligned(16))) char s_truth[];
    using Image = WaveImage<PERM, kSamPairs>;
    const uint32_t lane = threadIdx.x, part = lane / kSamPairs, seg = part >> 1, half = part & 1u;
    if (Image::first() >= n_pairs) return;
    if (offsets[n_pairs] > cap || *fastq_end0 > fastq_cap0 || *fastq_end1 > fastq_cap1) return;      // a buffer of the call is too small: write nothing (RSQ_ENOSPC)
    const Image im(offsets, n_pairs, dst, lds_bytes, perm, lane);
    const uint64_t pair = im.item;
    ReadMeta m{};
    Fragment f{};
    typename Format::Pair p{};
    uint64_t r = 0;
    if (im.active) {
        r = (uint64_t)seg * n_pairs + im.row;
        m = raw.meta[r];
        p = side[im.row];
        if (frags) f = frags[pair];
    }
    const bool has_f = frags != nullptr;
    const WordColumn seq = raw.seq_of(r), qual = raw.qual_of(r), ops = raw.ops_of(r);
    const uint64_t ao_number = adapter_only_first + pair + 1u;
    const typename Format::Mate e = seg ? p.mate[1] : p.mate[0];
    const uint32_t rec_at = seg ? Format::bytes(p.mate[0]) : 0u;       // of the record within its pair's bytes
    if constexpr (Format::kVariants) {
        const bool has_fv = has_f && fvars != nullptr && im.active;
        FragmentVar fv{};
        if (has_fv) fv = fvars[pair];
        const SamVarId id = sam_var_id(S, f, has_fv, fv);
        const SamAlign a = sam_var_align(has_f, f, seg, Format::var(p.mate[0]), Format::var(p.mate[1]));
        if (!im.through_lds) {
            if (im.active && half == 0u) Format::record(S, names, has_f, f, id, ao_number, m, seq, qual, ops, e, a, dst + offsets[pair] + rec_at);
            return;
        }
        im.clear(s_truth, lds_bytes);
        if (im.active) {
            ImageSink t(im.item_text(s_truth) + rec_at + (half ? Format::tail_at(e, m, id) : 0u));
            if (half == 0u) Format::head(S, names, has_f, f, id, ao_number, m, seq, ops, e, a, t);
            else if constexpr (Format::kMd) Format::tail(S, f, m, id, seq, qual, ops, e, a, t);      // (the tail lane compares SEQ with the reference again and prints MD)
            else Format::tail(S, m, id, qual, ops, a, t);
            t.finish();
        }
    } else {
        const SamAlign a = sam_align(has_f, f, seg, Format::walk(p.mate[0]), Format::walk(p.mate[1]));
        if (!im.through_lds) {
            if (im.active && half == 0u) Format::record(S, names, has_f, f, ao_number, m, seq, qual, ops, e, a, dst + offsets[pair] + rec_at);
            return;
        }
        im.clear(s_truth, lds_bytes);
        if (im.active) {
            ImageSink t(im.item_text(s_truth) + rec_at + (half ? Format::tail_at(e, m) : 0u));
            if (half == 0u) Format::head(S, names, has_f, f, ao_number, m, seq, ops, e, a, t);
            else if constexpr (Format::kMd) Format::tail(S, f, m, seq, qual, ops, e, a, t);
            else Format::tail(S, m, qual, ops, a, t);
            t.finish();
        }
    }
    im.store_out(s_truth);
}
#endif

}  // namespace rsq
