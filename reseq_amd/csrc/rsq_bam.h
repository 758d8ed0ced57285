// rsq_bam.h -- truth alignments as BAM: the records of rsq_sam.h, one per simulated read, in BAM's binary layout (SAM specification 4.2), written on the device from
// the same raw rows and the same fragment list.  A BAM record is a pure re-encoding of its SAM line: the walk (sam_walk), the alignment (sam_align), the QNAME
// (sam_qname), the CIGAR's elements (sam_cigar) and the XC tag (cigar_replay) are rsq_sam.h's own, called with other sinks; this file adds what is BAM's.
//
// The record, little-endian, no padding:
//   block_size i32 (the bytes behind it) | refID i32 | pos i32 (POS - 1) | l_read_name u8 | mapq u8 | bin u16 | n_cigar_op u16 | flag u16 | l_seq u32 |
//   next_refID i32 | next_pos i32 | tlen i32 | read_name NUL | cigar u32[n] (len << 4 | op; M 0, I 1, D 2, S 4) | seq u8[(l_seq + 1) / 2] | qual u8[l_seq] |
//   "XC" 'Z' <the id's CIGAR> NUL | "XE" 'S' u16
// bin = reg2bin(pos, pos + max(span, 1)), span the reference bases of the cleaned CIGAR (t - dL - dR).  Unmapped records (adapter-only pairs, fragment length 0):
// refID = next_refID = pos = next_pos = -1, mapq 0, bin 4680 (reg2bin(-1, 0)), no CIGAR, tlen 0, flags 77 / 141, SEQ and QUAL as in the FASTQ.
// SEQ holds 4-bit codes (A 1, C 2, G 4, T 8, N 15), the earlier base in the high nibble; a reverse mate (0x10) stores the reverse complement -- on these codes the
// complement is the nibble's bit reversal, N stays 15 -- and its qualities reversed.  QUAL is the character minus the profile's Phred offset.
//
// bam_seq is the part with a shape of its own: a row word holds four base codes, one byte each; one byte permute turns them into four nibbles (the table of the
// forward or of the complemented codes), a shift-or puts neighbouring nibbles into one byte, and a second permute gathers the four bytes of two row words into one
// output word.  The words come from sam_line's row walk (RowRound, rsq_sam.h) in OUTPUT order, so the pairing of nibbles is always (0, 1), (2, 3), ... of the
// output, whatever read_len & 1: an odd length leaves the last low nibble 0 in either orientation.
//
// Per lane, host and device (tests/hostemu/truth_trial.h runs them on the CPU): bam_record_size, bam_fixed, bam_cigar, bam_seq, bam_qual, bam_tags, bam_record, bam_mate.
// BamVarFormat (the end of this file) is the same encoding of SamVarFormat's record, for a reference with variants: "XI" 'I' u32 follows XE.
// BamFormat makes them a format of rsq_sam.h: its kernels (k_truth_sizes, k_truth_write), frame and fallback are that file's, with a side array of BAM's own --
// records are not word-aligned, the frame handles that as it does for text.  Not part of what hiprtc compiles for a profile (rsq_spec.h): nothing of the read
// kernel's text includes this file.
#pragma once
#include "rsq_sam.h"

namespace rsq {

// a mate's walk and what its BAM record needs beside it (k_truth_sizes keeps them so that the writer neither walks the ops nor counts again)
struct BamMate {
    SamMate w;                 // w.bytes: of the mate's BAM record, its block_size field included
    uint16_t n_cigar;          // elements of the CIGAR (0: unmapped, or "*")
    uint16_t l_read_name;      // QNAME length + 1
    uint32_t pad;
};
static_assert(sizeof(BamMate) == 24, "the side array's entry");
struct BamPair {
    BamMate mate[2];
};

constexpr uint32_t kBamMaxQname = 254;                                  // l_read_name is a byte and counts the NUL
constexpr uint32_t kBamMaxRefLen = 1u << 29;                            // what the binning scheme covers
constexpr uint32_t kBamUnmappedBin = 4680;                              // reg2bin(-1, 0)

// SAM specification 5.3: the smallest bin that holds [beg, end), 0-based, end > beg
RSQ_HD uint32_t bam_reg2bin(uint32_t beg, uint32_t end) {
    --end;
    if (beg >> 14 == end >> 14) return ((1u << 15) - 1u) / 7u + (beg >> 14);
    if (beg >> 17 == end >> 17) return ((1u << 12) - 1u) / 7u + (beg >> 17);
    if (beg >> 20 == end >> 20) return ((1u << 9) - 1u) / 7u + (beg >> 20);
    if (beg >> 23 == end >> 23) return ((1u << 6) - 1u) / 7u + (beg >> 23);
    if (beg >> 26 == end >> 26) return ((1u << 3) - 1u) / 7u + (beg >> 26);
    return 0u;
}

// sam_cigar's elements, counted and as BAM's words (its "*" is no element)
struct BamCigarCount {
    uint32_t n = 0;
    RSQ_HD void element(char, uint32_t) { ++n; }
    RSQ_HD void ch(char) {}
};
template <class Sink>
struct BamCigarWords {
    Sink &t;
    RSQ_HD void element(char op, uint32_t count) { t.bytes((count << 4) | (op == 'M' ? 0u : op == 'I' ? 1u : op == 'D' ? 2u : 4u), 4u); }
    RSQ_HD void ch(char) {}
};
RSQ_HD uint32_t bam_cigar_ops(const WordColumn &ops, const ReadMeta &m, const SamMate &w, const SamAlign &a) {
    if (!a.mapped) return 0u;
    BamCigarCount c;
    sam_cigar(ops, m, w, a.reverse != 0u, c);
    return c.n;
}
template <class Sink>
RSQ_HD void bam_cigar(const WordColumn &ops, const ReadMeta &m, const SamMate &w, const SamAlign &a, Sink &t) {
    if (!a.mapped) return;
    BamCigarWords<Sink> c{t};
    sam_cigar(ops, m, w, a.reverse != 0u, c);
}

RSQ_HD uint32_t bam_tags_size(const ReadMeta &m) { return 3u + m.cigar_chars + 1u + 5u; }
// length of a record (with its block_size field) without producing it
RSQ_HD uint32_t bam_record_size(const ReadMeta &m, uint32_t l_read_name, uint32_t n_cigar) {
    return 36u + l_read_name + 4u * n_cigar + (((uint32_t)m.read_len + 1u) >> 1) + m.read_len + bam_tags_size(m);
}

// block_size and the 32 bytes of fixed fields: nine words
template <class Sink>
RSQ_HD void bam_fixed_span(const Fragment &f, const ReadMeta &m, uint32_t span, const SamAlign &a, uint32_t l_read_name, uint32_t n_cigar, uint32_t block_size, Sink &t) {
    const uint32_t none = 0xFFFFFFFFu;
    const uint32_t ref_id = a.mapped ? f.seq : none, pos = a.mapped ? a.pos - 1u : none, pnext = a.mapped ? a.pnext - 1u : none;
    const uint32_t bin = a.mapped ? bam_reg2bin(pos, pos + (span ? span : 1u)) : kBamUnmappedBin, mapq = a.mapped ? 60u : 0u;
    t.bytes(block_size, 4u);
    t.bytes(ref_id, 4u);
    t.bytes(pos, 4u);
    t.bytes(l_read_name | (mapq << 8) | (bin << 16), 4u);
    t.bytes(n_cigar | (a.flag << 16), 4u);
    t.bytes((uint32_t)m.read_len, 4u);
    t.bytes(ref_id, 4u);
    t.bytes(pnext, 4u);
    t.bytes((uint32_t)a.tlen, 4u);
}
template <class Sink>
RSQ_HD void bam_fixed(const Fragment &f, const ReadMeta &m, const SamMate &w, const SamAlign &a, uint32_t l_read_name, uint32_t n_cigar, uint32_t block_size, Sink &t) {
    bam_fixed_span(f, m, (uint32_t)w.t - w.lead - w.trail, a, l_read_name, n_cigar, block_size, t);
}

// (bam_nibbles: four base codes -> their 4-bit codes; bam_pack: eight 4-bit codes -> four bytes; both rsq_portable.h)
// SEQ: the row's words in output order (sam_line's walk), two of them an output word.  What lies behind the row's last code becomes nibble 0.
template <class Sink>
RSQ_HD void bam_seq(const WordColumn &row, uint32_t read_len, bool reverse, Sink &t) {
    static_assert(kRowAhead % 2u == 0u, "an output word never spans two rounds");
    const uint32_t words = (read_len + 3u) >> 2;
    for (uint32_t i = 0; i < words; i += kRowAhead) {
        const RowRound round(row, read_len, reverse, i);
        uint32_t nib[kRowAhead];
#pragma unroll
        for (uint32_t k = 0; k < kRowAhead; ++k) {
            const uint32_t at = 4u * (i + k), left = at < read_len ? read_len - at : 0u;
            nib[k] = bam_nibbles(round.at(k), reverse) & (left >= 4u ? 0xFFFFFFFFu : (1u << (8u * left)) - 1u);
        }
#pragma unroll
        for (uint32_t k = 0; k < kRowAhead; k += 2u) {
            if (i + k >= words) break;
            const uint32_t left = read_len - 4u * (i + k);
            t.bytes(bam_pack(nib[k], nib[k + 1u]), left >= 8u ? 4u : (left + 1u) >> 1);
        }
    }
}
// QUAL: sam_line's qualities with the whole offset taken off (it subtracts its offset argument - 33)
template <class Sink>
RSQ_HD void bam_qual(const WordColumn &row, uint32_t read_len, bool reverse, uint32_t phred_offset, Sink &t) {
    sam_line(row, read_len, true, reverse, phred_offset + 33u, t);
}
template <class Sink>
RSQ_HD void bam_tags(const ReadMeta &m, const WordColumn &ops, Sink &t) {
    t.bytes(chars4('X', 'C', 'Z'), 3u);
    cigar_replay(ops, m, t);
    t.bytes(chars4(0, 'X', 'E', 'S'), 4u);
    t.bytes((uint32_t)m.num_errors, 2u);
}
// the record's first stretch: everything in front of QUAL
template <class Sink>
RSQ_HD void bam_head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq, const WordColumn &ops,
                     const BamMate &b, const SamAlign &a, Sink &t) {
    bam_fixed(f, m, b.w, a, b.l_read_name, b.n_cigar, b.w.bytes - 4u, t);
    sam_qname(S, names, has_f, f, adapter_only_number, m, t);
    t.ch(0);
    bam_cigar(ops, m, b.w, a, t);
    bam_seq(seq, m.read_len, a.reverse != 0u, t);
}
// the whole record at dst; returns its length
template <class P>
RSQ_HD uint32_t bam_record(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                           const WordColumn &qual, const WordColumn &ops, const BamMate &b, const SamAlign &a, P dst) {
    WordSinkT<P> t(dst);
    bam_head(S, names, has_f, f, adapter_only_number, m, seq, ops, b, a, t);
    bam_qual(qual, m.read_len, a.reverse != 0u, S.phred_offset, t);
    bam_tags(m, ops, t);
    t.finish();
    return t.n;
}
// a mate's side entry from its walk
RSQ_HD BamMate bam_mate(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &ops, const SamMate &w,
                        const SamAlign &a) {
    BamMate b{};
    b.w = w;
    b.n_cigar = (uint16_t)bam_cigar_ops(ops, m, w, a);
    b.l_read_name = (uint16_t)(sam_qname_size(S, names, has_f, f, adapter_only_number, m) + 1u);
    b.w.bytes = bam_record_size(m, b.l_read_name, b.n_cigar);
    return b;
}


// BAM records as a format (rsq_sam.h states what a format is)
struct BamFormat {
    static constexpr bool kVariants = false, kMd = false, kBam = true;
    using Mate = BamMate;
    using Pair = BamPair;
    static RSQ_HD void grow(Mate &e, uint32_t n) { e.w.bytes += n; }    // more tags behind the record's own (rsq_md.h): block_size covers them
    static RSQ_HD const SamMate &walk(const Mate &e) { return e.w; }
    static RSQ_HD uint32_t bytes(const Mate &e) { return e.w.bytes; }
    static RSQ_HD Mate mate(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &ops, const SamMate &w,
                            const SamAlign &a) {
        return bam_mate(S, names, has_f, f, adapter_only_number, m, ops, w, a);
    }
    template <class Sink>
    static RSQ_HD void head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                            const WordColumn &ops, const Mate &e, const SamAlign &a, Sink &t) {
        bam_head(S, names, has_f, f, adapter_only_number, m, seq, ops, e, a, t);
    }
    template <class Sink>
    static RSQ_HD void tail(const DevSim &S, const ReadMeta &m, const WordColumn &qual, const WordColumn &ops, const SamAlign &a, Sink &t) {
        bam_qual(qual, m.read_len, a.reverse != 0u, S.phred_offset, t);
        bam_tags(m, ops, t);
    }
    template <class Sink>
    static RSQ_HD void tail_open(const DevSim &S, const ReadMeta &m, const WordColumn &qual, const WordColumn &ops, const SamAlign &a, Sink &t) {      // (a BAM record has no terminator)
        tail(S, m, qual, ops, a, t);
    }
    static RSQ_HD uint32_t tail_at(const Mate &e, const ReadMeta &m) { return e.w.bytes - bam_tags_size(m) - m.read_len; }
    template <class P>
    static RSQ_HD uint32_t record(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                                  const WordColumn &qual, const WordColumn &ops, const Mate &e, const SamAlign &a, P dst) {
        return bam_record(S, names, has_f, f, adapter_only_number, m, seq, qual, ops, e, a, dst);
    }
};

// ------------------------------------------------------------------------------------------------ a reference with variants (rsq_sam.h SamVarFormat)
// The same re-encoding of the same record: POS, the bin and the CIGAR's words come from the variant entry, the QNAME carries the id's "_allele<a>" and end position,
// and "XI" 'I' u32 follows XE.
struct BamVarMate {
    SamVarMate v;              // v.w.bytes: of the mate's BAM record, its block_size field included
    uint16_t n_cigar;
    uint16_t l_read_name;
    uint32_t pad;
};
static_assert(sizeof(BamVarMate) == 40, "the side array's entry");
struct BamVarPair {
    BamVarMate mate[2];
};
constexpr uint32_t kBamVarTag = 7u;                                     // "XI" 'I' u32
struct BamVarFormat {
    static constexpr bool kVariants = true, kMd = false, kBam = true;
    using Mate = BamVarMate;
    using Pair = BamVarPair;
    static RSQ_HD void grow(Mate &e, uint32_t n) { e.v.w.bytes += n; }
    static RSQ_HD const SamVarMate &var(const Mate &e) { return e.v; }
    static RSQ_HD uint32_t bytes(const Mate &e) { return e.v.w.bytes; }
    static RSQ_HD Mate mate(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &ops,
                            const SamVarMate &w, uint32_t n_cigar, const SamAlign &a) {
        Mate b{};
        b.v = w;
        b.n_cigar = (uint16_t)(w.w.pad ? (a.mapped ? n_cigar : 0u) : bam_cigar_ops(ops, m, w.w, a));
        b.l_read_name = (uint16_t)(sam_qname_size_at(S, names, has_f, f, id.end, id.allele != 0u, adapter_only_number, m) + 1u);
        b.v.w.bytes = bam_record_size(m, b.l_read_name, b.n_cigar) + kBamVarTag;
        return b;
    }
    template <class Sink>
    static RSQ_HD void head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                            const WordColumn &ops, const Mate &e, const SamAlign &a, Sink &t) {
        bam_fixed_span(f, m, e.v.ref_bases, a, e.l_read_name, e.n_cigar, e.v.w.bytes - 4u, t);
        sam_qname_at(S, names, has_f, f, id.end, id.allele != 0u, adapter_only_number, m, t);
        t.ch(0);
        if (a.mapped) {
            BamCigarWords<Sink> c{t};
            sam_var_cigar(S, f, ops, m, e.v, a.reverse != 0u, c);
        }
        bam_seq(seq, m.read_len, a.reverse != 0u, t);
    }
    template <class Sink>
    static RSQ_HD void tail(const DevSim &S, const ReadMeta &m, const SamVarId &id, const WordColumn &qual, const WordColumn &ops, const SamAlign &a, Sink &t) {
        bam_qual(qual, m.read_len, a.reverse != 0u, S.phred_offset, t);
        bam_tags(m, ops, t);
        t.bytes(chars4('X', 'I', 'I'), 3u);
        t.bytes(id.xi, 4u);
    }
    template <class Sink>
    static RSQ_HD void tail_open(const DevSim &S, const ReadMeta &m, const SamVarId &id, const WordColumn &qual, const WordColumn &ops, const SamAlign &a, Sink &t) {
        tail(S, m, id, qual, ops, a, t);
    }
    static RSQ_HD uint32_t tail_at(const Mate &e, const ReadMeta &m, const SamVarId &) { return e.v.w.bytes - bam_tags_size(m) - kBamVarTag - m.read_len; }
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

// ------------------------------------------------------------------------------------------------ ... in allele coordinates (rsq_sam.h SamAlleleFormat)
// The same re-encoding of that record: refID = next_refID = seq * num_alleles + allele, the index of the allele's record in the alleles' FASTA text and in the
// header of rsq_ref_bam_header_alleles; pos and the bin over allele positions; the CIGAR's words from the plain walk.  The entry is BamVarFormat's.
struct BamAlleleFormat : BamVarFormat {
    static constexpr bool kAlleles = true;
    template <class Sink>
    static RSQ_HD void head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                            const WordColumn &ops, const Mate &e, const SamAlign &a, Sink &t) {
        Fragment in_allele = f;
        in_allele.seq = f.seq * S.num_alleles + f.allele;
        bam_fixed_span(in_allele, m, e.v.ref_bases, a, e.l_read_name, e.n_cigar, e.v.w.bytes - 4u, t);
        sam_qname_at(S, names, has_f, f, id.end, id.allele != 0u, adapter_only_number, m, t);
        t.ch(0);
        bam_cigar(ops, m, e.v.w, a, t);
        bam_seq(seq, m.read_len, a.reverse != 0u, t);
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

}  // namespace rsq
