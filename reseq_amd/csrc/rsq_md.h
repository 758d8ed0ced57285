// rsq_md.h -- truth alignments: the tags NM:i and MD:Z behind a mapped record's own tags (rsq_sim_truth_md; DESIGN.md 4.8 states the rule).  Both are a pure
// function of the finished record and the reference as loaded -- copy 0 of the packed reference (DevSim::ref_words), never an allele's copy:
//   r = POS - 1, q = 0, run = 0; over the CIGAR: M: per base, SEQ[q] == ref[r] ? ++run : (MD += run, ref[r]; run = 0; ++NM); I: q += n, NM += n; S: q += n;
//   D: MD += run, '^', ref[r, r + n); run = 0; r += n; NM += n; at the end MD += run.
// which is what samtools calmd writes: a 0 between neighbouring mismatches and between a deletion and a mismatch behind it, a number at the end.  A read base N
// is a mismatch (MD names the reference base); a mate without an M column has MD:Z:0.  Unmapped records carry neither tag.
//
// Per lane, host and device (tests/hostemu/truth_md_trial.cpp runs them on the CPU).  The comparison takes up to 32 bases a step: md_seq_chunk packs the SEQ row's
// words -- RowRound (rsq_sam.h) hands them out oriented for output -- to two bits a base and a bit for N, MdRef funnels the same stretch out of two reference
// words (it holds the words it last read), and a stretch without a mismatch costs an exclusive-or, a test and an add.  The columns come from the walks the CIGAR
// comes from: md_plain_columns replays the ops as sam_cigar does (16 plain iterations at once), a mate with an allele-map entry in reach goes through
// sam_var_columns with the same visitor.  MdCols merges equal neighbours, so an M run is compared in whole steps however its columns arrive, and drops D runs at
// either end as sam_walk and SamVarRuns drop them.
//
// MdFormat<Base> makes a format with the tags out of each of the four (rsq_sam.h states what a format is): its entry is Base's with NM and the MD string's length
// behind it -- k_truth_sizes compares once, the writer's tail lane compares again and prints, and places its part from the entry alone.
#pragma once
#include "rsq_bam.h"

namespace rsq {

// four base codes, one per byte (0..3 ACGT, 4..7 N) -> two bits each, the first lowest; the N bits of the same four at bits 0, 2, 4, 6
// (the products' partial sums meet no other's bits: no carries)
RSQ_HD uint32_t md_pack_codes(uint32_t v) { return ((v & 0x03030303u) * 0x01041040u) >> 24; }
RSQ_HD uint32_t md_pack_n(uint32_t v) { return (((v >> 2) & 0x01010101u) * 0x01041040u) >> 24; }
RSQ_HD uint32_t md_ref_letter(uint32_t code) { return (0x54474341u >> (8u * code)) & 0xFFu; }      // "ACGT"

// SEQ as written, from base q to the end of the eight output words q lies in the first of (32 - (q & 3) bases, fewer at the read's end: what lies behind is not
// to be looked at): two bits a base in output order -- a reverse mate's are the complements --, and bit 2i set where base i is N
struct MdSeqChunk {
    uint64_t codes, n;
};
RSQ_HD MdSeqChunk md_seq_chunk(const WordColumn &row, uint32_t read_len, bool reverse, uint32_t q) {
    static_assert(kRowAhead >= 8u, "a chunk is one round of row words");
    const RowRound round(row, read_len, reverse, q >> 2);
    uint64_t c = 0, n = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
        const uint32_t v = round.at(k);
        c |= (uint64_t)md_pack_codes(v) << (8u * k);
        n |= (uint64_t)md_pack_n(v) << (8u * k);
    }
    if (reverse) c = ~c;
    const uint32_t s = 2u * (q & 3u);
    return MdSeqChunk{c >> s, n >> s};
}

// The reference sequence's words of copy 0, streamed: codes(p) are the 32 bases from position p, out of the two words they lie in.  The word behind a sequence's
// last base exists (every sequence is packed with one more word than it needs, rsq_pack.h upload_reference); a position behind the sequence reads its last words.
struct MdRef {
    const uint64_t *w;
    uint32_t last;             // the word of the sequence's last base
    uint32_t at = 0;
    bool have = false;
    uint64_t lo = 0, hi = 0;
    RSQ_HD MdRef(const DevSim &S, uint32_t seq) : w(S.ref_words + S.seq_word_off[seq]), last(S.seq_len[seq] ? (S.seq_len[seq] - 1u) >> 5 : 0u) {}
    RSQ_HD uint64_t codes(uint32_t p) {
        uint32_t idx = p >> 5;
        if (idx > last) idx = last;
        if (!have || idx != at) {
            lo = have && idx == at + 1u ? hi : w[idx];
            hi = w[idx + 1u];
            at = idx;
            have = true;
        }
        const uint32_t sh = 2u * (p & 31u);
        return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
    }
};

// A sink that wants to know WHERE a mismatch stands has a member mismatch(q), q the column's place in SEQ as written (rsq_stats.h); the sinks that write the
// string have none and are handed nothing more than before.
template <class Out>
RSQ_HD auto md_note_mismatch(Out &o, uint32_t q, int) -> decltype(o.mismatch(q), void()) { o.mismatch(q); }
template <class Out>
RSQ_HD void md_note_mismatch(Out &, uint32_t, long) {}
// A sink that wants the columns themselves (rsq_pileup.h) has two members more, found the same way: column_run(op, p, n) for every merged run before it is taken
// -- op 0 M, 1 a kept D run, 2 I (p means nothing), 3 a D run dropped at either end --, and mismatch_base(p, code) with the reference position of a mismatch and
// the read's base as written (0..3 ACGT, 4 N).
template <class Out>
RSQ_HD auto md_note_run(Out &o, uint32_t op, uint32_t p, uint32_t n, int) -> decltype(o.column_run(op, p, n), void()) { o.column_run(op, p, n); }
template <class Out>
RSQ_HD void md_note_run(Out &, uint32_t, uint32_t, uint32_t, long) {}
template <class Out>
RSQ_HD auto md_note_base(Out &o, uint32_t p, uint32_t n_bit, uint32_t code, int) -> decltype(o.mismatch_base(p, code), void()) { o.mismatch_base(p, n_bit ? 4u : code); }
template <class Out>
RSQ_HD void md_note_base(Out &, uint32_t, uint32_t, uint32_t, long) {}

// The visitor of a mate's columns in ascending reference order (op: 0 M, 1 D, 2 I; p: the reference position of the first of `count` M or D columns): the MD
// string into `o` (num, ch, bytes, element: any sink of rsq_text.h / rsq_format.h, or MdCount), NM in nm.  q: the column's place in SEQ as written.
template <class Out>
struct MdCols {
    Out &o;
    MdRef ref;
    const WordColumn &seq;
    uint32_t read_len;
    bool reverse;
    uint32_t q;
    uint32_t run = 0, nm = 0;
    uint32_t cur = 3u, cp = 0, cn = 0;                                  // the columns not yet taken: cn of op cur from reference position cp
    bool any = false;                                                   // a column in front of them was kept: a D run is no longer the first
    RSQ_HD MdCols(Out &o_, const DevSim &S, uint32_t seq_id, const WordColumn &seq_, uint32_t read_len_, bool reverse_, uint32_t q_)
        : o(o_), ref(S, seq_id), seq(seq_), read_len(read_len_), reverse(reverse_), q(q_) {}
    RSQ_HD void compare(uint32_t p, uint32_t n) {
        while (n) {
            const uint32_t room = 32u - (q & 3u), c = n < room ? n : room;
            const MdSeqChunk s = md_seq_chunk(seq, read_len, reverse, q);
            const uint64_t r = ref.codes(p), x = s.codes ^ r;
            uint64_t mm = ((x | (x >> 1)) & 0x5555555555555555ull) | s.n;
            if (c < 32u) mm &= (1ull << (2u * c)) - 1ull;
            uint32_t done = 0;
            while (mm) {                                                // (the rare step: one round a mismatch)
                const uint32_t i = lowest_set_bit64(mm) >> 1;
                o.element((char)md_ref_letter((uint32_t)(r >> (2u * i)) & 3u), run + i - done);
                md_note_mismatch(o, q + i, 0);
                md_note_base(o, p + i, (uint32_t)(s.n >> (2u * i)) & 1u, (uint32_t)(s.codes >> (2u * i)) & 3u, 0);
                run = 0;
                done = i + 1u;
                ++nm;
                mm &= mm - 1ull;
            }
            run += c - done;
            q += c;
            p += c;
            n -= c;
        }
    }
    RSQ_HD void deletion(uint32_t p, uint32_t n) {
        o.element('^', run);
        run = 0;
        nm += n;
        while (n) {
            const uint32_t c = n < 32u ? n : 32u;
            const uint64_t r = ref.codes(p);
            for (uint32_t i = 0; i < c; i += 4u) {
                const uint32_t b = (uint32_t)(r >> (2u * i)) & 0xFFu, left = c - i;
                o.bytes(base_letters((b & 3u) | ((b & 0xCu) << 6) | ((b & 0x30u) << 12) | ((b & 0xC0u) << 18)), left < 4u ? left : 4u);
            }
            p += c;
            n -= c;
        }
    }
    RSQ_HD void take(bool last) {
        if (!cn) return;
        md_note_run(o, cur == 1u && !(any && !last) ? 3u : cur, cp, cn, 0);
        if (cur == 0u) compare(cp, cn);
        else if (cur == 2u) {
            nm += cn;
            q += cn;
        } else if (any && !last) deletion(cp, cn);                      // (a D run at either end is no part of the alignment)
        if (cur != 1u) any = true;
        cn = 0;
    }
    RSQ_HD void col(uint32_t op, uint32_t count, uint32_t p) {
        if (op == cur && cn && (op == 2u || cp + cn == p)) {
            cn += count;
            return;
        }
        take(false);
        cur = op;
        cp = p;
        cn = count;
    }
    RSQ_HD void end() {
        take(true);
        o.num(run);
    }
};
struct MdCount {                                                        // the MD string's length
    uint32_t chars = 0;
    RSQ_HD void num(uint32_t v) { chars += digits_u32(v); }
    RSQ_HD void ch(char) { ++chars; }
    RSQ_HD void bytes(uint32_t, uint32_t count) { chars += count; }
    RSQ_HD void element(char, uint32_t v) { chars += digits_u32(v) + 1u; }
};

// the columns of a mate whose stretch no allele-map entry with a coordinate effect reaches (every mate of a reference without variants): the ops inside the
// dropped D runs, in read order or (reverse) from the last one down, as sam_cigar replays them; p: the reference position of the first, POS - 1
template <class V>
RSQ_HD void md_plain_columns(const WordColumn &ops, const ReadMeta &m, const SamMate &w, bool reverse, uint32_t p, V &v) {
    if (m.plain) {
        if (m.n_iter_m) v.col(0u, m.n_iter_m, p);
    } else {
        const uint32_t lo = w.lead, hi = (uint32_t)m.n_iter_m - w.trail;
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t it = reverse ? hi - 1u - (i - lo) : i;
            if ((reverse ? (it & 15u) == 15u && it >= lo + 15u : !(it & 15u) && it + 16u <= hi) && !ops.at(it >> 4)) {      // 16 plain iterations at once
                v.col(0u, 16u, p);
                p += 16u;
                i += 15u;
                continue;
            }
            const uint32_t c = sam_op_at(ops, it);
            v.col(c, 1u, p);
            p += c != 2u;
        }
    }
    v.end();
}

// NM and MD of a mapped mate: MD into o, returns NM.  w: the mate's walk; var: its variant entry (nullptr: a format without variants); a: its alignment
template <class Out>
RSQ_HD uint32_t md_walk(const DevSim &S, const Fragment &f, const ReadMeta &m, const WordColumn &seq, const WordColumn &ops, const SamMate &w, const SamVarMate *var, const SamAlign &a,
                        Out &o) {
    const bool reverse = a.reverse != 0u;
    MdCols<Out> v(o, S, f.seq, seq, m.read_len, reverse, reverse ? (uint32_t)m.read_len - w.q : 0u);      // (a reverse mate's SEQ begins with the clip)
    if (var && var->w.pad) {
        AlleleCursor c(allele_view(S, f.seq, f.allele), (int64_t)var->at, var->entry);
        sam_var_columns(ops, m, c, reverse, v);
    } else md_plain_columns(ops, m, w, reverse, a.pos - 1u, v);
    return v.nm;
}

// The format with the two tags behind Base's.  An entry is Base's and { NM, the MD string's length (0: unmapped, no tags) }, padded to 16 bytes; a Pair is
// aligned to 32 and a multiple of it -- 64 bytes over SamFormat and BamFormat, 96 over the two with variants: a row's two entries stay one aligned load.
template <class BaseMate>
struct alignas(16) MdMate {
    BaseMate b;
    uint32_t nm, md_chars;
};
template <class BaseMate>
struct alignas(32) MdPair {
    MdMate<BaseMate> mate[2];
};
template <class Base>
struct MdFormat {
    static constexpr bool kVariants = Base::kVariants, kMd = true, kBam = Base::kBam;
    using Mate = MdMate<typename Base::Mate>;
    using Pair = MdPair<typename Base::Mate>;
    static RSQ_HD const auto &walk(const Mate &e) { return Base::walk(e.b); }
    static RSQ_HD const auto &var(const Mate &e) { return Base::var(e.b); }
    static RSQ_HD uint32_t bytes(const Mate &e) { return Base::bytes(e.b); }
    // the tags' bytes: "\tNM:i:<n>\tMD:Z:<md>", or "NM" 'I' u32 "MD" 'Z' <md> NUL
    static RSQ_HD uint32_t tags_size(const Mate &e) { return !e.md_chars ? 0u : kBam ? 11u + e.md_chars : 12u + digits_u32(e.nm) + e.md_chars; }
    static RSQ_HD void measure(const DevSim &S, const Fragment &f, const ReadMeta &m, const WordColumn &seq, const WordColumn &ops, const SamMate &w, const SamVarMate *var,
                               const SamAlign &a, Mate &e) {
        e.nm = e.md_chars = 0;
        if (!a.mapped) return;
        MdCount count;
        e.nm = md_walk(S, f, m, seq, ops, w, var, a, count);
        e.md_chars = count.chars;
        Base::grow(e.b, tags_size(e));
    }
    template <class Sink>
    static RSQ_HD void tags(const DevSim &S, const Fragment &f, const ReadMeta &m, const WordColumn &seq, const WordColumn &ops, const SamMate &w, const SamVarMate *var, const Mate &e,
                            const SamAlign &a, Sink &t) {
        if (a.mapped) {
            if (kBam) {
                t.bytes(chars4('N', 'M', 'I'), 3u);
                t.bytes(e.nm, 4u);
                t.bytes(chars4('M', 'D', 'Z'), 3u);
            } else {
                t.str("\tNM:i:", 6);
                t.num(e.nm);
                t.str("\tMD:Z:", 6);
            }
            md_walk(S, f, m, seq, ops, w, var, a, t);
            if (kBam) t.ch(0);
        }
        if (!kBam) t.ch('\n');
    }

    // ---- over a format without variants
    static RSQ_HD Mate mate(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                            const WordColumn &ops, const SamMate &w, const SamAlign &a) {
        Mate e{};
        e.b = Base::mate(S, names, has_f, f, adapter_only_number, m, ops, w, a);
        measure(S, f, m, seq, ops, w, nullptr, a, e);
        return e;
    }
    template <class Sink>
    static RSQ_HD void head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                            const WordColumn &ops, const Mate &e, const SamAlign &a, Sink &t) {
        Base::head(S, names, has_f, f, adapter_only_number, m, seq, ops, e.b, a, t);
    }
    template <class Sink>
    static RSQ_HD void tail(const DevSim &S, const Fragment &f, const ReadMeta &m, const WordColumn &seq, const WordColumn &qual, const WordColumn &ops, const Mate &e, const SamAlign &a,
                            Sink &t) {
        Base::tail_open(S, m, qual, ops, a, t);
        tags(S, f, m, seq, ops, Base::walk(e.b), nullptr, e, a, t);
    }
    static RSQ_HD uint32_t tail_at(const Mate &e, const ReadMeta &m) { return Base::tail_at(e.b, m) - tags_size(e); }
    template <class P>
    static RSQ_HD uint32_t record(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                                  const WordColumn &qual, const WordColumn &ops, const Mate &e, const SamAlign &a, P dst) {
        WordSinkT<P> t(dst);
        head(S, names, has_f, f, adapter_only_number, m, seq, ops, e, a, t);
        tail(S, f, m, seq, qual, ops, e, a, t);
        t.finish();
        return t.n;
    }

    // ---- over a format of a reference with variants
    static RSQ_HD Mate mate(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m,
                            const WordColumn &seq, const WordColumn &ops, const SamVarMate &w, uint32_t n_cigar, const SamAlign &a) {
        Mate e{};
        e.b = Base::mate(S, names, has_f, f, id, adapter_only_number, m, ops, w, n_cigar, a);
        measure(S, f, m, seq, ops, w.w, &w, a, e);
        return e;
    }
    template <class Sink>
    static RSQ_HD void head(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &seq,
                            const WordColumn &ops, const Mate &e, const SamAlign &a, Sink &t) {
        Base::head(S, names, has_f, f, id, adapter_only_number, m, seq, ops, e.b, a, t);
    }
    template <class Sink>
    static RSQ_HD void tail(const DevSim &S, const Fragment &f, const ReadMeta &m, const SamVarId &id, const WordColumn &seq, const WordColumn &qual, const WordColumn &ops, const Mate &e,
                            const SamAlign &a, Sink &t) {
        Base::tail_open(S, m, id, qual, ops, a, t);
        const SamVarMate &v = Base::var(e.b);
        tags(S, f, m, seq, ops, v.w, &v, e, a, t);
    }
    static RSQ_HD uint32_t tail_at(const Mate &e, const ReadMeta &m, const SamVarId &id) { return Base::tail_at(e.b, m, id) - tags_size(e); }
    template <class P>
    static RSQ_HD uint32_t record(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, const SamVarId &id, uint64_t adapter_only_number, const ReadMeta &m,
                                  const WordColumn &seq, const WordColumn &qual, const WordColumn &ops, const Mate &e, const SamAlign &a, P dst) {
        WordSinkT<P> t(dst);
        head(S, names, has_f, f, id, adapter_only_number, m, seq, ops, e, a, t);
        tail(S, f, m, id, seq, qual, ops, e, a, t);
        t.finish();
        return t.n;
    }
};
using SamMdFormat = MdFormat<SamFormat>;
using BamMdFormat = MdFormat<BamFormat>;
using SamVarMdFormat = MdFormat<SamVarFormat>;
using BamVarMdFormat = MdFormat<BamVarFormat>;
static_assert(sizeof(SamMdFormat::Pair) == 64 && sizeof(BamMdFormat::Pair) == 64, "two mates are one aligned 64-byte load");
static_assert(sizeof(SamVarMdFormat::Pair) == 96 && sizeof(BamVarMdFormat::Pair) == 96, "two mates are one aligned 96-byte load");

}  // namespace rsq
