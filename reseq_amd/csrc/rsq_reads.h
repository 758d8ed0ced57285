// rsq_reads.h -- the read kernels (Simulator.cpp:454-594, a2/a3), one lane per read, persistent waves:
//   k_fill_reads     both mates of the pairs of a batch of fragments (or of adapter-only pairs)
//   k_fill_records   the reads of seqToIllumina records
// and what they are made of: where a read goes, the sources of its template (reference, bisulfite conversion, variants, records), the LDS image of the
// tables, the loop of a wave.  The library instantiates both for every row width of the image; for a loaded profile the two bodies are compiled again
// at run time with the profile's geometry as literals (rsq_spec.h).  This file and what it includes are the text of that compilation and of its cache
// key (Makefile: EMBED): a kernel that only the library launches belongs in rsq_format.h or with its own stage.
// All arithmetic lives in rsq_core.h; this file only maps work to lanes and moves bytes.
#pragma once
#include "rsq_core.h"
#include "rsq_variants.h"
#include "rsq_text.h"

namespace rsq {

// ------------------------------------------------------------------------------------------------- reads
struct ReadOut {                        // destination of one lane's read; bases and qualities leave in 4-byte stores
    WordColumn seq, qual, ops;
    uint32_t cur_word, cur_index;       // CIGAR ops: 2 bits per iteration, 16 per word
    uint32_t seq_word, qual_word, n_put;
    RSQ_HD void put(uint32_t pos, uint32_t base, uint32_t qual_char) {      // pos runs 0,1,2,... (read_pos)
        const uint32_t sh = (pos & 3u) * 8u;
        seq_word |= base << sh;
        qual_word |= qual_char << sh;
        n_put = pos + 1u;
        if ((pos & 3u) == 3u) {
            seq.at(pos >> 2) = seq_word;
            qual.at(pos >> 2) = qual_word;
            seq_word = qual_word = 0;
        }
    }
    RSQ_HD void op(uint32_t it, uint32_t code) {
        const uint32_t wi = it >> 4;
        if (wi != cur_index) {
            ops.at(cur_index) = cur_word;
            cur_word = 0;
            cur_index = wi;
        }
        cur_word |= code << ((it & 15u) * 2u);
    }
    RSQ_HD void finish() {
        ops.at(cur_index) = cur_word;
        if (n_put & 3u) {
            seq.at(n_put >> 2) = seq_word;
            qual.at(n_put >> 2) = qual_word;
        }
    }
    RSQ_HD void finish(uint32_t, uint32_t) { finish(); }      // WaveReadOut is told what this one counts itself
};
RSQ_HD ReadOut make_read_out(const WordColumn &seq, const WordColumn &qual, const WordColumn &ops) { return ReadOut{seq, qual, ops, 0u, 0u, 0u, 0u, 0u}; }

// The same destination for the wave kernels, without a 64-bit address per lane and array.  The three arrays are the kernel's argument (wave-uniform: scalar
// registers) and share one pitch; the lane keeps its row, and a store forms ONE 32-bit byte offset from word and row (global_store_dword v_off, v_data,
// s[base:base+1], as PoolRow32 loads).  A call's arrays can span 4 GB or more (38 words x pitch x 4 B): the host says so per call (RawLayout::wide) and the
// store then forms the 64-bit address as WordColumn does -- a wave-uniform branch at the store, which a lane reaches once in four steps; the state
// carried through the steps is the same either way.  [The alternative, the chunk's first row in the scalar base, shortens only the row's share of the
// offset: the word's share, w * pitch * 4, passes 2^32 all the same, and the rows of a chunk of records are not neighbours.]
// Words are stored as ReadOut stores them: a seq / qual word when its fourth base arrives, an ops word when the first iteration of the next one
// arrives; the rest in finish().  The positions come 0, 1, 2, ... and the iterations with an op 0, 1, 2, ... up to the tail, so "which word" is the
// counter's high bits and needs no register of its own.
RSQ_HD constexpr uint32_t read_out_offset(uint32_t w, uint32_t pitch, uint32_t row) { return (w * pitch + row) * 4u; }      // bytes; exact while words * pitch * 4 <= 2^32
RSQ_HD constexpr bool read_out_is_wide(uint64_t words, uint64_t pitch) { return words * pitch * 4u > 0x100000000ull; }      // words: of the longest array; pitch below 2^32 (raw_layout refuses more)
struct WaveReadOut {
    uint32_t *seq, *qual, *ops;         // wave-uniform
    uint32_t pitch;                     // wave-uniform
    bool wide;                          // wave-uniform
    uint32_t row;                       // the lane's row
    uint32_t cur_word, seq_word, qual_word;
    RSQ_HD uint32_t *at(uint32_t *base, uint32_t w) const {      // word w of the lane's row of array `base`
        if (wide) {
            uint32_t r = row;
            RSQ_KEEP_IN_VGPR(r);             // or the compiler carries base + row, a 64-bit address per array, through the steps for this branch
            return base + ((uint64_t)w * pitch + r);
        }
        return reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(base) + read_out_offset(w, pitch, row));
    }
    RSQ_HD void store(uint32_t *base, uint32_t w, uint32_t v) const { *at(base, w) = v; }
    RSQ_HD void put(uint32_t pos, uint32_t base, uint32_t qual_char) {
        const uint32_t sh = (pos & 3u) * 8u;
        seq_word |= base << sh;
        qual_word |= qual_char << sh;
        if ((pos & 3u) == 3u) {
            store(seq, pos >> 2, seq_word);
            store(qual, pos >> 2, qual_word);
            seq_word = qual_word = 0;
        }
    }
    RSQ_HD void op(uint32_t it, uint32_t code) {
        if (!(it & 15u) && it) {
            store(ops, (it >> 4) - 1u, cur_word);
            cur_word = 0;
        }
        cur_word |= code << ((it & 15u) * 2u);
    }
    // n_put: bases put (the read's length so far), n_ops: iterations that had an op
    RSQ_HD void finish(uint32_t n_put, uint32_t n_ops) {
        store(ops, n_ops ? (n_ops - 1u) >> 4 : 0u, cur_word);
        if (n_put & 3u) {
            store(seq, n_put >> 2, seq_word);
            store(qual, n_put >> 2, qual_word);
        }
    }
};

struct RawLayout {                      // word-major arrays of the read kernel, read index = segment * n_pairs + pair
    uint32_t *seq, *qual;               // [read_words][pitch]: 4 bases / 4 quality characters per word
    uint32_t *ops;                      // [ops_words][pitch]: 16 two-bit CIGAR ops per word
    ReadMeta *meta;
    uint64_t pitch;                     // reads per word row (>= number of reads)
    uint64_t *templates;                // --methylation: [reads][template_words] converted templates, else nullptr
    uint32_t template_words;
    uint32_t wide;                      // read_out_is_wide of the arrays: a byte offset into them needs more than 32 bits (WaveReadOut)
    const uint32_t *order;              // seqToIllumina, after a read kernel that ran binned by tile: row r holds record order[r]; nullptr: record r
    RSQ_HD uint64_t item_of(uint64_t row) const { return order ? order[row] : row; }
    RSQ_HD WordColumn seq_of(uint64_t r) const { return WordColumn{seq + r, pitch}; }
    RSQ_HD WordColumn qual_of(uint64_t r) const { return WordColumn{qual + r, pitch}; }
    RSQ_HD WordColumn ops_of(uint64_t r) const { return WordColumn{ops + r, pitch}; }
    RSQ_HD ReadOut out_of(uint64_t r) const { return make_read_out(seq_of(r), qual_of(r), ops_of(r)); }
    RSQ_HD WaveReadOut wave_out_of(uint64_t r) const { return WaveReadOut{seq, qual, ops, (uint32_t)pitch, wide != 0u, (uint32_t)r, 0u, 0u, 0u}; }
};

struct FragmentSrc {                    // template of one mate cut from the 2-bit reference (Reference.cpp:483-496)
    const uint64_t *words;
    uint64_t word_off;
    uint32_t first;                     // forward: start position; reverse: end position
    uint32_t len;
    bool reverse;
    const uint16_t *sys_;               // systematic errors at the first template base
    const uint64_t *converted;          // --methylation: the template after CTConversion, 2 bits per base in read orientation; else nullptr
    const uint32_t *gc_prefix;          // DevSim::gc_prefix
    // Per-lane streams: a load instruction of the wave touches 64 cache lines here, so the source holds what it last read -- the 64-bit word of the
    // template (32 bases; of the reference or of the converted template, a source reads only one of them) and a group of four systematic errors
    // (the tracks end in 8 spare entries, pack_reference).
    mutable uint32_t held_word = 0xFFFFFFFFu, held_sys = 0xFFFFFFFFu;
    mutable uint64_t word = 0, sys4 = 0;
    RSQ_HD uint64_t template_word(const uint64_t *from, uint32_t index) const {
        if (index != held_word) {
            held_word = index;
            word = from[index];
        }
        return word;
    }
    RSQ_HD uint32_t org_len() const { return len; }
    RSQ_HD uint32_t ref(uint32_t k) const {
        const uint32_t pos = reverse ? first - 1u - k : first + k, b = (uint32_t)(template_word(words + word_off, pos >> 5) >> ((pos & 31u) * 2u)) & 3u;
        return reverse ? 3u - b : b;
    }
    RSQ_HD uint32_t base(uint32_t k) const { return converted ? (uint32_t)(template_word(converted, k >> 5) >> ((k & 31u) * 2u)) & 3u : ref(k); }
    RSQ_HD uint32_t sys_base(uint32_t k) const {
        if ((k >> 2) != held_sys) {
            held_sys = k >> 2;
            sys4 = load_as<uint64_t, 2>(sys_ + (k & ~3u));
        }
        return (uint32_t)(sys4 >> ((k & 3u) * 16u)) & 0xFFFFu;
    }
    RSQ_HD uint32_t sys_deleted(uint32_t k) const { return sys_base(k); }
    // Simulator.cpp:482-489 without a load per base: the G/C count of the template's reference range from the per-word prefix sums
    // (the complement strand has the same count), the error rates four per 8-byte load
    RSQ_HD void totals(uint32_t n, uint32_t &gc, uint32_t &rate_sum) const {
        if (!converted && !gc_prefix) return template_totals_loop(*this, n, gc, rate_sum);
        if (converted) gc += ref_gc_count(converted, 0, 0, n);                  // the converted template is packed like the reference, from base 0
        else gc += reverse ? ref_gc_count_prefix(words, gc_prefix, word_off, first - n, first) : ref_gc_count_prefix(words, gc_prefix, word_off, first, first + n);
        rate_sum += rate_total(n);
    }
    // eight entries per 16-byte load (the tracks end in 8 spare entries); the rate is an entry's high byte
    RSQ_HD uint32_t rate_total(uint32_t n) const {
        struct __attribute__((packed, aligned(2))) Eight {
            uint64_t a, b;
        };
        uint32_t sum = 0;
        for (uint32_t k = 0; k < n; k += 8u) {
            Eight e = load_as<Eight, 2>(sys_ + k);
            const uint32_t left = n - k;                               // entries of this group that count
            if (left < 8u) {
                if (left <= 4u) {
                    e.b = 0;
                    if (left < 4u) e.a &= (1ull << (16u * left)) - 1ull;
                } else e.b &= (1ull << (16u * (left - 4u))) - 1ull;
            }
            const uint64_t kHigh = 0x00FF00FF00FF00FFull, kAdd = 0x0001000100010001ull;
            sum += (uint32_t)((((e.a >> 8) & kHigh) * kAdd) >> 48) + (uint32_t)((((e.b >> 8) & kHigh) * kAdd) >> 48);
        }
        return sum;
    }
};

// What the STEPS of a wave kernel need of a FragmentSrc (init() takes the whole one: its totals want gc_prefix and both forms of the template).  The arrays --
// the 2-bit reference or the converted templates, the two error tracks -- are wave-uniform and stay in scalar registers; the lane keeps ELEMENT indices of
// its first template word and its first error entry and forms the address at the load, once in 32 steps (template) and once in four (errors).  An index is
// 32 bits and a few high bits: a human-sized error track has more than 2^31 entries (above 4 GB in bytes), a larger reference more than 2^32; the high bits
// share one register with the two flags (WaveSrcBits), so the state is four registers and what the source last read.
namespace WaveSrcBits {
constexpr uint32_t kBackward = 1u, kRevStrand = 2u;      // the template is read downwards and complemented; the errors are the reverse strand's
constexpr uint32_t kWordHighShift = 8u, kWordHighBits = 8u, kSysHighShift = 16u, kSysHighBits = 16u;
RSQ_HD constexpr uint32_t pack(bool backward, bool rev_strand, uint64_t word0, uint64_t sys0) {
    return (backward ? kBackward : 0u) | (rev_strand ? kRevStrand : 0u) | ((uint32_t)(word0 >> 32) << kWordHighShift) | ((uint32_t)(sys0 >> 32) << kSysHighShift);
}
RSQ_HD constexpr uint64_t word_index(uint32_t bits, uint32_t word0, uint32_t index) { return (((uint64_t)((bits >> kWordHighShift) & ((1u << kWordHighBits) - 1u)) << 32) | word0) + index; }
RSQ_HD constexpr uint64_t sys_index(uint32_t bits, uint32_t sys0, uint32_t k) { return (((uint64_t)(bits >> kSysHighShift) << 32) | sys0) + k; }
}  // namespace WaveSrcBits
struct WaveFragmentSrc {
    const uint64_t *words;              // wave-uniform: the 2-bit reference (with the alleles' copies behind it), or the converted templates
    const uint16_t *sys_fwd, *sys_rev;  // wave-uniform
    uint32_t word0;                     // the word of `words` that holds template position 0 of the lane's sequence (or template): low 32 bits
    uint32_t first;                     // as FragmentSrc::first; 0 in a converted template
    uint32_t sys0;                      // the entry of the strand's track at the first template base: low 32 bits
    uint32_t bits;                      // WaveSrcBits
    mutable uint32_t held_word = 0xFFFFFFFFu, held_sys = 0xFFFFFFFFu;
    mutable uint64_t word = 0, sys4 = 0;
    RSQ_HD const uint64_t *word_at(uint32_t index) const { return words + WaveSrcBits::word_index(bits, word0, index); }      // word `index` of the lane's sequence (or template)
    RSQ_HD const uint16_t *sys_at(uint32_t k) const { return ((bits & WaveSrcBits::kRevStrand) ? sys_rev : sys_fwd) + WaveSrcBits::sys_index(bits, sys0, k); }
    RSQ_HD uint32_t base(uint32_t k) const {
        const bool backward = bits & WaveSrcBits::kBackward;
        const uint32_t pos = backward ? first - 1u - k : first + k, index = pos >> 5;
        if (index != held_word) {
            held_word = index;
            word = *word_at(index);
        }
        const uint32_t b = (uint32_t)(word >> ((pos & 31u) * 2u)) & 3u;
        return backward ? 3u - b : b;
    }
    RSQ_HD uint32_t sys_base(uint32_t k) const {
        if ((k >> 2) != held_sys) {
            held_sys = k >> 2;
            sys4 = load_as<uint64_t, 2>(sys_at(k & ~3u));
        }
        return (uint32_t)(sys4 >> ((k & 3u) * 16u)) & 0xFFFFu;
    }
    RSQ_HD uint32_t sys_deleted(uint32_t k) const { return sys_base(k); }
};
// of a FragmentSrc whose template is `converted_word0` words into `templates` (src.converted set) or the reference's own (templates == nullptr)
RSQ_HD WaveFragmentSrc wave_fragment_src(const DevSim &S, const FragmentSrc &src, const uint64_t *templates, uint64_t converted_word0) {
    const uint64_t word0 = templates ? converted_word0 : (uint64_t)(src.words - S.ref_words) + src.word_off, sys0 = (uint64_t)(src.sys_ - (src.reverse ? S.sys_rev : S.sys_fwd));
    return WaveFragmentSrc{templates ? templates : S.ref_words, S.sys_fwd, S.sys_rev, (uint32_t)word0, templates ? 0u : src.first, (uint32_t)sys0, WaveSrcBits::pack(!templates && src.reverse, src.reverse, word0, sys0)};
}

// ------------------------------------------------------------------------------------- bisulfite conversion (a16)
// Simulator::CTConversion (Simulator.cpp:1925-2247): a C of a template becomes a T with probability 1 - methylation where the template lies in an
// unmethylated region of the BED file; once per (start, length, strand) site and mate, so that all duplicates of a site share the converted template.
// The uniform of template position k is word k&3 of Philox block (start, sequence, length, 7<<28 | reversed<<27 | k>>2) -- a pure function of k, so
// the walk below may visit positions in any grouping.
//
// The reference walks template and reference base by base, in three overloads times two mirrored directions.  Here ONE walk serves both strands and
// both cases (with and without variants): positions are taken in the strand's own direction (MethSide: x = pos on the forward strand, -pos on the
// reverse strand, so regions and variants are met in increasing x either way), and the walk advances by EVENTS -- a region's entry and exit, the
// variant the cursor points at, the template's end -- converting whole runs of template positions at once (the C's of a run are found 32 bases per
// word).  What the reference's walk does beyond the plain geometry is kept, because it decides bytes of the output (DESIGN.md section 1 lists it):
//   * the template position is 16 bits wide (uintReadLen): a jump over more than 65535 bases wraps, and the walk goes on if the wrapped value is
//     below the template length;
//   * the reverse mate's walk begins at the fragment's end position (one past its last base), not at the last base;
//   * without variants the reverse walk never enters the sequence's first region (`while(cur_meth && ...)`); with variants it does;
//   * a deleted base inside a region takes a template position (without converting it);
//   * only the variant under the cursor is looked at: variants of other alleles at a position are passed over when the walk stands on them, but a
//     second variant at the position of one that was just used stays under the cursor and hides all later ones until the next stretch without regions;
//   * the reference reads its `deletion` flag before writing it (Simulator.cpp:2026): here it starts as false.
struct MethView {
    const uint32_t *first, *second;
    const double *rate;                 // of the allele asked for: rate[region * stride]
    uint32_t n, stride;
    RSQ_HD double rate_of(int32_t region) const { return rate[(size_t)region * stride]; }
};
// Reference::Unmethylation(seq, allele): meth_rate holds num_alleles values per region (a file with one column repeats it)
RSQ_HD MethView meth_view(const DevSim &S, uint32_t seq, uint32_t allele = 0) {
    const uint32_t off = S.meth_ptr[seq];
    return MethView{S.meth_first + off, S.meth_second + off, S.meth_rate + (size_t)off * S.num_alleles + allele, S.meth_ptr[seq + 1] - off, S.num_alleles};
}
// cur_methylation_start of SimulateFromGivenBlock (:2273,:2293-2297, CreateBlock :1214-1219): the first region that ends after pos
RSQ_HD uint32_t meth_start_index(const MethView &m, uint32_t pos) {
    uint32_t lo = 0, hi = m.n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (m.second[mid] <= pos) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
constexpr uint32_t kTemplateWordsMax = 64;      // 2048 template bases
struct MethDraws {                      // lazily evaluated Philox blocks of one template
    uint64_t seed;
    uint32_t c0, c1, c2, c3base, have;
    Words w;
    RSQ_HD double uniform(uint32_t k) {
        if (have != (k >> 2)) {
            w = philox(seed, c0, c1, c2, c3base | (k >> 2));
            have = k >> 2;
        }
        const uint32_t j = k & 3u;
        return u32_to_unit(j == 0u ? w.w0 : (j == 1u ? w.w1 : (j == 2u ? w.w2 : w.w3)));
    }
};
// template positions [t, t + n) lie in a region with conversion probability `rate`: the C's among them (code 1: low bit set, high bit clear), word by word
RSQ_HD void ct_convert_run(uint64_t *tmpl, uint32_t t, uint32_t n, double rate, MethDraws &d) {
    const uint32_t end = t + n;
    for (uint32_t w = t >> 5; (w << 5) < end; ++w) {
        const uint32_t lo = t > (w << 5) ? t - (w << 5) : 0u, hi = end - (w << 5) < 32u ? end - (w << 5) : 32u;      // bases lo .. hi-1 of the word
        uint64_t cs = tmpl[w] & ~(tmpl[w] >> 1) & 0x5555555555555555ull;
        cs &= (hi == 32u ? ~0ull : (1ull << (2u * hi)) - 1ull) & ~((1ull << (2u * lo)) - 1ull);
        while (cs) {
            const uint32_t bit = lowest_set_bit64(cs);
            cs &= cs - 1ull;
            if (d.uniform((w << 5) + (bit >> 1)) < rate) tmpl[w] |= (uint64_t)3u << bit;                             // C (1) -> T (3)
        }
    }
}
// regions and variants as the walk of one strand meets them
template <bool REV>
struct MethSide {
    const MethView &m;
    const VarView *r;                   // nullptr: no variants loaded
    uint32_t allele;
    int32_t lowest;                     // the reverse walk's last region: 1 without variants, 0 with
    RSQ_HD int64_t coord(uint32_t pos) const { return REV ? -(int64_t)pos : (int64_t)pos; }
    RSQ_HD int64_t entry(int32_t i) const { return REV ? 1 - (int64_t)m.second[i] : (int64_t)m.first[i]; }      // the first x inside the region
    RSQ_HD int64_t exit(int32_t i) const { return REV ? 1 - (int64_t)m.first[i] : (int64_t)m.second[i]; }       // the first x behind it
    RSQ_HD bool region(int32_t i) const { return REV ? i >= lowest : i < (int32_t)m.n; }
    RSQ_HD bool variant(int32_t j) const { return r && (REV ? j >= 0 : j < (int32_t)r->n); }
    RSQ_HD static int32_t next(int32_t i) { return REV ? i - 1 : i + 1; }
    RSQ_HD int64_t at(int32_t j) const { return coord(r->v[j].pos); }
    RSQ_HD uint32_t len(int32_t j) const { return r->v[j].len; }
    RSQ_HD bool mine(int32_t j) const { return r->in_allele(r->v[j], allele); }
    // the region the walk begins in or in front of: forward the first that ends behind the position, reverse the last that begins at or before it
    RSQ_HD int32_t first_region(uint32_t pos) const {
        if (!REV) return (int32_t)meth_start_index(m, pos);
        uint32_t lo = 0, hi = m.n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (m.first[mid] <= pos) lo = mid + 1;
            else hi = mid;
        }
        return (int32_t)lo - 1;
    }
};
template <bool REV>
RSQ_HD void methylation_walk(uint64_t *tmpl, uint32_t length, const MethView &m, const VarView *r, uint32_t allele, uint32_t start_pos, VarStart from, MethDraws &d) {
    const MethSide<REV> side{m, r, allele, r ? 0 : 1};
    int64_t x = side.coord(start_pos);
    uint16_t t = 0;                                                   // uintReadLen
    int32_t region = side.first_region(start_pos), var = r ? from.first_variant_id : -1;
    uint32_t left = 0;                                                // bases of the variant at x the walk has not passed yet
    if (side.variant(var) && side.at(var) == x && side.len(var) > 1u && side.mine(var)) left = side.len(var) - from.start_variant_pos;
    // the stretch without information in front of `region`: the template position moves on by what the allele holds there
    auto skip_to = [&](int32_t reg) {
        if (left) {
            t = (uint16_t)(t + left);
            left = 0;
            ++x;
            var = side.next(var);
        }
        while (side.variant(var) && side.at(var) < side.entry(reg) && t < length) {
            if (side.mine(var)) {
                t = (uint16_t)(t + (uint16_t)(side.at(var) - x) + (uint16_t)side.len(var));
                x = side.at(var) + 1;
            }
            var = side.next(var);
        }
        t = (uint16_t)(t + (uint16_t)(side.entry(reg) - x));
        x = side.entry(reg);
    };
    if (side.region(region) && side.entry(region) > x) skip_to(region);
    while (side.region(region) && t < length) {
        const double rate = m.rate_of(region);
        const int64_t out = side.exit(region);
        while (x < out && t < length) {
            if (!left) {                                              // does a variant of the allele begin here?
                while (side.variant(var) && side.at(var) == x && !side.mine(var)) var = side.next(var);
                if (side.variant(var) && side.at(var) == x) {
                    if (0u == side.len(var)) {                        // the deleted base: a template position passes unconverted
                        var = side.next(var);
                        ++x;
                        ++t;
                        continue;
                    }
                    left = side.len(var);
                }
            }
            uint32_t run;
            if (left) {                                               // the variant's bases, all at this x
                run = left < length - t ? left : length - t;
                left -= run;
                if (!left) {
                    var = side.next(var);
                    ++x;
                }
            } else {                                                  // reference bases up to the region's end or the variant under the cursor
                int64_t until = out;
                if (side.variant(var) && side.at(var) > x && side.at(var) < until) until = side.at(var);
                run = until - x < (int64_t)(length - t) ? (uint32_t)(until - x) : length - t;
                x += run;
            }
            ct_convert_run(tmpl, t, run, rate, d);
            t = (uint16_t)(t + run);
        }
        region = side.next(region);
        if (side.region(region) && side.entry(region) > x) skip_to(region);
    }
}
// CTConversion of one mate's template: `start_pos` = the fragment's start (forward mate) or END position (reverse mate), `r` = the sequence's variants or nullptr
RSQ_HD void ct_conversion(uint64_t *tmpl, uint32_t length, const MethView &m, const VarView *r, uint32_t allele, uint32_t start_pos, bool reversed, VarStart from, MethDraws &d) {
    if (reversed) methylation_walk<true>(tmpl, length, m, r, allele, start_pos, from, d);
    else methylation_walk<false>(tmpl, length, m, r, allele, start_pos, from, d);
}

struct EmptySrc {                       // adapter-only pair: org_seq_ = "" (Simulator.cpp:2369-2371)
    RSQ_HD void totals(uint32_t, uint32_t &, uint32_t &) const {}
    RSQ_HD uint32_t org_len() const { return 0; }
    RSQ_HD uint32_t base(uint32_t) const { return 0; }
    RSQ_HD uint32_t sys_base(uint32_t) const { return 0; }
    RSQ_HD uint32_t sys_deleted(uint32_t) const { return 0; }
};

RSQ_HD uint32_t draw_tile(const DevSim &S, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3base) {      // Simulator.h:176-181
    if (RSQ_SIM(S, n_tiles) > 1) return discrete_draw(S.tile_cp, RSQ_SIM(S, n_tiles), u32_to_unit(philox(S.seed, c0, c1, c2, c3base).w0));
    return 0;
}

// ------------------------------------------------------------------------------------------- LDS staging
// A lane evaluates about 250 table entries per base (quality K = 40 over four margins, base call and indel over four and three).
// Measured on gfx950 (exp/ta_bench.hip): a wave-level global_load_dwordx4 costs the CU's vector-memory path >= 23 cycles (64 lanes
// x 16 B returned at 64 B/clk) however few lanes are active, and about 2.3 cycles per distinct cache line touched; a ds_read_b128
// costs 8.  So the read kernel draws SCREENED (rsq_core.h): single-precision copies of the tables, four columns per 16-byte load,
// and the rows whose addresses scatter most across the lanes of a wave live in the workgroup's LDS image (LdsPlan, rsq_types.h):
//  * rows chosen by per-read state -- quality margins over sequence quality (0) and previous quality (1), base-call margins over
//    the quality (0) and the number of errors (2), indel margin over the indel position (0);
//  * the first rows of the error-rate margins (88 % of all positions have rate 0).  A lane whose rate is not staged reads its
//    own row from HBM (MixedRow32, rsq_core.h).
// The rows over the read position and the read's G/C percent stay in HBM (L2): the lanes of a wave share the position rows (4
// cache lines per load).  A draw the screen cannot decide is repeated in double precision from HBM (GlobalTables).
// Image layout (32-bit words), Ti = LdsPlan::img_tiles: descriptors [quality 4 Ti][base_call 20 Ti][indels 12][seq_quality Ti] (18 words
// each), the outcome values of these tables, the outcome values by column and the staged margins of the three families (FamilyGeo), error-rate rows at q3_off / b3_off.
// An image serves the reads of one template segment and of tiles first_tile .. first_tile + Ti - 1 (Ti = n_tiles: all tiles; Ti = 1: the reads
// are binned by tile and a workgroup stages the image of the bin it serves, fill_binned_loop); it is identified by the index of its first
// quality table, qbase = (segment * n_tiles + first_tile) * 4.  Descriptors in the image have par0_off relative to the image's outcome values.
RSQ_HD uint32_t lds_desc_count(uint32_t n_tiles) { return 25u * n_tiles + 12u; }
RSQ_HD uint32_t image_qbase(const DevSim &S, uint32_t seg, uint32_t first_tile) { return (seg * RSQ_SIM(S, n_tiles) + first_tile) * 4u; }
constexpr uint32_t kDescWords = sizeof(DevTable) / 4u;

// the host emulation counts what the screen decided (tests/hostemu): [family][0 = draws, 1 = left to double precision]
#if defined(RSQ_SCREEN_STATS) && !RSQ_ON_DEVICE
#define RSQ_SCREEN_COUNT(family, decided) (++RSQ_SCREEN_STATS[family][0], RSQ_SCREEN_STATS[family][1] += !(decided))
#else
#define RSQ_SCREEN_COUNT(family, decided) ((void)0)
#endif

// A draw the screen left open, as a call: the double-precision recipe (draw_slim) is rare and large, and inlined at every draw site it costs the read
// kernel's loop registers and a tenth of its time.  The callee reads the descriptor from the image again; the result carries prob_sum == 0 in bit 31.
template <int NM>
RSQ_NOINLINE uint32_t exact_draw_call(const double *pool, const RSQ_LDS float *img, uint32_t par0_words, uint32_t desc, uint32_t i0, uint32_t i1, uint32_t i2, uint32_t i3, uint32_t word) {
    const DevTable t = reinterpret_cast<const RSQ_LDS DevTable *>(img)[desc];
    uint32_t idx[NM];
    idx[0] = i0;
    idx[1] = i1;
    idx[2] = i2;
    if constexpr (NM == 4) idx[3] = i3;
    double ps;
    const uint32_t value = draw_slim<NM>(t, pool, reinterpret_cast<const RSQ_LDS uint8_t *>(img + par0_words), idx, u32_to_unit(word), ps);
    return value | (0.0 == ps ? 0x80000000u : 0u);
}

// row of margin n for value v: AdjustIndeces over the family's common range
#define RSQ_GEO_ROW(S, fam, n, v) ((uint32_t)clamp_from_zero((int32_t)(v) - (int32_t)RSQ_PLAN(S, fam.from[n]), (int32_t)RSQ_PLAN(S, fam.last[n])))

// the trial program of tests/hostemu counts the base calls the random word alone decided
#if defined(RSQ_WORD_SCREEN_STATS) && !RSQ_ON_DEVICE
#define RSQ_WORD_SCREEN_COUNT(sure) RSQ_WORD_SCREEN_STATS(sure)
#else
#define RSQ_WORD_SCREEN_COUNT(sure) ((void)0)
#endif

// A base call decided by the random word alone.  a, p, e, r: the lane's four pairs of scalars (rsq_pack.h base_call_word_bounds: x = columns below the template
// base's column z, y = columns above it), each at least (1 + 2^-21) times the largest ratio it stands for, so that b = the single-precision product of the four x
// (three roundings of 2^-24) is at least the sum of the lower columns' products over p_z, and likewise g for the columns above.  With u = word * 2^-32 column z is
// certain when u (1 + b) <= 1 - 1e-9 and (1 - u) (1 + g) <= 1 - 1e-9 g (pack_tables, "Draws decided by the random word alone").  In single precision:
//  * uf = u (1 + d), |d| <= 2^-24; t = fma(uf, b, uf) >= uf (1 + b) (1 - 2^-24), so t < 1 - 2^-20 gives u (1 + b) < (1 - 2^-20) (1 + 2^-24)^2 < 1 - 2^-21;
//  * 1 - uf is off by at most 2^-23 from 1 - u, absolutely, so with g < 512 and s = fma(1 - uf, g, 1 - uf) < 1 - 2^-13:
//    (1 - u) (1 + g) < s (1 + 2^-23) + 513 * 2^-23 < 1 - 2^-14 + 2^-23 <= 1 - 1e-9 g.  (A lane with g of 512 and more could be sure for one word in 513.)
// `sides` (LdsPlan::bw_sides): bit 0 = some table has a column below z, bit 1 = above; a side no table has is not checked (P0: the template base is column 0).
// An infinite scalar ("this row has no bound") makes t or s infinite or NaN: every compare is written so that NaN is "not sure".
RSQ_HD bool word_screen_sure(const Float2 &a, const Float2 &p, const Float2 &e, const Float2 &r, uint32_t word, uint32_t sides) {
    const Float2 f = ((a * p) * e) * r;
    const float uf = (float)word * 2.3283064365386963e-10f;
    bool sure = true;
    if (sides & 1u) sure = fma1(uf, f.x, uf) < 0.99999904632568359375f;   // 1 - 2^-20
    if (sides & 2u) {
        const float om = 1.f - uf;
        sure = sure && f.y < 512.f && fma1(om, f.y, om) < 0.9998779296875f;      // 1 - 2^-13
    }
    return sure;
}

// QQ = quads per row of the quality family (LdsPlan::quads_q).  `t` is the step the wave is in: the quality rows over the read
// positions t, ... t-kRingLag are in the wave's ring (lds_ring_load / lds_ring_store).  Rows are found from (table, value) by the families' common
// geometry; a table's descriptor is read only on the double-precision route and for the rare fallbacks of FillReadPart.
// QB = quads per batch of the quality draw (draw_screened_batched): its QQ quads are QQ / QB dependent round trips to LDS in every step.  RSQ_SCREEN_BATCH unless
// the kernel asks for more (the kernel of the plain pairs: kQualityBatchPairs); the draws of short rows take RSQ_SCREEN_BATCH through draw_screened.
// KEYS: from which Philox round on the step's draw forms its round keys at their use (philox, rsq_core.h); kKeysAhead unless the kernel asks (the pairs' read
// kernels: kKeysFromStep).
template <uint32_t MASK, int QB = RSQ_SCREEN_BATCH, int KEYS = kKeysAhead>
struct ScreenTables {
    using Sum = uint32_t;              // 0: prob_sum is 0, else 1 (all the callers ask; a double here costs the loop moves and 64-bit compares)
    static constexpr int kKeysFrom = KEYS;
    static constexpr int QQ = (int)MASK;
    const DevSim &S;
    const RSQ_LDS float *img;          // image of the workgroup
    uint32_t qbase;                    // index of the image's first quality table (image_qbase)
    const RSQ_LDS float *ring_;        // the wave's ring
    uint32_t t;
    uint32_t demand = 0xFFFFFFFFu;     // the read position whose rows the wave staged in the slot behind the ring at this step (a read that lags by more than kRingLag), or none
    RSQ_HD DevTable desc(uint32_t local) const { return reinterpret_cast<const RSQ_LDS DevTable *>(img)[local]; }
    RSQ_HD uint32_t par0_at() const { return RSQ_PLAN(S, desc_words) - RSQ_PLAN(S, par0_words); }
    RSQ_HD DevTable quality(uint32_t i) const { return desc(i - qbase); }
    RSQ_HD DevTable seq_quality(uint32_t i) const { return desc(24u * RSQ_PLAN(S, img_tiles) + 12u + i - qbase / 4u); }
    // the ring's rows of read position p; in_ring: p is one of the last steps' positions (a read lags by its deletions)
    RSQ_HD const RSQ_LDS float *ring(uint32_t p) const { return ring_ + (p % kRingSlots) * RSQ_PLAN(S, ring_stride); }
    RSQ_HD bool in_ring(uint32_t p) const { return t - p <= kRingLag; }
    // a draw the screen left open (or a table outside its preconditions): the reference's recipe in double precision
    template <int NM>
    RSQ_HD uint32_t exact(uint32_t desc, const uint32_t (&idx)[NM], uint32_t word, uint32_t &ps) const {
        const uint32_t r = exact_draw_call<NM>(S.pool, img, par0_at(), desc, idx[0], idx[1], idx[2], NM == 4 ? idx[NM - 1] : 0u, word);
        ps = (r >> 31) ^ 1u;                                  // the callers only ask whether prob_sum is 0
        return r & 0x7FFFFFFFu;
    }
    // `values`: FamilyGeo::values of the family, `column` = table of the image * slot + column
    template <int NM>
    RSQ_HD uint32_t settle(bool decided, uint32_t values, uint32_t column, uint32_t desc, const uint32_t (&idx)[NM], uint32_t u, uint32_t &ps) const {
        uint32_t value = reinterpret_cast<const RSQ_LDS uint8_t *>(img)[values + column];
        ps = 1u;
        decided = decided && !RSQ_SIM(S, force_exact);
        // a divergent branch around a call is skipped by the wave when no lane takes it (s_cbranch_execz): no ballot needed in front of it -- the ballot of a
        // predicate that is a conjunction of compares costs a select, a compare and three scalar instructions per draw
        if (!decided) value = exact<NM>(desc, idx, u, ps);
        return value;
    }

    RSQ_HD uint32_t draw_quality(uint32_t i, const uint32_t (&idx)[4], uint32_t u, uint32_t &ps) const {
        const uint32_t local = i - qbase, slot = RSQ_PLAN(S, slot_q), nr = RSQ_PLAN(S, rate_rows_q), r3 = RSQ_GEO_ROW(S, q, 3, idx[3]);
        const RSQ_LDS float *mine = img + RSQ_PLAN(S, q.lds) + local * RSQ_PLAN(S, q.lds_stride);      // margins 0 and 1 of the table
        const LdsRow32 m0{mine + RSQ_GEO_ROW(S, q, 0, idx[0]) * slot}, m1{mine + (RSQ_PLAN(S, q.before[1]) + RSQ_GEO_ROW(S, q, 1, idx[1])) * slot};
        // the rows over the read position: in the ring, or for a read that lags further in the slot behind it when the wave staged this position there
        const bool near = in_ring(idx[2]);
        const LdsRow32 m2{ring_ + (near ? idx[2] % kRingSlots : kRingSlots) * RSQ_PLAN(S, ring_stride) + local * slot};
        const LdsRow32 m3{img + RSQ_PLAN(S, q3_off) + local * RSQ_PLAN(S, q3_stride) + (r3 < nr ? r3 : 0u) * slot};
        uint32_t col = 0;
        const bool decided = draw_screened_batched<QQ, QQ % QB == 0 ? QB : (QQ % 2 == 0 ? 2 : 1)>(u, col, m0, m1, m2, m3) && (near || idx[2] == demand) && r3 < nr;      // a rate or a position whose row is not staged: double precision
        RSQ_SCREEN_COUNT(0, decided);
        return settle<4>(decided, RSQ_PLAN(S, q.values), local * slot + col, local, idx, u, ps);
    }
    // The lane's scalars of the word screen (LdsPlan::bw_off): lists by VALUE -- AdjustIndeces is folded into them when they are packed --, so a lane clamps at
    // the top only; no row address is formed.
    RSQ_HD bool base_call_word(uint32_t local, const uint32_t (&idx)[4], uint32_t u) const {
        if (RSQ_PLAN(S, bw_off) == kNoLds || RSQ_SIM(S, force_exact)) return false;
        const RSQ_LDS float *mine = img + RSQ_PLAN(S, bw_off) + local * RSQ_PLAN(S, bw_stride);
        const uint32_t sides = RSQ_PLAN(S, bw_sides);
        auto entry = [&](uint32_t n, uint32_t value) {
            const uint32_t e = RSQ_PLAN(S, bw_at[n]) + (value < RSQ_PLAN(S, bw_cap[n]) ? value : RSQ_PLAN(S, bw_cap[n]));
            Float2 f;
            if (3u == sides) f = *reinterpret_cast<const RSQ_LDS Float2 *>(mine + 2u * e);
            else {
                const float x = mine[e];
                f.x = 2u == sides ? 0.f : x;
                f.y = 2u == sides ? x : 0.f;
            }
            return f;
        };
        return word_screen_sure(entry(0, idx[0]), entry(1, idx[1] >> kWordPosShift), entry(2, idx[2]), entry(3, idx[3]), u, sides);
    }
    RSQ_HD uint32_t draw_base_call(uint32_t i, const uint32_t (&idx)[4], uint32_t u, uint32_t &ps) const {
        const uint32_t local = i - qbase * 5u;
        // nearly every draw: the random word alone says "the template base" (the table's base: tables come five to a base, four bases to a tile).  Such a lane
        // reads four scalars and no row; the others draw among themselves, and a wave without one skips the branch (s_cbranch_execz)
        const bool sure = base_call_word(local, idx, u);
        RSQ_WORD_SCREEN_COUNT(sure);
        if (sure) {
            RSQ_SCREEN_COUNT(1, true);
            ps = 1u;
            return ((local * 52429u) >> 18) & 3u;              // local / 5 % 4 (local is far below 2^16: the image's tables fit LDS)
        }
        const uint32_t slot = RSQ_PLAN(S, slot_b), nr = RSQ_PLAN(S, rate_rows_b), r3 = RSQ_GEO_ROW(S, b, 3, idx[3]);
        const uint32_t g = 4u * (RSQ_PLAN(S, b.off32) + i * (RSQ_PLAN(S, b.table_rows) * slot));               // the table's rows in device memory: bytes from the pool's address (below 4 GB: pack_tables)
        const LdsRow32 m0{img + RSQ_PLAN(S, b.lds) + local * RSQ_PLAN(S, b.lds_stride) + RSQ_GEO_ROW(S, b, 0, idx[0]) * slot};
        const PoolRow32 m1{S.pool32, g + 4u * (RSQ_PLAN(S, b.before[1]) + RSQ_GEO_ROW(S, b, 1, idx[1])) * slot};
        const uint32_t r2 = RSQ_GEO_ROW(S, b, 2, idx[2]);
        const bool m2_staged = RSQ_PLAN(S, b.lds2) != kNoLds, staged = r3 < nr;
        const MixedRow32 m2{LdsRow32{img + (m2_staged ? RSQ_PLAN(S, b.lds2) + local * RSQ_PLAN(S, b.lds2_stride) + r2 * slot : 0u)},
                            PoolRow32{S.pool32, g + 4u * (RSQ_PLAN(S, b.before[2]) + r2) * slot}, m2_staged};
        const MixedRow32 m3{LdsRow32{img + RSQ_PLAN(S, b3_off) + local * RSQ_PLAN(S, b3_stride) + (staged ? r3 : 0u) * slot}, PoolRow32{S.pool32, g + 4u * (RSQ_PLAN(S, b.before[3]) + r3) * slot}, staged};
        uint32_t col = 0;
        const bool decided = draw_screened<(int)kQuadsSmall>(u, col, m0, m1, m2, m3);
        RSQ_SCREEN_COUNT(1, decided);
        return settle<4>(decided, RSQ_PLAN(S, b.values), local * slot + col, 4u * RSQ_PLAN(S, img_tiles) + local, idx, u, ps);
    }
    RSQ_HD uint32_t draw_indel(uint32_t i, const uint32_t (&idx)[3], uint32_t u, uint32_t &ps) const {
        // nearly every draw: the random word alone says "no indel" (DevTable::sure_range, 0 for an empty table; margin 0 at its row 0: the index is not above the
        // margin's first); the wave skips the rows when all its lanes are that sure, and has read two words of the descriptor
        const RSQ_LDS DevTable *d = reinterpret_cast<const RSQ_LDS DevTable *>(img) + (24u * RSQ_PLAN(S, img_tiles) + i);
        const uint32_t range = d->sure_range, lo16 = range & 0xFFFFu;
        const bool sure = (u >> 16) - lo16 < (range >> 16) - lo16 && idx[0] <= d->from[0];
        RSQ_SCREEN_COUNT(3, sure);
        ps = 1u;
        if (sure) return 0;                                 // the lanes that are not sure draw among themselves; a wave without one skips the branch (s_cbranch_execz)
        const uint32_t slot = RSQ_PLAN(S, slot_i), r0 = RSQ_GEO_ROW(S, i, 0, idx[0]);
        const uint32_t g = 4u * (RSQ_PLAN(S, i.off32) + i * (RSQ_PLAN(S, i.table_rows) * slot));
        const bool m0_staged = RSQ_PLAN(S, i.lds) != kNoLds;
        const MixedRow32 m0{LdsRow32{img + (m0_staged ? RSQ_PLAN(S, i.lds) + i * RSQ_PLAN(S, i.lds_stride) + r0 * slot : 0u)}, PoolRow32{S.pool32, g + 4u * r0 * slot}, m0_staged};
        const PoolRow32 m1{S.pool32, g + 4u * (RSQ_PLAN(S, i.before[1]) + RSQ_GEO_ROW(S, i, 1, idx[1])) * slot}, m2{S.pool32, g + 4u * (RSQ_PLAN(S, i.before[2]) + RSQ_GEO_ROW(S, i, 2, idx[2])) * slot};
        uint32_t col = 0;
        const bool decided = draw_screened<(int)kQuadsSmall>(u, col, m0, m1, m2);
        RSQ_SCREEN_COUNT(2, decided);
        return settle<3>(decided, RSQ_PLAN(S, i.values), i * slot + col, 24u * RSQ_PLAN(S, img_tiles) + i, idx, u, ps);
    }
    RSQ_HD uint32_t draw_seq_quality(uint32_t i, const uint32_t (&idx)[3], uint32_t u, uint32_t &ps) const {     // once per read: double precision
        const uint32_t r = exact_draw_call<3>(S.pool, img, par0_at(), 24u * RSQ_PLAN(S, img_tiles) + 12u + i - qbase / 4u, idx[0], idx[1], idx[2], 0u, u);
        ps = (r >> 31) ^ 1u;
        return r & 0x7FFFFFFFu;
    }
};

// Builds the LDS image `qbase` (image_qbase); tid/nthreads describe the calling thread (the host emulation calls it with
// 0/1).  The caller synchronises the workgroup between the two phases and after the second.
RSQ_HD void lds_stage_descriptors(const DevSim &S, RSQ_LDS float *img, uint32_t qbase, uint32_t tid, uint32_t nthreads) {
    const uint32_t T = RSQ_PLAN(S, img_tiles);
    RSQ_LDS uint32_t *dst = reinterpret_cast<RSQ_LDS uint32_t *>(img);
    const uint32_t wq = 4u * T * kDescWords, wb = 20u * T * kDescWords, wi = 12u * kDescWords, ws = T * kDescWords;
    const uint32_t *q = reinterpret_cast<const uint32_t *>(S.quality + qbase), *b = reinterpret_cast<const uint32_t *>(S.base_call + qbase * 5u),
                   *in = reinterpret_cast<const uint32_t *>(S.indels), *sq = reinterpret_cast<const uint32_t *>(S.seq_quality + qbase / 4u);
    // outcome values: the indel tables' are the first bytes of the pool, the image's tiles' a contiguous range from its first quality table's on;
    // par0_off (word 1 of a descriptor) becomes relative to the image's copy
    const uint32_t tiles_at = S.quality[qbase].par0_off, shift = tiles_at - RSQ_PLAN(S, par0_indel_bytes);
    for (uint32_t i = tid; i < wq; i += nthreads) dst[i] = q[i] - (i % kDescWords == 1u ? shift : 0u);
    for (uint32_t i = tid; i < wb; i += nthreads) dst[wq + i] = b[i] - (i % kDescWords == 1u ? shift : 0u);
    for (uint32_t i = tid; i < wi; i += nthreads) dst[wq + wb + i] = in[i];
    for (uint32_t i = tid; i < ws; i += nthreads) dst[wq + wb + wi + i] = sq[i] - (i % kDescWords == 1u ? shift : 0u);
    const uint32_t *p0 = reinterpret_cast<const uint32_t *>(S.par0), *p1 = reinterpret_cast<const uint32_t *>(S.par0 + tiles_at);      // ranges start on words; the pool has spare bytes at its end
    const uint32_t indel_words = RSQ_PLAN(S, par0_indel_bytes) / 4u, par0_at = RSQ_PLAN(S, desc_words) - RSQ_PLAN(S, par0_words);
    for (uint32_t i = tid; i < RSQ_PLAN(S, par0_words); i += nthreads) dst[par0_at + i] = i < indel_words ? p0[i] : p1[i - indel_words];
    // the outcome values by column of the image's tables (FamilyGeo::values; whole words: slots are multiples of four columns)
    const uint32_t nq = T * RSQ_PLAN(S, slot_q), nb = 5u * T * RSQ_PLAN(S, slot_b), ni = 3u * RSQ_PLAN(S, slot_i);
    const uint32_t *vq = reinterpret_cast<const uint32_t *>(S.par0 + RSQ_PLAN(S, q.values_src)) + qbase / 4u * RSQ_PLAN(S, slot_q),
                   *vb = reinterpret_cast<const uint32_t *>(S.par0 + RSQ_PLAN(S, b.values_src)) + qbase / 4u * 5u * RSQ_PLAN(S, slot_b),
                   *vi = reinterpret_cast<const uint32_t *>(S.par0 + RSQ_PLAN(S, i.values_src));
    for (uint32_t i = tid; i < nq; i += nthreads) dst[RSQ_PLAN(S, q.values) / 4u + i] = vq[i];
    for (uint32_t i = tid; i < nb; i += nthreads) dst[RSQ_PLAN(S, b.values) / 4u + i] = vb[i];
    for (uint32_t i = tid; i < ni; i += nthreads) dst[RSQ_PLAN(S, i.values) / 4u + i] = vi[i];
}
// rows [first_row, first_row + n_rows) of `n_tables` tables of a family, from table `first` of the profile on, to [table][n_rows][slot] at dst_off: whole 16-byte groups
RSQ_HD void lds_stage_family_rows(const DevSim &S, RSQ_LDS float *img, uint32_t off32, uint32_t table_rows, uint32_t first, uint32_t n_tables, uint32_t first_row, uint32_t n_rows,
                                  uint32_t slot, uint32_t dst_off, uint32_t dst_stride, uint32_t tid, uint32_t nthreads) {
    const uint32_t per_table = n_rows * (slot / 4u);
    for (uint32_t i = tid; i < n_tables * per_table; i += nthreads) {
        const uint32_t table = i / per_table, g = i - table * per_table;
        reinterpret_cast<RSQ_LDS Quad *>(img + dst_off + table * dst_stride)[g] = reinterpret_cast<const Quad *>(S.pool32 + off32 + ((size_t)(first + table) * table_rows + first_row) * slot)[g];
    }
}
RSQ_HD void lds_stage_rows(const DevSim &S, RSQ_LDS float *img, uint32_t qbase, uint32_t tid, uint32_t nthreads) {
    const uint32_t T = RSQ_PLAN(S, img_tiles), sq = RSQ_PLAN(S, slot_q), sb = RSQ_PLAN(S, slot_b), si = RSQ_PLAN(S, slot_i);
    // quality: margins 0 and 1; base call: margin 0, margin 2; indel: margin 0; then the first rows of the two error-rate margins
    lds_stage_family_rows(S, img, RSQ_PLAN(S, q.off32), RSQ_PLAN(S, q.table_rows), qbase, 4u * T, 0u, RSQ_PLAN(S, q.lds_rows), sq, RSQ_PLAN(S, q.lds), RSQ_PLAN(S, q.lds_stride), tid, nthreads);
    lds_stage_family_rows(S, img, RSQ_PLAN(S, b.off32), RSQ_PLAN(S, b.table_rows), qbase * 5u, 20u * T, 0u, RSQ_PLAN(S, b.lds_rows), sb, RSQ_PLAN(S, b.lds), RSQ_PLAN(S, b.lds_stride), tid, nthreads);
    if (RSQ_PLAN(S, b.lds2) != kNoLds)
        lds_stage_family_rows(S, img, RSQ_PLAN(S, b.off32), RSQ_PLAN(S, b.table_rows), qbase * 5u, 20u * T, RSQ_PLAN(S, b.before[2]), RSQ_PLAN(S, b.last[2]) + 1u, sb, RSQ_PLAN(S, b.lds2),
                              RSQ_PLAN(S, b.lds2_stride), tid, nthreads);
    if (RSQ_PLAN(S, i.lds) != kNoLds)
        lds_stage_family_rows(S, img, RSQ_PLAN(S, i.off32), RSQ_PLAN(S, i.table_rows), 0u, 12u, 0u, RSQ_PLAN(S, i.lds_rows), si, RSQ_PLAN(S, i.lds), RSQ_PLAN(S, i.lds_stride), tid, nthreads);
    lds_stage_family_rows(S, img, RSQ_PLAN(S, q.off32), RSQ_PLAN(S, q.table_rows), qbase, 4u * T, RSQ_PLAN(S, q.before[3]), RSQ_PLAN(S, rate_rows_q), sq, RSQ_PLAN(S, q3_off), RSQ_PLAN(S, q3_stride), tid,
                          nthreads);
    lds_stage_family_rows(S, img, RSQ_PLAN(S, b.off32), RSQ_PLAN(S, b.table_rows), qbase * 5u, 20u * T, RSQ_PLAN(S, b.before[3]), RSQ_PLAN(S, rate_rows_b), sb, RSQ_PLAN(S, b3_off), RSQ_PLAN(S, b3_stride), tid,
                          nthreads);
    // the word screen's scalars of the image's base-call tables: one contiguous piece of the pool
    if (RSQ_PLAN(S, bw_off) != kNoLds) {
        const float *src = S.pool32 + RSQ_PLAN(S, bw_src) + (size_t)qbase * 5u * RSQ_PLAN(S, bw_stride);
        for (uint32_t i = tid; i < 20u * T * RSQ_PLAN(S, bw_stride); i += nthreads) img[RSQ_PLAN(S, bw_off) + i] = src[i];
    }
}
// The ring: the quality rows (margin 2) over read position p of the segment's tables, copied by the wave itself at the beginning of
// step p into slot p % kRingSlots of its ring: one load of 16 bytes per lane instead of one per lane and quad of the row.  Item i is
// one 16-byte group of one table's row.
RSQ_HD uint32_t lds_ring_items(const DevSim &S) { return 4u * RSQ_PLAN(S, img_tiles) * RSQ_PLAN(S, quads_q); }
// What does not change from step to step is worked out once per chunk of reads (RingItem): where the table's rows over the read position begin and the
// item's place in a ring slot (first position and last row of the margin are the family's).
struct RingItem {
    uint32_t rows;                     // row 0 of margin 2, at the item's group of four columns: bytes from the pool's address
    uint32_t at;                       // floats from the slot's start
};
RSQ_HD RingItem lds_ring_item(const DevSim &S, uint32_t qbase, uint32_t item) {
    const uint32_t table = item / RSQ_PLAN(S, quads_q), c = item % RSQ_PLAN(S, quads_q), slot = RSQ_PLAN(S, slot_q);
    return RingItem{4u * (RSQ_PLAN(S, q.off32) + ((qbase + table) * RSQ_PLAN(S, q.table_rows) + RSQ_PLAN(S, q.before[2])) * slot + 4u * c), table * slot + 4u * c};
}
RSQ_HD Quad lds_ring_load(const DevSim &S, const RingItem &it, uint32_t p) { return PoolRow32{S.pool32, it.rows + 4u * RSQ_GEO_ROW(S, q, 2, p) * RSQ_PLAN(S, slot_q)}.quad(0u); }
RSQ_HD void lds_ring_store(const DevSim &S, const RingItem &it, RSQ_LDS float *ring, uint32_t p, const Quad &q) {
    *reinterpret_cast<RSQ_LDS Quad *>(ring + (p % kRingSlots) * RSQ_PLAN(S, ring_stride) + it.at) = q;
}
RSQ_HD void lds_ring_stage(const DevSim &S, const RingItem &it, RSQ_LDS float *ring, uint32_t p) { lds_ring_store(S, it, ring, p, lds_ring_load(S, it, p)); }
// the rows over position p into the slot behind the ring (ScreenTables::demand)
RSQ_HD void lds_ring_stage_demand(const DevSim &S, const RingItem &it, RSQ_LDS float *ring, uint32_t p) {
    *reinterpret_cast<RSQ_LDS Quad *>(ring + kRingSlots * RSQ_PLAN(S, ring_stride) + it.at) = lds_ring_load(S, it, p);
}
RSQ_HD void lds_ring_stage(const DevSim &S, uint32_t qbase, RSQ_LDS float *ring, uint32_t p, uint32_t item) { lds_ring_stage(S, lds_ring_item(S, qbase, item), ring, p); }
// CreateReads for one mate of a fragment (Simulator.cpp:634-721, GetOrgSeq :1916-1922)
// template and systematic errors of mate `seg` of fragment f (GetOrgSeq :1916-1922, CreateReads :680-684)
RSQ_HD FragmentSrc fragment_src(const DevSim &S, const Fragment &f, uint32_t seg, uint32_t end) {
    const uint32_t L = S.seq_len[f.seq];
    const uint32_t want = S.read_lengths[seg].to + RSQ_SIM(S, max_len_deletion);           // Simulator.cpp:1918-1921
    FragmentSrc src;
    src.words = hap_words(S, f.allele);                                        // with variants: the allele's copy (substitutions applied)
    src.word_off = S.seq_word_off[f.seq];
    src.len = f.len < want ? f.len : want;
    src.reverse = seg != f.strand;                                              // block.at(strand) = start_block
    src.first = src.reverse ? end : f.start;
    src.sys_ = src.reverse ? S.sys_rev + S.seq_base_off[f.seq] + (L - end) : S.sys_fwd + S.seq_base_off[f.seq] + f.start;
    src.converted = nullptr;
    src.gc_prefix = hap_gc_prefix(S, f.allele);
    return src;
}
RSQ_HD FragmentSrc fragment_src(const DevSim &S, const Fragment &f, uint32_t seg) { return fragment_src(S, f, seg, f.start + f.len); }

// The template of a mate with variants: FragmentSrc (on the allele's copy of the reference when all variants are substitutions,
// else with the template written beforehand by k_variant_templates), and the systematic errors through the walk of
// GetSysErrorFromBlock / IncrementBlockPos (Simulator.cpp:232-292) and of FillReadPart's deletion branch (:380-392), stated in strand
// coordinates (position on the strand the mate reads; variants in that strand's order): the reverse blocks' lists are the mirror
// image of the forward ones.  cur walks the variants of ALL alleles; a block's err_variants_ list ends where the block ends, and
// cur_var = 0 after a block change is the first variant of the new block.  As written in the reference: after a substitution is
// used cur is incremented twice (the next variant is skipped unless a block starts in between); inside an insertion the error of the
// reference position is returned, not the inserted base's; the deletion branch does not look at variants (a passed variant is
// applied late).
struct VariantSrc : FragmentSrc {
    const DevVariant *var;              // the sequence's variants in forward order
    const uint16_t *err;                // the variants' systematic errors on the strand the mate reads
    uint32_t n_var, L, allele;
    uint32_t *walk_error;               // DevSim::walk_error
    uint32_t spos0, cur0, var_pos0;     // start of the walk: strand position of the first template base, variant index, position in an insertion
    mutable uint32_t spos, cur, var_pos;
    RSQ_HD const DevVariant &var_at(uint32_t i) const { return reverse ? var[n_var - 1u - i] : var[i]; }
    RSQ_HD uint32_t var_spos(uint32_t i) const { return reverse ? L - 1u - var_at(i).pos : var_at(i).pos; }
    RSQ_HD uint32_t var_err(uint32_t i, uint32_t k) const { return err[var_at(i).off + k]; }
    RSQ_HD uint32_t lower_bound(uint32_t sp) const {
        uint32_t lo = 0, hi = n_var;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (var_spos(mid) < sp) lo = mid + 1u;
            else hi = mid;
        }
        return lo;
    }
    // lower_bound(sp) from where the walk stands: a block change asks for the first variant at or behind the new block's first position, and that is `cur` itself or
    // a neighbour (a variant skipped behind a substitution) -- one or two loads in the place of a binary search over the sequence's variants (17 dependent loads
    // for 100 000 variants, at every thousandth step of every lane)
    RSQ_HD uint32_t seek(uint32_t sp) const {
        uint32_t c = cur < n_var ? cur : n_var;
        while (c > 0u && var_spos(c - 1u) >= sp) --c;
        while (c < n_var && var_spos(c) < sp) ++c;
        return c;
    }
    // blocks are cut on the forward strand (Simulator.h:254): first strand position of the block after the one holding sp
    RSQ_HD uint32_t block_end(uint32_t sp) const { return reverse ? L - ((L - sp - 1u) / kBlockSize) * kBlockSize : (sp / kBlockSize + 1u) * kBlockSize; }
    // what the common step -- a plain reference base, no variant in reach -- needs, kept between steps: the strand position of variant `cur`
    // (none: 0xFFFFFFFF) and the end of the block holding spos; refreshed whenever cur or the block changes
    mutable uint32_t vs_cur, bend_cur;
    // ... and, for the step itself, ONE number: the strand position before which nothing of the walk can happen -- no variant of the block at or before the
    // position, not the block's last position (the step behind it changes the block), not inside an insertion, not beyond the strand.  A step in front of it
    // is the plain track's (one compare); everything else goes the long way below, which keeps its own state (cur, var_pos, the block's end) wherever the
    // compiler finds room for it -- these are read once in a few hundred steps.
    mutable uint32_t quiet_until;
    RSQ_HD void refresh() const {
        vs_cur = cur < n_var ? var_spos(cur) : 0xFFFFFFFFu;
        bend_cur = block_end(spos);
        uint32_t q = bend_cur - 1u;
        if (vs_cur < q) q = vs_cur;
        if (L < q) q = L;
        quiet_until = var_pos ? 0u : q;
    }
    RSQ_HD void rewind() const {
        spos = spos0;
        cur = cur0;
        var_pos = var_pos0;
        refresh();
    }
    RSQ_HD void increment_block_pos() const {                                   // :232-238
        if (++spos == bend_cur) cur = seek(spos);
        refresh();
    }
    // With variants a few bases apart the walk (its skipped variants, its late ones) can use up more reference positions than the
    // template has and run off the end of the strand: the reference follows a NULL next_block_ there.  Reported, not simulated.
    RSQ_HD bool off_strand() const {
        if (spos < L) return false;
        *walk_error = 1u;
        return true;
    }
    RSQ_HD uint32_t sys_base(uint32_t) const {                                  // :240-292
#if defined(RSQ_NO_QUIET)                                                        // measurements: the walk without its short cut
        if (false) {
#else
        if (__builtin_expect(spos < quiet_until, 1)) {                          // nearly every step
#endif
            const uint32_t se = FragmentSrc::sys_base(spos - spos0);
            ++spos;
            return se;
        }
        return sys_base_event();
    }
    RSQ_HD uint32_t sys_base_event() const {
        if (off_strand()) return 0;
        if (!var_pos && !(vs_cur < bend_cur && vs_cur <= spos)) {               // no variant of the block at or before this position: the block's last position
            const uint32_t se = FragmentSrc::sys_base(spos - spos0);
            if (++spos == bend_cur) {
                cur = seek(spos);
                refresh();
            }
            return se;
        }
        if (var_pos) {
            const uint32_t se = FragmentSrc::sys_base(spos - spos0);
            if (++var_pos >= var_at(cur).len) {
                var_pos = 0;
                ++cur;
                increment_block_pos();
            }
            return se;
        }
        uint32_t bend = bend_cur;
        while (cur < n_var) {
            const uint32_t vs = var_spos(cur);
            if (!(vs < bend && vs <= spos)) break;                              // cur_var < err_variants_.size() && position_ <= block_pos
            const DevVariant &v = var_at(cur);
            if ((v.allele[allele >> 6] >> (allele & 63u)) & 1u) {
                if (0u == v.len) {                                              // deletion
                    ++cur;
                    increment_block_pos();
                    if (off_strand()) return 0;
                    bend = bend_cur;
                } else {
                    const uint32_t se = var_err(cur, 0);
                    if (1u == v.len) {                                          // substitution
                        ++cur;
                        increment_block_pos();
                        ++cur;
                        refresh();
                    } else {
                        var_pos = 1;                                            // insertion
                        refresh();
                    }
                    return se;
                }
            } else ++cur;
        }
        const uint32_t se = FragmentSrc::sys_base(spos - spos0);
        increment_block_pos();
        return se;
    }
    RSQ_HD uint32_t sys_deleted(uint32_t) const {                               // :380-392
        if (off_strand()) return 0;
        const uint32_t se = FragmentSrc::sys_base(spos - spos0);
        if (var_pos && ++var_pos >= var_at(cur).len) var_pos = 0;
        if (0u == var_pos) {
            if (++spos == bend_cur) cur = seek(spos);
        }
        refresh();
        return se;
    }
    RSQ_HD void totals(uint32_t n, uint32_t &gc, uint32_t &rate_sum) const {    // :480-504: the error rates through a copy of the walk
        if (converted) gc += ref_gc_count(converted, 0, 0, n);
        else gc += reverse ? ref_gc_count_prefix(words, gc_prefix, word_off, first - n, first) : ref_gc_count_prefix(words, gc_prefix, word_off, first, first + n);
        // no variant in reach of these n steps (the walk starts at the first variant at or behind the first base, and that one lies behind the
        // last): the walk returns the strand's own errors, a block change finds the same variant again
        if (!var_pos0 && vs_cur >= spos0 + n && (0u == cur0 || var_spos(cur0 - 1u) < spos0)) {
            rate_sum += rate_total(n);
            return;
        }
        for (uint32_t k = 0; k < n; ++k) rate_sum += sys_base(k) >> 8;
        rewind();
    }
};
// fv == nullptr: substitutions only (the walk starts at the first variant at or after the first template base)
RSQ_HD VariantSrc variant_src(const DevSim &S, const Fragment &f, const FragmentVar *fv, uint32_t seg) {
    VariantSrc src;
    static_cast<FragmentSrc &>(src) = fragment_src(S, f, seg, fv ? fv->end : f.start + f.len);
    src.var = S.variants + S.var_ptr[f.seq];
    src.err = src.reverse ? S.var_err_rev : S.var_err_fwd;
    src.n_var = S.var_ptr[f.seq + 1] - S.var_ptr[f.seq];
    src.L = S.seq_len[f.seq];
    src.allele = f.allele;
    src.walk_error = S.walk_error;
    src.spos0 = src.reverse ? src.L - src.first : src.first;
    if (!fv) {
        src.cur0 = src.lower_bound(src.spos0);
        src.var_pos0 = 0;
    } else if (!src.reverse) {                                                  // CreateReads :686-688: variant.at(strand) = start variant
        src.cur0 = (uint32_t)fv->start_var;
        src.var_pos0 = fv->start_var_pos;
    } else {                                                                    // the end variant, seen from the reverse block's list
        src.cur0 = src.n_var - 1u - (uint32_t)fv->end_var;                      // end_var -1: one past the last
        src.var_pos0 = fv->end_var_pos ? src.var[fv->end_var].len - fv->end_var_pos : 0u;
    }
    src.rewind();
    return src;
}
// The converted template of mate `seg` of fragment f (CTConversion's dispatcher, Simulator.cpp:2219-2247): the forward mate is
// converted from the start position on, the reverse mate from the end position on (`reversed`).
RSQ_HD void convert_template(const DevSim &S, const Fragment &f, uint32_t seg, uint64_t *tmpl, uint32_t template_words) {
    const FragmentSrc src = fragment_src(S, f, seg);
    for (uint32_t w = 0; w < template_words; ++w) tmpl[w] = 0;
    for (uint32_t k = 0; k < src.len; ++k) tmpl[k >> 5] |= (uint64_t)src.ref(k) << ((k & 31u) * 2u);
    const MethView m = meth_view(S, f.seq);
    MethDraws d{S.seed, f.start, f.seq, f.len, (kDomMethylation << 28) | ((src.reverse ? 1u : 0u) << 27), 0xFFFFFFFFu, Words{0, 0, 0, 0}};
    ct_conversion(tmpl, src.len, m, nullptr, 0u, src.first, src.reverse, VarStart{0, 0u}, d);
}

// the template of mate `seg` with variants of any kind: the forward mate from the start variant, the reverse mate from the end variant
RSQ_HD void variant_template(const DevSim &S, const Fragment &f, const FragmentVar &fv, uint32_t seg, uint64_t *tmpl, uint32_t template_words) {
    const uint32_t want = S.read_lengths[seg].to + RSQ_SIM(S, max_len_deletion), tl = f.len < want ? f.len : want;
    const VarView r = var_view(S, f.seq);
    const bool reversed = seg != f.strand;
    const VarStart from = reversed ? VarStart{fv.end_var, fv.end_var_pos} : VarStart{fv.start_var, fv.start_var_pos};
    const uint32_t at = reversed ? fv.end : f.start;
    allele_template(allele_view(S, f.seq, f.allele), at, from, tl, reversed, tmpl, template_words);
    if (S.meth_ptr) {                                                           // CTConversion with variants (:2232-2237)
        const MethView m = meth_view(S, f.seq, f.allele);
        MethDraws d{S.seed, f.start, f.seq | (fv.sub << 22), f.len, (kDomMethylation << 28) | ((reversed ? 1u : 0u) << 27) | ((uint32_t)f.allele << 17), 0xFFFFFFFFu,
                    Words{0, 0, 0, 0}};
        ct_conversion(tmpl, tl, m, &r, f.allele, at, reversed, from, d);
    }
}

template <class Tab>
RSQ_HD void fill_fragment_read(const DevSim &S, const Tab &tab, const Fragment &f, uint32_t seg, ReadOut &out, ReadMeta &meta) {
    const uint32_t c2 = f.len | ((uint32_t)f.dup << 16);
    const uint32_t tile = draw_tile(S, f.start, f.seq, c2, pair_c3(kDomPair, f.strand, 2, f.allele));
    const Stream st{S.seed, f.start, f.seq, c2, pair_c3(kDomPair, f.strand, seg, f.allele)};
    if (S.variants_loaded) fill_read(S, tab, st, seg, tile, f.len, variant_src(S, f, nullptr, seg), out, meta);
    else fill_read(S, tab, st, seg, tile, f.len, fragment_src(S, f, seg), out, meta);
}
// one mate of adapter-only pair i (Simulator.cpp:2359-2382)
template <class Tab>
RSQ_HD void fill_adapter_only_read(const DevSim &S, const Tab &tab, uint64_t i, uint32_t seg, ReadOut &out, ReadMeta &meta) {
    const uint32_t tile = draw_tile(S, (uint32_t)i, 0xFFFFFFFFu, (uint32_t)(i >> 32), pair_c3(kDomPair, 0, 2));
    const Stream st{S.seed, (uint32_t)i, 0xFFFFFFFFu, (uint32_t)(i >> 32), pair_c3(kDomPair, 0, seg)};
    fill_read(S, tab, st, seg, tile, 0u, EmptySrc{}, out, meta);
}

// seqToIllumina records (Simulator.cpp:2403-2512): templates and systematic errors come from byte arrays, a record per lane -- 64 cache lines per
// load instruction.  The source therefore holds the 8-byte group (k >> 3) of the three arrays it last read: three loads per eight bases instead of per
// base, and the totals of FillRead's start (G/C count, rate sum) come from the same groups.  `safe`: bytes from the record's first byte to the end of
// the arrays; a group reaching beyond it is read byte by byte.
struct RecordSrc {
    const uint8_t *seq;
    const uint8_t *dom, *rate;
    uint32_t len;
    uint32_t safe;
    mutable uint32_t group;
    mutable uint64_t w_seq, w_dom, w_rate;
    RSQ_HD static uint64_t load8(const uint8_t *p, uint32_t off, uint32_t safe) {
        if (off + 8u <= safe) return load_as<uint64_t, 1>(p + off);
        uint64_t w = 0;
        for (uint32_t j = 0; j < 8u && off + j < safe; ++j) w |= (uint64_t)p[off + j] << (8u * j);
        return w;
    }
    RSQ_HD void hold(uint32_t k) const {
        const uint32_t g = k >> 3;
        if (g == group) return;
        group = g;
        w_seq = load8(seq, g * 8u, safe);
        w_dom = load8(dom, g * 8u, safe);
        w_rate = load8(rate, g * 8u, safe);
    }
    RSQ_HD uint32_t org_len() const { return len; }
    RSQ_HD uint32_t base(uint32_t k) const {
        hold(k);
        return (uint32_t)(w_seq >> ((k & 7u) * 8u)) & 0xFFu;
    }
    RSQ_HD uint32_t sys_base(uint32_t k) const {
        hold(k);
        const uint32_t sh = (k & 7u) * 8u;
        return ((uint32_t)(w_dom >> sh) & 0xFFu) | (((uint32_t)(w_rate >> sh) & 0xFFu) << 8);
    }
    RSQ_HD uint32_t sys_deleted(uint32_t k) const { return sys_base(k); }
    // Simulator.cpp:482-489 over the groups, from the last one down (the first stays held): a base is G/C iff it is 1 or 2, the rates add up bytewise
    RSQ_HD void totals(uint32_t n, uint32_t &gc, uint32_t &rate_sum) const {
        const uint64_t kOnes = 0x0101010101010101ull, kEven = 0x00FF00FF00FF00FFull;
        for (uint32_t g = (n + 7u) >> 3; g--;) {
            hold(g * 8u);
            const uint32_t left = n - g * 8u;                                 // bases of this group that count
            const uint64_t keep = left >= 8u ? ~0ull : (1ull << (8u * left)) - 1ull;
            const uint64_t w = w_seq & keep, r = w_rate & keep;
            const uint64_t high = (w >> 2) | (w >> 3) | (w >> 4) | (w >> 5) | (w >> 6) | (w >> 7);
            const uint64_t is = (w ^ (w >> 1)) & ~high & kOnes;
            gc += (uint32_t)((is * kOnes) >> 56);
            const uint64_t pairs = (r & kEven) + ((r >> 8) & kEven);
            rate_sum += (uint32_t)((pairs * 0x0001000100010001ull) >> 48);
        }
    }
};
// record i of n: the arrays hold read_len bytes per record
RSQ_HD RecordSrc record_src(const uint8_t *seqs, const uint8_t *dom, const uint8_t *rate, uint32_t read_len, uint64_t i, uint64_t n) {
    const uint64_t rest = (n - i) * read_len;
    return RecordSrc{seqs + i * read_len, dom + i * read_len, rate + i * read_len, read_len, rest > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rest, 0xFFFFFFFFu, 0, 0, 0};
}
// a record of `len` bytes at offset `at` of arrays of `bytes` bytes (records parsed on the device lie where their text lay, rsq_fasta.h)
RSQ_HD RecordSrc record_src_at(const uint8_t *seqs, const uint8_t *dom, const uint8_t *rate, uint32_t at, uint32_t len, uint32_t bytes) {
    return RecordSrc{seqs + at, dom + at, rate + at, len, bytes - at, 0xFFFFFFFFu, 0, 0, 0};
}
// Workgroup sizes of the read kernels: 1024 threads -- four waves per SIMD at 128 VGPRs.  The step is a chain of dependent draws that leaves VALU and LDS idle a
// fifth of the time at three waves per SIMD; a fourth wave fills more of it than the spills cost that 128 registers bring (the profile's own kernel for read pairs:
// then 11 spilled VGPRs, 80 B of scratch; with variants 67 and 208 B).  Measured then against 768 threads, 157-168 VGPRs and no spill (profiles/r04_zz_block_*): read pairs
// 47.2 -> 42.5 ms per 10 M pairs, seqToIllumina records 22.9 -> 22.1 ms per 8 M, configs[4] at 1/10 scale 107.5 -> 112.8 M pairs/s -- with the screen's loads
// issued a quad at a time in every kernel (RSQ_SCREEN_BATCH 1; two at a time the walking kernels lose 3-7 % at 1024 threads, and they still take one).  Since the
// kernel of the plain pairs carries WaveReadOut and WaveFragmentSrc it has the registers for two quads of the quality draw at a time: 11 spilled VGPRs and 88 B with
// them, 17 and 104 B before (DESIGN_LOG.md section 23).  RSQ_FILL_BLOCK_WALK: the kernels whose source walks
// per-lane state (variants, records), should a build want them smaller.
// The same for records parsed on the device (rsq_fasta.h Packed): a half-word per base -- base code in bits 0-1, dominant error in bits 2-4, error percent in
// bits 8-15 -- so the lane's eight bases of all three come with ONE 16-byte load (RecordSrc: three 8-byte loads, each touching a cache line of the lane's own).
struct PackedRecordSrc {
    const uint16_t *codes;
    uint32_t len;
    uint32_t safe;                   // half-words from the record's first one to the end of the array
    mutable uint32_t group;
    mutable uint64_t lo, hi;         // bases 0-3 and 4-7 of the held group
    RSQ_HD void hold(uint32_t k) const {
        const uint32_t g = k >> 3;
        if (g == group) return;
        group = g;
        const uint16_t *p = codes + 8u * g;
        if (8u * g + 8u <= safe) {
            lo = load_as<uint64_t, 2>(p);
            hi = load_as<uint64_t, 2>(p + 4);
        } else {
            lo = hi = 0;
            for (uint32_t j = 0; j < 8u && 8u * g + j < safe; ++j) (j < 4u ? lo : hi) |= (uint64_t)p[j] << (16u * (j & 3u));
        }
    }
    RSQ_HD uint32_t half(uint32_t k) const {
        hold(k);
        return (uint32_t)(((k & 4u) ? hi : lo) >> (16u * (k & 3u))) & 0xFFFFu;
    }
    RSQ_HD uint32_t org_len() const { return len; }
    RSQ_HD uint32_t base(uint32_t k) const { return half(k) & 3u; }
    RSQ_HD uint32_t sys_base(uint32_t k) const {
        const uint32_t h = half(k);
        return ((h >> 2) & 7u) | (h & 0xFF00u);
    }
    RSQ_HD uint32_t sys_deleted(uint32_t k) const { return sys_base(k); }
    // Simulator.cpp:482-489 over the groups, from the last one down (the first stays held): a base is G/C iff its two bits differ, the rates are the high bytes
    RSQ_HD void totals(uint32_t n, uint32_t &gc, uint32_t &rate_sum) const {
        const uint64_t kHalfOnes = 0x0001000100010001ull;
        for (uint32_t g = (n + 7u) >> 3; g--;) {
            hold(g * 8u);
            const uint32_t left = n - g * 8u;                                 // bases of this group that count
            for (uint32_t part = 0; part < 2u; ++part) {
                const uint32_t mine = left > 4u * part ? (left - 4u * part < 4u ? left - 4u * part : 4u) : 0u;
                if (!mine) continue;
                const uint64_t keep = mine >= 4u ? ~0ull : (1ull << (16u * mine)) - 1ull, w = (part ? hi : lo) & keep;
                gc += popcount64((w ^ (w >> 1)) & kHalfOnes);
                rate_sum += (uint32_t)((((w >> 8) & 0x00FF00FF00FF00FFull) * kHalfOnes) >> 48);
            }
        }
    }
};
RSQ_HD PackedRecordSrc packed_record_src(const uint16_t *codes, uint32_t at, uint32_t len, uint32_t halfwords) {
    return PackedRecordSrc{codes + at, len, halfwords - at, 0xFFFFFFFFu, 0, 0};
}
#ifndef RSQ_FILL_BLOCK
#define RSQ_FILL_BLOCK 1024
#endif
#ifndef RSQ_FILL_BLOCK_WALK
#define RSQ_FILL_BLOCK_WALK 1024
#endif
constexpr int kQualityBatchPairs = RSQ_SCREEN_BATCH > 2 ? RSQ_SCREEN_BATCH : 2;      // quads per batch of the quality draw in the kernel of the plain pairs (ScreenTables QB): at least two
// Where the read kernels of the pairs (plain and with variants) form the Philox round keys of a step (ScreenTables KEYS, philox's KEYS_FROM): from the third round on.
// The seed is their argument, and both run at the scalar-register cap: with twenty keys held across the step loop they reload spilled ones through the vector pipe.
// The first two rounds stay ahead of the barrier because the compiler computes their per-read-constant halves once per read.  The record kernel keeps the keys
// ahead of the loop: it spills half as many scalar registers, gains four reloads and loses a vector register under one code generator (DESIGN_LOG.md section 30).
// (Measurements: RSQ_SPEC_OPTIONS="-DRSQ_KEYS_FROM_STEP=10" compiles the kernel without the barrier, 0 with it in front of every round.)
#ifndef RSQ_KEYS_FROM_STEP
#define RSQ_KEYS_FROM_STEP 2
#endif
constexpr int kKeysFromStep = RSQ_KEYS_FROM_STEP;
constexpr uint32_t kFillBlock = RSQ_FILL_BLOCK, kFillBlockWalk = RSQ_FILL_BLOCK_WALK;
constexpr uint32_t kFillWavesMax = (kFillBlock > kFillBlockWalk ? kFillBlock : kFillBlockWalk) / 64u;      // the LDS image has a ring for every wave of the larger one
RSQ_HD constexpr uint32_t fill_block(bool walk) { return walk ? kFillBlockWalk : kFillBlock; }

// Reads binned by tile (LdsPlan::binned): bin = segment * n_tiles + tile.  `perm` lists the items (pairs of a batch: both segments share the list of a
// tile; seqToIllumina records: a record has one segment) bin after bin.  A workgroup joins a bin, stages its image and its waves pull the bin's chunks
// of 64 items from the bin's counter -- like the plain kernel's waves, without meeting each other -- until the bin is used up; only then does the
// workgroup synchronise, choose the bin with the most chunks left per workgroup already on it, and stage again.
struct FillBins {
    const uint32_t *perm;           // items sorted by bin
    const uint32_t *bin_first;      // [n_bins] first entry of the bin in perm
    const uint32_t *bin_count;      // [n_bins]
    const uint32_t *chunk_ptr;      // [n_bins + 1] chunks of the bins in front
    uint32_t *next_chunk;           // [n_bins] the bin's chunks handed out so far
    uint32_t *workers;              // [n_bins] workgroups on the bin
    uint32_t n_bins;
    const Fragment *frags;          // pairs: the fragments (and what the sieve found of their variants) in perm's order, so that a wave reads them in one piece and
    const FragmentVar *fvars;       // the pair index is needed only before and after a chunk's reads
};
constexpr uint32_t kSchedWords = 8;              // LDS words behind the image in which fill_binned_loop keeps the bin its workgroup is on

// the stream of one mate of a pair (CreateReads :634-721 / SimulateAdapterOnlyPairs :2359-2382): what k_fill_reads and the tile binning agree on
struct PairStream {
    uint32_t c0, c1, c2, strand;
};
RSQ_HD PairStream pair_stream(const Fragment *f, uint32_t sub, uint64_t adapter_only_number) {
    if (f) return PairStream{f->start, f->seq | (sub << 22), f->len | ((uint32_t)f->dup << 16), f->strand};
    return PairStream{(uint32_t)adapter_only_number, 0xFFFFFFFFu, (uint32_t)(adapter_only_number >> 32), 0u};
}

#if RSQ_DEVICE_BUILD
// One lane per read, persistent waves.  A workgroup serves one LDS image at a time -- a template segment (blockIdx.x & 1) with all tiles, built once, every
// wave pulling chunks of 64 pairs from the segment's counter until the batch is exhausted (no tail); or, BINNED, the (segment, tile) of the work unit
// it took (fill_binned_loop).  All lanes of a wave walk their reads' state machines in one uniform loop.  MASK = quads per quality row of the
// screened draws (0: every table access goes to HBM in double precision).
// the LDS image `qbase` of the workgroup (all waves call it; returns after the final barrier)
template <uint32_t MASK>
__device__ RSQ_LDS float *fill_stage_image(const DevSim &S, float *lds_image, uint32_t qbase) {
    RSQ_LDS float *img = (RSQ_LDS float *)lds_image;
    if (MASK) {
        lds_stage_descriptors(S, img, qbase, threadIdx.x, blockDim.x);
        __syncthreads();
        lds_stage_rows(S, img, qbase, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    return img;
}
// 64 reads of one wave through the state machine: one uniform step loop.  Screened (MASK != 0): at the beginning of a step the wave
// copies the quality rows over the step's read position into its ring.  `tile` (index among the profile's tiles) is the lane's own.
// `whole`: the template as init() wants it (the totals of the read's start); `src`: as the steps read it (the same object, or its WaveFragmentSrc).
template <uint32_t MASK, int QB = RSQ_SCREEN_BATCH, int KEYS = kKeysAhead, class Whole, class Src, class Out>
__device__ void fill_wave_reads(const DevSim &S, RSQ_LDS float *img, uint32_t qbase, uint32_t seg, bool active, const Stream &st, uint32_t tile, uint32_t fragment_length,
                                const Whole &whole, const Src &src, Out &out, ReadMeta &meta) {
    ReadMachine m;
    if constexpr (MASK == 0) {
        const GlobalTables tab{S};
        if (active) {
            m.init(S, tab, st, seg, tile, fragment_length, whole);
            while (m.step(S, tab, st, src, out)) {}
        }
    } else {
        const uint32_t lane = threadIdx.x & 63u, n_items = lds_ring_items(S);
        RSQ_LDS float *ring = img + RSQ_PLAN(S, ring_off) + (threadIdx.x >> 6) * kRingRows * RSQ_PLAN(S, ring_stride);
        ScreenTables<MASK, QB, KEYS> tab{S, img, qbase, ring, 0u};
        m.idle();
        if (active) m.init(S, tab, st, seg, tile, fragment_length, whole);
        const RingItem mine = lds_ring_item(S, qbase, lane < n_items ? lane : 0u);      // the lane's first item (with one tile per image: its only one)
        // the lane's item of the NEXT step is loaded while this step runs (the row comes from L2: its latency would stand at the head of every step)
        Quad ahead = lane < n_items ? lds_ring_load(S, mine, 0u) : zero_quad();
        // What the wave does at the beginning of a step: its ring slot of the step (and the prefetch of the next), and the slot behind the ring for a read that has
        // lost more than kRingLag steps to deletions -- such a read no longer finds the rows over its position in the ring, and left to the double-precision call at
        // every step it would double the time of its wave's remaining steps (one read in 1600 with profile P0; the whole launch waits for such a wave when the call
        // is small).  The wave stages the rows over the first such read's position; another one at another position is rarer still.
        auto begin_step = [&](uint32_t t) {
            if (lane < n_items) {
                lds_ring_store(S, mine, ring, t, ahead);
                ahead = lds_ring_load(S, mine, t + 1u);
            }
            for (uint32_t item = lane + 64u; item < n_items; item += 64u) lds_ring_stage(S, qbase, ring, t, item);
            __builtin_amdgcn_wave_barrier();                 // the wave's LDS writes precede its reads (in order in hardware; this orders the compiler)
            tab.t = t;
            const uint64_t lagging = __builtin_amdgcn_ballot_w64(m.phase != ReadMachine::kDone && t - m.par.read_pos > kRingLag);
            tab.demand = 0xFFFFFFFFu;
            if (lagging) {
                const uint32_t p = __builtin_amdgcn_readlane(m.par.read_pos, __builtin_ctzll(lagging));
                if (lane < n_items) lds_ring_stage_demand(S, mine, ring, p);
                for (uint32_t item = lane + 64u; item < n_items; item += 64u) lds_ring_stage_demand(S, lds_ring_item(S, qbase, item), ring, p);
                __builtin_amdgcn_wave_barrier();
                tab.demand = p;
            }
        };
        uint32_t t = 0;
        // TWO loops.  While EVERY lane of the wave has a template base in front of it -- all but a chunk's last steps -- the step has no lane that sits it out, no
        // adapter and no tail: the iteration runs unmasked and compiled for the template part alone.  The second loop is the general one (lanes whose read is
        // complete or that have none return at once; phase changes; adapter and tail iterations).  One loop for both kept the read's state in two register sets with
        // moves between them around the "lane not running" join of EVERY step: 20.36 G -> 19.57 G vector instructions per launch of 10 M pairs, 216 -> 223 M pairs/s
        // (What did NOT move those copies, each measured on the device -- DESIGN_LOG.md section 11: tied asm operands on the state, both kinds of step behind a
        // wave-uniform branch inside ONE loop (11 % more instructions), the loop tested at its bottom, the phase changes behind a call.)
        for (; !wave_any(!m.in_template()); ++t) {
            begin_step(t);
            m.template iterate<true>(S, tab, st, src, out);
            __builtin_amdgcn_wave_barrier();
        }
        for (; wave_any(m.phase != ReadMachine::kDone); ++t) {      // a read is complete (or a lane has none) exactly when its machine is in kDone: a plain compare for the ballot
            begin_step(t);
            m.step(S, tab, st, src, out);                    // a lane whose read is complete (or that has none: phase kDone from the start) returns at once
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (active) {
        m.finalize(meta);
        out.finish(m.par.read_pos, m.par.iteration - m.hard_clip);      // every tail iteration (the iterations without an op) emits one of the hard_clip bases
    }
}

// The scheduler of the binned kernels.  The workgroup's first wave chooses the bin: the one with the most chunks left per workgroup on it (counting the
// newcomer), found by a strided scan of the bins' counters (the first choice: by the workgroup's number); the choice is left in the LDS words behind the image ([0] the bin or 0xFFFFFFFF: nothing
// left anywhere, [1] the bin whose image is staged).  chunk(img, qbase, seg, tile, place, active) runs the 64 items perm[place + lane] (place is wave-uniform).
template <uint32_t MASK, class Chunk>
__device__ void fill_binned_loop(const DevSim &S, float *lds_image, const FillBins &bins, Chunk &&chunk) {
    RSQ_LDS float *img = (RSQ_LDS float *)lds_image;
    RSQ_LDS uint32_t *sched = reinterpret_cast<RSQ_LDS uint32_t *>(img + (MASK ? RSQ_PLAN(S, total_words) : 0u));
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x == 0) sched[1] = 0xFFFFFFFFu;
    for (bool first_choice = true;; first_choice = false) {
        if (threadIdx.x < 64u) {
            uint64_t best = 0;
            if (first_choice) {
                // all workgroups choose at once and cannot see each other yet: workgroup g of G begins with the bin that holds chunk (g + 1/2) / G of all chunks,
                // so that the bins start with workgroups in proportion to their sizes
                const uint64_t total = bins.chunk_ptr[bins.n_bins], target = ((2u * (uint64_t)blockIdx.x + 1u) * total) / (2u * gridDim.x);
                uint32_t lo = 0, hi = bins.n_bins;                     // the last bin with chunk_ptr[bin] <= target
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (bins.chunk_ptr[mid] <= target) lo = mid;
                    else hi = mid;
                }
                best = total ? ((uint64_t)1 << 32) | (0xFFFFFFFFu - lo) : 0u;
            } else {
                // score = chunks left * 4096 / (workgroups on the bin + 1); ties go to the lower bin
                for (uint32_t b = lane; b < bins.n_bins; b += 64u) {
                    // other workgroups change these two with atomics while this one scans them: loads that go to the device-coherent level, not to this CU's vector cache
                    // (a stale "chunks left" would send the workgroup back to a used-up bin, from which it returns here)
                    const uint32_t n = (bins.bin_count[b] + 63u) / 64u, done = __hip_atomic_load(&bins.next_chunk[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                                   on_it = __hip_atomic_load(&bins.workers[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), left = done < n ? n - done : 0u;
                    const uint64_t score = (uint64_t)left * 4096u / (on_it + 1u), packed = (score << 32) | (0xFFFFFFFFu - b);
                    if (left && packed > best) best = packed;
                }
            }
            for (uint32_t d = 32; d; d >>= 1) {
                const uint64_t other = ((uint64_t)(uint32_t)__shfl_xor((int)(best >> 32), (int)d, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)best, (int)d, 64);
                best = other > best ? other : best;
            }
            if (lane == 0) {
                const uint32_t bin = best ? 0xFFFFFFFFu - (uint32_t)best : 0xFFFFFFFFu;
                sched[0] = bin;
                if (best) atomicAdd(&bins.workers[bin], 1u);
            }
        }
        __syncthreads();
        // what comes out of LDS is wave-uniform, but a vector register to the compiler: readfirstlane makes it scalar again (else every index derived
        // from the segment and the image becomes per-lane arithmetic)
        const uint32_t bin = (uint32_t)__builtin_amdgcn_readfirstlane((int)sched[0]);
        if (bin == 0xFFFFFFFFu) break;
        const uint32_t seg = bin / RSQ_SIM(S, n_tiles), tile = bin - seg * RSQ_SIM(S, n_tiles), qbase = image_qbase(S, seg, tile);
        if (bin != (uint32_t)__builtin_amdgcn_readfirstlane((int)sched[1])) {      // all read before anyone writes (barriers inside the staging)
            fill_stage_image<MASK>(S, lds_image, qbase);
            if (threadIdx.x == 0) sched[1] = bin;
        }
        const uint32_t first = bins.bin_first[bin], n_items = bins.bin_count[bin];
        for (;;) {
            uint32_t c = 0;
            if (lane == 0) c = atomicAdd(&bins.next_chunk[bin], 1u);
            c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
            if ((uint64_t)c * 64u >= n_items) break;
            chunk(img, qbase, seg, tile, first + c * 64u, c * 64u + lane < n_items);
        }
        __syncthreads();                                               // every wave is done with the bin
        if (threadIdx.x == 0) atomicSub(&bins.workers[bin], 1u);
    }
}

// one chunk of 64 pairs, mate `seg`: lane = row `row` of the segment's raw arrays if active.  Not binned: row = pair of the batch.  Binned: row = place in
// perm, the pair is perm[row] and its fragment record sorted[row] (a wave's rows are consecutive either way: 256-byte stores; k_format_write goes
// through perm as well); the pair index itself is read where it is needed, before and after the reads, and does not live through them.
template <uint32_t MASK, bool VAR, bool BINNED>
__device__ void fill_pair_chunk(const DevSim &S, const NameTable &names, RSQ_LDS float *img, uint32_t qbase, uint32_t seg, uint32_t bin_tile, uint64_t row, bool active,
                                const Fragment *frags, uint64_t n_pairs, uint64_t adapter_only_first, const RawLayout &raw, uint32_t *sizes, const FragmentVar *fvars,
                                const uint32_t *perm) {
    const uint64_t at = active ? row : 0u, r_out = (uint64_t)seg * n_pairs + at;
    Fragment f{};
    if (active && frags) f = frags[at];
    // the read's stream and template (CreateReads :634-721 / SimulateAdapterOnlyPairs :2359-2382)
    const bool from_fragment = frags != nullptr;
    FragmentVar fv{};
    if (VAR && active && fvars) fv = fvars[at];
    const bool need_pair = !from_fragment || raw.templates != nullptr;              // wave-uniform
    const uint64_t pair0 = BINNED ? (need_pair && active ? perm[at] : 0u) : at;
    const PairStream ps = pair_stream(from_fragment ? &f : nullptr, fv.sub, adapter_only_first + pair0);
    const Stream st{S.seed, ps.c0, ps.c1, ps.c2, pair_c3(kDomPair, ps.strand, seg, f.allele)};
    const uint32_t tile = BINNED ? bin_tile : (active ? draw_tile(S, ps.c0, ps.c1, ps.c2, pair_c3(kDomPair, ps.strand, 2, f.allele)) : 0u);
    ReadMeta meta;
    if constexpr (VAR) {                                            // launched for fragments only
        VariantSrc src = variant_src(S, f, fvars ? &fv : nullptr, seg);
        if (raw.templates) src.converted = raw.templates + ((uint64_t)seg * n_pairs + pair0) * raw.template_words;
        ReadOut out = raw.out_of(r_out);
        fill_wave_reads<MASK, RSQ_SCREEN_BATCH, kKeysFromStep>(S, img, qbase, seg, active, st, tile, f.len, src, src, out, meta);
    } else {
        // The kernel of the plain pairs carries the slim forms of cursor and template through its steps, and with the registers they leave it draws the quality
        // two quads at a time.  The kernels whose source walks per-lane state (variants above, records) have no registers to gain from them: compiled for P0
        // they trade the vector registers for scalar ones that spill in turn, and two quads at a time spill more than one (DESIGN_LOG.md section 23).
        FragmentSrc src = from_fragment && active ? fragment_src(S, f, seg) : FragmentSrc{S.ref_words, 0, 0, 0, false, S.sys_fwd, nullptr, nullptr};      // len 0 = empty template
        const uint64_t *templates = from_fragment ? raw.templates : nullptr;                          // wave-uniform
        const uint64_t template_at = ((uint64_t)seg * n_pairs + pair0) * raw.template_words;
        if (templates) src.converted = templates + template_at;
        const WaveFragmentSrc walk = wave_fragment_src(S, src, templates, template_at);
        WaveReadOut out = raw.wave_out_of(r_out);
        fill_wave_reads<MASK, kQualityBatchPairs, kKeysFromStep>(S, img, qbase, seg, active, st, tile, f.len, src, walk, out, meta);
    }
    if (active) {
        raw.meta[r_out] = meta;
        const uint64_t pair = BINNED ? perm[at] : at;
        sizes[(uint64_t)seg * n_pairs + pair] = record_size(S, names, from_fragment ? &f : nullptr, adapter_only_first + pair + 1u, meta, VAR && fvars ? &fv : nullptr);       // bytes of its FASTQ record
    }
}

template <uint32_t MASK, bool VAR, bool BINNED>
__device__ __forceinline__ void fill_reads_body(const DevSim &S, const NameTable &names, const Fragment *frags, uint64_t n_pairs, uint64_t adapter_only_first, const RawLayout &raw,
                                                uint32_t *sizes, uint32_t *chunk_counters, const FragmentVar *fvars, const FillBins &bins) {
    extern __shared__ __attribute__((aligned(16))) float lds_image[];
    if constexpr (BINNED) {
        fill_binned_loop<MASK>(S, lds_image, bins, [&](RSQ_LDS float *img, uint32_t qbase, uint32_t seg, uint32_t tile, uint32_t place, bool active) {
            fill_pair_chunk<MASK, VAR, true>(S, names, img, qbase, seg, tile, place + (threadIdx.x & 63u), active, frags ? bins.frags : nullptr, n_pairs, adapter_only_first, raw,
                                             sizes, fvars ? bins.fvars : nullptr, bins.perm);
        });
    } else {
        const uint32_t seg = blockIdx.x & 1u, qbase = image_qbase(S, seg, 0u);
        RSQ_LDS float *img = fill_stage_image<MASK>(S, lds_image, qbase);
        const uint32_t lane = threadIdx.x & 63u;
        for (;;) {
            uint32_t chunk = 0;
            if (lane == 0) chunk = atomicAdd(&chunk_counters[seg], 1u);
            chunk = __shfl(chunk, 0, 64);
            const uint64_t first = (uint64_t)chunk * 64u;                   // past the end: the wave is done
            if (first >= n_pairs) break;
            fill_pair_chunk<MASK, VAR, false>(S, names, img, qbase, seg, 0u, first + lane, first + lane < n_pairs, frags, n_pairs, adapter_only_first, raw, sizes, fvars, nullptr);
        }
    }
}
// the library's own instantiations (every shape of profile); a kernel compiled for one profile wraps the same body (rsq_spec.h)
template <uint32_t MASK, bool VAR = false, bool BINNED = false>
__global__ void __launch_bounds__(fill_block(VAR)) k_fill_reads(DevSim S, NameTable names, const Fragment *frags, uint64_t n_pairs, uint64_t adapter_only_first,
                                                          RawLayout raw, uint32_t *sizes, uint32_t *chunk_counters, const FragmentVar *fvars, FillBins bins) {
    fill_reads_body<MASK, VAR, BINNED>(S, names, frags, n_pairs, adapter_only_first, raw, sizes, chunk_counters, fvars, bins);
}

// seqToIllumina (ApplyErrorsAndQualityToFastaInput, Simulator.cpp:2403-2512) through the same workgroups: the records were
// partitioned by template segment (rec_index: segment-0 records first; rec_count[2] on the device), a workgroup serves one
// segment and its waves pull chunks of 64 records; or, BINNED, by (segment, tile) like the pairs.
struct RecordJob {
    uint64_t first_index;
    uint32_t read_len;
    const uint8_t *seqs, *dom, *rate;
    const uint32_t *frag_len;
    const uint32_t *rec_index, *rec_count;
    uint64_t n_records;
    // nullptr: record i is bytes [i * read_len, (i + 1) * read_len) of the arrays; else bytes [rec_at[i], rec_at[i] + rec_len[i]) of arrays of array_bytes bytes
    const uint32_t *rec_at, *rec_len;
    uint32_t array_bytes;
    // records parsed on the device (the PACKED kernels): a half-word per base at rec_at[i] of `codes` (array_bytes half-words), seqs / dom / rate unused
    const uint16_t *codes;
};
// lane = record i if active; `row`: its row of the raw arrays (i, or binned its place in perm: the text / array kernels go through perm as well)
template <uint32_t MASK, bool BINNED, bool PACKED>
__device__ void fill_record_chunk(const DevSim &S, const RecordJob &job, RSQ_LDS float *img, uint32_t qbase, uint32_t seg, uint32_t bin_tile, uint64_t i, uint64_t row, bool active,
                                  const RawLayout &raw) {
    const uint64_t idx = job.first_index + i;
    const Stream st{S.seed, (uint32_t)idx, (uint32_t)(idx >> 32), 0u, pair_c3(kDomErrModel, 0, seg)};
    ReadOut out = raw.out_of(active ? row : 0u);
    ReadMeta meta;
    const uint32_t tile = BINNED ? bin_tile : (active ? draw_tile(S, st.c0, st.c1, st.c2, pair_c3(kDomErrModel, 0, 2)) : 0u);
    if constexpr (PACKED) {
        const PackedRecordSrc src = packed_record_src(job.codes, job.rec_at[i], job.rec_len[i], job.array_bytes);
        fill_wave_reads<MASK>(S, img, qbase, seg, active, st, tile, job.frag_len[i], src, src, out, meta);
    } else {
        const RecordSrc src = job.rec_at ? record_src_at(job.seqs, job.dom, job.rate, job.rec_at[i], job.rec_len[i], job.array_bytes)
                                         : record_src(job.seqs, job.dom, job.rate, job.read_len, i, job.n_records);
        fill_wave_reads<MASK>(S, img, qbase, seg, active, st, tile, job.frag_len[i], src, src, out, meta);
    }
    if (active) raw.meta[row] = meta;
}
template <uint32_t MASK, bool BINNED, bool PACKED>
__device__ __forceinline__ void fill_records_body(const DevSim &S, const RecordJob &job, const RawLayout &raw, uint32_t *chunk_counters, const FillBins &bins) {
    extern __shared__ __attribute__((aligned(16))) float lds_image[];
    if constexpr (BINNED) {
        fill_binned_loop<MASK>(S, lds_image, bins, [&](RSQ_LDS float *img, uint32_t qbase, uint32_t seg, uint32_t tile, uint32_t place, bool active) {
            const uint32_t row = place + (threadIdx.x & 63u);
            fill_record_chunk<MASK, true, PACKED>(S, job, img, qbase, seg, tile, active ? bins.perm[row] : 0u, row, active, raw);
        });
    } else {
        const uint32_t seg = blockIdx.x & 1u, qbase = image_qbase(S, seg, 0u);
#if defined(RSQ_TRACE_FILL)      // measurements (exp/): when a workgroup began, had its image, and ended -- device clock, three words per workgroup behind the counters
        uint64_t *trace = reinterpret_cast<uint64_t *>(chunk_counters) + 2 + 4 * blockIdx.x;
        if (threadIdx.x == 0) trace[0] = wall_clock64();
#endif
        RSQ_LDS float *img = fill_stage_image<MASK>(S, lds_image, qbase);
#if defined(RSQ_TRACE_FILL)
        if (threadIdx.x == 0) trace[1] = wall_clock64();
#endif
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t n_mine = job.rec_count[seg];
        const uint32_t *index = job.rec_index + (seg ? job.rec_count[0] : 0u);
        for (;;) {
            uint32_t chunk = 0;
            if (lane == 0) chunk = atomicAdd(&chunk_counters[seg], 1u);
            chunk = __shfl(chunk, 0, 64);
            const uint64_t first = (uint64_t)chunk * 64u;                   // past the end: the wave is done
            if (first >= n_mine) break;
            const bool active = first + lane < n_mine;
            const uint32_t i = active ? index[first + lane] : 0u;
            fill_record_chunk<MASK, false, PACKED>(S, job, img, qbase, seg, 0u, i, i, active, raw);
#if defined(RSQ_TRACE_FILL)
            if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long *>(trace + 3), 1ull);      // chunks this workgroup ran
#endif
        }
#if defined(RSQ_TRACE_FILL)
        if (lane == 0) atomicMax(reinterpret_cast<unsigned long long *>(trace + 2), (unsigned long long)wall_clock64());      // the workgroup's last wave
#endif
    }
}
template <uint32_t MASK, bool BINNED = false, bool PACKED = false>
__global__ void __launch_bounds__(kFillBlockWalk) k_fill_records(DevSim S, RecordJob job, RawLayout raw, uint32_t *chunk_counters, FillBins bins) {
    fill_records_body<MASK, BINNED, PACKED>(S, job, raw, chunk_counters, bins);
}
#endif

}  // namespace rsq
