// stats_trial.cpp -- TEST-ONLY: the per-lane functions of the simulation report (reseq_amd/csrc/rsq_stats.h) on the CPU.
//   stats_rows_trial   stats_row_lane looped over crafted word-major rows the way k_stats_rows loops it: workgroups over (segment, chunk) units and slabs, a wave's
//                      64 reads a lane each, with the kernel's skew, a 32-bit image per workgroup flushed into the 64-bit counters.
//   stats_mates_trial  stats_mate, both instantiations, over a crafted pair (truth_md_trial.cpp's input: rows, a fragment, an allele, a packed reference) beside the
//                      SAM records with NM and MD that the same rows give.
// tests/test_sim_stats.py builds it with g++ and compares every table with tests/sim_stats.py's statements.
#include "truth_trial.h"

#include "../../reseq_amd/csrc/rsq_stats.h"

extern "C" {
struct truth_md_in {          // as in truth_md_trial.cpp
    truth_trial_pair pair;
    uint32_t allele, num_alleles;
    uint32_t seq_len;
    uint32_t n_variants;
    const uint32_t *var_pos, *var_len;
    int32_t has_fv;
    uint32_t end, sub;
    int32_t start_var;
    uint32_t start_var_pos;
    int32_t end_var;
    uint32_t end_var_pos;
    const uint8_t *ref;
};
}

// the layout: off[t], and {segments, dim0, dim1} per table; returns the words of the array
extern "C" uint32_t stats_trial_layout(uint32_t len0, uint32_t len1, uint32_t F, uint32_t Q, uint32_t T, uint32_t phred, uint32_t lds_bytes, uint32_t *off, uint32_t *dims,
                                       uint32_t *image_words) {
    const StatsLayout y = stats_layout(len0, len1, F, Q, T, phred, lds_bytes);
    for (uint32_t t = 0; t < kStTables; ++t) {
        off[t] = y.off[t];
        dims[3u * t] = y.segments(t);
        dims[3u * t + 1u] = y.dim0(t);
        dims[3u * t + 2u] = y.dim1(t);
    }
    *image_words = y.image_words;
    return y.words;
}

// the rows kernel's geometry as the library chooses it (options 0: its own choice) -> out = {chunk, slab, units of segment 0, of segment 1, lds, groups}
extern "C" void stats_trial_geometry(uint32_t lmax, uint32_t len0, uint32_t len1, uint32_t Q, int32_t skew, uint32_t row_words, uint32_t n_cu, uint64_t n_pairs, int64_t opt_chunk,
                                     int64_t opt_slab, int64_t opt_groups, uint32_t *out) {
    const StatsRowsGeometry g = stats_rows_geometry(lmax, len0, len1, Q, skew != 0, row_words, n_cu, n_pairs, opt_chunk, opt_slab, opt_groups);
    const uint32_t v[6] = {g.plan.chunk, g.plan.slab, g.plan.units[0], g.plan.units[1], g.lds, g.groups};
    for (uint32_t i = 0; i < 6u; ++i) out[i] = v[i];
}
// ... for every Q in [1, q_hi], lmax in [1, l_hi] and both forms (len0 = lmax, len1 = lmax / 2): out[((Q - 1) * l_hi + lmax - 1) * 2 + skew][6]
extern "C" void stats_trial_geometry_table(uint32_t q_hi, uint32_t l_hi, uint32_t n_cu, uint64_t n_pairs, uint32_t *out) {
    for (uint32_t Q = 1; Q <= q_hi; ++Q)
        for (uint32_t lmax = 1; lmax <= l_hi; ++lmax)
            for (int32_t skew = 0; skew < 2; ++skew, out += 6) stats_trial_geometry(lmax, lmax, lmax / 2u, Q, skew, (lmax + 3u) / 4u, n_cu, n_pairs, 0, 0, 0, out);
}

struct RowSrc {
    const uint32_t *s, *q;
    uint64_t pitch;
    uint32_t seq(uint32_t j) const { return s[(uint64_t)j * pitch]; }
    uint32_t qual(uint32_t j) const { return q[(uint64_t)j * pitch]; }
};
struct ImageAdd {
    std::vector<uint32_t> &image;
    int32_t &outside;
    void operator()(uint32_t i) {
        if (i < image.size()) ++image[i];
        else ++outside;
    }
};
// seq, qual: [row_words][pitch]; read_len: [2 n_pairs].  counts: the layout's words (added to).  Returns the additions that fell outside a workgroup's image (0).
extern "C" int32_t stats_rows_trial(const uint32_t *seq, const uint32_t *qual, const uint16_t *read_len, uint64_t pitch, uint64_t n_pairs, uint32_t row_words, uint32_t len0,
                                    uint32_t len1, uint32_t Q, uint32_t phred, uint32_t chunk, uint32_t slab, uint32_t G, int32_t skew, uint64_t *counts) {
    const StatsLayout y = stats_layout(len0, len1, 10u, Q, 1u, phred);
    const StatsRowsPlan plan{chunk, slab, {stats_chunks(len0, chunk), stats_chunks(len1, chunk)}, row_words};
    const uint32_t stride = stats_row_stride(Q), n_units = plan.units[0] + plan.units[1];
    const uint64_t n_slabs = (n_pairs + slab - 1u) / slab;
    int32_t outside = 0;
    uint64_t bad = 0;
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t k = g / n_units, K = (G - 1u - g % n_units) / n_units + 1u;
        for (uint32_t unit = g % n_units; unit < n_units; unit += G) {
            const uint32_t seg = unit >= plan.units[0] ? 1u : 0u, p0 = (unit - seg * plan.units[0]) * chunk, L = y.len[seg];
            const uint32_t positions = L - p0 < chunk ? L - p0 : chunk, w_lo = p0 / 4u, w_n = (positions + 3u) / 4u;
            std::vector<uint32_t> image((size_t)chunk * stride, 0u);
            ImageAdd add{image, outside};
            for (uint64_t sl = k; sl < n_slabs; sl += K) {
                const uint64_t lo = sl * slab, hi = lo + slab < n_pairs ? lo + slab : n_pairs;
                for (uint64_t base = lo; base < hi; base += 64u)
                    for (uint32_t lane = 0; lane < 64u && base + lane < hi; ++lane) {
                        const uint64_t r = seg * n_pairs + base + lane;
                        uint32_t len = read_len[r];
                        if (len > L) len = L;
                        if (len > 4u * row_words) len = 4u * row_words;
                        const RowSrc src{seq + (uint64_t)w_lo * pitch + r, qual + (uint64_t)w_lo * pitch + r, pitch};
                        bad += stats_row_lane(src, len, w_lo, w_n, skew ? lane % w_n : 0u, Q, stride, phred, add);
                    }
            }
            for (uint32_t i = 0; i < positions * stride; ++i) {
                const uint32_t v = image[i], p = i / stride, c = i - p * stride;
                if (!v) continue;
                if (c < Q) counts[y.off[kStBaseQuality] + ((uint64_t)seg * y.lmax + p0 + p) * Q + c] += v;
                else if (c < Q + 5u) counts[y.off[kStBaseCall] + ((uint64_t)seg * y.lmax + p0 + p) * 5u + (c - Q)] += v;
                else ++outside;
            }
            for (uint32_t i = positions * stride; i < image.size(); ++i)
                if (image[i]) ++outside;
        }
    }
    counts[y.off[kStBad]] += bad;
    return outside;
}

struct CountsAdd {
    uint64_t *c;
    void add(uint32_t i, uint32_t v) { c[i] += v; }
    void shared(uint32_t i, bool on) {
        if (on) ++c[i];
    }
};

// counts: the words of stats_layout(len0, len1, F, Q, 1, the pair's offset) (added to).  sam / sizes: the pair's two records with NM and MD.  -1: a buffer is too small.
template <bool VARIANTS>
static int stats_mates_trial_of(const truth_md_in *vin, uint32_t len0, uint32_t len1, uint32_t F, uint32_t Q, uint64_t *counts, char *sam, uint32_t cap, uint32_t *sizes) {
    using Format = typename std::conditional<VARIANTS, SamVarMdFormat, SamMdFormat>::type;
    const truth_trial_pair *in = &vin->pair;
    constexpr uint32_t kSeqs = 3;
    DevSim S{};
    const uint16_t tiles[1] = {(uint16_t)in->tile};
    S.tiles = tiles;
    S.phred_offset = (uint8_t)in->phred_offset;
    S.num_alleles = VARIANTS ? vin->num_alleles : 1u;
    S.n_seqs = kSeqs;
    S.variants_loaded = !VARIANTS ? 0u : vin->has_fv ? 2u : 1u;
    const uint32_t n = VARIANTS ? vin->n_variants : 0u;
    std::vector<DevVariant> variants;
    std::vector<AlleleVar> map;
    std::vector<uint32_t> var_ptr{0u}, map_ptr{0u}, seq_len(kSeqs, vin->seq_len);
    std::vector<uint64_t> word_off(kSeqs, 0u);
    for (uint32_t s = 0; s < kSeqs; ++s) {
        for (uint32_t i = 0; i < n; ++i) variants.push_back(DevVariant{vin->var_pos[i], vin->var_len[i], 0u, 0u, {~0ull, ~0ull}});
        var_ptr.push_back((uint32_t)variants.size());
    }
    for (uint32_t m = 0; m < kSeqs * S.num_alleles; ++m) {
        int32_t shift = 0;
        for (uint32_t i = 0; i < n; ++i) {
            map.push_back(AlleleVar{vin->var_pos[i], i, shift, 0});
            shift += (int32_t)vin->var_len[i] - 1;
        }
        map.push_back(AlleleVar{vin->seq_len, n, shift, 0});
        map_ptr.push_back((uint32_t)map.size());
    }
    S.variants = variants.data();
    S.var_ptr = var_ptr.data();
    S.allele_map = map.data();
    S.allele_map_ptr = map_ptr.data();
    S.seq_len = seq_len.data();
    S.seq_word_off = word_off.data();
    std::vector<uint64_t> words((vin->seq_len + 31u) / 32u + 1u, ~0ull);
    for (uint32_t p = 0; p < vin->seq_len; ++p) words[p >> 5] = (words[p >> 5] & ~(3ull << (2u * (p & 31u)))) | ((uint64_t)(vin->ref[p] & 3u) << (2u * (p & 31u)));
    S.ref_words = words.data();

    NameTable names{};
    names.names = in->names;
    names.name_ptr = in->name_ptr;
    names.base_len = (uint32_t)strlen(in->base_identifier);
    if (names.base_len > sizeof names.base_identifier) return -1;
    memcpy(names.base_identifier, in->base_identifier, names.base_len);
    Fragment f{};
    f.seq = in->seq;
    f.start = in->start;
    f.len = in->has_fragment ? in->len : 0u;
    f.strand = (uint8_t)in->strand;
    f.allele = VARIANTS ? (uint8_t)vin->allele : 0;
    f.block = in->block;
    f.number = in->number;
    const bool has_f = in->has_fragment != 0, has_fv = VARIANTS && has_f && vin->has_fv != 0;
    if (has_f && f.seq >= kSeqs) return -1;
    const FragmentVar fv{vin->end, vin->sub, vin->start_var, vin->start_var_pos, vin->end_var, vin->end_var_pos};

    std::vector<uint32_t> seq[2], qual[2], ops[2];
    ReadMeta meta[2];
    for (int seg = 0; seg < 2; ++seg) {
        const truth_trial_mate &r = in->mate[seg];
        const uint32_t n_words = (r.read_len + 3u) / 4u, n_ops = r.n_iter_m + r.n_iter_s;
        seq[seg].assign(n_words + 1u, 0xA7A7A7A7u);                  // what lies behind a row's last character must not matter
        qual[seg].assign(n_words + 1u, 0xA7A7A7A7u);
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
    }
    // the report: a lane a mate, as k_stats_mates
    const StatsLayout y = stats_layout(len0, len1, F, Q, 1u, in->phred_offset);
    CountsAdd a{counts};
    uint64_t bad = 0;
    for (uint32_t seg = 0; seg < 2u; ++seg)
        bad += stats_mate<VARIANTS>(S, y, true, f, has_fv, fv, seg, WordColumn{seq[seg].data(), 1}, WordColumn{ops[seg].data(), 1}, meta[seg], a);
    counts[y.off[kStBad]] += bad;
    // the records of the same mates
    uint32_t at = 0;
    if constexpr (VARIANTS) {
        const SamVarId id = sam_var_id(S, f, has_fv, fv);
        SamVarMate walk[2];
        uint32_t n_cigar[2];
        for (uint32_t seg = 0; seg < 2u; ++seg) walk[seg] = sam_var_walk(S, has_f, f, has_fv, fv, seg, WordColumn{ops[seg].data(), 1}, meta[seg], n_cigar[seg]);
        for (uint32_t seg = 0; seg < 2u; ++seg) {
            const WordColumn s{seq[seg].data(), 1}, q{qual[seg].data(), 1}, o{ops[seg].data(), 1};
            const SamAlign al = sam_var_align(has_f, f, seg, walk[0], walk[1]);
            const typename Format::Mate e = Format::mate(S, names, has_f, f, id, in->adapter_only_number, meta[seg], s, o, walk[seg], n_cigar[seg], al);
            if (at + Format::bytes(e) > cap) return -1;
            sizes[seg] = Format::record(S, names, has_f, f, id, in->adapter_only_number, meta[seg], s, q, o, e, al, sam + at);
            at += sizes[seg];
        }
    } else {
        SamMate walk[2];
        for (uint32_t seg = 0; seg < 2u; ++seg) walk[seg] = sam_walk(WordColumn{ops[seg].data(), 1}, meta[seg]);
        for (uint32_t seg = 0; seg < 2u; ++seg) {
            const WordColumn s{seq[seg].data(), 1}, q{qual[seg].data(), 1}, o{ops[seg].data(), 1};
            const SamAlign al = sam_align(has_f, f, seg, walk[0], walk[1]);
            const typename Format::Mate e = Format::mate(S, names, has_f, f, in->adapter_only_number, meta[seg], s, o, walk[seg], al);
            if (at + Format::bytes(e) > cap) return -1;
            sizes[seg] = Format::record(S, names, has_f, f, in->adapter_only_number, meta[seg], s, q, o, e, al, sam + at);
            at += sizes[seg];
        }
    }
    return 0;
}

extern "C" int stats_mates_trial(const truth_md_in *in, int variants, uint32_t len0, uint32_t len1, uint32_t F, uint32_t Q, uint64_t *counts, char *sam, uint32_t cap, uint32_t *sizes) {
    return variants ? stats_mates_trial_of<true>(in, len0, len1, F, Q, counts, sam, cap, sizes) : stats_mates_trial_of<false>(in, len0, len1, F, Q, counts, sam, cap, sizes);
}
