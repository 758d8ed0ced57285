// pileup_trial.cpp -- TEST-ONLY: the per-lane function of the truth pileup (reseq_amd/csrc/rsq_pileup.h pileup_mate, both instantiations) on the CPU, over crafted rows,
// a crafted fragment, a crafted allele and a crafted packed reference (truth_md_trial.cpp's input), into planes laid out as depth_trial.cpp lays out its array,
// beside the SAM records the same rows give (sam_record / SamVarFormat::record).  tests/test_truth_pileup.py builds it with g++ and requires that the planes are
// what its own reading of those records gives.
#include "truth_trial.h"

#include "../../reseq_amd/csrc/rsq_pileup.h"

extern "C" {
struct truth_md_in {           // as in truth_md_trial.cpp
    truth_trial_pair pair;
    uint32_t allele, num_alleles;
    uint32_t seq_len;             // of every sequence
    uint32_t n_variants;          // of the allele, sorted by position
    const uint32_t *var_pos, *var_len;
    int32_t has_fv;               // 0: no FragmentVar (no variants, or allele copies)
    uint32_t end, sub;
    int32_t start_var;
    uint32_t start_var_pos;
    int32_t end_var;
    uint32_t end_var_pos;
    const uint8_t *ref;           // seq_len base codes 0..3: every sequence's bases
};
}

// planes: (strands ? 16 : 8) planes of `words` >= 3 * (seq_len + 1) words, three sequences of seq_len bases each with its extra word (the caller zeroes them and may
// keep them over several calls); both mates are added.  sam / sizes: the two records of the pair (segment 0 first) and their sizes.  Returns the elements that
// fell outside their sequence, -1: a buffer is too small.
template <bool VARIANTS>
static int pileup_trial_of(const truth_md_in *vin, bool strands, uint32_t *planes, uint64_t plane_words, char *sam, uint32_t cap, uint32_t *sizes) {
    const truth_trial_pair *in = &vin->pair;
    constexpr uint32_t kSeqs = 3;
    if (plane_words < (uint64_t)kSeqs * (vin->seq_len + 1u)) return -1;
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
    std::vector<uint64_t> word_off(kSeqs, 0u), base_off;
    for (uint32_t s = 0; s < kSeqs; ++s) {
        base_off.push_back((uint64_t)s * vin->seq_len);
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
    S.seq_base_off = base_off.data();
    // the packed reference: one word more than the bases need, as upload_reference packs it; the bits behind the last base are set (they must not matter)
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
    f.len = in->len;
    f.strand = (uint8_t)in->strand;
    f.allele = VARIANTS ? (uint8_t)vin->allele : 0;
    f.block = in->block;
    f.number = in->number;
    const bool has_f = in->has_fragment != 0, has_fv = VARIANTS && has_f && vin->has_fv != 0;
    if (!has_f || f.seq >= kSeqs) return -1;                            // (a pair without a fragment never reaches k_pileup_add's part: adapter-only calls add nothing)
    const FragmentVar fv{vin->end, vin->sub, vin->start_var, vin->start_var_pos, vin->end_var, vin->end_var_pos};

    std::vector<uint32_t> seq[2], qual[2], ops[2];
    ReadMeta meta[2];
    for (int seg = 0; seg < 2; ++seg) {
        const truth_trial_mate &r = in->mate[seg];
        const uint32_t n_words = (r.read_len + 3u) / 4u, n_ops = r.n_iter_m + r.n_iter_s;
        seq[seg].assign(n_words + 8u, 0xA5A5A5A5u);                  // what lies behind a row's last character must not matter (md_seq_chunk takes eight words a round)
        qual[seg].assign(n_words + 8u, 0xA5A5A5A5u);
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
    // the pileup: a lane a mate, as k_pileup_add
    int bad = 0;
    for (uint32_t seg = 0; seg < 2u; ++seg)
        bad += (int)pileup_mate<VARIANTS>(S, f, has_fv, fv, seg, WordColumn{seq[seg].data(), 1}, WordColumn{ops[seg].data(), 1}, meta[seg], planes, plane_words, strands);
    // the records of the same mates
    uint32_t at = 0;
    if constexpr (VARIANTS) {
        const SamVarId id = sam_var_id(S, f, has_fv, fv);
        SamVarMate walk[2];
        uint32_t n_cigar[2];
        for (uint32_t seg = 0; seg < 2u; ++seg) walk[seg] = sam_var_walk(S, has_f, f, has_fv, fv, seg, WordColumn{ops[seg].data(), 1}, meta[seg], n_cigar[seg]);
        for (uint32_t seg = 0; seg < 2u; ++seg) {
            const WordColumn s{seq[seg].data(), 1}, q{qual[seg].data(), 1}, o{ops[seg].data(), 1};
            const SamAlign a = sam_var_align(has_f, f, seg, walk[0], walk[1]);
            const SamVarMate e = SamVarFormat::mate(S, names, has_f, f, id, in->adapter_only_number, meta[seg], o, walk[seg], n_cigar[seg], a);
            if (at + SamVarFormat::bytes(e) > cap) return -1;
            sizes[seg] = SamVarFormat::record(S, names, has_f, f, id, in->adapter_only_number, meta[seg], s, q, o, e, a, sam + at);
            at += sizes[seg];
        }
    } else {
        SamMate walk[2];
        for (uint32_t seg = 0; seg < 2u; ++seg) walk[seg] = sam_walk(WordColumn{ops[seg].data(), 1}, meta[seg]);
        for (uint32_t seg = 0; seg < 2u; ++seg) {
            const WordColumn s{seq[seg].data(), 1}, q{qual[seg].data(), 1}, o{ops[seg].data(), 1};
            const SamAlign a = sam_align(has_f, f, seg, walk[0], walk[1]);
            if (at + sam_record_size(S, names, has_f, f, in->adapter_only_number, meta[seg], walk[seg], a) > cap) return -1;
            sizes[seg] = sam_record(S, names, has_f, f, in->adapter_only_number, meta[seg], s, q, o, walk[seg], a, sam + at);
            at += sizes[seg];
        }
    }
    return bad;
}

extern "C" int pileup_trial(const truth_md_in *in, int variants, int strands, uint32_t *planes, uint64_t plane_words, char *sam, uint32_t cap, uint32_t *sizes) {
    return variants ? pileup_trial_of<true>(in, strands != 0, planes, plane_words, sam, cap, sizes) : pileup_trial_of<false>(in, strands != 0, planes, plane_words, sam, cap, sizes);
}
// the full counts of a position from the eight plane words of each strand set (pileup_row), and whether the row has a line (pileup_keep)
extern "C" int pileup_row_trial(const uint32_t *in, uint32_t sets, uint32_t ref, int all, uint32_t *v) {
    for (uint32_t s = 0; s < sets; ++s) pileup_row(in + s * kPileupPlanes, ref, v + s * kPileupPlanes);
    return pileup_keep(v, sets, ref, all != 0) ? 1 : 0;
}
// a line as k_pileup_text's lanes write it (an ImageSink into a zeroed image, at an unaligned place) and its stated size; returns the bytes written, -1 if they
// differ from the same line through the plain sink or touch what lies around them
extern "C" int pileup_line_trial(const char *names, const uint32_t *name_ptr, uint32_t seq, uint32_t pos, uint32_t ref, const uint32_t *v, uint32_t sets, uint32_t at, char *out,
                                 uint32_t cap) {
    NameTable t{};
    t.names = names;
    t.name_ptr = name_ptr;
    const uint32_t size = pileup_line_size(name_ptr[seq + 1] - name_ptr[seq], pos, v, sets);
    if (at + size + 8u > cap) return -1;
    std::vector<uint32_t> image((at + size) / 4u + 2u, 0u);
    ImageSink lane(reinterpret_cast<RSQ_LDS char *>(image.data()) + at);
    pileup_line(t, seq, pos, ref, v, sets, lane);
    lane.finish();
    TextSink plain(out, 0);
    pileup_line(t, seq, pos, ref, v, sets, plain);
    if (lane.n != size || plain.n != size || memcmp(reinterpret_cast<const char *>(image.data()) + at, out, size) != 0) return -1;
    for (uint32_t i = 0; i < 4u * image.size(); ++i)
        if ((i < at || i >= at + size) && reinterpret_cast<const char *>(image.data())[i]) return -1;
    const uint32_t lds = pileup_lds_bytes(name_ptr[seq + 1] - name_ptr[seq], sets);
    if (lds < kPileupLdsMax && (uint64_t)kPileupLines * size + 16u > lds) return -1;       // 64 lines of any size fit an image that is not capped
    return (int)size;
}
