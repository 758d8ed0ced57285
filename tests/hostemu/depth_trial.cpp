// depth_trial.cpp -- TEST-ONLY: the per-lane function of the truth depth (reseq_amd/csrc/rsq_depth.h depth_mate, both instantiations) on the CPU, over crafted rows,
// a crafted fragment and -- for the instantiation with variants -- a crafted allele (truth_var_trial.cpp's input: the allele's variants as (position, length of the
// replacement), a FragmentVar), beside the SAM records the same rows give (sam_record / SamVarFormat::record).  tests/test_truth_depth.py builds it with g++ and
// requires that the prefix sum of the differences is the depth its own reading of those records gives.
#include "truth_trial.h"

#include "../../reseq_amd/csrc/rsq_depth.h"

extern "C" {
struct truth_var_in {          // as in truth_var_trial.cpp
    truth_trial_pair pair;
    uint32_t allele, num_alleles;
    uint32_t seq_len;             // of every sequence
    uint32_t n_variants;          // of the allele, sorted by position
    const uint32_t *var_pos, *var_len;
    int32_t has_fv;               // 0: allele copies (substitutions only), no FragmentVar
    uint32_t end, sub;
    int32_t start_var;
    uint32_t start_var_pos;
    int32_t end_var;
    uint32_t end_var_pos;
};
}

// diff: 3 * (seq_len + 1) words, the run's array of three sequences of seq_len bases (the caller zeroes it and may keep it over several calls); both mates' differences are
// added to it.  sam / sizes: the two records of the pair (segment 0 first) and their sizes.  Returns the elements that fell outside their sequence, -1: a buffer is too small.
template <bool VARIANTS>
static int depth_trial_of(const truth_var_in *vin, uint32_t *diff, char *sam, uint32_t cap, uint32_t *sizes) {
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
    if (!has_f || f.seq >= kSeqs) return -1;                            // (a pair without a fragment never reaches k_depth_add's part: adapter-only calls add nothing)
    const FragmentVar fv{vin->end, vin->sub, vin->start_var, vin->start_var_pos, vin->end_var, vin->end_var_pos};

    std::vector<uint32_t> seq[2], qual[2], ops[2];
    ReadMeta meta[2];
    for (int seg = 0; seg < 2; ++seg) {
        const truth_trial_mate &r = in->mate[seg];
        const uint32_t words = (r.read_len + 3u) / 4u, n_ops = r.n_iter_m + r.n_iter_s;
        seq[seg].assign(words + 1u, 0xA5A5A5A5u);
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
    }
    // the depth: a lane a mate, as k_depth_add
    int bad = 0;
    for (uint32_t seg = 0; seg < 2u; ++seg) bad += (int)depth_mate<VARIANTS>(S, f, has_fv, fv, seg, WordColumn{ops[seg].data(), 1}, meta[seg], diff);
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

extern "C" int depth_trial(const truth_var_in *in, int variants, uint32_t *diff, char *sam, uint32_t cap, uint32_t *sizes) {
    return variants ? depth_trial_of<true>(in, diff, sam, cap, sizes) : depth_trial_of<false>(in, diff, sam, cap, sizes);
}
// a bedGraph line as k_depth_text's lanes write it (an ImageSink into a zeroed image, at an unaligned place) and its stated size; returns the bytes written, -1 if they
// differ from the same line through the plain sink
extern "C" int depth_line_trial(const char *names, const uint32_t *name_ptr, uint32_t seq, uint32_t start, uint32_t end, uint32_t depth, uint32_t at, char *out, uint32_t cap) {
    NameTable t{};
    t.names = names;
    t.name_ptr = name_ptr;
    const uint32_t size = depth_line_size(name_ptr[seq + 1] - name_ptr[seq], start, end, depth);
    if (at + size + 8u > cap) return -1;
    std::vector<uint32_t> image((at + size) / 4u + 2u, 0u);
    ImageSink lane(reinterpret_cast<RSQ_LDS char *>(image.data()) + at);
    depth_line(t, seq, start, end, depth, lane);
    lane.finish();
    TextSink plain(out, 0);
    depth_line(t, seq, start, end, depth, plain);
    if (lane.n != size || plain.n != size || memcmp(reinterpret_cast<const char *>(image.data()) + at, out, size) != 0) return -1;
    return (int)size;
}
