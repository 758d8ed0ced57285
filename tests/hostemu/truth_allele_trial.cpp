// truth_allele_trial.cpp -- TEST-ONLY: the per-lane functions of the truth alignments in ALLELE coordinates (rsq_sam.h SamAlleleFormat, rsq_bam.h BamAlleleFormat:
// sam_allele_span, sam_allele_walk, the formats' mate / head / tail / record) on the CPU, over the input of truth_var_trial.cpp -- an allele the caller crafts as
// (position, length of the replacement), a crafted Fragment and FragmentVar, crafted rows -- and under that trial's entry point and signature, so that
// tests/test_truth_variants.py's run_var_pair drives either.  tests/test_alleles.py builds it with g++ and compares both formats' records with its statement: the
// plain record of tests/test_truth_sam.py with the fragment moved to its place in the allele spelled out base by base.
#include "truth_trial.h"

extern "C" {
struct truth_var_in {
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

// As truth_trial; placed[seg] = {hs, he, 0 (no columns are walked), POS - 1, reference bases}.
template <class Format>
static int truth_var_trial_of(const truth_var_in *vin, char *fastq0, char *fastq1, char *out, uint32_t at, uint32_t cap, uint32_t *sizes, uint32_t *placed) {
    const truth_trial_pair *in = &vin->pair;
    constexpr uint32_t kSeqs = 3;
    DevSim S{};
    const uint16_t tiles[1] = {(uint16_t)in->tile};
    S.tiles = tiles;
    S.phred_offset = (uint8_t)in->phred_offset;
    S.num_alleles = vin->num_alleles;
    S.n_seqs = kSeqs;
    S.variants_loaded = vin->has_fv ? 2u : 1u;
    // every sequence, every allele: the same variants and the same map
    const uint32_t n = vin->n_variants;
    std::vector<DevVariant> variants;
    std::vector<AlleleVar> map;
    std::vector<uint32_t> var_ptr{0u}, map_ptr{0u}, seq_len(kSeqs, vin->seq_len);
    std::vector<uint64_t> word_off(kSeqs, 0u);
    for (uint32_t s = 0; s < kSeqs; ++s) {
        for (uint32_t i = 0; i < n; ++i) variants.push_back(DevVariant{vin->var_pos[i], vin->var_len[i], 0u, 0u, {~0ull, ~0ull}});
        var_ptr.push_back((uint32_t)variants.size());
    }
    for (uint32_t m = 0; m < kSeqs * vin->num_alleles; ++m) {
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
    f.allele = (uint8_t)vin->allele;
    f.block = in->block;
    f.number = in->number;
    const bool has_f = in->has_fragment != 0, has_fv = has_f && vin->has_fv != 0;
    if (has_f && f.seq >= kSeqs) return -1;
    const FragmentVar fv{vin->end, vin->sub, vin->start_var, vin->start_var_pos, vin->end_var, vin->end_var_pos};
    const SamVarId id = sam_var_id(S, f, has_fv, fv);

    std::vector<uint32_t> seq[2], qual[2], ops[2];
    ReadMeta meta[2];
    SamVarMate walk[2];
    uint32_t n_cigar[2];
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
        n_cigar[seg] = 0;
    }
    const AlleleSpan span = sam_allele_span(S, has_f, f, has_fv, fv);
    for (int seg = 0; seg < 2; ++seg) {
        walk[seg] = sam_allele_walk(has_f, f, span, (uint32_t)seg, WordColumn{ops[seg].data(), 1}, meta[seg]);
        const uint32_t p[5] = {span.hs, span.he, walk[seg].w.pad, walk[seg].pos, walk[seg].ref_bases};
        memcpy(placed + 5 * seg, p, sizeof p);
    }
    for (int seg = 0; seg < 2; ++seg) {
        const ReadMeta &m = meta[seg];
        const WordColumn s{seq[seg].data(), 1}, q{qual[seg].data(), 1}, o{ops[seg].data(), 1};
        if (record_size(S, names, has_f, f, in->adapter_only_number, m, has_fv, fv) > cap) return -1;
        sizes[seg] = format_record(S, names, has_f, f, in->adapter_only_number, m, s, q, o, seg ? fastq1 : fastq0, has_fv, fv);
        const SamAlign a = sam_var_align(has_f, f, (uint32_t)seg, walk[0], walk[1]);
        const typename Format::Mate e = Format::mate(S, names, has_f, f, id, in->adapter_only_number, m, o, walk[seg], n_cigar[seg], a);
        sizes[4 + seg] = Format::bytes(e);
        if (at + sizes[4 + seg] > cap) return -1;
        sizes[2 + seg] = Format::record(S, names, has_f, f, id, in->adapter_only_number, m, s, q, o, e, a, out + at);
        // the writer's lane roles on the host: half 0 the head, half 1 the tail, at the same unaligned place of a zeroed image
        std::vector<uint32_t> image((at + sizes[2 + seg]) / 4u + 2u, 0u);
        RSQ_LDS char *text = reinterpret_cast<RSQ_LDS char *>(image.data()) + at;
        ImageSink head(text);
        Format::head(S, names, has_f, f, id, in->adapter_only_number, m, s, o, e, a, head);
        head.finish();
        ImageSink tail(text + Format::tail_at(e, m, id));
        Format::tail(S, m, id, q, o, a, tail);
        tail.finish();
        if (head.n + tail.n != sizes[2 + seg] || memcmp(text, out + at, sizes[2 + seg]) != 0) return -2;
        for (uint32_t i = 0; i < 4u * image.size(); ++i)
            if ((i < at || i >= at + sizes[2 + seg]) && reinterpret_cast<const char *>(image.data())[i]) return -2;
        at += sizes[2 + seg];
    }
    return 0;
}

extern "C" int truth_var_trial(const truth_var_in *in, int bam, char *fastq0, char *fastq1, char *out, uint32_t at, uint32_t cap, uint32_t *sizes, uint32_t *placed) {
    return bam ? truth_var_trial_of<BamAlleleFormat>(in, fastq0, fastq1, out, at, cap, sizes, placed) : truth_var_trial_of<SamAlleleFormat>(in, fastq0, fastq1, out, at, cap, sizes, placed);
}
