// truth_md_trial.cpp -- TEST-ONLY: the per-lane functions of the truth alignments with NM:i and MD:Z (rsq_md.h MdFormat over the four formats of rsq_sam.h and
// rsq_bam.h) on the CPU: crafted rows (truth_trial.h's input), a crafted Fragment, a crafted allele as in truth_var_trial.cpp -- its variants as (position, length
// of the replacement) -- and a crafted reference, packed here 32 bases a word as the device holds it.  The same trial writes the records of the format without the
// tags, so that tests/test_truth_md.py can take the tags off and compare byte for byte; it checks the tags against `md_nm` (tests/truth_md.py) applied to the
// record's own POS, CIGAR and SEQ.
#include "truth_trial.h"
#include "../../reseq_amd/csrc/rsq_md.h"

extern "C" {
struct truth_md_in {
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

// As truth_trial: the two records at out + at, sizes = {fastq 0, fastq 1, record 0, record 1} as written and the two sizes Format::mate states.  -1: a buffer is
// too small.  -2: the records written as k_truth_write's lanes write them -- head and tail through an ImageSink each into a zeroed image, the tail at
// Format::tail_at -- differ from Format::record's bytes, or touch what lies around them.
template <class Format>
static int truth_md_trial_of(const truth_md_in *vin, char *fastq0, char *fastq1, char *out, uint32_t at, uint32_t cap, uint32_t *sizes) {
    const truth_trial_pair *in = &vin->pair;
    constexpr uint32_t kSeqs = 3;
    DevSim S{};
    const uint16_t tiles[1] = {(uint16_t)in->tile};
    S.tiles = tiles;
    S.phred_offset = (uint8_t)in->phred_offset;
    S.num_alleles = vin->num_alleles;
    S.n_seqs = kSeqs;
    S.variants_loaded = !Format::kVariants ? 0u : vin->has_fv ? 2u : 1u;
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
    f.allele = (uint8_t)vin->allele;
    f.block = in->block;
    f.number = in->number;
    const bool has_f = in->has_fragment != 0, has_fv = Format::kVariants && has_f && vin->has_fv != 0;
    if (has_f && f.seq >= kSeqs) return -1;
    const FragmentVar fv{vin->end, vin->sub, vin->start_var, vin->start_var_pos, vin->end_var, vin->end_var_pos};
    const SamVarId id = sam_var_id(S, f, has_fv, fv);

    std::vector<uint32_t> seq[2], qual[2], ops[2];
    ReadMeta meta[2];
    SamMate walk[2];
    SamVarMate var_walk[2];
    uint32_t n_cigar[2] = {0u, 0u};
    for (int seg = 0; seg < 2; ++seg) {
        const truth_trial_mate &r = in->mate[seg];
        const uint32_t n_words = (r.read_len + 3u) / 4u, n_ops = r.n_iter_m + r.n_iter_s;
        seq[seg].assign(n_words + 1u, 0xA5A5A5A5u);                  // what lies behind a row's last character must not matter
        qual[seg].assign(n_words + 1u, 0xA5A5A5A5u);
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
        if constexpr (Format::kVariants) var_walk[seg] = sam_var_walk(S, has_f, f, has_fv, fv, (uint32_t)seg, WordColumn{ops[seg].data(), 1}, m, n_cigar[seg]);
        else walk[seg] = sam_walk(WordColumn{ops[seg].data(), 1}, m);
    }
    for (int seg = 0; seg < 2; ++seg) {
        const ReadMeta &m = meta[seg];
        const WordColumn s{seq[seg].data(), 1}, q{qual[seg].data(), 1}, o{ops[seg].data(), 1};
        if (record_size(S, names, has_f, f, in->adapter_only_number, m, has_fv, fv) > cap) return -1;
        sizes[seg] = format_record(S, names, has_f, f, in->adapter_only_number, m, s, q, o, seg ? fastq1 : fastq0, has_fv, fv);
        std::vector<uint32_t> image;
        uint32_t image_bytes = 0;
        auto lanes = [&](auto head_part, auto tail_part, uint32_t tail_at) {      // the writer's lane roles: half 0 the head, half 1 the tail, at the same unaligned place
            image.assign((at + sizes[2 + seg]) / 4u + 2u, 0u);
            RSQ_LDS char *text = reinterpret_cast<RSQ_LDS char *>(image.data()) + at;
            ImageSink head(text);
            head_part(head);
            head.finish();
            ImageSink tail(text + tail_at);
            tail_part(tail);
            tail.finish();
            image_bytes = head.n + tail.n;
        };
        if constexpr (Format::kVariants) {
            const SamAlign a = sam_var_align(has_f, f, (uint32_t)seg, var_walk[0], var_walk[1]);
            typename Format::Mate e;
            if constexpr (Format::kMd) e = Format::mate(S, names, has_f, f, id, in->adapter_only_number, m, s, o, var_walk[seg], n_cigar[seg], a);
            else e = Format::mate(S, names, has_f, f, id, in->adapter_only_number, m, o, var_walk[seg], n_cigar[seg], a);
            sizes[4 + seg] = Format::bytes(e);
            if (at + sizes[4 + seg] > cap) return -1;
            sizes[2 + seg] = Format::record(S, names, has_f, f, id, in->adapter_only_number, m, s, q, o, e, a, out + at);
            lanes([&](ImageSink &t) { Format::head(S, names, has_f, f, id, in->adapter_only_number, m, s, o, e, a, t); },
                  [&](ImageSink &t) {
                      if constexpr (Format::kMd) Format::tail(S, f, m, id, s, q, o, e, a, t);
                      else Format::tail(S, m, id, q, o, a, t);
                  },
                  Format::tail_at(e, m, id));
        } else {
            const SamAlign a = sam_align(has_f, f, (uint32_t)seg, walk[0], walk[1]);
            typename Format::Mate e;
            if constexpr (Format::kMd) e = Format::mate(S, names, has_f, f, in->adapter_only_number, m, s, o, walk[seg], a);
            else e = Format::mate(S, names, has_f, f, in->adapter_only_number, m, o, walk[seg], a);
            sizes[4 + seg] = Format::bytes(e);
            if (at + sizes[4 + seg] > cap) return -1;
            sizes[2 + seg] = Format::record(S, names, has_f, f, in->adapter_only_number, m, s, q, o, e, a, out + at);
            lanes([&](ImageSink &t) { Format::head(S, names, has_f, f, in->adapter_only_number, m, s, o, e, a, t); },
                  [&](ImageSink &t) {
                      if constexpr (Format::kMd) Format::tail(S, f, m, s, q, o, e, a, t);
                      else Format::tail(S, m, q, o, a, t);
                  },
                  Format::tail_at(e, m));
        }
        const char *text = reinterpret_cast<const char *>(image.data()) + at;
        if (image_bytes != sizes[2 + seg] || memcmp(text, out + at, sizes[2 + seg]) != 0) return -2;
        for (uint32_t i = 0; i < 4u * image.size(); ++i)
            if ((i < at || i >= at + sizes[2 + seg]) && reinterpret_cast<const char *>(image.data())[i]) return -2;
        at += sizes[2 + seg];
    }
    return 0;
}

// format: bit 0 BAM, bit 1 the formats of a reference with variants, bit 2 with the tags
extern "C" int truth_md_trial(const truth_md_in *in, int format, char *fastq0, char *fastq1, char *out, uint32_t at, uint32_t cap, uint32_t *sizes) {
    switch (format & 7) {
        case 0: return truth_md_trial_of<SamFormat>(in, fastq0, fastq1, out, at, cap, sizes);
        case 1: return truth_md_trial_of<BamFormat>(in, fastq0, fastq1, out, at, cap, sizes);
        case 2: return truth_md_trial_of<SamVarFormat>(in, fastq0, fastq1, out, at, cap, sizes);
        case 3: return truth_md_trial_of<BamVarFormat>(in, fastq0, fastq1, out, at, cap, sizes);
        case 4: return truth_md_trial_of<SamMdFormat>(in, fastq0, fastq1, out, at, cap, sizes);
        case 5: return truth_md_trial_of<BamMdFormat>(in, fastq0, fastq1, out, at, cap, sizes);
        case 6: return truth_md_trial_of<SamVarMdFormat>(in, fastq0, fastq1, out, at, cap, sizes);
        default: return truth_md_trial_of<BamVarMdFormat>(in, fastq0, fastq1, out, at, cap, sizes);
    }
}
