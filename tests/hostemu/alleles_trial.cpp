// alleles_trial.cpp -- TEST-ONLY: the FASTA text of the alleles (rsq_alleles.h) on the CPU.  The kernel's two per-lane steps -- alleles_fasta_lane into the tile's
// image, alleles_fasta_store out of it -- run as loops over tiles and lanes, on a reference the caller crafts: sequences as base codes, variants as (position,
// replacement, allele bits).  The packed words, the allele copies of a substitution-only set and the coordinate maps (allele_maps_of_sequence, the library's own)
// are made here.  tests/test_alleles.py builds it with g++ and compares every piece with Python's text of the alleles spelled out base by base.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../reseq_amd/csrc/rsq_alleles.h"
#include "../../reseq_amd/csrc/rsq_pack.h"

using namespace rsq;

extern "C" {
struct alleles_trial_in {
    uint32_t n_seqs, num_alleles;
    const uint32_t *seq_len;          // [n_seqs]
    const uint8_t *codes;             // the sequences' base codes 0..3, one after the other
    const char *names;                // the first words of their names, one after the other
    const uint32_t *name_ptr;         // [n_seqs + 1]
    const uint32_t *var_ptr;          // [n_seqs + 1]: a sequence's variants, sorted by position
    const uint32_t *var_pos, *var_len, *var_off;      // the replacement of variant i is var_bases[var_off[i], var_off[i] + var_len[i])
    const uint8_t *var_bases;
    const uint64_t *var_allele;       // two words per variant
    int32_t copies;                   // 1: a substitution-only set as the library packs it: a copy of the packed reference per allele (DevSim::hap_stride)
};

// n_pieces pieces of the text, piece i = bytes [at[i], at[i] + bytes[i]) produced at an address that is lead[i] modulo 16, one after the other into out; *total =
// bytes of the whole text.  -1: a piece reaches beyond the text (nothing more is written).  -2: a byte outside a piece was touched.
int alleles_trial(const alleles_trial_in *in, uint32_t n_pieces, const uint64_t *piece_at, const uint64_t *piece_bytes, const uint32_t *piece_lead, char *out, uint64_t *total) {
    const uint32_t na = in->num_alleles, n_seqs = in->n_seqs;
    DevSim S{};
    S.n_seqs = n_seqs;
    S.num_alleles = na;
    S.variants_loaded = in->copies ? 1u : 2u;
    std::vector<uint64_t> word_off;
    std::vector<uint32_t> seq_len(in->seq_len, in->seq_len + n_seqs), var_ptr(in->var_ptr, in->var_ptr + n_seqs + 1), map_ptr{0u};
    std::vector<std::string> names;
    uint64_t words = 0, base0 = 0;
    for (uint32_t s = 0; s < n_seqs; ++s) {
        word_off.push_back(words);
        words += (seq_len[s] + 31u) / 32u + 1u;
        names.emplace_back(in->names + in->name_ptr[s], in->name_ptr[s + 1] - in->name_ptr[s]);
    }
    const uint64_t stride = words + 1u;
    std::vector<uint64_t> packed(in->copies ? stride * (1u + na) : stride, 0ull);
    std::vector<uint32_t> gc_prefix(packed.size(), 0u);
    std::vector<DevVariant> variants;
    std::vector<AlleleVar> map;
    std::vector<uint64_t> length;
    for (uint32_t s = 0; s < n_seqs; ++s) {
        const std::vector<uint8_t> codes(in->codes + base0, in->codes + base0 + seq_len[s]);
        base0 += seq_len[s];
        for (uint32_t p = 0; p < seq_len[s]; ++p) packed[word_off[s] + (p >> 5)] |= (uint64_t)(codes[p] & 3u) << (2u * (p & 31u));
        std::vector<Variant> host;
        for (uint32_t i = var_ptr[s]; i < var_ptr[s + 1]; ++i) {
            variants.push_back(DevVariant{in->var_pos[i], in->var_len[i], in->var_off[i], 0u, {in->var_allele[2 * i], in->var_allele[2 * i + 1]}});
            Variant v;
            v.position = in->var_pos[i];
            v.var_seq = BaseSeq(std::vector<uint8_t>(in->var_bases + in->var_off[i], in->var_bases + in->var_off[i] + in->var_len[i]));
            v.allele[0] = in->var_allele[2 * i];
            v.allele[1] = in->var_allele[2 * i + 1];
            host.push_back(v);
        }
        std::vector<uint32_t> ends;
        const size_t map0 = map.size();
        std::vector<AlleleVar> mine;
        allele_maps_of_sequence(host, codes, na, names[s], mine, ends);
        map.insert(map.end(), mine.begin(), mine.end());
        for (uint32_t a = 0; a < na; ++a) {
            map_ptr.push_back((uint32_t)(map0 + ends[a]));
            length.push_back((uint64_t)((int64_t)seq_len[s] + mine[ends[a] - 1u].shift));
        }
    }
    if (in->copies) {
        S.hap_stride = stride;
        for (uint32_t a = 0; a < na; ++a) {
            uint64_t *hp = &packed[stride * (1u + a)];
            std::copy(packed.begin(), packed.begin() + (ptrdiff_t)stride, hp);
            for (uint32_t s = 0; s < n_seqs; ++s)
                for (uint32_t i = var_ptr[s]; i < var_ptr[s + 1]; ++i) {
                    if (in->var_len[i] != 1u) return -3;
                    if (!((in->var_allele[2 * i + (a >> 6)] >> (a & 63u)) & 1u)) continue;
                    uint64_t &w = hp[word_off[s] + (in->var_pos[i] >> 5)];
                    const uint32_t sh = (in->var_pos[i] & 31u) * 2u;
                    w = (w & ~((uint64_t)3u << sh)) | ((uint64_t)in->var_bases[in->var_off[i]] << sh);
                }
        }
    }
    const std::vector<uint32_t> bases_gc(variants.size() * 8u + 8u, 0u);
    S.ref_words = packed.data();
    S.gc_prefix = gc_prefix.data();
    S.seq_word_off = word_off.data();
    S.seq_len = seq_len.data();
    S.variants = variants.data();
    S.var_ptr = var_ptr.data();
    S.var_bases = in->var_bases;
    S.var_bases_gc = bases_gc.data();
    S.allele_map = map.data();
    S.allele_map_ptr = map_ptr.data();
    NameTable nt{};
    nt.names = in->names;
    nt.name_ptr = in->name_ptr;

    const std::vector<AlleleRecord> records = allele_records(names, na, length);
    *total = records.back().at;
    constexpr char kMarker = (char)0xEE;
    std::vector<TextQuad> image(kTileLanes * kLaneRow / 16u);
    int rc = 0;
    for (uint32_t i = 0; i < n_pieces; ++i) {
        const uint64_t at = piece_at[i], bytes = piece_bytes[i];
        const uint32_t lead = piece_lead[i];
        if (at > *total || bytes > *total - at || lead > 15u) return -1;
        if (!bytes) continue;
        const uint64_t tiles = (lead + bytes + kTileBytes - 1u) / kTileBytes, room = tiles * kTileBytes + 64u;
        char *buffer = static_cast<char *>(aligned_alloc(16, room));
        memset(buffer, kMarker, room);
        for (uint64_t tile = 0; tile < tiles; ++tile) {
            memset(image.data(), 0x5A, image.size() * sizeof(TextQuad));      // what another workgroup left in the LDS
            char *img = reinterpret_cast<char *>(image.data());
            for (uint32_t lane = 0; lane < kTileLanes; ++lane) alleles_fasta_lane(S, nt, records.data(), (uint32_t)records.size() - 1u, at, bytes, lead, tile, lane, img);
            for (uint32_t lane = 0; lane < kTileLanes; ++lane) alleles_fasta_store(bytes, lead, tile, lane, img, buffer + lead);
        }
        for (uint64_t k = 0; k < room; ++k)
            if ((k < lead || k >= lead + bytes) && buffer[k] != kMarker) rc = -2;
        memcpy(out, buffer + lead, bytes);
        out += bytes;
        free(buffer);
    }
    return rc;
}
}
