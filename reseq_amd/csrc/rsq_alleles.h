// rsq_alleles.h -- the alleles of a reference with variants written out as FASTA text (rsq_sim_alleles_fasta; `reseq illuminaPE -V ... --writeAlleles`).
//
// An allele is the reference with that allele's variants applied (rsq_variants.h): the sequences the fragments are drawn from.  The text has one record per
// (sequence, allele), in order of seq * num_alleles + allele:
//   ">" first word of the sequence's name "_allele" a "\n", then the allele's bases as ACGT in lines of kFastaLine, every line ended by "\n" (an allele of
//   length 0: the header line alone).
// So a record's size is closed form -- header + n + ceil(n / 70) -- and the host knows every record's place in the text without producing it (allele_records:
// the table the kernel, the .fai and the sizes are all made from).  The kernel runs over DESTINATION bytes: a lane owns kLaneBytes consecutive bytes of the
// caller's piece [at, at + bytes) of the text, finds the record of its first byte by bisection of the table, finds header byte / line / column by arithmetic,
// places itself ONCE in the allele's coordinate map and then takes 32 bases a time from allele_bits with the map entry it stands at as the hint.  Substitution-only
// variant sets have an allele copy of the packed reference instead of a map and read that.  The lanes of a workgroup leave their bytes in LDS, 16 at a time; then
// the workgroup stores its tile with aligned 16-byte stores, consecutive lanes at consecutive addresses, and single bytes where the piece begins or ends inside
// a group of 16.  A piece's bytes do not depend on how the text is cut, nor on the destination's alignment.
// Not part of the text hiprtc compiles for a profile (rsq_spec.h kSpecHeaders).
#pragma once
#include <string>
#include <vector>

#include "rsq_text.h"
#include "rsq_variants.h"

namespace rsq {

constexpr uint32_t kFastaLine = 70;                     // bases per line: SeqAn's default, what rsq_ref_write_fasta wraps at
struct AlleleRecord {                                   // one record of the text; the table ends with {bytes of the whole text, 0, 0}
    uint64_t at;                                        // offset of its '>' in the text
    uint32_t header;                                    // bytes of the header line with its line end
    uint32_t length;                                    // bases
};
RSQ_HD uint64_t allele_record_bytes(uint32_t header, uint32_t length) { return (uint64_t)header + length + ((uint64_t)length + kFastaLine - 1u) / kFastaLine; }
RSQ_HD uint32_t allele_header_bytes(uint32_t name_len, uint32_t allele) { return 1u + name_len + 7u + digits_u32(allele) + 1u; }

// the table of a reference: names = the first words of the sequences' names, length[seq * num_alleles + allele] = bases of that allele
inline std::vector<AlleleRecord> allele_records(const std::vector<std::string> &names, uint32_t num_alleles, const std::vector<uint64_t> &length) {
    std::vector<AlleleRecord> out;
    uint64_t at = 0;
    for (size_t seq = 0; seq < names.size(); ++seq)
        for (uint32_t a = 0; a < num_alleles; ++a) {
            const AlleleRecord r{at, allele_header_bytes((uint32_t)names[seq].size(), a), (uint32_t)length[seq * num_alleles + a]};
            out.push_back(r);
            at += allele_record_bytes(r.header, r.length);
        }
    out.push_back(AlleleRecord{at, 0u, 0u});
    return out;
}

// byte k of a record's header line
RSQ_HD char allele_header_byte(const NameTable &names, uint32_t seq, uint32_t allele, uint32_t k) {
    const uint32_t name_at = names.name_ptr[seq], name_len = names.name_ptr[seq + 1] - name_at;
    if (0u == k) return '>';
    if (k <= name_len) return names.names[name_at + k - 1u];
    k -= 1u + name_len;
    if (k < 7u) return (char)(0x00656C656C6C615Full >> (8u * k));        // "_allele"
    k -= 7u;
    const uint32_t n = digits_u32(allele);
    if (k >= n) return '\n';
    for (uint32_t drop = n - 1u - k; drop; --drop) allele /= 10u;
    return (char)('0' + allele % 10u);
}

// 32 consecutive bases of one allele from base `h` on (fewer at its end), first base in the lowest bits: of its copy of the packed reference, or over its map
struct AlleleBases {
    const uint64_t *copy;                               // substitution-only sets (DevSim::hap_stride); nullptr: the map
    uint64_t word_off;
    AlleleView a;
    uint32_t hint;                                      // entries of the map at or before the last word asked for; kNoHint: the lane has not placed itself yet
    RSQ_HD AlleleBases(const DevSim &S, uint32_t seq, uint32_t allele) : copy(S.hap_stride ? hap_words(S, allele) : nullptr), word_off(S.seq_word_off[seq]), a{}, hint(AlleleView::kNoHint) {
        if (!copy) a = allele_view(S, seq, allele);
    }
    RSQ_HD uint64_t bits(uint32_t h, uint32_t n) {
        if (copy) return ref_bits64(copy, word_off, h);
        hint = a.entries_upto((int64_t)h, hint);        // the one bisection of the lane; from then on a short walk, and allele_bits finds its place at once
        return allele_bits(a, (int64_t)h, n, hint);
    }
};

// four 2-bit codes of a byte, first in the lowest bits -> their four letters, first in the lowest byte
RSQ_HD uint32_t four_base_letters(uint32_t packed) {
    return base_letters((packed | packed << 6 | packed << 12 | packed << 18) & 0x03030303u);
}

// Bytes [t, t + n) of the text into `sink` (push(word, count): count <= 4 bytes, the first in the low byte, nothing above them).  t + n lies inside the text.
template <class Sink>
RSQ_HD void allele_text_run(const DevSim &S, const NameTable &names, const AlleleRecord *__restrict__ records, uint32_t n_records, uint64_t t, uint32_t n, Sink &sink) {
    uint32_t m = 0, above = n_records;                                    // the last record that begins at or before t
    while (above - m > 1u) {
        const uint32_t mid = (m + above) >> 1;
        if (records[mid].at <= t) m = mid;
        else above = mid;
    }
    for (; n; ++m) {
        const AlleleRecord r = records[m];
        const uint32_t seq = m / S.num_alleles, allele = m - seq * S.num_alleles;
        uint64_t off = t - r.at;
        for (; off < r.header && n; ++off, ++t, --n) sink.push((uint8_t)allele_header_byte(names, seq, allele, (uint32_t)off), 1u);
        const uint64_t body = allele_record_bytes(r.header, r.length) - off;      // what is left of the record's lines
        uint32_t take = body < n ? (uint32_t)body : n;
        if (!take) continue;
        t += take;
        n -= take;
        const uint64_t line = (off - r.header) / (kFastaLine + 1u);
        uint32_t col = (uint32_t)((off - r.header) - line * (kFastaLine + 1u)), base = (uint32_t)line * kFastaLine + col, have = 0;
        uint64_t bits = 0;
        AlleleBases src(S, seq, allele);
        while (take) {
            if (col == kFastaLine || base == r.length) {                 // a full line's end, or the last line's
                sink.push('\n', 1u);
                col = 0;
                --take;
                continue;
            }
            if (!have) {
                have = r.length - base < 32u ? r.length - base : 32u;
                bits = src.bits(base, have);
            }
            uint32_t k = kFastaLine - col < have ? kFastaLine - col : have;
            if (k > 4u) k = 4u;
            if (k > take) k = take;
            const uint32_t letters = four_base_letters((uint32_t)bits & 0xFFu);
            sink.push(k < 4u ? letters & ((1u << (8u * k)) - 1u) : letters, k);
            bits >>= 2u * k;
            have -= k;
            base += k;
            col += k;
            take -= k;
        }
    }
}

// ---- the workgroup's tile: kTileLanes lanes of kLaneBytes destination bytes each, rows of kLaneRow bytes in LDS (an odd number of 16-byte groups: the groups
// 16 lanes write at once lie in 16 different bank groups)
constexpr uint32_t kLaneBytes = 64, kLaneRow = kLaneBytes + 16u, kTileLanes = 256, kTileBytes = kTileLanes * kLaneBytes;
struct alignas(16) TextQuad {
    uint64_t lo, hi;
};
template <class P>
struct QuadPtr {
    using type = TextQuad *;
};
template <>
struct QuadPtr<RSQ_LDS char *> {         // (the host: RSQ_LDS is empty and this is the general case again)
    using type = RSQ_LDS TextQuad *;
};
// bytes collect in two registers and leave 16 at a time, to a 16-byte aligned place; `skip` leading bytes of the first group stay zero
template <class P>
struct QuadSinkT {
    P p;
    uint64_t lo, hi;
    uint32_t pending;
    RSQ_HD QuadSinkT(P dst, uint32_t skip) : p(dst), lo(0), hi(0), pending(skip) {}
    RSQ_HD void store() { *reinterpret_cast<typename QuadPtr<P>::type>(p) = TextQuad{lo, hi}; }
    RSQ_HD void push(uint32_t word, uint32_t count) {
        const uint32_t at = pending;
        if (at < 8u) {
            lo |= (uint64_t)word << (8u * at);
            if (at > 4u) hi |= (uint64_t)word >> (8u * (8u - at));
        } else hi |= (uint64_t)word << (8u * (at - 8u));
        pending += count;
        if (pending >= 16u) {
            store();
            p += 16;
            pending -= 16u;
            lo = pending ? (uint64_t)word >> (8u * (count - pending)) : 0ull;
            hi = 0;
        }
    }
    RSQ_HD void finish() {
        if (pending) store();
    }
};

// The piece [at, at + bytes) of the text goes to dst; `lead` = dst's address modulo 16.  Tiles and lanes count bytes from the aligned address in front of dst:
// byte v of that numbering is byte at + v - lead of the text, and it exists for lead <= v < lead + bytes.
// step 1, every lane of the tile: its bytes into its row of the tile's image
RSQ_HD void alleles_fasta_lane(const DevSim &S, const NameTable &names, const AlleleRecord *__restrict__ records, uint32_t n_records, uint64_t at, uint64_t bytes, uint32_t lead,
                               uint64_t tile, uint32_t lane, RSQ_LDS char *image) {
    const uint64_t first = tile * kTileBytes + (uint64_t)lane * kLaneBytes, end = lead + bytes;
    const uint64_t lo = first < lead ? lead : first, hi = first + kLaneBytes < end ? first + kLaneBytes : end;
    if (lo >= hi) return;
    const uint32_t skip = (uint32_t)(lo - first);
    QuadSinkT<RSQ_LDS char *> sink(image + lane * kLaneRow + (skip & ~15u), skip & 15u);
    allele_text_run(S, names, records, n_records, at + lo - lead, (uint32_t)(hi - lo), sink);
    sink.finish();
}
// step 2, every lane of the tile after all of them have done step 1: the tile's 16-byte groups, consecutive lanes consecutive groups
RSQ_HD void alleles_fasta_store(uint64_t bytes, uint32_t lead, uint64_t tile, uint32_t lane, const RSQ_LDS char *image, char *dst) {
    const uint64_t end = lead + bytes;
    for (uint32_t g = lane; g < kTileBytes / 16u; g += kTileLanes) {
        const uint64_t v = tile * kTileBytes + (uint64_t)g * 16u;
        if (v >= end) return;
        const RSQ_LDS char *from = image + (g / (kLaneBytes / 16u)) * kLaneRow + (g % (kLaneBytes / 16u)) * 16u;
        char *to = dst + (int64_t)v - (int64_t)lead;
        if (v >= lead && v + 16u <= end) {
            *reinterpret_cast<TextQuad *>(to) = *reinterpret_cast<const RSQ_LDS TextQuad *>(from);
        } else {
            for (uint32_t k = 0; k < 16u; ++k)
                if (v + k >= lead && v + k < end) to[k] = from[k];
        }
    }
}

#if RSQ_DEVICE_BUILD
__global__ void __launch_bounds__(kTileLanes) k_alleles_fasta(DevSim S, NameTable names, const AlleleRecord *__restrict__ records, uint32_t n_records, uint64_t at, uint64_t bytes, uint32_t lead,
                                                              char *dst) {
    __shared__ TextQuad image[kTileLanes * kLaneRow / 16u];
    RSQ_LDS char *img = (RSQ_LDS char *)image;
    alleles_fasta_lane(S, names, records, n_records, at, bytes, lead, blockIdx.x, threadIdx.x, img);
    __syncthreads();
    alleles_fasta_store(bytes, lead, blockIdx.x, threadIdx.x, img, dst);
}
#endif

}  // namespace rsq
