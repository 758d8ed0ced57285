// rsq_format.h -- the library's kernels in front of and behind the read kernels (rsq_reads.h):
//   k_pair_tiles, k_record_tiles, k_bins_plan, k_bin_scatter    reads binned by tile: keys, the bins' places, the scatter
//   k_fragment_range, k_record_flags, k_record_partition        seqToIllumina records: the check of their fragment lengths, their partition by segment
//   k_methylation_templates, k_variant_templates                one lane per read writes its template before the read kernel runs
//   WaveImage                                                   the frame of the kernels that write text through an LDS image of the wave's byte range (also rsq_sam.h)
//   k_max_size, k_format_write                                  FASTQ text: one wave per 16 records                 (Simulator.cpp:596-632, a5)
//   k_record_text_sizes, k_record_text_waves                    seqToIllumina records: their FASTQ text             (Simulator.cpp:2497-2504)
#pragma once
#include "rsq_reads.h"

namespace rsq {

#if RSQ_DEVICE_BUILD
#ifndef RSQ_BIN_KEYS_LDS
#define RSQ_BIN_KEYS_LDS 4096
#endif
constexpr uint32_t kBinKeysLds = RSQ_BIN_KEYS_LDS;      // up to so many bin keys the counting kernels aggregate in LDS (a build with 2 runs the tile tests through the other branch)
constexpr uint32_t kBinItemsPerThread = 16, kBinBlock = 256;

// bin keys of the items + their histogram.  Pairs: key = tile (TileId() once per pair, Simulator.cpp:701-704); records: key = segment * n_tiles + tile.
__device__ inline void bin_count_key(uint32_t key, bool valid, uint32_t n_keys, uint32_t *hist, uint32_t *s_hist) {
    if (n_keys <= kBinKeysLds) {
        for (uint32_t k = threadIdx.x; k < n_keys; k += blockDim.x) s_hist[k] = 0;
        __syncthreads();
        if (valid) atomicAdd(&s_hist[key], 1u);
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < n_keys; k += blockDim.x)
            if (s_hist[k]) atomicAdd(&hist[k], s_hist[k]);
    } else if (valid) atomicAdd(&hist[key], 1u);
}
__global__ void __launch_bounds__(kBinBlock) k_pair_tiles(DevSim S, const Fragment *frags, const FragmentVar *fvars, uint64_t n_pairs, uint64_t adapter_only_first, uint16_t *key_of,
                                                         uint32_t *hist) {
    __shared__ uint32_t s_hist[kBinKeysLds];
    const uint64_t pair = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = pair < n_pairs;
    uint32_t key = 0;
    if (valid) {
        Fragment f{};
        if (frags) f = frags[pair];
        const PairStream ps = pair_stream(frags ? &f : nullptr, fvars ? fvars[pair].sub : 0u, adapter_only_first + pair);
        key = draw_tile(S, ps.c0, ps.c1, ps.c2, pair_c3(kDomPair, ps.strand, 2, f.allele));
        key_of[pair] = (uint16_t)key;
    }
    bin_count_key(key, valid, S.n_tiles, hist, s_hist);
}
__global__ void __launch_bounds__(kBinBlock) k_record_tiles(DevSim S, const uint8_t *segs, uint64_t first_index, uint64_t n, uint16_t *key_of, uint32_t *hist) {
    __shared__ uint32_t s_hist[kBinKeysLds];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    uint32_t key = 0;
    if (valid) {
        const uint64_t idx = first_index + i;
        key = (segs[i] ? S.n_tiles : 0u) + draw_tile(S, (uint32_t)idx, (uint32_t)(idx >> 32), 0u, pair_c3(kDomErrModel, 0, 2));
        key_of[i] = (uint16_t)key;
    }
    bin_count_key(key, valid, 2u * S.n_tiles, hist, s_hist);
}
// one workgroup: the bins' places in perm (exclusive scan of the histogram), the scatter's cursors, the scheduler's counters.  pairs: n_keys = n_tiles, bins
// (segment, tile) of both segments share tile's entries; records: n_keys = 2 n_tiles = the bins.
__global__ void __launch_bounds__(1024) k_bins_plan(const uint32_t *hist, uint32_t n_keys, uint32_t n_bins, uint32_t *bin_first, uint32_t *bin_count, uint32_t *cursor,
                                                    uint32_t *chunk_ptr, uint32_t *next_chunk, uint32_t *workers) {
    __shared__ uint32_t s_part[1024], s_chunks[1024];
    const uint32_t t = threadIdx.x, per = (n_bins + 1023u) / 1024u, lo = t * per < n_bins ? t * per : n_bins, hi = lo + per < n_bins ? lo + per : n_bins;
    // bins lo .. hi-1 of this thread; bin b has the items of key b % n_keys (the first n_keys bins place them)
    uint32_t items = 0, chunks = 0;
    for (uint32_t b = lo; b < hi; ++b) {
        const uint32_t c = hist[b % n_keys];
        if (b < n_keys) items += c;
        chunks += (c + 63u) / 64u;
    }
    s_part[t] = items;
    s_chunks[t] = chunks;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {                       // inclusive scans over the threads
        const uint32_t a = t >= d ? s_part[t - d] : 0u, c = t >= d ? s_chunks[t - d] : 0u;
        __syncthreads();
        s_part[t] += a;
        s_chunks[t] += c;
        __syncthreads();
    }
    uint32_t at = s_part[t] - items, chunk_at = s_chunks[t] - chunks;
    for (uint32_t b = lo; b < hi; ++b) {
        const uint32_t c = hist[b % n_keys];
        if (b < n_keys) {
            cursor[b] = at;
            for (uint32_t r = b; r < n_bins; r += n_keys) bin_first[r] = at, bin_count[r] = c;
            at += c;
        }
        chunk_ptr[b] = chunk_at;
        chunk_at += (c + 63u) / 64u;
        next_chunk[b] = workers[b] = 0;
    }
    if (t == 1023u) chunk_ptr[n_bins] = s_chunks[1023];
}
// items to their bins' places: ranks inside the workgroup from LDS counters, one global reservation per workgroup and key
__global__ void __launch_bounds__(kBinBlock) k_bin_scatter(const uint16_t *key_of, uint64_t n, uint32_t n_keys, uint32_t *cursor, uint32_t *perm, const Fragment *frags,
                                                          const FragmentVar *fvars, Fragment *frags_sorted, FragmentVar *fvars_sorted) {
    __shared__ uint32_t s_count[kBinKeysLds], s_base[kBinKeysLds];
    const uint64_t first = (uint64_t)blockIdx.x * (kBinBlock * kBinItemsPerThread);
    auto place = [&](uint32_t at, uint64_t i) {
        perm[at] = (uint32_t)i;
        if (frags) frags_sorted[at] = frags[i];
        if (fvars) fvars_sorted[at] = fvars[i];
    };
    if (n_keys > kBinKeysLds) {
        for (uint32_t j = 0; j < kBinItemsPerThread; ++j) {
            const uint64_t i = first + (uint64_t)j * kBinBlock + threadIdx.x;
            if (i < n) place(atomicAdd(&cursor[key_of[i]], 1u), i);
        }
        return;
    }
    for (uint32_t k = threadIdx.x; k < n_keys; k += kBinBlock) s_count[k] = 0;
    __syncthreads();
    uint32_t rank[kBinItemsPerThread], key[kBinItemsPerThread];
#pragma unroll
    for (uint32_t j = 0; j < kBinItemsPerThread; ++j) {
        const uint64_t i = first + (uint64_t)j * kBinBlock + threadIdx.x;
        key[j] = i < n ? key_of[i] : 0xFFFFFFFFu;
        rank[j] = i < n ? atomicAdd(&s_count[key[j]], 1u) : 0u;
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n_keys; k += kBinBlock)
        if (s_count[k]) s_base[k] = atomicAdd(&cursor[k], s_count[k]);
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kBinItemsPerThread; ++j)
        if (key[j] != 0xFFFFFFFFu) place(s_base[key[j]] + rank[j], first + (uint64_t)j * kBinBlock + threadIdx.x);
}

// ReadLength (Simulator.h:185-198) looks a record's fragment length up in InsertLengths() and ReadLengthsByFragmentLength(segment) with Vect::at, which ends the
// reference's run for a length outside ("Called index ... range is from ... to ..."): the first such record, so that the caller can say the same instead of
// reading beyond the tables.  lo / hi per segment: the lengths that have rows in both (all of them for a profile with one read length).
struct FragmentRange {
    uint32_t lo[2], hi[2];
};
__global__ void k_fragment_range(const uint8_t *segs, const uint32_t *frag_len, uint64_t n, FragmentRange range, uint32_t *first_bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t seg = segs[i] ? 1u : 0u, fl = frag_len[i];
    if (fl < range.lo[seg] || fl >= range.hi[seg]) atomicMin(first_bad, (uint32_t)i);
}
// the partition: flags for the scan, then the scatter once the number of segment-1 records before every record is known
__global__ void k_record_flags(const uint8_t *segs, uint64_t n, uint32_t *flags) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = segs[i] ? 1u : 0u;
}
__global__ void k_record_partition(const uint8_t *segs, uint64_t n, const uint64_t *ones_before, uint32_t *rec_index, uint32_t *rec_count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n1 = (uint32_t)ones_before[n], n0 = (uint32_t)n - n1;
    if (i == 0) {
        rec_count[0] = n0;
        rec_count[1] = n1;
    }
    if (i >= n) return;
    const uint32_t before = (uint32_t)ones_before[i];
    if (segs[i]) rec_index[n0 + before] = (uint32_t)i;
    else rec_index[(uint32_t)i - before] = (uint32_t)i;
}

// --methylation: one lane per read writes its converted template before the read kernel runs
__global__ void __launch_bounds__(256) k_methylation_templates(DevSim S, const Fragment *frags, uint64_t n_pairs, RawLayout raw) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 2u * n_pairs) return;
    const uint32_t seg = r >= n_pairs ? 1u : 0u;
    convert_template(S, frags[r - seg * n_pairs], seg, raw.templates + r * raw.template_words, raw.template_words);
}

// variants of any kind: Reference::ReferenceSequence with variants (GetOrgSeq, Simulator.cpp:1909-1914) for both mates of every pair
__global__ void __launch_bounds__(256) k_variant_templates(DevSim S, const Fragment *frags, const FragmentVar *fvars, uint64_t n_pairs, RawLayout raw) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 2u * n_pairs) return;
    const uint32_t seg = r >= n_pairs ? 1u : 0u;
    const uint64_t pair = r - seg * n_pairs;
    variant_template(S, frags[pair], fvars[pair], seg, raw.templates + r * raw.template_words, raw.template_words);
}

// Text through an LDS image: the frame of the kernels that write text (k_format_write and k_record_text_waves below, k_sam_write in rsq_sam.h).  One wave
// takes ITEMS consecutive raw rows, 64 / ITEMS lanes an item (lane & (ITEMS - 1) is the item, lane / ITEMS the lane's part of it).  The items' texts occupy one
// contiguous byte range of the output, so the wave formats them into an LDS image of that range (laid out with the same alignment modulo 16 as the destination)
// and then copies the image out with aligned 16-byte stores, all lanes over the range.  PERM (the read kernel ran binned by tile): the wave's items are those
// whose raw rows are consecutive -- perm[first .. first + ITEMS - 1] --, their texts lie anywhere in the output, so every item has a slot of the image (same
// alignment modulo 16 as its destination) and its lanes copy it out.  A wave whose text does not fit (through_lds false, wave-uniform) writes it straight to HBM.
// The writers are latency-bound (dependent byte pushes, four load round trips), so short per-lane work and many waves per CU matter more than instruction
// count: the image is as large as the items need (lds_bytes, dynamic: the host sizes it from the longest item of the call before -- for the pairs' FASTQ 8 KiB a
// wave were twenty waves per CU and 5.6 ms per 10 M pairs, 6 KiB are 26 and 4.7 ms).
// (items per wave: 16, four lanes each.  Eight records with eight lanes each need half the LDS and half the work per lane, but their loads of the raw
// rows cover 32 bytes instead of 64: 2.3 ms slower per 10 M pairs)
template <bool PERM, uint32_t ITEMS>
struct WaveImage {
    const uint64_t *offsets;
    char *dst;
    uint32_t lane, skew, bytes, slot_at;           // skew: where the text starts modulo 16; bytes: of the wave's text (PERM: of the lane's item); slot_at: the item's slot
    uint64_t row, item, g_begin;                   // the lane's raw row and its item (perm[row] or row); where the text starts in dst
    bool active, through_lds;
    static __device__ __forceinline__ uint64_t first() { return (uint64_t)blockIdx.x * ITEMS; }
    // behind the kernel's early returns (first() < n, its capacity checks): the loads start here
    __device__ __forceinline__ WaveImage(const uint64_t *offsets, uint64_t n, char *dst, uint32_t lds_bytes, const uint32_t *perm, uint32_t lane) : offsets(offsets), dst(dst), lane(lane) {
        const uint64_t last = first() + ITEMS < n ? first() + ITEMS : n;
        row = first() + (lane & (ITEMS - 1u));
        active = row < last;
        item = PERM ? (active ? perm[row] : 0u) : row;
        g_begin = PERM ? (active ? offsets[item] : 0u) : offsets[first()];
        const uint64_t g_end = PERM ? (active ? offsets[item + 1u] : 0u) : offsets[last];
        skew = (uint32_t)((uint64_t)(uintptr_t)(dst + g_begin) & 15u);
        bytes = (uint32_t)(g_end - g_begin);
        const uint32_t slot = (lds_bytes / ITEMS) & ~15u;
        through_lds = PERM ? __all(skew + bytes <= slot) != 0 : skew + bytes <= lds_bytes;
        slot_at = PERM ? (lane & (ITEMS - 1u)) * slot : 0u;
    }
    // where the lane's item starts in the image (active lanes)
    __device__ __forceinline__ RSQ_LDS char *item_text(char *image) const { return (RSQ_LDS char *)image + slot_at + skew + (PERM ? 0u : (uint32_t)(offsets[item] - g_begin)); }
    // the image goes out in aligned 16-byte stores: all lanes over the wave's range, or (PERM) an item's lanes over its slot
    __device__ __forceinline__ void store_out(const char *image) const {
        __syncthreads();
        const uint32_t lo = skew, hi = skew + bytes;                               // LDS byte range (within the slot) holding text
        char *g_chunk0 = dst + g_begin - skew;                                     // 16-byte aligned
        const char *s_from = image + slot_at;
        for (uint32_t c = (PERM ? lane / ITEMS : lane) * 16u; c < hi; c += (PERM ? 64u / ITEMS : 64u) * 16u) {
            if (c >= lo && c + 16u <= hi) {
                *reinterpret_cast<uint4 *>(g_chunk0 + c) = *reinterpret_cast<const uint4 *>(s_from + c);
            } else {
                for (uint32_t b = c < lo ? lo : c; b < c + 16u && b < hi; ++b) g_chunk0[b] = s_from[b];
            }
        }
    }
};

#ifndef RSQ_FORMAT_RECORDS
#define RSQ_FORMAT_RECORDS 16
#endif
constexpr uint32_t kFormatRecords = RSQ_FORMAT_RECORDS, kFormatLdsMax = 16u * 1024u, kFormatLdsMin = 1024u;
// the image for records of at most `record_bytes` (the longest record of the call before and a few bytes for a digit more in its numbers), whole 128 bytes;
// slots: binned rows, each record's slot with its own alignment
RSQ_HD uint32_t format_lds_bytes(uint64_t record_bytes, bool slots) {
    const uint64_t want = (kFormatRecords * record_bytes + 16u + 127u) & ~(uint64_t)127u;
    const uint32_t image = (uint32_t)(want < kFormatLdsMin ? kFormatLdsMin : want > kFormatLdsMax ? kFormatLdsMax : want);
    return !slots ? image : image + 16u * kFormatRecords < kFormatLdsMax ? image + 16u * kFormatRecords : kFormatLdsMax;
}
// the longest of n record sizes (one atomic per wave)
__global__ void __launch_bounds__(256) k_max_size(const uint32_t *sizes, uint64_t n, uint32_t *longest) {
    uint32_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) m = max(m, sizes[i]);
    for (uint32_t d = 32; d; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, (int)d, 64));
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(longest, m);
}
// FASTQ text of the pairs: one wave per 16 consecutive records of one file (grid.y = template segment = output file), through the wave's image.  Four lanes
// share a record: lanes 0-15 write the id line and the first half of the bases, lanes 16-31 the second half, lanes 32-47 and 48-63 the two halves of the
// qualities.
template <bool PERM>
__global__ void __launch_bounds__(64) k_format_write(DevSim S, NameTable names, const Fragment *frags, uint64_t n_pairs, uint64_t adapter_only_first, RawLayout raw,
                                                    const uint64_t *offsets0, const uint64_t *offsets1, char *dst0, char *dst1, uint64_t cap0, uint64_t cap1,
                                                    const FragmentVar *fvars, const uint32_t *perm, uint32_t lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) char s_text[];
    using Image = WaveImage<PERM, kFormatRecords>;
    const uint32_t lane = threadIdx.x, seg = blockIdx.y, part = lane / kFormatRecords;
    constexpr uint32_t kLineParts = 32u / kFormatRecords;                          // lanes that share a line of a record
    const bool is_qual = part >= kLineParts;
    const uint32_t sub = part % kLineParts;
    if (Image::first() >= n_pairs) return;
    const uint64_t *offsets = seg ? offsets1 : offsets0;
    char *dst = seg ? dst1 : dst0;
    if (offsets[n_pairs] > (seg ? cap1 : cap0)) return;                            // the caller's buffer is too small: write nothing (RSQ_ENOSPC)
    const Image im(offsets, n_pairs, dst, lds_bytes, perm, lane);
    const uint64_t pair = im.item;
    ReadMeta m;
    Fragment f;
    FragmentVar fv;
    uint64_t r = 0;
    if (im.active) {
        r = (uint64_t)seg * n_pairs + im.row;                                      // of the raw arrays
        m = raw.meta[r];
        if (frags) f = frags[pair];
        if (frags && fvars) fv = fvars[pair];
    }
    const WordColumn seq = raw.seq_of(r), qual = raw.qual_of(r), ops = raw.ops_of(r);
    const uint64_t ao_number = adapter_only_first + pair + 1u;
    if (!im.through_lds) {                                                         // oversized ids: write straight to HBM
        if (im.active && part == 0u) format_record(S, names, frags != nullptr, f, ao_number, m, seq, qual, ops, dst + offsets[pair], frags && fvars, fv);
        return;
    }
    if (im.active) {
        const uint32_t header = (uint32_t)(offsets[pair + 1u] - offsets[pair]) - 2u * m.read_len - 4u;
        const uint32_t all_words = (m.read_len + 3u) >> 2, per = (all_words + kLineParts - 1u) / kLineParts;      // the parts end on word boundaries
        const uint32_t first_word = sub * per, line_at = header + (is_qual ? m.read_len + 3u : 0u);
        const uint32_t part_at = part == 0u ? 0u : line_at + (4u * first_word < m.read_len ? 4u * first_word : m.read_len);
        WordSinkT<RSQ_LDS char *> t(im.item_text(s_text) + part_at);
        if (part == 0u) format_header(S, names, frags != nullptr, f, ao_number, m, ops, t, frags && fvars, fv);
        format_line_part(is_qual ? qual : seq, m.read_len, is_qual, first_word, per, sub == kLineParts - 1u, t);
        t.finish();
    }
    im.store_out(s_text);
}

// seqToIllumina's FASTQ text on the device (Simulator.cpp:2497-2504: "@{id} {CIGAR} E{errors}", bases, "+", qualities): sizes, then the
// records at the offsets of their exclusive scan; one lane per record, word-granular stores
RSQ_HD uint32_t error_model_record_size(const ReadMeta &m, uint32_t id_len) { return 1u + id_len + 1u + m.cigar_chars + 2u + digits_u32(m.num_errors) + 1u + 2u * m.read_len + 4u; }
// the records' ids: packed one after the other (off: n + 1 offsets) or where they stand in the FASTA text (at: offset of the record's '>', len: the id's length)
struct RecordIds {
    const char *chars;
    const uint64_t *off;
    const uint32_t *at, *len;
    RSQ_HD const char *begin(uint64_t i) const { return chars + (off ? off[i] : (uint64_t)at[i] + 1u); }
    RSQ_HD uint32_t length(uint64_t i) const { return off ? (uint32_t)(off[i + 1] - off[i]) : len[i]; }
};
__global__ void __launch_bounds__(256) k_record_text_sizes(RawLayout raw, uint64_t n, RecordIds ids, uint32_t *sizes) {
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const uint64_t i = raw.item_of(row);
    sizes[i] = error_model_record_size(raw.meta[row], ids.length(i));
}
// The text by waves through the wave's image, with k_format_write's lane roles: 16 consecutive raw rows, four lanes per record (the header and the first half
// of the bases, the second half, the two halves of the qualities).  (One lane per record with word-granular stores, the kernel of rounds 2-4, wrote 0.3 TB/s:
// 8.3 ms per 8 M records.)  A wave whose records do not fit the image writes them lane by lane.
template <bool PERM>
__global__ void __launch_bounds__(64) k_record_text_waves(RawLayout raw, uint64_t n, RecordIds ids, const uint64_t *offsets, char *dst, uint64_t cap, uint32_t lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) char s_text[];
    using Image = WaveImage<PERM, kFormatRecords>;
    constexpr uint32_t kLineParts = 32u / kFormatRecords;
    const uint32_t lane = threadIdx.x, part = lane / kFormatRecords, sub = part % kLineParts;
    const bool is_qual = part >= kLineParts;
    if (Image::first() >= n || offsets[n] > cap) return;                             // (the caller's buffer is too small: write nothing, RSQ_ENOSPC)
    const Image im(offsets, n, dst, lds_bytes, raw.order, lane);
    const uint64_t row = im.row, item = im.item;
    const bool active = im.active;
    ReadMeta m{};
    if (active) m = raw.meta[row];
    const WordColumn seq = raw.seq_of(active ? row : 0u), qual = raw.qual_of(active ? row : 0u), ops = raw.ops_of(active ? row : 0u);
    auto header = [&](auto &t) {
        t.ch('@');
        t.str(ids.begin(item), ids.length(item));
        t.ch(' ');
        cigar_replay(ops, m, t);
        t.str(" E", 2);
        t.num((uint32_t)m.num_errors);
        t.ch('\n');
    };
    if (!im.through_lds) {
        if (active && part == 0u) {
            WordSinkT<char *> t(dst + offsets[item]);
            header(t);
            format_line(seq, m.read_len, false, t);
            format_line(qual, m.read_len, true, t);
            t.finish();
        }
        return;
    }
    if (active) {
        const uint32_t head = (uint32_t)(offsets[item + 1u] - offsets[item]) - 2u * m.read_len - 4u;
        const uint32_t all_words = (m.read_len + 3u) >> 2, per = (all_words + kLineParts - 1u) / kLineParts, first_word = sub * per;
        const uint32_t line_at = head + (is_qual ? m.read_len + 3u : 0u), part_at = part == 0u ? 0u : line_at + (4u * first_word < m.read_len ? 4u * first_word : m.read_len);
        WordSinkT<RSQ_LDS char *> t(im.item_text(s_text) + part_at);
        if (part == 0u) header(t);
        format_line_part(is_qual ? qual : seq, m.read_len, is_qual, first_word, per, sub == kLineParts - 1u, t);
        t.finish();
    }
    im.store_out(s_text);
}

#endif

}  // namespace rsq
