// rsq_format.h -- the library's kernels in front of and behind the read kernels (rsq_reads.h):
//   k_pair_tiles, k_record_tiles, k_bins_plan, k_bin_scatter    reads binned by tile: keys, the bins' places, the scatter
//   k_fragment_range, k_record_flags, k_record_partition        seqToIllumina records: the check of their fragment lengths, their partition by segment
//   k_methylation_templates, k_variant_templates                one lane per read writes its template before the read kernel runs
//   k_max_size, k_format_write                                  FASTQ text: one wave per 16 records                 (Simulator.cpp:596-632, a5)
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

// FASTQ text: one wave per 16 consecutive records of one file (grid.y = template segment = output file).  The records
// occupy one contiguous byte range of the output, so the wave formats them into an LDS image of that range (laid out with
// the same alignment modulo 16 as the destination) and then copies the image out with aligned 16-byte stores.  Four lanes
// share a record: lanes 0-15 write the id line and the first half of the bases, lanes 16-31 the second half, lanes 32-47 and
// 48-63 the two halves of the qualities.  The kernel is latency-bound (dependent byte pushes, four load round trips), so
// short per-lane work and many waves per CU matter more than instruction count: the image is as large as the records need (lds_bytes, dynamic: the host sizes
// it from the longest record of the call before -- 8 KiB a wave were twenty waves per CU and 5.6 ms per 10 M pairs, 6 KiB are 26 and 4.7 ms); a wave whose records do
// not fit writes them straight to HBM.
// (records per wave: 16, four lanes each.  Eight records with eight lanes each need half the LDS and half the work per lane, but their loads of the raw
// rows cover 32 bytes instead of 64: 2.3 ms slower per 10 M pairs)
#ifndef RSQ_FORMAT_RECORDS
#define RSQ_FORMAT_RECORDS 16
#endif
constexpr uint32_t kFormatRecords = RSQ_FORMAT_RECORDS, kFormatLdsMax = 16u * 1024u, kFormatLdsMin = 1024u;
// the image for records of at most `record_bytes` (the longest record of the call before and a few bytes for a digit more in its numbers), whole 128 bytes
RSQ_HD uint32_t format_lds_bytes(uint64_t record_bytes) {
    const uint64_t want = (kFormatRecords * record_bytes + 16u + 127u) & ~(uint64_t)127u;
    return (uint32_t)(want < kFormatLdsMin ? kFormatLdsMin : want > kFormatLdsMax ? kFormatLdsMax : want);
}
// the longest of n record sizes (one atomic per wave)
__global__ void __launch_bounds__(256) k_max_size(const uint32_t *sizes, uint64_t n, uint32_t *longest) {
    uint32_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) m = max(m, sizes[i]);
    for (uint32_t d = 32; d; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, (int)d, 64));
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(longest, m);
}
// PERM (the read kernel ran binned by tile): the wave's 16 records are those whose raw rows are consecutive -- pairs perm[first .. first + 15] --, their
// texts lie anywhere in the output, so every record has a 512-byte slot of the image (same alignment modulo 16 as its destination) and its four lanes
// copy it out.
template <bool PERM>
__global__ void __launch_bounds__(64) k_format_write(DevSim S, NameTable names, const Fragment *frags, uint64_t n_pairs, uint64_t adapter_only_first, RawLayout raw,
                                                    const uint64_t *offsets0, const uint64_t *offsets1, char *dst0, char *dst1, uint64_t cap0, uint64_t cap1,
                                                    const FragmentVar *fvars, const uint32_t *perm, uint32_t lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) char s_text[];
    const uint32_t lane = threadIdx.x, seg = blockIdx.y, rec = lane & (kFormatRecords - 1u), part = lane / kFormatRecords;
    constexpr uint32_t kLineParts = 32u / kFormatRecords;                          // lanes that share a line of a record
    const bool is_qual = part >= kLineParts;
    const uint32_t sub = part % kLineParts;
    const uint64_t first = (uint64_t)blockIdx.x * kFormatRecords;
    if (first >= n_pairs) return;
    const uint64_t *offsets = seg ? offsets1 : offsets0;
    char *dst = seg ? dst1 : dst0;
    if (offsets[n_pairs] > (seg ? cap1 : cap0)) return;                            // the caller's buffer is too small: write nothing (RSQ_ENOSPC)
    const uint64_t last = first + kFormatRecords < n_pairs ? first + kFormatRecords : n_pairs;
    const uint64_t row = first + rec;                                              // of the raw arrays, within the segment
    const bool active = row < last;
    const uint64_t pair = PERM ? (active ? perm[row] : 0u) : row;
    // the byte range of the wave's text (PERM: of the lane's record) and where it starts modulo 16
    const uint64_t g_begin = PERM ? (active ? offsets[pair] : 0u) : offsets[first], g_end = PERM ? (active ? offsets[pair + 1u] : 0u) : offsets[last];
    const uint32_t skew = (uint32_t)((uint64_t)(uintptr_t)(dst + g_begin) & 15u), bytes = (uint32_t)(g_end - g_begin);
    const uint32_t kSlot = (lds_bytes / kFormatRecords) & ~15u;
    const bool through_lds = PERM ? __all(skew + bytes <= kSlot) != 0 : skew + bytes <= lds_bytes;      // wave-uniform
    ReadMeta m;
    Fragment f;
    FragmentVar fv;
    uint64_t r = 0;
    if (active) {
        r = (uint64_t)seg * n_pairs + row;
        m = raw.meta[r];
        if (frags) f = frags[pair];
        if (frags && fvars) fv = fvars[pair];
    }
    const WordColumn seq = raw.seq_of(r), qual = raw.qual_of(r), ops = raw.ops_of(r);
    const uint64_t ao_number = adapter_only_first + pair + 1u;
    if (!through_lds) {                                                            // oversized ids: write straight to HBM
        if (active && part == 0u) format_record(S, names, frags != nullptr, f, ao_number, m, seq, qual, ops, dst + offsets[pair], frags && fvars, fv);
        return;
    }
    const uint32_t slot_at = PERM ? rec * kSlot : 0u;
    if (active) {
        RSQ_LDS char *rec_text = (RSQ_LDS char *)s_text + slot_at + skew + (PERM ? 0u : (uint32_t)(offsets[pair] - g_begin));
        const uint32_t header = (uint32_t)(offsets[pair + 1u] - offsets[pair]) - 2u * m.read_len - 4u;
        const uint32_t all_words = (m.read_len + 3u) >> 2, per = (all_words + kLineParts - 1u) / kLineParts;      // the parts end on word boundaries
        const uint32_t first_word = sub * per, line_at = header + (is_qual ? m.read_len + 3u : 0u);
        const uint32_t part_at = part == 0u ? 0u : line_at + (4u * first_word < m.read_len ? 4u * first_word : m.read_len);
        WordSinkT<RSQ_LDS char *> t(rec_text + part_at);
        if (part == 0u) format_header(S, names, frags != nullptr, f, ao_number, m, ops, t, frags && fvars, fv);
        format_line_part(is_qual ? qual : seq, m.read_len, is_qual, first_word, per, sub == kLineParts - 1u, t);
        t.finish();
    }
    __syncthreads();
    const uint32_t lo = skew, hi = skew + bytes;                                   // LDS byte range (within the slot) holding text
    char *g_chunk0 = dst + g_begin - skew;                                         // 16-byte aligned
    const char *s_from = s_text + slot_at;
    // the image goes out in aligned 16-byte stores: all lanes over the wave's range, or (PERM) a record's four lanes over its slot
    for (uint32_t c = (PERM ? part : lane) * 16u; c < hi; c += (PERM ? 64u / kFormatRecords : 64u) * 16u) {
        if (c >= lo && c + 16u <= hi) {
            *reinterpret_cast<uint4 *>(g_chunk0 + c) = *reinterpret_cast<const uint4 *>(s_from + c);
        } else {
            for (uint32_t b = c < lo ? lo : c; b < c + 16u && b < hi; ++b) g_chunk0[b] = s_from[b];
        }
    }
}

#endif

}  // namespace rsq
