// rsq_format.h -- the library's kernels in front of and behind the read kernels (rsq_reads.h):
//   k_pair_tiles, k_record_tiles, k_bins_plan, k_bin_scatter    reads binned by tile: keys, the bins' places, the scatter
//   k_fragment_range, k_record_flags, k_record_partition        seqToIllumina records: the check of their fragment lengths, their partition by segment
//   k_methylation_templates, k_variant_templates                one lane per read writes its template before the read kernel runs
//   ImageSink, image_header, image_line_part, image_record_part what a lane writes into that image: aligned words ORed into zeroed LDS, no control flow per push (host/device)
//   WaveImage                                                   the frame of the kernels that write text through an LDS image of the wave's byte range (also rsq_sam.h)
//   k_format_write                                              FASTQ text: one wave per 16 records                 (Simulator.cpp:596-632, a5)
//   k_record_text_sizes, k_record_text_waves                    seqToIllumina records: their FASTQ text             (Simulator.cpp:2497-2504)
#pragma once
#include "rsq_reads.h"

namespace rsq {

// ---------------------------------------------------------------------------------------------- text into a zeroed image, by aligned words
// The writers of rsq_text.h (WordSinkT, TextOps) serve any destination: every push tests for the unaligned bytes in front of the first word, loops over them, and
// may or may not store a word; TextOps::num loops over v % 10.  Inlined a few hundred times into a kernel that is busy issuing VALU instructions, that control
// flow -- masks saved and restored, branches, 64-bit shifts -- is most of what the kernel executes.  The writers below serve one destination only, the image of
// WaveImage (or, on the host, a byte buffer whose first byte lies on a word boundary), which the wave ZEROES first: a lane then ORs aligned words into it.  The
// bytes of a word that belong to a neighbouring part are zero in the lane's own word, so a word shared by two parts needs no special case, in either order,
// and the first and last partial word of a part are dealt with where the part begins (the sink starts with the phase of its address) and in finish().  They
// stay host/device functions: tests/hostemu/text_trial.cpp runs them on the CPU against format_record.  What they rest on is in rsq_portable.h: image_or (the OR
// into the image), bytes_at (four bytes of a pair of words from a part's phase on) and wave_any (skips work that no lane of the wave needs without a divergent branch).
RSQ_HD uint32_t image_word(const uint32_t *p) { return load_as<uint32_t, 4>(p); }      // a word of text that is kept as characters
RSQ_HD constexpr uint32_t chars4(char a, char b = 0, char c = 0, char d = 0) {
    return (uint32_t)(uint8_t)a | ((uint32_t)(uint8_t)b << 8) | ((uint32_t)(uint8_t)c << 16) | ((uint32_t)(uint8_t)d << 24);
}
// g < 10000 as four characters with its leading zeros, the first in the low byte: both pairs of digits at once, sixteen bits each
RSQ_HD uint32_t four_digits(uint32_t g) {
    const uint32_t q = (g * 5243u) >> 19, r = g - 100u * q;                   // g / 100 (exact below 43699) and g % 100
    const uint32_t x = q | (r << 16);
    const uint32_t t = ((x * 103u) >> 10) & 0x000F000Fu;                      // tens of both (x / 10 is exact below 179; 99 * 103 < 2^16: the low half does not carry)
    const uint32_t u = x - 10u * t;                                           // units of both
    return (t | (u << 8)) + 0x30303030u;
}
RSQ_HD uint32_t count_digits4(uint32_t g) { return 1u + (g >= 10u) + (g >= 100u) + (g >= 1000u); }      // g < 10000

// The sink: the interface of TextOps (ch, bytes, str, num, element), so cigar_replay and the writers of rsq_sam.h take it as they take a WordSinkT.  A push has
// no loop and one predicated OR; the pending bytes are fewer than four between pushes, so they live in 32 bits.
struct ImageSink {
    RSQ_LDS uint32_t *w;       // the word the pending bytes belong to
    uint32_t lo;               // the pending bytes at their places in that word
    uint32_t pending, n;       // how many, the bytes in front of the part's first one included; bytes pushed so far
    RSQ_HD explicit ImageSink(RSQ_LDS char *dst)
        : w(reinterpret_cast<RSQ_LDS uint32_t *>(dst - ((uint32_t)(uintptr_t)dst & 3u))), lo(0), pending((uint32_t)(uintptr_t)dst & 3u), n(0) {}
    RSQ_HD void push(uint32_t bytes, uint32_t count) {         // count <= 4 bytes, the first in the low byte, the rest zero
        const uint64_t wide = (uint64_t)bytes << (8u * pending);
        lo |= (uint32_t)wide;
        pending += count;
        n += count;
        const bool full = pending >= 4u;
        if (full) image_or(w, lo);
        lo = full ? (uint32_t)(wide >> 32) : lo;
        w += full ? 1 : 0;
        pending &= 3u;
    }
    RSQ_HD void push4(uint32_t bytes) {                        // four bytes: nothing to decide
        const uint64_t wide = (uint64_t)bytes << (8u * pending);
        image_or(w, lo | (uint32_t)wide);
        lo = (uint32_t)(wide >> 32);
        w += 1;
        n += 4u;
    }
    RSQ_HD void finish() {
        if (pending) image_or(w, lo);
    }
    RSQ_HD void ch(char c) { push((uint8_t)c, 1u); }
    RSQ_HD void bytes(uint32_t word, uint32_t count) { push(count < 4u ? word & ((1u << (8u * count)) - 1u) : word, count); }
    // len characters at s, read as the aligned words they lie in (never a word without one of them), `head` in front and `tail` behind (0: none).  Fixed text
    // (the compiler knows it) becomes immediates.
    RSQ_HD void str(const char *s, uint32_t len, uint32_t head = 0, uint32_t tail = 0) {
        if (__builtin_constant_p(len) && __builtin_constant_p(s[0]) && !head && !tail) {
            uint32_t i = 0;
            for (; i + 4u <= len; i += 4u) push4(chars4(s[i], s[i + 1u], s[i + 2u], s[i + 3u]));
            if (i < len) {
                uint32_t word = 0;
                for (uint32_t k = 0; i + k < len; ++k) word |= (uint32_t)(uint8_t)s[i + k] << (8u * k);
                push(word, len - i);
            }
            return;
        }
        const uint32_t a = (uint32_t)(uintptr_t)s & 3u;
        words(reinterpret_cast<const uint32_t *>(s - a), a, len, head, tail);
    }
    // the same for len characters from byte a < 4 of the words at `from` (a caller that knows them aligned: no pointer becomes a number)
    RSQ_HD void words(const uint32_t *from, uint32_t a, uint32_t len, uint32_t head = 0, uint32_t tail = 0) {
        uint32_t low = 0, next = 0;                            // next: index of the word behind `low` (an index, not a walking pointer: `from` may be a kernel argument's member)
        if (len) low = image_word(from + next++);
        if (head) {                                            // the stream begins one byte earlier, with `head` there
            if (a) {
                --a;
                low = (low & ~(0xFFu << (8u * a))) | (head << (8u * a));
            } else {
                a = 3u;
                next = 0;
                low = head << 24;
            }
            ++len;
        }
        uint32_t i = 0;
        for (; i + 4u <= len; i += 4u, ++next) {               // the stream: len bytes from byte a of (low, from[next], ...)
            const uint32_t high = a + len > i + 4u ? image_word(from + next) : 0u;
            push4(bytes_at(high, low, a));
            low = high;
        }
        uint32_t rest = len - i;
        const uint32_t high = a + len > i + 4u ? image_word(from + next) : 0u;
        uint32_t word = bytes_at(high, low, a) & ((1u << (8u * rest)) - 1u);
        if (tail) {
            word |= tail << (8u * rest);
            ++rest;
        }
        push(word, rest);
    }
    // decimal digits without a loop: four at a time by multiply and shift, their number from compares, the leading zeros shifted out; `tail`: tail_len <= 4
    // characters behind the number (the fixed text that follows it) in the same pushes
    RSQ_HD void num(uint32_t v, uint32_t tail = 0, uint32_t tail_len = 0) {
        if (!wave_any(v >= 10000u)) {                         // the common number
            const uint32_t digits = count_digits4(v), total = digits + tail_len, at = 4u - digits;
            push(bytes_at(tail, four_digits(v), at), total < 4u ? total : 4u);
            if (wave_any(total > 4u)) push(tail >> (8u * at), total > 4u ? total - 4u : 0u);
            return;
        }
        const uint32_t upper = v / 10000u, hi = upper / 10000u, mid = upper - 10000u * hi;
        const uint32_t top = hi ? hi : upper ? mid : v, digits = (hi ? 8u : upper ? 4u : 0u) + count_digits4(top);
        const uint32_t x[4] = {four_digits(hi), four_digits(mid), four_digits(v - 10000u * upper), tail};      // twelve characters and the tail: skip 12 - digits
        const uint32_t skip = 12u - digits, sw = skip >> 2, at = skip & 3u, total = digits + tail_len;
        const uint32_t x0 = sw == 0u ? x[0] : sw == 1u ? x[1] : x[2], x1 = sw == 0u ? x[1] : sw == 1u ? x[2] : x[3], x2 = sw == 0u ? x[2] : sw == 1u ? x[3] : 0u, x3 = sw == 0u ? x[3] : 0u;
        push(bytes_at(x1, x0, at), total < 4u ? total : 4u);
        push(bytes_at(x2, x1, at), total < 4u ? 0u : total < 8u ? total - 4u : 4u);
        if (wave_any(total > 8u)) push(bytes_at(x3, x2, at), total < 8u ? 0u : total < 12u ? total - 8u : 4u);
        if (wave_any(total > 12u)) push(x3 >> (8u * at), total < 12u ? 0u : total - 12u);
    }
    RSQ_HD void nine_digits(uint32_t v) {                      // v < 10^9 with its leading zeros
        const uint32_t upper = v / 10000u, hi = upper / 10000u;
        push('0' + hi, 1u);
        push4(four_digits(upper - 10000u * hi));
        push4(four_digits(v - 10000u * upper));
    }
    RSQ_HD void num(uint64_t v, uint32_t tail = 0, uint32_t tail_len = 0) {      // beyond 32 bits (read numbers of a job of more than 4 G pairs): a rare branch
        if (v <= 0xFFFFFFFFull) return num((uint32_t)v, tail, tail_len);
        const uint64_t kE9 = 1000000000ull, upper = v / kE9;
        if (upper >= kE9) {
            num((uint32_t)(upper / kE9));
            nine_digits((uint32_t)(upper % kE9));
        } else num((uint32_t)upper);
        nine_digits((uint32_t)(v % kE9));
        push(tail, tail_len);
    }
    RSQ_HD void element(char op, uint32_t count) { num(count, (uint8_t)op, 1u); }
};

// format_header (rsq_text.h) for the sink above, character for character: every fixed character rides with the number or the name in front of it
RSQ_HD void image_header(const DevSim &S, const NameTable &names, bool has_f, const Fragment &f, uint64_t adapter_only_number, const ReadMeta &m, const WordColumn &ops, ImageSink &t,
                         bool has_fv, const FragmentVar &fv) {
    t.words(reinterpret_cast<const uint32_t *>(names.base_identifier), 0u, names.base_len, '@');
    if (has_f) {
        const uint32_t end = has_fv ? fv.end : f.start + f.len;
        t.num(f.block, '_', 1u);
        if (1u < S.num_alleles) {
            t.num(f.number, chars4('_', 'a', 'l', 'l'), 4u);
            t.push(chars4('e', 'l', 'e'), 3u);
            t.num((uint32_t)f.allele, ':', 1u);
        } else t.num(f.number, ':', 1u);
        t.num(f.strand ? end : f.start + 1u, ':', 1u);
        t.str(names.names + names.name_ptr[f.seq], names.name_ptr[f.seq + 1] - names.name_ptr[f.seq], 0u, ':');
        t.num(f.strand ? f.start + 1u : end, ':', 1u);
    } else {
        t.push(chars4('0', '_'), 2u);
        t.num(adapter_only_number, chars4(':', '0', ':', 'A'), 4u);
        t.push4(chars4('d', 'a', 'p', 't'));
        t.push4(chars4('e', 'r', ':', '0'));
        t.push(':', 1u);
    }
    t.num((uint32_t)S.tiles[m.tile_id], chars4(':', '1', '3', '3'), 4u);
    t.push4(chars4('7', ':', '1', '3'));
    t.push(chars4('3', '7', ' '), 3u);
    cigar_replay(ops, m, t);
    t.push(chars4(' ', 'E'), 2u);
    t.num((uint32_t)m.num_errors, '\n', 1u);
}

// format_line_part (rsq_text.h) without a sink: the part's phase is fixed, so output word j is one byte permute of the text of row words j and j - 1 and one
// OR; the row's last characters (a read length that is no multiple of four) and the line end join the same stream behind the whole words.
RSQ_HD void image_line_part(const WordColumn &row, uint32_t read_len, bool is_qual, uint32_t first_word, uint32_t n_words, bool with_end, RSQ_LDS char *dst) {
    const uint32_t begin = 4u * first_word < read_len ? 4u * first_word : read_len, left = read_len - begin;
    const uint32_t n_bytes = left < 4u * n_words ? left : 4u * n_words, full = n_bytes >> 2, rest = n_bytes & 3u;
    const uint32_t phase = (uint32_t)(uintptr_t)dst & 3u, at = 4u - phase;
    RSQ_LDS uint32_t *out = reinterpret_cast<RSQ_LDS uint32_t *>(dst - phase);
    constexpr uint32_t kAhead = 10u;                                 // loads in flight
    uint32_t before = 0;
    for (uint32_t i = 0; i < full; i += kAhead) {
        uint32_t w[kAhead];
        if (i + kAhead <= full) {                                    // ten whole words: nothing to decide per word
#pragma unroll
            for (uint32_t k = 0; k < kAhead; ++k) w[k] = row.at(first_word + i + k);
#pragma unroll
            for (uint32_t k = 0; k < kAhead; ++k) {
                const uint32_t text = is_qual ? w[k] : base_letters(w[k]);
                image_or(out + i + k, bytes_at(text, before, at));
                before = text;
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kAhead; ++k) w[k] = i + k < full ? row.at(first_word + i + k) : 0u;
#pragma unroll
            for (uint32_t k = 0; k < kAhead; ++k) {
                if (i + k < full) {
                    const uint32_t text = is_qual ? w[k] : base_letters(w[k]);
                    image_or(out + i + k, bytes_at(text, before, at));
                    before = text;
                }
            }
        }
    }
    // behind the whole words: up to three characters of the line, up to three of its end, and what the last whole word left over
    uint64_t x = with_end ? (is_qual ? (uint64_t)'\n' : (uint64_t)chars4('\n', '+', '\n')) : 0u;
    const uint32_t used = phase + rest + (with_end ? (is_qual ? 1u : 3u) : 0u);
    x <<= 8u * rest;
    if (rest) {
        const uint32_t last = row.at(first_word + full);
        x |= (is_qual ? last : base_letters(last)) & ((1u << (8u * rest)) - 1u);
    }
    const uint32_t x0 = (uint32_t)x, x1 = (uint32_t)(x >> 32);
    if (used > 0u) image_or(out + full, bytes_at(x0, before, at));
    if (used > 4u) image_or(out + full + 1u, bytes_at(x1, x0, at));
    if (used > 8u) image_or(out + full + 2u, bytes_at(0u, x1, at));
}

#ifndef RSQ_FORMAT_RECORDS
#define RSQ_FORMAT_RECORDS 16
#endif
constexpr uint32_t kFormatRecords = RSQ_FORMAT_RECORDS, kFormatLineParts = 32u / kFormatRecords;      // records of a wave; lanes that share a line of a record
// What lane `part` (0 .. 2 kFormatLineParts - 1) of a FASTQ record's lanes writes: the first kFormatLineParts the bases, the others the qualities, each its share
// of the line's words (the shares end on word boundaries of the row); part 0 the id line of head_bytes in front (head(sink) writes it).  text: where the record
// begins in the image.
template <class Head>
RSQ_HD void image_record_part(const ReadMeta &m, const WordColumn &seq, const WordColumn &qual, uint32_t head_bytes, uint32_t part, RSQ_LDS char *text, Head &&head) {
    const bool is_qual = part >= kFormatLineParts;
    const uint32_t sub = part % kFormatLineParts;
    const uint32_t all_words = ((uint32_t)m.read_len + 3u) >> 2, per = (all_words + kFormatLineParts - 1u) / kFormatLineParts;
    const uint32_t first_word = sub * per, line_at = head_bytes + (is_qual ? m.read_len + 3u : 0u);
    RSQ_LDS char *at = text + line_at + (4u * first_word < m.read_len ? 4u * first_word : m.read_len);
    if (part == 0u) {
        ImageSink t(text);
        head(t);
        t.finish();
    }
    image_line_part(is_qual ? qual : seq, m.read_len, is_qual, first_word, per, sub == kFormatLineParts - 1u, at);
}

#if RSQ_DEVICE_BUILD
#ifndef RSQ_BIN_KEYS_LDS
#define RSQ_BIN_KEYS_LDS 4096
#endif
constexpr uint32_t kBinKeysLds = RSQ_BIN_KEYS_LDS;      // up to so many bin keys the counting kernels aggregate in LDS (a build with 2 runs the tile tests through the other branch)
constexpr uint32_t kBinItemsPerThread = 16, kBinBlock = 256;

// bin keys of the items + their histogram.  Pairs: key = tile (TileId() once per pair, Simulator.cpp:701-704); records: key = segment * n_tiles + tile.
// (tests/hostemu/kernel_trial.cpp runs bin_count_key, k_bins_plan and k_bin_scatter alone on given keys, on either side of kBinKeysLds)
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

// Text through an LDS image: the frame of the kernels that write text (k_format_write and k_record_text_waves below, k_truth_write in rsq_sam.h).  One wave
// takes ITEMS consecutive raw rows, 64 / ITEMS lanes an item (lane & (ITEMS - 1) is the item, lane / ITEMS the lane's part of it).  The items' texts occupy one
// contiguous byte range of the output, so the wave formats them into an LDS image of that range (laid out with the same alignment modulo 16 as the destination)
// and then copies the image out with aligned 16-byte stores, all lanes over the range.  PERM (the read kernel ran binned by tile): the wave's items are those
// whose raw rows are consecutive -- perm[first .. first + ITEMS - 1] --, their texts lie anywhere in the output, so every item has a slot of the image (same
// alignment modulo 16 as its destination) and its lanes copy it out.  A wave whose text does not fit (through_lds false, wave-uniform) writes it straight to HBM.
// The writers are bound by the instructions they issue, not by latency: with WordSinkT (rsq_text.h) k_format_write executed 880 vector and 659 scalar instructions
// per wave, ten lane-instructions per byte of text, at 73 % VALU busy, most of it the control flow of the sink's pushes; hence ImageSink and image_line_part above
// (the wave zeroes the image with clear(), the lanes OR aligned words into it).  Waves per CU matter as well: the image is as large as the items need (lds_bytes,
// dynamic: the host sizes it from the longest item of the call before -- for the pairs' FASTQ 8 KiB a wave were twenty waves per CU and 5.6 ms per 10 M pairs,
// 6 KiB are 26 and 4.7 ms with the old sink).
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
    // the writers OR their words into the image (ImageSink, image_line_part): zero it first, all lanes, 16 bytes a store (lds_bytes is a multiple of 16)
    __device__ __forceinline__ void clear(char *image, uint32_t lds_bytes) const {
        for (uint32_t c = lane * 16u; c < lds_bytes; c += 64u * 16u) *reinterpret_cast<uint4 *>(image + c) = uint4{0u, 0u, 0u, 0u};
        __syncthreads();
    }
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

constexpr uint32_t kFormatLdsMax = 16u * 1024u, kFormatLdsMin = 1024u;
// the image for records of at most `record_bytes` (the longest record of the call before and a few bytes for a digit more in its numbers), whole 128 bytes;
// slots: binned rows, each record's slot with its own alignment
RSQ_HD uint32_t format_lds_bytes(uint64_t record_bytes, bool slots) {
    const uint64_t want = (kFormatRecords * record_bytes + 16u + 127u) & ~(uint64_t)127u;
    const uint32_t image = (uint32_t)(want < kFormatLdsMin ? kFormatLdsMin : want > kFormatLdsMax ? kFormatLdsMax : want);
    return !slots ? image : image + 16u * kFormatRecords < kFormatLdsMax ? image + 16u * kFormatRecords : kFormatLdsMax;
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
    im.clear(s_text, lds_bytes);
    if (im.active) {
        const uint32_t header = (uint32_t)(offsets[pair + 1u] - offsets[pair]) - 2u * m.read_len - 4u;
        image_record_part(m, seq, qual, header, part, im.item_text(s_text), [&](ImageSink &t) { image_header(S, names, frags != nullptr, f, ao_number, m, ops, t, frags && fvars, fv); });
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
    const uint32_t lane = threadIdx.x, part = lane / kFormatRecords;
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
    auto image_head = [&](ImageSink &t) {                                            // the same characters, the fixed ones with their neighbours
        t.str(ids.begin(item), ids.length(item), '@', ' ');
        cigar_replay(ops, m, t);
        t.push(chars4(' ', 'E'), 2u);
        t.num((uint32_t)m.num_errors, '\n', 1u);
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
    im.clear(s_text, lds_bytes);
    if (active) {
        const uint32_t head = (uint32_t)(offsets[item + 1u] - offsets[item]) - 2u * m.read_len - 4u;
        image_record_part(m, seq, qual, head, part, im.item_text(s_text), image_head);
    }
    im.store_out(s_text);
}

#endif

}  // namespace rsq
