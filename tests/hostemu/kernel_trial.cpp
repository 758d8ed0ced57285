// kernel_trial.cpp -- TEST-ONLY: the library's cooperative kernels run alone on inputs made in Python (tests/kernel_trial_cases.py, tests/test_kernel_trial_gpu.py).
// These are the kernels whose code exists only for the device -- ballots, shuffles, LDS counters, tile sums -- so that the host emulation replaces them with a
// loop: the scan (rsq_scan.h), the sorted BAM's radix passes, cut, gather and index kernels (rsq_bamsort.h), the bins' plan and scatter (rsq_format.h) and the
// FASTA record starts (rsq_fasta.h); and the kernels that turn a run's arrays into results: the truth depth's in-place prefix sum and its bedGraph text
// (rsq_depth.h), the truth pileup's rows and TSV text (rsq_pileup.h), the simulation report's rows kernel and its ballot-aggregated adds (rsq_stats.h).
// Compiled by hipcc for the library's architecture with the library's flags (tests/hostemu/Makefile: kernel_trial).
//
//   kernel_trial FAMILY input.bin output.bin        FAMILY: scan | sort | gather | index | bins | fasta | depthscan | bedgraph | pileup | stats
//
// input.bin:  a word (uint64) with the number of cases; per case sixteen words of parameters, then the case's blobs, each a word with its bytes followed by the
//             bytes, padded to a multiple of eight.
// output.bin: per case its result blobs in the same form.
// Launches go through scan_launch and bam_sort_passes where the library's do; the sequences with a host read in the middle are restated here with the library's
// grid formulas (rsq_sim.hip: sorted_finish, build_fill_bins, rsq_sim_error_model_fasta, rsq_sim_depth_finish, rsq_sim_depth_bedgraph, rsq_sim_pileup_counts,
// rsq_sim_pileup_text, stats_take) and the library's LDS sizes (depth_lds_bytes, pileup_lds_bytes, stats_rows_geometry).  The kernels of its own: k_trial_keys, which
// reads bin keys from memory where k_pair_tiles / k_record_tiles draw them, and counts them with the library's bin_count_key; k_trial_shared, which reads the
// indices of StatsMatesAdd's adds from memory where k_stats_mates walks a mate for them.
// High positions without large arrays: the depth, pileup and reference arrays of a case exist from a position `base` on, and the kernels get the address moved back
// by `base` elements (moved_back), so that position p of the sequence is element p - base of the buffer; a right kernel reads nothing in front of the window.
// Every HIP call is checked; the first error ends the program with a message and a non-zero status.  Nothing is tried twice.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../reseq_amd/csrc/rsq_fasta.h"
#include "../../reseq_amd/csrc/rsq_scan.h"
#include "../../reseq_amd/csrc/rsq_text.h"
#include "../../reseq_amd/csrc/rsq_reads.h"
#include "../../reseq_amd/csrc/rsq_format.h"
#include "../../reseq_amd/csrc/rsq_sam.h"
#include "../../reseq_amd/csrc/rsq_bam.h"
#include "../../reseq_amd/csrc/rsq_md.h"
#include "../../reseq_amd/csrc/rsq_bamsort.h"
#include "../../reseq_amd/csrc/rsq_depth.h"
#include "../../reseq_amd/csrc/rsq_pileup.h"
#include "../../reseq_amd/csrc/rsq_stats.h"

using namespace rsq;

#define CHECK(expr)                                                                                   \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "HIP error: %s: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(3);                                                                                  \
        }                                                                                             \
    } while (0)

static void fail(const std::string &what) {
    fprintf(stderr, "kernel_trial: %s\n", what.c_str());
    exit(2);
}
static uint32_t cdiv32(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1u) / b); }

// ------------------------------------------------------------------------------------------------ files
typedef std::vector<uint8_t> Blob;
struct Reader {
    FILE *f;
    uint64_t word() {
        uint64_t v = 0;
        if (fread(&v, 8, 1, f) != 1) fail("the input ends inside a case");
        return v;
    }
    Blob blob() {
        const uint64_t bytes = word();
        Blob b((bytes + 7u) & ~(uint64_t)7u);
        if (!b.empty() && fread(b.data(), 1, b.size(), f) != b.size()) fail("the input ends inside a blob");
        b.resize(bytes);
        return b;
    }
};
struct Writer {
    FILE *f;
    void blob(const void *p, uint64_t bytes) {
        static const char zeros[8] = {0};
        const uint64_t pad = (8u - (bytes & 7u)) & 7u;
        if (fwrite(&bytes, 8, 1, f) != 1 || (bytes && fwrite(p, 1, bytes, f) != bytes) || (pad && fwrite(zeros, 1, pad, f) != pad)) fail("cannot write the output");
    }
};

// ------------------------------------------------------------------------------------------------ device memory of one case
struct Arena {
    std::vector<void *> held;
    ~Arena() {
        for (void *p : held) (void)hipFree(p);
    }
    // `bytes` + 256 spare ones, all set to `fill` (allocations begin on a 256-byte boundary)
    template <class T>
    T *get(uint64_t bytes, int fill = 0) {
        void *p = nullptr;
        CHECK(hipMalloc(&p, bytes + 256u));
        held.push_back(p);
        CHECK(hipMemset(p, fill, bytes + 256u));
        return static_cast<T *>(p);
    }
    template <class T>
    T *put(const Blob &b, uint64_t lead = 0, uint64_t spare = 0, int fill = 0) {
        char *p = get<char>(lead + b.size() + spare, fill);
        if (!b.empty()) CHECK(hipMemcpy(p + lead, b.data(), b.size(), hipMemcpyHostToDevice));
        return reinterpret_cast<T *>(p + lead);
    }
};
template <class T>
static std::vector<T> fetch(const void *dev, uint64_t count) {
    std::vector<T> v(count);
    if (count) CHECK(hipMemcpy(v.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}
template <class T>
static void emit(Writer &w, const void *dev, uint64_t count) {
    const std::vector<T> v = fetch<T>(dev, count);
    w.blob(v.data(), count * sizeof(T));
}
static void finish_launches() {
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
}
// the library's scan of one array, its scratch allocated for the case
static void scan_one(Arena &mem, const uint32_t *in, uint64_t n, uint64_t *out) {
    uint64_t *tile_sums = mem.get<uint64_t>(((uint64_t)cdiv32(n, kScanTile) + 1u) * 8u), *total = mem.get<uint64_t>(8);
    scan_launch(ScanArrays{{in, nullptr}, {out, nullptr}, {nullptr, nullptr}, {total, nullptr}}, 1, n, tile_sums, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------ scan
// parameters: n, arrays, init given, init, in shifted by so many elements, out shifted by so many, longest's value before.  blob: arrays * n elements.
// results: the out buffer -- per array two guard words, n + 1 offsets, two guard words --, the totals, longest
static void run_scan(const uint64_t *par, Reader &in, Writer &out) {
    const uint64_t n = par[0], arrays = par[1], in_shift = par[4], out_shift = par[5];
    const Blob values = in.blob();
    if (n < 1 || arrays < 1 || arrays > 2 || values.size() != arrays * n * 4u || in_shift > 3 || out_shift > 1) fail("scan: bad case");
    Arena mem;
    const uint32_t *d_in = mem.put<uint32_t>(values, in_shift * 4u);
    const uint64_t per = n + 1u + 4u, stride = per + (per & 1u);          // an even stride, so that both arrays' offsets are shifted alike
    uint64_t *d_out = mem.get<uint64_t>((arrays * stride + out_shift) * 8u, 0xA5) + out_shift;
    uint64_t *d_init = mem.get<uint64_t>(16), *d_total = mem.get<uint64_t>(16, 0xA5), *d_tiles = mem.get<uint64_t>(arrays * ((uint64_t)cdiv32(n, kScanTile) + 1u) * 8u, 0xA5);
    uint32_t *d_longest = mem.get<uint32_t>(4);
    const uint64_t inits[2] = {par[3], par[3] + 1u};
    const uint32_t longest_before = (uint32_t)par[6];
    CHECK(hipMemcpy(d_init, inits, 16, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_longest, &longest_before, 4, hipMemcpyHostToDevice));
    ScanArrays a{};
    for (uint64_t k = 0; k < arrays; ++k) {
        a.in[k] = d_in + k * n;
        a.out[k] = d_out + k * stride + 2u;
        a.init[k] = par[2] ? d_init + k : nullptr;
        a.total[k] = d_total + k;
    }
    scan_launch(a, (uint32_t)arrays, n, d_tiles, nullptr, d_longest);
    finish_launches();
    for (uint64_t k = 0; k < arrays; ++k) emit<uint64_t>(out, a.out[k] - 2u, per);
    emit<uint64_t>(out, d_total, 2);
    emit<uint32_t>(out, d_longest, 1);
}

// ------------------------------------------------------------------------------------------------ sort
// parameters: n, n_seqs, longest, what k_bam_cut finds in *out_of_order.  blobs: the keys, the records' sizes, the cuts.
// results: the sorted keys, the order, six words per cut, the plan {pos_bits, bits, passes}
static void run_sort(const uint64_t *par, Reader &in, Writer &out) {
    const uint64_t n = par[0];
    const uint32_t n_seqs = (uint32_t)par[1], longest = (uint32_t)par[2], out_of_order = (uint32_t)par[3];
    const Blob keys = in.blob(), sizes = in.blob(), cuts = in.blob();
    if (n < 1 || keys.size() != n * 8u || sizes.size() != n * 4u || cuts.size() % 8u) fail("sort: bad case");
    std::vector<BamDirEntry> dir(n);
    for (uint64_t i = 0; i < n; ++i) dir[i] = BamDirEntry{reinterpret_cast<const uint64_t *>(keys.data())[i], 0, reinterpret_cast<const uint32_t *>(sizes.data())[i], 1};
    Arena mem;
    BamDirEntry *d_dir = mem.get<BamDirEntry>(n * sizeof(BamDirEntry));
    CHECK(hipMemcpy(d_dir, dir.data(), n * sizeof(BamDirEntry), hipMemcpyHostToDevice));
    const BamSortPlan plan = bam_sort_plan(n_seqs, longest);
    const uint32_t tiles = cdiv32(n, kBamSortTile), blocks = cdiv32(n, 256);
    uint64_t *const d_keys[2] = {mem.get<uint64_t>(n * 8u, 0xA5), mem.get<uint64_t>(n * 8u, 0xA5)};
    uint32_t *const d_idx[2] = {mem.get<uint32_t>(n * 4u, 0xA5), mem.get<uint32_t>(n * 4u, 0xA5)};
    uint32_t *d_hist = mem.get<uint32_t>((uint64_t)tiles * kBamSortBins * 4u), *d_sizes = mem.get<uint32_t>(n * 4u), *d_ooo = mem.get<uint32_t>(4);
    uint64_t *d_hist_at = mem.get<uint64_t>(((uint64_t)tiles * kBamSortBins + 1u) * 8u), *d_at = mem.get<uint64_t>((n + 1u) * 8u);
    const uint64_t n_cuts = cuts.size() / 8u;
    uint64_t *d_result = mem.get<uint64_t>(n_cuts * 48u, 0xA5);
    CHECK(hipMemcpy(d_ooo, &out_of_order, 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_bam_sort_init, dim3(blocks), dim3(256), 0, nullptr, (const BamDirEntry *)d_dir, n, d_keys[0], d_idx[0]);
    const int from = bam_sort_passes(d_keys, d_idx, n, plan, d_hist, d_hist_at, [&](const uint32_t *counts, uint64_t count, uint64_t *at) { scan_one(mem, counts, count, at); }, nullptr);
    hipLaunchKernelGGL(k_bam_sorted_sizes, dim3(blocks), dim3(256), 0, nullptr, (const BamDirEntry *)d_dir, (const uint32_t *)d_idx[from], n, d_sizes);
    scan_one(mem, d_sizes, n, d_at);
    for (uint64_t c = 0; c < n_cuts; ++c)
        hipLaunchKernelGGL(k_bam_cut, dim3(1), dim3(1), 0, nullptr, (const uint64_t *)d_keys[from], n, reinterpret_cast<const uint64_t *>(cuts.data())[c], bam_unmapped_key(n_seqs),
                           (const uint64_t *)d_at, (const uint32_t *)d_ooo, d_result + 6u * c);
    finish_launches();
    emit<uint64_t>(out, d_keys[from], n);
    emit<uint32_t>(out, d_idx[from], n);
    emit<uint64_t>(out, d_result, 6u * n_cuts);
    const uint32_t p[3] = {plan.pos_bits, plan.bits, plan.passes};
    out.blob(p, sizeof p);
}

// ------------------------------------------------------------------------------------------------ gather
// parameters: n, n_final, bytes of the final records, bytes of the held ones, the destinations' offsets from a 16-byte boundary (out, held).
// blobs: the directory (n entries), the order (n indices), the staging buffer (the trial adds the library's 32 spare bytes).
// results: out and held, each with 64 marker bytes in front and behind; the held records' directory
constexpr uint32_t kMarker = 64;
static void run_gather(const uint64_t *par, Reader &in, Writer &out) {
    const uint64_t n = par[0], n_final = par[1], final_bytes = par[2], held_bytes = par[3], out_lead = par[4], held_lead = par[5];
    const Blob dir = in.blob(), idx = in.blob(), stage = in.blob();
    if (n < 1 || n_final > n || dir.size() != n * sizeof(BamDirEntry) || idx.size() != n * 4u || out_lead > 15 || held_lead > 15) fail("gather: bad case");
    Arena mem;
    const BamDirEntry *d_dir = mem.put<BamDirEntry>(dir);
    const uint32_t *d_idx = mem.put<uint32_t>(idx);
    const char *d_stage = mem.put<char>(stage, 0, 32, 0x5A);
    char *d_out = mem.get<char>(kMarker + out_lead + final_bytes + kMarker, 0xA5) + kMarker + out_lead;
    char *d_held = mem.get<char>(kMarker + held_lead + held_bytes + kMarker, 0xA5) + kMarker + held_lead;
    BamDirEntry *d_held_dir = mem.get<BamDirEntry>((n - n_final + 1u) * sizeof(BamDirEntry), 0xA5);
    uint32_t *d_sizes = mem.get<uint32_t>(n * 4u);
    uint64_t *d_at = mem.get<uint64_t>((n + 1u) * 8u);
    hipLaunchKernelGGL(k_bam_sorted_sizes, dim3(cdiv32(n, 256)), dim3(256), 0, nullptr, d_dir, d_idx, n, d_sizes);
    scan_one(mem, d_sizes, n, d_at);
    hipLaunchKernelGGL(k_bam_gather, dim3(cdiv32(n, 16)), dim3(256), 0, nullptr, d_dir, d_idx, (const uint64_t *)d_at, n, n_final, d_stage, d_out, d_held, d_held_dir);
    finish_launches();
    emit<char>(out, d_out - kMarker, kMarker + final_bytes + kMarker);
    emit<char>(out, d_held - kMarker, kMarker + held_bytes + kMarker);
    emit<BamDirEntry>(out, d_held_dir, n - n_final + 1u);
    emit<uint64_t>(out, d_at, n + 1u);
}

// ------------------------------------------------------------------------------------------------ index
// parameters: the mapped records, stream_at, n_seqs.  blobs: the directory, the order, at (n + 1), window_first (n_seqs + 1).
// results: the flags, the runs, the windows
static void run_index(const uint64_t *par, Reader &in, Writer &out) {
    const uint64_t mapped = par[0], stream_at = par[1], n_seqs = par[2];
    const Blob dir = in.blob(), idx = in.blob(), at = in.blob(), window_first = in.blob();
    if (mapped < 1 || dir.size() % sizeof(BamDirEntry) || idx.size() != mapped * 4u || at.size() != (mapped + 1u) * 8u || window_first.size() != (n_seqs + 1u) * 8u) fail("index: bad case");
    const uint64_t n_windows = reinterpret_cast<const uint64_t *>(window_first.data())[n_seqs];
    Arena mem;
    const BamDirEntry *d_dir = mem.put<BamDirEntry>(dir);
    const uint32_t *d_idx = mem.put<uint32_t>(idx);
    const uint64_t *d_at = mem.put<uint64_t>(at), *d_first = mem.put<uint64_t>(window_first);
    unsigned long long *d_windows = mem.get<unsigned long long>(n_windows * 8u, 0xFF);                  // kBamNoOffset
    uint32_t *d_flags = mem.get<uint32_t>(mapped * 4u, 0xA5);
    uint64_t *d_run_of = mem.get<uint64_t>((mapped + 1u) * 8u);
    hipLaunchKernelGGL(k_bam_index_flags, dim3(cdiv32(mapped, 256)), dim3(256), 0, nullptr, d_dir, d_idx, d_at, mapped, stream_at, d_first, d_windows, d_flags);
    scan_one(mem, d_flags, mapped, d_run_of);
    finish_launches();
    const uint64_t n_runs = fetch<uint64_t>(d_run_of + mapped, 1)[0];
    if (n_runs > mapped) fail("index: more runs than records");
    BamRunStart *d_runs = mem.get<BamRunStart>((n_runs + 1u) * sizeof(BamRunStart), 0xA5);
    hipLaunchKernelGGL(k_bam_index_runs, dim3(cdiv32(mapped, 256)), dim3(256), 0, nullptr, d_dir, d_idx, d_at, mapped, stream_at, (const uint32_t *)d_flags, (const uint64_t *)d_run_of, d_runs);
    finish_launches();
    emit<uint32_t>(out, d_flags, mapped);
    emit<BamRunStart>(out, d_runs, n_runs + 1u);
    emit<unsigned long long>(out, d_windows, n_windows + 1u);
}

// ------------------------------------------------------------------------------------------------ bins
// the stand-in for k_pair_tiles / k_record_tiles: the keys are given, the histogram is the library's
__global__ void __launch_bounds__(kBinBlock) k_trial_keys(const uint16_t *key_of, uint64_t n, uint32_t n_keys, uint32_t *hist) {
    __shared__ uint32_t s_hist[kBinKeysLds];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    bin_count_key(valid ? key_of[i] : 0u, valid, n_keys, hist, s_hist);
}
// parameters: n, n_keys, n_bins, fragments carried along.  blobs: the keys, the fragments (or none).
// results: the small arrays as build_fill_bins lays them out -- [hist n_keys][cursor n_keys][bin_first n_bins][bin_count n_bins][next_chunk n_bins][workers n_bins]
// [chunk_ptr n_bins + 1] and one guard word --, the cursors as the plan left them, perm (n and one guard word), the fragments in perm's order
static void run_bins(const uint64_t *par, Reader &in, Writer &out) {
    const uint64_t n = par[0];
    const uint32_t n_keys = (uint32_t)par[1], n_bins = (uint32_t)par[2];
    const Blob keys = in.blob(), frags = in.blob();
    if (n < 1 || n >= 0xFFFFFFFFull || n_keys < 1 || n_keys > 65536 || n_bins % n_keys || keys.size() != n * 2u || (par[3] && frags.size() != n * sizeof(Fragment))) fail("bins: bad case");
    for (uint64_t i = 0; i < n; ++i)
        if (reinterpret_cast<const uint16_t *>(keys.data())[i] >= n_keys) fail("bins: a key outside the case's keys");
    Arena mem;
    const uint16_t *d_keys = mem.put<uint16_t>(keys);
    const Fragment *d_frags = par[3] ? mem.put<Fragment>(frags) : nullptr;
    Fragment *d_frags_sorted = par[3] ? mem.get<Fragment>(n * sizeof(Fragment), 0xA5) : nullptr;
    const uint64_t words = 2u * (uint64_t)n_keys + 5u * (uint64_t)n_bins + 1u;
    uint32_t *hist = mem.get<uint32_t>((words + 1u) * 4u, 0xA5), *cursor = hist + n_keys, *bin_first = cursor + n_keys, *bin_count = bin_first + n_bins, *next_chunk = bin_count + n_bins,
             *workers = next_chunk + n_bins, *chunk_ptr = workers + n_bins;
    uint32_t *d_perm = mem.get<uint32_t>((n + 1u) * 4u, 0xA5);
    CHECK(hipMemsetAsync(hist, 0, (size_t)n_keys * 4u, nullptr));
    hipLaunchKernelGGL(k_trial_keys, dim3(cdiv32(n, kBinBlock)), dim3(kBinBlock), 0, nullptr, d_keys, n, n_keys, hist);
    hipLaunchKernelGGL(k_bins_plan, dim3(1), dim3(1024), 0, nullptr, (const uint32_t *)hist, n_keys, n_bins, bin_first, bin_count, cursor, chunk_ptr, next_chunk, workers);
    finish_launches();
    const std::vector<uint32_t> planned = fetch<uint32_t>(cursor, n_keys);
    hipLaunchKernelGGL(k_bin_scatter, dim3(cdiv32(n, kBinBlock * kBinItemsPerThread)), dim3(kBinBlock), 0, nullptr, d_keys, n, n_keys, cursor, d_perm, d_frags, (const FragmentVar *)nullptr,
                       d_frags_sorted, (FragmentVar *)nullptr);
    finish_launches();
    emit<uint32_t>(out, hist, words + 1u);
    out.blob(planned.data(), planned.size() * 4u);
    emit<uint32_t>(out, d_perm, n + 1u);
    emit<Fragment>(out, d_frags_sorted, par[3] ? n : 0u);
}

// ------------------------------------------------------------------------------------------------ fasta
// parameters: the text pointer's offset from a 256-byte boundary.  blob: the text.
// results: the tiles' counts, at (the starts and the text's length, one guard word), k_fasta_lead's flag
static void run_fasta(const uint64_t *par, Reader &in, Writer &out) {
    const Blob text = in.blob();
    const uint64_t text_len = text.size(), shift = par[0];
    if (text_len < 1 || text_len >= 0xFFFFFFF0ull || shift > 255) fail("fasta: bad case");
    Arena mem;
    const uint8_t *d_text = mem.put<uint8_t>(text, shift, 0, '>');                                       // (a start in front of or behind the text is not one of the text)
    const uint32_t n_tiles = cdiv32(text_len, fasta::kTileBytes);
    uint32_t *d_counts = mem.get<uint32_t>((uint64_t)n_tiles * 4u, 0xA5);
    uint64_t *d_first = mem.get<uint64_t>(((uint64_t)n_tiles + 1u) * 8u);
    const dim3 tgrid(cdiv32(n_tiles, fasta::kStartsBlock / 64u)), tblock(fasta::kStartsBlock);
    hipLaunchKernelGGL(fasta::k_fasta_count, tgrid, tblock, 0, nullptr, d_text, text_len, n_tiles, d_counts);
    scan_one(mem, d_counts, n_tiles, d_first);
    finish_launches();
    const uint64_t starts = fetch<uint64_t>(d_first + n_tiles, 1)[0];
    if (starts > text_len) fail("fasta: more starts than bytes");
    uint32_t *d_at = mem.get<uint32_t>((starts + 2u) * 4u, 0xA5);
    hipLaunchKernelGGL(fasta::k_fasta_starts, tgrid, tblock, 0, nullptr, d_text, text_len, n_tiles, (const uint64_t *)d_first, d_at);
    finish_launches();
    const uint32_t lead_end = fetch<uint32_t>(d_at, 1)[0];
    if (lead_end > text_len) fail("fasta: the first start lies behind the text");
    uint32_t *d_summary = mem.get<uint32_t>(16);
    if (lead_end) hipLaunchKernelGGL(fasta::k_fasta_lead, dim3(std::min(1024u, cdiv32(lead_end, 256))), dim3(256), 0, nullptr, d_text, lead_end, d_summary);
    finish_launches();
    emit<uint32_t>(out, d_counts, n_tiles);
    emit<uint32_t>(out, d_at, starts + 2u);
    emit<uint32_t>(out, d_summary, 4);
}

// ------------------------------------------------------------------------------------------------ guarded buffers of the families below
// `count` elements between kMarker guard bytes (0xA5) on either side; emitted with both, so that the checker sees what was written in front of and behind them
template <class T>
static T *guarded(Arena &mem, uint64_t count, uint64_t shift_bytes = 0) {
    return reinterpret_cast<T *>(mem.get<char>(kMarker + shift_bytes + count * sizeof(T) + kMarker, 0xA5) + kMarker + shift_bytes);
}
template <class T>
static T *guarded_put(Arena &mem, const Blob &b) {
    return reinterpret_cast<T *>(mem.put<char>(b, kMarker, kMarker, 0xA5));
}
template <class T>
static void emit_guarded(Writer &w, const T *dev, uint64_t count) {
    emit<char>(w, reinterpret_cast<const char *>(dev) - kMarker, kMarker + count * sizeof(T) + kMarker);
}
// the address of element 0 of an array of which only the elements from `base` on exist, at `window`: element p is window[p - base]
template <class T>
static const T *moved_back(const T *window, uint64_t base) {
    return reinterpret_cast<const T *>(reinterpret_cast<uintptr_t>(window) - (uintptr_t)(base * sizeof(T)));
}
// a name table of one sequence
static NameTable one_name(Arena &mem, const Blob &name) {
    NameTable names{};
    names.names = mem.put<char>(name, 0, 8);
    const uint32_t ptr[2] = {0u, (uint32_t)name.size()};
    uint32_t *d_ptr = mem.get<uint32_t>(8);
    CHECK(hipMemcpy(d_ptr, ptr, 8, hipMemcpyHostToDevice));
    names.name_ptr = d_ptr;
    return names;
}

// ------------------------------------------------------------------------------------------------ depthscan
// parameters: tiles.  blob: tiles * kDepthTile words.
// results: the array after the three launches of rsq_sim_depth_finish, tile_sums (the library's tiles * 4 + 16 bytes lie inside the guards' reach), both guarded
static void run_depthscan(const uint64_t *par, Reader &in, Writer &out) {
    const uint64_t tiles = par[0];
    const Blob values = in.blob();
    if (tiles < 1 || tiles > 65536 || values.size() != tiles * kDepthTile * 4u) fail("depthscan: bad case");
    Arena mem;
    uint32_t *d_a = guarded_put<uint32_t>(mem, values), *d_sums = guarded<uint32_t>(mem, tiles);
    hipLaunchKernelGGL(k_depth_tile_sums, dim3((uint32_t)tiles), dim3(kDepthBlock), 0, nullptr, (const uint32_t *)d_a, d_sums);
    hipLaunchKernelGGL(k_depth_tiles, dim3(1), dim3(kDepthTilesBlock), 0, nullptr, d_sums, (uint32_t)tiles);
    hipLaunchKernelGGL(k_depth_apply, dim3((uint32_t)tiles), dim3(kDepthBlock), 0, nullptr, d_a, (const uint32_t *)d_sums);
    finish_launches();
    emit_guarded<uint32_t>(out, d_a, tiles * kDepthTile);
    emit_guarded<uint32_t>(out, d_sums, tiles);
}

// ------------------------------------------------------------------------------------------------ bedgraph
// parameters: len, base (a multiple of 32; the first piece's carry), the text's offset from a 16-byte boundary, the bytes of all pieces' text (the destination's
// capacity: a piece that needs more ends the trial).  blobs: the depths of [base, len], the name, the piece bounds (uint64, rising from base).
// The pieces in order as rsq_sim_depth_bedgraph runs them, their texts one behind the other.  results: {lines, bytes, carry after it} per piece; the text, guarded
static void run_bedgraph(const uint64_t *par, Reader &in, Writer &out) {
    const uint64_t len = par[0], base = par[1], lead = par[2], cap = par[3];
    const Blob depths = in.blob(), name = in.blob(), bounds_blob = in.blob();
    const uint64_t *bounds = reinterpret_cast<const uint64_t *>(bounds_blob.data()), n_bounds = bounds_blob.size() / 8u;
    if (len < 1 || len > 0xFFFFFFFFull || base >= len || base % 32u || lead > 15 || depths.size() != (len - base + 1u) * 4u || name.empty() || n_bounds < 2 || bounds_blob.size() % 8u ||
        bounds[0] != base || bounds[n_bounds - 1u] > len)
        fail("bedgraph: bad case");
    for (uint64_t k = 1; k < n_bounds; ++k)
        if (bounds[k] < bounds[k - 1u]) fail("bedgraph: the bounds fall");
    Arena mem;
    const uint32_t *d = moved_back(mem.put<uint32_t>(depths, kMarker, kMarker, 0xA5), base);
    const NameTable names = one_name(mem, name);
    const uint32_t name_len = (uint32_t)name.size(), lds = depth_lds_bytes(name_len);
    char *d_dst = guarded<char>(mem, cap, lead);
    uint64_t at = 0;
    uint32_t carry = (uint32_t)base;
    std::vector<uint64_t> per_piece;
    for (uint64_t k = 0; k + 1u < n_bounds; ++k) {
        const uint64_t lo = bounds[k], n = bounds[k + 1u] - lo;
        uint64_t lines = 0, bytes = 0;
        if (n) {
            Arena piece;
            uint32_t *d_flags = piece.get<uint32_t>(n * 4u + 16u, 0xA5);
            uint64_t *d_rank = piece.get<uint64_t>((n + 1u) * 8u);
            hipLaunchKernelGGL(k_depth_ends, dim3(cdiv32(n, 256)), dim3(256), 0, nullptr, d, (uint32_t)len, (uint32_t)lo, n, d_flags);
            scan_one(piece, d_flags, n, d_rank);
            finish_launches();
            lines = fetch<uint64_t>(d_rank + n, 1)[0];
            if (lines > n) fail("bedgraph: more lines than positions");
            if (lines) {
                uint32_t *d_ends = piece.get<uint32_t>(lines * 4u + 16u, 0xA5), *d_sizes = piece.get<uint32_t>(lines * 4u + 16u, 0xA5);
                uint64_t *d_offsets = piece.get<uint64_t>((lines + 1u) * 8u);
                hipLaunchKernelGGL(k_depth_run_ends, dim3(cdiv32(n, 256)), dim3(256), 0, nullptr, (const uint32_t *)d_flags, (const uint64_t *)d_rank, (uint32_t)lo, n, d_ends);
                hipLaunchKernelGGL(k_depth_line_sizes, dim3(cdiv32(lines, 256)), dim3(256), 0, nullptr, d, (const uint32_t *)d_ends, lines, carry, name_len, d_sizes);
                scan_one(piece, d_sizes, lines, d_offsets);
                finish_launches();
                bytes = fetch<uint64_t>(d_offsets + lines, 1)[0];
                const uint32_t last_end = fetch<uint32_t>(d_ends + (lines - 1u), 1)[0];
                if (bytes > cap - at) fail("bedgraph: a piece's text does not fit what the case allows");
                hipLaunchKernelGGL(k_depth_text, dim3(cdiv32(lines, kDepthLines)), dim3(64), lds, nullptr, names, 0u, d, (const uint32_t *)d_ends, carry, lines, (const uint64_t *)d_offsets,
                                   d_dst + at, lds);
                finish_launches();
                carry = last_end;
                at += bytes;
            }
        }
        per_piece.insert(per_piece.end(), {lines, bytes, (uint64_t)carry});
    }
    out.blob(per_piece.data(), per_piece.size() * 8u);
    emit_guarded<char>(out, d_dst, cap);
}

// ------------------------------------------------------------------------------------------------ pileup
// parameters: the window's length n, base (a multiple of 32), sets, all, the text's offset from a 16-byte boundary, the rows' offset from one in words, the bytes
// of all pieces' text.  blobs: the planes [sets * 8][n], the packed reference codes of the window (uint64), the name, the piece bounds (uint64, rising from base).
// results: the rows of the window (rsq_sim_pileup_counts); per piece, as rsq_sim_pileup_text runs it, flags, sizes, {lines, bytes}, line_pos, offsets; the text.
// Every array guarded.
static void run_pileup(const uint64_t *par, Reader &in, Writer &out) {
    const uint64_t n_all = par[0], base = par[1], sets = par[2], all = par[3], lead = par[4], rows_shift = par[5], cap = par[6];
    const Blob planes = in.blob(), ref = in.blob(), name = in.blob(), bounds_blob = in.blob();
    const uint64_t *bounds = reinterpret_cast<const uint64_t *>(bounds_blob.data()), n_bounds = bounds_blob.size() / 8u;
    if (n_all < 1 || base + n_all > 0xFFFFFFFFull || base % 32u || sets < 1 || sets > 2 || all > 1 || lead > 15 || rows_shift > 3 || planes.size() != sets * kPileupPlanes * n_all * 4u ||
        ref.size() != (n_all + 31u) / 32u * 8u || name.empty() || n_bounds < 2 || bounds_blob.size() % 8u || bounds[0] != base || bounds[n_bounds - 1u] > base + n_all)
        fail("pileup: bad case");
    for (uint64_t k = 1; k < n_bounds; ++k)
        if (bounds[k] < bounds[k - 1u]) fail("pileup: the bounds fall");
    Arena mem;
    const uint64_t words = n_all;
    const uint32_t *at = moved_back(mem.put<uint32_t>(planes, kMarker, kMarker, 0xA5), base);
    const uint64_t *ref_words = moved_back(mem.put<uint64_t>(ref, kMarker, kMarker, 0xA5), base / 32u);
    const NameTable names = one_name(mem, name);
    const uint32_t name_len = (uint32_t)name.size(), lds = pileup_lds_bytes(name_len, (uint32_t)sets);
    uint32_t *d_rows = guarded<uint32_t>(mem, n_all * sets * kPileupPlanes, rows_shift * 4u);
    hipLaunchKernelGGL(k_pileup_rows, dim3(cdiv32(n_all, 256)), dim3(256), 0, nullptr, at, words, (uint32_t)sets, ref_words, (uint32_t)base, n_all, d_rows);
    finish_launches();
    emit_guarded<uint32_t>(out, d_rows, n_all * sets * kPileupPlanes);
    char *d_dst = guarded<char>(mem, cap, lead);
    uint64_t text_at = 0;
    for (uint64_t k = 0; k + 1u < n_bounds; ++k) {
        const uint64_t lo = bounds[k], n = bounds[k + 1u] - lo;
        Arena piece;
        uint32_t *d_flags = guarded<uint32_t>(piece, n), *d_sizes = guarded<uint32_t>(piece, n);
        uint64_t lines = 0, bytes = 0;
        uint64_t *d_rank = piece.get<uint64_t>((n + 1u) * 8u), *d_at_pos = piece.get<uint64_t>((n + 1u) * 8u);
        if (n) {
            uint64_t *d_tiles = piece.get<uint64_t>(2u * ((uint64_t)cdiv32(n, kScanTile) + 1u) * 8u), *d_totals = piece.get<uint64_t>(16);      // (exclusive_scans: the totals' scratch)
            hipLaunchKernelGGL(k_pileup_lines, dim3(cdiv32(n, 256)), dim3(256), 0, nullptr, at, words, (uint32_t)sets, ref_words, (uint32_t)lo, n, (uint32_t)all, name_len, d_flags, d_sizes);
            scan_launch(ScanArrays{{d_flags, d_sizes}, {d_rank, d_at_pos}, {nullptr, nullptr}, {d_totals, d_totals + 1}}, 2, n, d_tiles, nullptr, nullptr);
            finish_launches();
            lines = fetch<uint64_t>(d_rank + n, 1)[0];
            bytes = fetch<uint64_t>(d_at_pos + n, 1)[0];
            if (lines > n) fail("pileup: more lines than positions");
        }
        uint32_t *d_line_pos = guarded<uint32_t>(piece, lines);
        uint64_t *d_offsets = guarded<uint64_t>(piece, lines ? lines + 1u : 0u);
        if (lines) {
            if (bytes > cap - text_at) fail("pileup: a piece's text does not fit what the case allows");
            hipLaunchKernelGGL(k_pileup_place, dim3(cdiv32(n + 1u, 256)), dim3(256), 0, nullptr, (const uint32_t *)d_flags, (const uint64_t *)d_rank, (const uint64_t *)d_at_pos, (uint32_t)lo, n,
                               d_line_pos, d_offsets);
            hipLaunchKernelGGL(k_pileup_text, dim3(cdiv32(lines, kPileupLines)), dim3(64), lds, nullptr, names, 0u, at, words, (uint32_t)sets, ref_words, (const uint32_t *)d_line_pos, lines,
                               (const uint64_t *)d_offsets, d_dst + text_at, lds);
            finish_launches();
            text_at += bytes;
        }
        emit_guarded<uint32_t>(out, d_flags, n);
        emit_guarded<uint32_t>(out, d_sizes, n);
        const uint64_t counts[2] = {lines, bytes};
        out.blob(counts, sizeof counts);
        emit_guarded<uint32_t>(out, d_line_pos, lines);
        emit_guarded<uint64_t>(out, d_offsets, lines ? lines + 1u : 0u);
    }
    emit_guarded<char>(out, d_dst, cap);
}

// ------------------------------------------------------------------------------------------------ stats
static_assert(sizeof(ReadMeta) == 16, "the trial builds the read kernel's ReadMeta entries");
// the stand-in for k_stats_mates' walk: per round every lane takes {index, on, index2, v} from memory, calls shared(index, on) with its whole wave and add(index2, v);
// the image is cleared and flushed as k_stats_mates does it
__global__ void __launch_bounds__(kStatsMatesBlock) k_trial_shared(const uint32_t *rounds, uint32_t n_rounds, uint32_t image_words, uint64_t *counts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_trial[];
    for (uint32_t i = threadIdx.x; i < image_words; i += kStatsMatesBlock) s_trial[i] = 0u;
    __syncthreads();
    const StatsMatesAdd a{s_trial, counts, image_words};
    for (uint32_t r = 0; r < n_rounds; ++r) {
        const uint32_t *e = rounds + ((uint64_t)r * kStatsMatesBlock + threadIdx.x) * 4u;
        a.shared(e[0], e[1] != 0u);
        a.add(e[2], e[3]);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < image_words; i += kStatsMatesBlock)
        if (const uint32_t v = s_trial[i]) stats_flush_add(counts + i, v);
}
// parameters: 0, n_pairs, len0, len1, Q, phred, row_words, pitch, chunk, slab, groups (chunk, slab, groups 0: the library's choice, stats_rows_geometry as
// stats_take calls it), skew.  blobs: the seq words and the qual words [row_words][pitch], read_len (uint16) of the 2 n_pairs rows.
// results: the layout {off of base_quality, of base_call, of bad, words}; the counts of stats_layout(len0, len1, 0, Q, 1, phred), guarded
// parameters: 1, the words of the counts, image_words, workgroups.  blob: the rounds [round][256]{index, on, index2, v}.  result: the counts, guarded
static void run_stats(const uint64_t *par, Reader &in, Writer &out) {
    Arena mem;
    if (par[0] == 1u) {
        const uint64_t words = par[1], image_words = par[2], groups = par[3];
        const Blob rounds = in.blob();
        const uint64_t n_rounds = rounds.size() / (kStatsMatesBlock * 16u);
        if (words < 1 || image_words > words || image_words * 4u > kStatsMatesLds || groups < 1 || groups > 64 || rounds.size() % (kStatsMatesBlock * 16u)) fail("stats: bad case of shared adds");
        for (uint64_t i = 0; i < rounds.size() / 16u; ++i) {
            const uint32_t *e = reinterpret_cast<const uint32_t *>(rounds.data()) + 4u * i;
            if (e[0] >= words || e[2] >= words) fail("stats: an index outside the counts");
        }
        uint64_t *d_counts = guarded<uint64_t>(mem, words);
        CHECK(hipMemset(d_counts, 0, words * 8u));
        hipLaunchKernelGGL(k_trial_shared, dim3((uint32_t)groups), dim3(kStatsMatesBlock), (uint32_t)image_words * 4u, nullptr, mem.put<uint32_t>(rounds), (uint32_t)n_rounds, (uint32_t)image_words,
                           d_counts);
        finish_launches();
        emit_guarded<uint64_t>(out, d_counts, words);
        return;
    }
    const uint64_t n_pairs = par[1], pitch = par[7];
    const uint32_t len0 = (uint32_t)par[2], len1 = (uint32_t)par[3], Q = (uint32_t)par[4], phred = (uint32_t)par[5], row_words = (uint32_t)par[6];
    const bool skew = par[11] != 0;
    const Blob seq = in.blob(), qual = in.blob(), lens = in.blob();
    if (par[0] || n_pairs < 1 || n_pairs > (1u << 24) || !(len0 | len1) || len0 > 4096 || len1 > 4096 || Q < 1 || Q > 250 || row_words < 1 || pitch < 2u * n_pairs ||
        seq.size() != (uint64_t)row_words * pitch * 4u || qual.size() != seq.size() || lens.size() != 4u * n_pairs || par[8] % 4u || par[8] > 1024)
        fail("stats: bad case of rows");
    const StatsLayout y = stats_layout(len0, len1, 0u, Q, 1u, phred);
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const StatsRowsGeometry geo = stats_rows_geometry(y.lmax, len0, len1, Q, skew, row_words, (uint32_t)prop.multiProcessorCount, n_pairs, (int64_t)par[8], (int64_t)par[9], (int64_t)par[10]);
    if (geo.lds > 64u * 1024u) fail("stats: the image does not fit the LDS");
    std::vector<ReadMeta> meta(2u * n_pairs, ReadMeta{});
    for (uint64_t r = 0; r < 2u * n_pairs; ++r) meta[r].read_len = reinterpret_cast<const uint16_t *>(lens.data())[r];
    ReadMeta *d_meta = mem.get<ReadMeta>(meta.size() * sizeof(ReadMeta));
    CHECK(hipMemcpy(d_meta, meta.data(), meta.size() * sizeof(ReadMeta), hipMemcpyHostToDevice));
    const uint32_t *d_seq = mem.put<uint32_t>(seq), *d_qual = mem.put<uint32_t>(qual);
    uint64_t *d_counts = guarded<uint64_t>(mem, y.words);
    CHECK(hipMemset(d_counts, 0, (uint64_t)y.words * 8u));
    if (skew) hipLaunchKernelGGL(k_stats_rows<true>, dim3(geo.groups), dim3(kStatsRowsBlock), geo.lds, nullptr, d_seq, d_qual, (const ReadMeta *)d_meta, pitch, n_pairs, y, geo.plan, d_counts);
    else hipLaunchKernelGGL(k_stats_rows<false>, dim3(geo.groups), dim3(kStatsRowsBlock), geo.lds, nullptr, d_seq, d_qual, (const ReadMeta *)d_meta, pitch, n_pairs, y, geo.plan, d_counts);
    finish_launches();
    const uint32_t layout[4] = {y.off[kStBaseQuality], y.off[kStBaseCall], y.off[kStBad], y.words};
    out.blob(layout, sizeof layout);
    emit_guarded<uint64_t>(out, d_counts, y.words);
}

int main(int argc, char **argv) {
    if (argc != 4) fail("usage: kernel_trial FAMILY input.bin output.bin");
    const std::string family = argv[1];
    void (*run)(const uint64_t *, Reader &, Writer &) = family == "scan" ? run_scan : family == "sort" ? run_sort : family == "gather" ? run_gather : family == "index" ? run_index
                                                        : family == "bins" ? run_bins : family == "fasta" ? run_fasta : family == "depthscan" ? run_depthscan
                                                        : family == "bedgraph" ? run_bedgraph : family == "pileup" ? run_pileup : family == "stats" ? run_stats : nullptr;
    if (!run) fail("no such family: " + family);
    Reader in{fopen(argv[2], "rb")};
    Writer out{fopen(argv[3], "wb")};
    if (!in.f || !out.f) fail("cannot open the files");
    CHECK(hipSetDevice(0));
    const uint64_t cases = in.word();
    for (uint64_t c = 0; c < cases; ++c) {
        uint64_t par[16];
        for (uint64_t &p : par) p = in.word();
        run(par, in, out);
    }
    if (fclose(out.f)) fail("cannot write the output");
    printf("%s: %llu cases\n", family.c_str(), (unsigned long long)cases);
    return 0;
}
