// rsq_sim.hip -- the simulator object behind the C ABI (include/reseq_amd.h): packs profile + reference into
// HBM, gives the pre-passes (rsq_prepass.h) their kernels and drives the kernels of the stages' headers (rsq_chains.h, rsq_sieve.h, rsq_scan.h, rsq_reads.h, rsq_format.h).  Compiled for gfx950 only.
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <math.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <thread>
#include <type_traits>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/reseq_amd.h"
#include "rsq_deflate.h"
#include "rsq_fasta.h"
#include "rsq_chains.h"
#include "rsq_sieve.h"
#include "rsq_scan.h"
#include "rsq_text.h"
#include "rsq_reads.h"
#include "rsq_format.h"
#include "rsq_sam.h"
#include "rsq_bam.h"
#include "rsq_md.h"
#include "rsq_bamsort.h"
#include "rsq_depth.h"
#include "rsq_pileup.h"
#include "rsq_stats.h"
#include "rsq_alleles.h"
#include "rsq_pack.h"
#include "rsq_prepass.h"
#include "rsq_spec.h"
#include "rsq_textio.h"

namespace rsq {

static thread_local std::string g_last_error, g_last_warning;

struct HipError : Error {
    using Error::Error;
};
#define HIP_CHECK(expr)                                                                                       \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) throw HipError(std::string(#expr) + ": " + hipGetErrorString(e_));              \
    } while (0)

// ------------------------------------------------------------------------------------------ device memory
class DevBuf {
   public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    ~DevBuf() { if (p_) (void)hipFree(p_); }
    void reserve(size_t bytes) {                   // grow-only
        if (bytes <= bytes_) return;
        if (p_) {
            HIP_CHECK(hipDeviceSynchronize());     // a pipelined call may still read the old array on another stream
            HIP_CHECK(hipFree(p_));
        }
        p_ = nullptr;
        bytes_ = 0;
        HIP_CHECK(hipMalloc(&p_, bytes ? bytes : 8));
        bytes_ = bytes;
    }
    template <class T>
    void upload(const std::vector<T> &v) {
        reserve(v.size() * sizeof(T) + 8);
        if (!v.empty()) HIP_CHECK(hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    void release() {
        if (p_) {
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipFree(p_));
        }
        p_ = nullptr;
        bytes_ = 0;
    }
    void reserve_keeping(size_t bytes, size_t keep, hipStream_t st) {      // grow-only, the first `keep` bytes kept: copied on `st`, which is idle afterwards
        if (bytes <= bytes_) return;
        DevBuf bigger;
        bigger.reserve(bytes);
        if (keep) HIP_CHECK(hipMemcpyAsync(bigger.p_, p_, keep, hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::swap(p_, bigger.p_);
        std::swap(bytes_, bigger.bytes_);
    }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p_); }
    size_t bytes() const { return bytes_; }

   private:
    void *p_ = nullptr;
    size_t bytes_ = 0;
};

}  // namespace rsq
#include "rsq_s2i.h"
namespace rsq {

struct Timer {                                     // HIP events on the stream the kernels are launched on; a call may time several launches (sub-ranges)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t used = 0;
    size_t marks = 0;                              // launches counted without being timed: which of two routes a call took (rsq_sim_last_kernel_launches)
    Timer() = default;
    Timer(const Timer &) = delete;
    Timer &operator=(const Timer &) = delete;
    ~Timer() {
        for (auto &e : events) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    }
    void reset() { used = marks = 0; }
    void mark() { ++marks; }
    void start(hipStream_t st) {
        if (used == events.size()) {
            hipEvent_t a, b;
            HIP_CHECK(hipEventCreate(&a));
            HIP_CHECK(hipEventCreate(&b));
            events.emplace_back(a, b);
        }
        HIP_CHECK(hipEventRecord(events[used].first, st));
    }
    void stop(hipStream_t st) {
        HIP_CHECK(hipEventRecord(events[used].second, st));
        ++used;
    }
    double ms() const {                            // sum over the launches since reset()
        double sum = 0.0;
        for (size_t i = 0; i < used; ++i) {
            float t = 0;
            if (hipEventElapsedTime(&t, events[i].first, events[i].second) == hipSuccess) sum += t;
        }
        return sum;
    }
    size_t launches() const { return used + marks; }
};

}  // namespace rsq

using namespace rsq;

struct rsq_profile {
    Profile p;
};
struct rsq_ref {
    Reference r;
    Variants variants;
    bool has_variants = false;
};

// arrays packed by rsq_pack.h go to HBM; they live as long as the simulator
struct DeviceUploader : Uploader {
    std::vector<std::unique_ptr<DevBuf>> owned[kUploadScopes];
    int device = 0;
    void bind_thread() override { HIP_CHECK(hipSetDevice(device)); }
    void release_scope(int scope) override {
        HIP_CHECK(hipDeviceSynchronize());                         // nothing may still read what goes away
        owned[scope].clear();
    }
    void *put_bytes(const void *data, size_t bytes) override {
        std::vector<std::unique_ptr<DevBuf>> &own = owned[current_scope];
        own.emplace_back(new DevBuf());
        own.back()->reserve(bytes + 8);
        HIP_CHECK(hipMemcpy(own.back()->as<void>(), data, bytes, hipMemcpyHostToDevice));
        return own.back()->as<void>();
    }
    void *put_zeros(size_t bytes) override {
        std::vector<std::unique_ptr<DevBuf>> &own = owned[current_scope];
        own.emplace_back(new DevBuf());
        own.back()->reserve(bytes + 8);
        HIP_CHECK(hipMemset(own.back()->as<void>(), 0, bytes + 8));
        return own.back()->as<void>();
    }
    void write_bytes(void *dst, const void *src, size_t bytes) override { HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); }
    void read_bytes(void *dst_host, const void *src, size_t bytes) override { HIP_CHECK(hipMemcpy(dst_host, src, bytes, hipMemcpyDeviceToHost)); }
};

struct MappedFile {                                                   // a whole file, read-only
    const char *data = nullptr;
    size_t size = 0;
    explicit MappedFile(const char *path) {
        const int fd = open(path, O_RDONLY);
        if (fd < 0) throw Error(std::string("cannot open ") + path + ": " + strerror(errno));
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size <= 0) {
            close(fd);
            throw Error(std::string(path) + " is empty or cannot be examined");
        }
        size = (size_t)st.st_size;
        void *p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (p == MAP_FAILED) throw Error(std::string("cannot map ") + path);
        data = static_cast<const char *>(p);
    }
    ~MappedFile() {
        if (data) munmap(const_cast<char *>(data), size);
    }
    MappedFile(const MappedFile &) = delete;
    MappedFile &operator=(const MappedFile &) = delete;
};

// ------------------------------------------------------------------------------------------------ rsq_sim
struct rsq_sim : PrepassSim {
    int device = 0;
    DeviceUploader up;
    // workspace of the hot path (grow-only): two sets, so that the sieve of one sub-range of a call can run beside the FASTQ text of the one before it
    struct Workspace {
        DevBuf fvars;                  // FragmentVar per fragment (variants of any kind)
        DevBuf slot_table;             // SlotInfo per slot of the batch (variants of any kind)
        DevBuf counts, offsets, tile_sums, scan_total, frags, raw_seq, raw_qual, raw_ops, raw_meta, sizes, off_r1, off_r2, fill_counters, hits, hit_count, cands, pairs_of, pair_off, templates, rec_flags, rec_index, rec_count;
        DevBuf bin_keys, bin_small, bin_perm, bin_frags, bin_fvars;      // reads binned by tile: key per item; histogram, bins, counters (one small buffer); the sorted items
        DevBuf fa_counts, fa_first, fa_at, fa_len, fa_id_len, fa_frag_len, fa_seg, fa_codes, fa_summary;      // rsq_sim_error_model_fasta (rsq_fasta.h)
        DevBuf sam_sizes, sam_side, off_sam;      // truth alignments (rsq_sam.h): bytes per pair, both mates' walks per raw row, the pairs' offsets in the SAM text
        DevBuf bam_side;                          // the same calls with BAM records (rsq_bam.h): their side entries; sizes and offsets live in sam_sizes / off_sam
        DevBuf cell_info;              // the sieve without variants: per candidate the first strand's count and the two strands (k_sieve_finish<0> -> k_sieve_emit<0>)
        hipEvent_t text_done = nullptr;      // the text stage that last read this set's arrays
    } ws[2];
    // rsq_sim_job_generate: the FASTQ text of a rank's block range, kept until rsq_sim_job_write / rsq_sim_job_free: per file a list of device arrays, filled in order
    struct JobText {
        std::vector<std::unique_ptr<DevBuf>> chunks[2];
        std::vector<size_t> used[2];
        uint64_t bytes[2] = {0, 0};
        bool complete = false;         // rsq_sim_job_generate ran to its end: the text is whole (not: never generated, freed, or left half-made by a failed call)
        std::vector<unsigned char> packed[2];      // rsq_sim_job_compress: the text as gzip members in host memory (the device arrays are released, bytes[] = these sizes)
        bool is_packed = false;
        bool device_packed = false;                // rsq_sim_job_compress on the device: chunks[] hold gzip members instead of text (used[] and bytes[] their sizes)
        void clear() {
            complete = false;
            is_packed = false;
            device_packed = false;
            for (auto &p : packed) std::vector<unsigned char>().swap(p);
            for (int f = 0; f < 2; ++f) {
                chunks[f].clear();
                used[f].clear();
                bytes[f] = 0;
            }
        }
    } job;
    DevBuf totals;                 // [sub-ranges + 1][2] bytes of FASTQ text in front of a sub-range, per file
    bool gz_dense = false;                                 // the route of the code in gz_codes: every position searched and probed (gz::dense_pays), else FASTQ by its lines
    bool gz_keep_code = false, gz_have_code = false;      // rsq_sim_gzip_keep_code: the code of the first call serves the calls after it
    DevBuf gz_slots, gz_sizes, gz_at, gz_hist, gz_codes, gz_total;      // gzip on the device (rsq_deflate.h): the members' slots, their sizes and places, the sample's counts, the call's code
    Workspace *cur = &ws[0];       // the set the stage being enqueued works on
    hipStream_t side[2] = {nullptr, nullptr};      // the sieve's and the text's stream of a pipelined call
    hipEvent_t ev_call = nullptr, ev_fill = nullptr, ev_emit = nullptr;
    std::map<std::string, Timer> timers;
    uint32_t n_cu = 256;
    // Pinned host words (one hipHostMalloc) the few device-to-host scalars of a call land in: one name, one meaning and one user each, 4 bytes wide where the copy is
    struct Mailbox {
        struct Sieve {                 // sieve_attempt -> sieve_collect, one per workspace: the sieve of part k + 1 is launched before the call of part k ends
            uint64_t total, n_cands;   // pairs of the range; candidates its lists would have needed
            uint32_t n_hits;
        } sieve[2];
        uint64_t r1_bytes, r2_bytes, truth_bytes;                // finish_call: one 16-byte copy fills the first two
        uint32_t walk_error, longest_record, truth_longest;      // finish_call: the call's longest FASTQ record and longest pair of truth records
        uint32_t bad_fragment;                         // check_fragment_lengths: the first record whose fragment length has no row, sent out as "none" and read back
        uint64_t text_bytes, fasta_starts;             // error_model_text; rsq_sim_error_model_fasta: record starts in the block of text
        uint32_t text_longest;                         // error_model_text
        struct {                                       // rsq_sim_error_model_fasta: rsq_fasta.h `summary`, sent out as its initial state and read back
            uint32_t longest, first_bad, stray_text, spare;
        } fasta_summary;
        uint32_t fasta_lead_end, fasta_last_start;     // rsq_sim_error_model_fasta: the first and the last record start
    } *mailbox = nullptr;
    uint64_t format_record_bytes = 480;      // the longest FASTQ record of the last rsq_sim_pairs call and a few bytes (text_stage sizes the formatter's LDS image with it)
    DevBuf longest_record;                   // where a call's text stages leave it
    DevBuf sam_totals, sam_longest;          // rsq_sim_pairs_sam: [sub-ranges + 1] bytes of SAM text in front of a sub-range; the call's longest pair of records
    uint64_t sam_pair_bytes = 1100;          // that of the last call and a few bytes (sam_stage sizes the writer's LDS image with it)
    uint64_t bam_pair_bytes = 700;           // the same for a call that writes BAM records
    bool truth_variants = false;             // rsq_sim_truth_variants: truth alignments of a reference with variants, in reference coordinates (SamVarFormat, BamVarFormat)
    bool truth_alleles = false;              // rsq_sim_truth_alleles: the same truth alignments in allele coordinates (SamAlleleFormat, BamAlleleFormat); never beside truth_variants
    bool truth_md = false;                   // rsq_sim_truth_md: NM:i and MD:Z behind every mapped truth record's tags (rsq_md.h: the four formats as MdFormat)
    // rsq_sim_bam_sorted_*: a run of calls whose BAM records leave in coordinate order (rsq_bamsort.h)
    struct BamSorted {
        bool active = false;
        bool open = false;                   // between rsq_sim_bam_sorted_begin and the flush: rsq_sim_truth_md may not change
        uint64_t stream_at = 0;              // the uncompressed offset in the file of the next final record
        uint32_t next_block = 0;             // where the next call begins (0: the run's first call begins where it likes)
        uint64_t prev_cut = 0;               // the cut of the call before: no record of a later call lies below it
        BamSortPlan plan{};
        DevBuf stage[2], dir[2];             // staging bytes and directory, [held | the call's]; `cur` holds the held ones, the gather moves them to the other
        int cur = 0;
        uint64_t n_held = 0, held_bytes = 0;
        uint64_t call_pairs = 0;             // pairs of the running call's parts so far
        uint32_t call_parts = 1;             // its sub-ranges (option overlap): the staging buffer grows once, for all of them
        uint64_t call_records = 0, call_mapped = 0;      // sorted_finish: the final records of the call (or the flush), and those of them with a position
        DevBuf keys[2], idx[2], hist, hist_at, sizes, at, flags, run_of, runs, result, out_of_order, windows, window_first;
        BamIndexState index;
    } bam_sorted;
    uint64_t record_text_bytes = 480;        // the same for the seqToIllumina records' text (error_model_text)
    // rsq_sim_depth_*: a run that accumulates the truth depth of the pairs calls (rsq_depth.h)
    struct Depth {
        bool open = false, finished = false;      // between rsq_sim_depth_begin and rsq_sim_depth_end; rsq_sim_depth_finish has turned the differences into depths
        DevBuf diff, bad, tile_sums;              // the array (differences, then depths); elements that fell outside their sequence; the prefix sum's scratch
        uint64_t words = 0;                       // of the array: depth_words()
        // rsq_sim_depth_bedgraph: the sequence and the end of the piece before, and where the run that was open there began
        uint32_t bg_seq = 0xFFFFFFFFu, bg_carry = 0;
        uint64_t bg_next = 0;
        DevBuf flags, rank, ends, sizes, offsets;
    } depth;
    // rsq_sim_stats_*: a run that accumulates the simulation report of the pairs calls (rsq_stats.h)
    struct Stats {
        bool open = false;                        // between rsq_sim_stats_begin and rsq_sim_stats_end
        DevBuf counts;                            // the run's array of 64-bit counters
        StatsLayout lay{};
    } stats;
    // rsq_sim_pileup_*: a run that accumulates the truth pileup of the pairs calls (rsq_pileup.h)
    struct Pileup {
        bool open = false, finished = false;      // between rsq_sim_pileup_begin and rsq_sim_pileup_end; rsq_sim_pileup_finish has turned plane 0 into depths
        uint32_t sets = 1;                        // strand sets: 1, or 2 (RSQ_PILEUP_STRANDS: forward, reverse)
        DevBuf planes, bad, tile_sums;            // sets * kPileupPlanes planes of `words`; elements that fell outside their sequence; the prefix sum's scratch
        uint64_t words = 0;                       // of a plane: depth_words()
        DevBuf flags, sizes, rank, at_pos, line_pos, offsets;      // rsq_sim_pileup_text's piece
    } pileup;
    // The part of the running pairs call that the open runs (depth, stats, pileup) take once the call's return code is RSQ_OK: while one is open a call is one part
    // (pairs_parts), whose fragments and raw arrays still lie in the workspace when the call ends.
    struct KeptPart {
        bool have = false;
        const Fragment *frags = nullptr;
        const FragmentVar *fvars = nullptr;
        uint64_t n_pairs = 0;
        RawLayout raw{};
        const uint32_t *row_order = nullptr;
    } kept;
    bool keeps_part() const { return depth.open || stats.open || pileup.open; }
    // rsq_sim_alleles_fasta (rsq_alleles.h): the records of the alleles' FASTA text, made at the first call (n == 0: not yet; a reference taken in later starts over)
    struct AllelesText {
        DevBuf records;
        uint32_t n = 0;
        uint64_t bytes = 0;
    } alleles_text;
    int force_fill_mode = -1;      // RSQ_FILL_MODE=0: every draw in double precision from HBM (tests run both paths)
    // read kernels compiled for this simulator's profile (rsq_spec.h); `specialize`: option specialize when the simulator was created
    SpecKernels spec;
    std::string arch;              // hipDeviceProp_t::gcnArchName
    bool specialize = true;
    // the device's part of the chain run PrepassSim::pre.run (DevicePrepass): the chains, the chain of every chunk, per chunk the state it was entered with and its
    // outgoing states of two passes, the count and the list of the chunks that run again
    struct ChainBufs {
        DevBuf chains, chunk_chain, used, out[2], changed, list;
    } chain_bufs;
    // The surrounding-bias tracks of the pre-pass's share, kept for the sieve's candidate kernel (BiasTracks, rsq_sieve.h): they depend on the reference and the
    // profile's sur_bias alone, so they serve every call until the next pre-pass or reference.  [lo, hi) of the concatenated sequences; lo == hi: none kept.
    struct SieveTracks {
        DevBuf start_bias, end_bias;
        uint64_t lo = 0, hi = 0;
        void drop() {
            lo = hi = 0;
            start_bias.release();
            end_bias.release();
        }
    } sieve_tracks;
};

static bool fill_is_binned(const rsq_sim &s) { return effective_fill_mask(s.dev.lds.mask, s.force_fill_mode) != 0 && s.dev.lds.binned; }
// The read kernel compiled for this simulator's profile (rsq_spec.h), or nullptr: the library's own instantiation runs.  Compiles at the first request of a variant;
// what happened is kept for rsq_sim_specialize / rsq_last_warning.
static thread_local std::string g_spec_note;
static hipFunction_t spec_kernel(rsq_sim &s, SpecKind kind, uint32_t mask, bool var, bool binned) {
    if (!s.specialize || mask == 0) return nullptr;                    // mask 0: no image, no plan to compile in
    std::string note;
    hipFunction_t fn = s.spec.get(s.dev, SpecVariant{kind, mask, var, binned}, s.arch, note);
    if (s.opt.trace_plan && note != g_spec_note) fprintf(stderr, "[rsq] %s\n", note.c_str());
    g_spec_note = note;
    return fn;
}

namespace rsq {

// ------------------------------------------------------------------------------------------ pre-passes
// what the drivers of rsq_prepass.h run on the device, on stream `st`
constexpr uint64_t kBiasWindow = 512ull << 20;       // start positions per pass of the bias sums: 2 x 4 GB of tracks
struct DevicePrepass : PrepassBackend {
    rsq_sim &s;
    hipStream_t st;
    DevicePrepass(rsq_sim &sim, void *stream) : s(sim), st((hipStream_t)stream) {}

    // FragmentDistributionStats.cpp:3504-3582 CalculateBiasNormalization; the SumBias scans (Reference.cpp:622-659) run on
    // the GPU, one launch for all (sequence, sampled length) pairs; partial sums are combined in a fixed order.
    void bias_partials(const BiasPlan &plan, uint64_t g_lo, uint64_t g_hi, std::vector<double> &h_sum, std::vector<double> &h_max) override {
        const bool trace = s.opt.trace_prepare != 0;
        auto t0 = std::chrono::steady_clock::now();
        auto lap = [&](const char *what) {
            if (!trace) return;
            HIP_CHECK(hipStreamSynchronize(st));
            const auto t1 = std::chrono::steady_clock::now();
            fprintf(stderr, "prepare:   bias sums: %-18s %8.3f s\n", what, std::chrono::duration<double>(t1 - t0).count());
            t0 = t1;
        };
        const uint32_t n_chunks = bias_chunks(plan);
        if (!n_chunks) return;
        DevBuf d_params, d_chunk_param, d_chunk_ptr, d_sum, d_max, own_start_bias, own_end_bias;
        d_params.upload(plan.params);
        d_chunk_param.upload(plan.chunk_param);
        d_chunk_ptr.upload(plan.chunk_ptr);
        d_sum.reserve((size_t)n_chunks * 8);
        d_max.reserve((size_t)n_chunks * 8);
        HIP_CHECK(hipMemsetAsync(d_sum.as<double>(), 0, (size_t)n_chunks * 8, st));
        HIP_CHECK(hipMemsetAsync(d_max.as<double>(), 0, (size_t)n_chunks * 8, st));
        lap("chunk tables");
        // The share in windows of kBiasWindow positions: the tracks of one window (16 bytes per position; allocating them for a whole human-sized
        // reference takes a second) are computed, its chunks summed, the buffers used again.  A window's chunks read start positions up to a chunk
        // behind its end and end positions a fragment length further.
        const uint64_t lo = std::min<uint64_t>(g_lo, s.total_ref_size), hi = std::min<uint64_t>(g_hi, s.total_ref_size);
        uint64_t window = kBiasWindow;
        if (s.opt.bias_window > 0) window = (uint64_t)s.opt.bias_window;
        const uint64_t reach = (uint64_t)kBiasBlock * kBiasRun + s.dev.insert_to, track_len = std::min(hi - lo, window) + reach;
        // without variants, one window over the whole share and within option sieve_tracks_mb: the tracks stay for the sieve (rsq_sim::SieveTracks)
        s.sieve_tracks.drop();
        const bool keep = 0 == s.variants_mode && hi - lo <= window && s.opt.sieve_tracks_mb > 0 && track_len * 16 <= ((uint64_t)s.opt.sieve_tracks_mb << 20);
        DevBuf &d_start_bias = keep ? s.sieve_tracks.start_bias : own_start_bias, &d_end_bias = keep ? s.sieve_tracks.end_bias : own_end_bias;
        d_start_bias.reserve(track_len * 8 + 16);
        d_end_bias.reserve(track_len * 8 + 16);
        lap("track buffers");
        for (uint64_t a = lo; a < hi; a += window) {
            const uint64_t b = std::min(hi, a + window), w_hi = std::min<uint64_t>(s.total_ref_size, b + reach);
            hipLaunchKernelGGL(k_surrounding_bias_tracks, dim3((uint32_t)cdiv(w_hi - a, 256)), dim3(256), 0, st, s.dev, d_start_bias.as<double>(), d_end_bias.as<double>(), a, w_hi);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_sum_bias, dim3(n_chunks), dim3(kBiasBlock), 0, st, s.dev, d_params.as<BiasParam>(), d_chunk_param.as<uint32_t>(), d_chunk_ptr.as<uint32_t>(),
                               d_start_bias.as<double>(), d_end_bias.as<double>(), a, d_sum.as<double>(), d_max.as<double>(), a, b);
            HIP_CHECK(hipGetLastError());
        }
        if (keep) {
            s.sieve_tracks.lo = lo;
            s.sieve_tracks.hi = std::min<uint64_t>(s.total_ref_size, hi + reach);
        }
        lap("track and sum kernels");
        HIP_CHECK(hipMemcpyAsync(h_sum.data(), d_sum.as<double>(), h_sum.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h_max.data(), d_max.as<double>(), h_max.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        lap("download");
    }

    // ---- systematic errors (a13): k_sys_chain over the run's chunks
    void begin_run(const ChainRun &run, const std::vector<uint32_t> &chunk_chain) override {
        rsq_sim::ChainBufs &b = s.chain_bufs;
        publish_chains(run);
        b.chunk_chain.upload(chunk_chain);
        b.used.reserve(run.n_chunks * 4);
        b.out[0].reserve(run.n_chunks * 4);
        b.out[1].reserve(run.n_chunks * 4);
        b.changed.reserve(8);
        b.list.reserve((size_t)run.n_chunks * 4 + 16);
    }
    void publish_chains(const ChainRun &run) override { s.chain_bufs.chains.upload(run.chains); }
    uint32_t run_pass(const ChainRun &run, uint32_t pass, int prev, int cur) override {
        rsq_sim::ChainBufs &b = s.chain_bufs;
        uint32_t *out_prev = b.out[prev].as<uint32_t>(), *out_new = b.out[cur].as<uint32_t>();
        uint32_t n_run = run.n_chunks;
        const uint32_t *list = nullptr;
        if (pass > 0) {                                             // which chunks were entered with a state that has changed since
            HIP_CHECK(hipMemsetAsync(b.changed.as<uint32_t>(), 0, 4, st));
            hipLaunchKernelGGL(k_sys_chain_select, dim3(cdiv(run.n_chunks, 256)), dim3(256), 0, st, b.chains.as<Chain>(), b.chunk_chain.as<uint32_t>(), run.n_chunks,
                               b.used.as<uint32_t>(), out_prev, out_new, b.list.as<uint32_t>(), b.changed.as<uint32_t>(), (int)pass);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(&n_run, b.changed.as<uint32_t>(), 4, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            list = b.list.as<uint32_t>();
        }
        if (n_run) {
            hipLaunchKernelGGL(k_sys_chain, dim3(cdiv(n_run, 64)), dim3(64), 0, st, s.dev, b.chains.as<Chain>(), b.chunk_chain.as<uint32_t>(), list, n_run, s.chain_chunk,
                               chain_warmup_len(s.chain_chunk, s.opt), b.used.as<uint32_t>(), out_prev, out_new, (int)pass);
            HIP_CHECK(hipGetLastError());
        }
        return n_run;
    }
    uint32_t out_state(const ChainRun &, int cur, size_t chunk) override {
        uint32_t state = 0;
        HIP_CHECK(hipMemcpy(&state, s.chain_bufs.out[cur].as<uint32_t>() + chunk, 4, hipMemcpyDeviceToHost));
        return state;
    }
    // The chain state in front of every variant comes from the device (k_variant_chain_states: 8 bytes per variant come back instead of the tracks' 4 bytes per
    // reference position), the pass over the variants' bases runs on the host's threads.
    void variant_sys_errors(const ChainRun &run) override {
        const uint32_t n_variants = (uint32_t)s.variants.size();
        if (!s.has_variants || !n_variants) return;
        std::vector<ChainSpan> span((size_t)s.dev.n_seqs * 2, ChainSpan{-1, 0});
        for (size_t c = 0; c < run.chains.size(); ++c) {
            const Chain &ch = run.chains[c];
            if (ch.kind > 1u) continue;
            span[(size_t)ch.id * 2 + ch.kind] = ChainSpan{(int32_t)c, (c + 1 < run.chains.size() ? run.chains[c + 1].first_chunk : run.n_chunks) - ch.first_chunk};
        }
        DevBuf d_span, d_states;
        d_span.upload(span);
        d_states.reserve((size_t)n_variants * 8);
        hipLaunchKernelGGL(k_variant_chain_states, dim3(cdiv(n_variants, 256), 2), dim3(256), 0, st, s.dev, s.chain_bufs.chains.as<Chain>(), d_span.as<ChainSpan>(),
                           s.chain_bufs.used.as<uint32_t>(), s.chain_chunk, n_variants, d_states.as<uint32_t>());
        HIP_CHECK(hipGetLastError());
        std::vector<uint32_t> states((size_t)n_variants * 2);
        HIP_CHECK(hipMemcpyAsync(states.data(), d_states.as<uint32_t>(), states.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const std::vector<StrandTask> windows = strand_tasks(s.opt, run.chains, run.n_chunks, s.chain_chunk, [](uint32_t) { return 0u; });      // the windows' entering states are not needed
        build_variant_sys_errors(s, s.up, &windows, states.data(), states.data() + n_variants);
    }
    // the read kernel for this profile (rsq_spec.h), so that no compilation falls into the first rsq_sim_pairs
    void ready_to_simulate() override {
        if (s.has_ref) (void)spec_kernel(s, SpecKind::kReads, effective_fill_mask(s.dev.lds.mask, s.force_fill_mode), s.has_variants, fill_is_binned(s));
    }
};

// --------------------------------------------------------------------------------------------- hot path
// out[i] = *init + in[0] + ... + in[i-1] for i = 0 .. n (init nullptr: 0); the total also goes to *total_out if given
// `arrays` (1 or 2) of n elements each in one set of launches; longest (nullptr: not wanted) takes the largest element by atomicMax
// n >= 1 (scan_launch): every caller returns early, or leaves the stage out, for a call, a part or a block of text without items
static void exclusive_scans(rsq_sim &s, ScanArrays a, uint32_t arrays, uint64_t n, hipStream_t st, uint32_t *longest = nullptr) {
    const uint32_t tiles = cdiv(n, kScanTile);
    s.cur->tile_sums.reserve((size_t)arrays * (tiles + 1) * 8);
    s.cur->scan_total.reserve(16);
    for (uint32_t i = 0; i < arrays; ++i)
        if (!a.total[i]) a.total[i] = s.cur->scan_total.as<uint64_t>() + i;
    scan_launch(a, arrays, n, s.cur->tile_sums.as<uint64_t>(), st, longest);
    HIP_CHECK(hipGetLastError());
}
static void exclusive_scan(rsq_sim &s, const uint32_t *in, uint64_t n, uint64_t *out, hipStream_t st, const uint64_t *init = nullptr, uint64_t *total_out = nullptr, uint32_t *longest = nullptr) {
    exclusive_scans(s, ScanArrays{{in, nullptr}, {out, nullptr}, {init, nullptr}, {total_out, nullptr}}, 1, n, st, longest);
}

static RawLayout raw_layout(rsq_sim &s, uint64_t n_reads) {
    const uint64_t pitch = (n_reads + 63u) & ~(uint64_t)63u;            // word rows start on 256-byte boundaries
    s.cur->raw_seq.reserve((uint64_t)(s.read_stride / 4u) * pitch * 4 + 16);
    s.cur->raw_qual.reserve((uint64_t)(s.read_stride / 4u) * pitch * 4 + 16);
    s.cur->raw_ops.reserve((uint64_t)s.ops_stride * pitch * 4 + 16);
    s.cur->raw_meta.reserve(n_reads * sizeof(ReadMeta) + 16);
    // the read kernels' stores take 32-bit byte offsets while the longest of the arrays stays within 4 GB (WaveReadOut)
    if (pitch > 0xFFFFFFFFull) throw Error("more than 2^32 reads in one call: use smaller block ranges");      // the cursor's row and pitch are 32-bit (no device holds such arrays)
    const uint32_t wide = s.opt.wide_rows || read_out_is_wide(std::max<uint64_t>(s.read_stride / 4u, s.ops_stride), pitch) ? 1u : 0u;
    return RawLayout{s.cur->raw_seq.as<uint32_t>(), s.cur->raw_qual.as<uint32_t>(), s.cur->raw_ops.as<uint32_t>(), s.cur->raw_meta.as<ReadMeta>(), pitch, nullptr, 0, wide, nullptr};
}

// Reads binned by tile (the LDS plan holds one tile per image): keys, histogram, the bins' places and units, the scatter.  n_keys = n_tiles (pairs:
// both mates of a pair have the pair's tile) or 2 n_tiles (records); bins = (segment, tile).
template <class CountKernel>
static FillBins build_fill_bins(rsq_sim &s, uint64_t n_items, uint32_t n_keys, hipStream_t st, CountKernel &&count_keys, const Fragment *frags = nullptr,
                                const FragmentVar *fvars = nullptr) {
    if (n_items >= 0xFFFFFFFFull) throw Error("more than 2^32 reads in one call of a profile with tiles: use smaller block ranges");
    const uint32_t n_bins = 2 * s.dev.n_tiles;
    s.cur->bin_keys.reserve(n_items * 2 + 16);
    s.cur->bin_perm.reserve(n_items * 4 + 16);
    // [hist n_keys][cursor n_keys][bin_first n_bins][bin_count n_bins][next_chunk n_bins][workers n_bins][chunk_ptr n_bins + 1]
    const size_t words = 2 * (size_t)n_keys + 5 * (size_t)n_bins + 1;
    s.cur->bin_small.reserve(words * 4 + 16);
    uint32_t *hist = s.cur->bin_small.as<uint32_t>(), *cursor = hist + n_keys, *bin_first = cursor + n_keys, *bin_count = bin_first + n_bins, *next_chunk = bin_count + n_bins,
             *workers = next_chunk + n_bins, *chunk_ptr = workers + n_bins;
    HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)n_keys * 4, st));
    s.timers["bin_tiles"].start(st);
    count_keys(s.cur->bin_keys.as<uint16_t>(), hist);
    hipLaunchKernelGGL(k_bins_plan, dim3(1), dim3(1024), 0, st, hist, n_keys, n_bins, bin_first, bin_count, cursor, chunk_ptr, next_chunk, workers);
    if (frags) s.cur->bin_frags.reserve(n_items * sizeof(Fragment) + 16);
    if (fvars) s.cur->bin_fvars.reserve(n_items * sizeof(FragmentVar) + 16);
    hipLaunchKernelGGL(k_bin_scatter, dim3(cdiv(n_items, kBinBlock * kBinItemsPerThread)), dim3(kBinBlock), 0, st, s.cur->bin_keys.as<uint16_t>(), n_items, n_keys, cursor,
                       s.cur->bin_perm.as<uint32_t>(), frags, fvars, s.cur->bin_frags.as<Fragment>(), s.cur->bin_fvars.as<FragmentVar>());
    s.timers["bin_tiles"].stop(st);
    HIP_CHECK(hipGetLastError());
    return FillBins{s.cur->bin_perm.as<uint32_t>(), bin_first, bin_count, chunk_ptr, next_chunk, workers, n_bins, s.cur->bin_frags.as<Fragment>(), s.cur->bin_fvars.as<FragmentVar>()};
}
// the same opt-in for a kernel compiled for the profile (a module function).  The runtime of this image launches module functions with up to the device's 160 KB
// without it and knows the attribute for host-registered functions only, so an error here is not one of the launch -- the launch itself is checked.
static void spec_allow_lds(hipFunction_t fn, size_t lds_bytes) {
    if (lds_bytes > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) (void)hipGetLastError();
}
template <class Kernel>
static size_t fill_lds_bytes(const rsq_sim &s, bool screened, bool binned, Kernel kernel) {
    const size_t lds_bytes = (screened ? (size_t)s.dev.lds.total_words * 4u : 0) + (binned ? kSchedWords * 4u : 0);
    if (lds_bytes > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    return lds_bytes;
}
// Shape of a read kernel's launch: persistent workgroups, one (or two, when two images fit) per CU, not more than there are rounds of chunks -- and for a call
// that does not fill the device, FEWER WAVES PER WORKGROUP ON MORE CUs: a wave that has its SIMD to itself walks a chunk's 150 steps in 0.40 ms, four waves that
// start on one SIMD at the same instant take 1.0 ms for theirs (they run in phase: all in the Philox rounds, then all waiting for LDS; the waves of a long launch
// drift apart and fill each other's stalls -- DESIGN.md 4.5).  A seqToIllumina call on 107 000 records took 1.08 ms on 106 workgroups of 16 waves and takes half of
// that on 256 workgroups of 8 (tools/time_small_calls.py, profiles/r05_e_small_calls_*).  The kernels take any workgroup size up to their launch bound: the image
// is staged by blockDim.x threads, a wave's ring lies at its number in the workgroup.
struct FillShape {
    uint32_t blocks, threads;
};
static FillShape fill_shape(const rsq_sim &s, size_t lds_bytes, uint64_t n_items, uint32_t segments_per_item, uint32_t max_threads) {
    const uint32_t per_cu = lds_bytes * 2 <= kLdsBudgetBytes ? 2u : 1u;         // workgroups resident per CU (LDS image, 2048 threads)
    const uint64_t chunks = segments_per_item * ((n_items + 63) / 64), slots = (uint64_t)s.n_cu * per_cu;
    uint32_t waves = (uint32_t)std::min<uint64_t>(max_threads / 64u, std::max<uint64_t>(4u, cdiv(chunks, slots)));
    waves = std::min(max_threads / 64u, (waves + 3u) & ~3u);                 // whole waves per SIMD
    if (s.opt.fill_waves > 0) waves = (uint32_t)std::min<int64_t>(max_threads / 64u, s.opt.fill_waves);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(slots, std::max<uint64_t>(2, cdiv(chunks, waves)));
    return FillShape{(blocks + 1u) & ~1u, waves * 64u};                     // segments alternate over blockIdx.x
}

// The tail of both read kernels' launches: the chunk counters reserved and cleared (counter_bytes: 8, or the longer trace area of an RSQ_TRACE_FILL build), then,
// under the fill_reads timer, the kernel compiled for the profile (`spec` with `args`, its parameters in order) or, without one, the library's own instantiation
// (`launch_own`).  `counters`: the caller's variable that `args` and `launch_own` read, set here once the area is reserved.
template <class LaunchOwn>
static void launch_read_kernel(rsq_sim &s, hipStream_t st, const FillShape &shape, size_t lds_bytes, size_t counter_bytes, hipFunction_t spec, void **args, uint32_t *&counters,
                               LaunchOwn &&launch_own) {
    s.cur->fill_counters.reserve(counter_bytes);
    counters = s.cur->fill_counters.as<uint32_t>();
    HIP_CHECK(hipMemsetAsync(counters, 0, counter_bytes, st));
    s.timers["fill_reads"].start(st);
    if (spec) {
        spec_allow_lds(spec, lds_bytes);
        HIP_CHECK(hipModuleLaunchKernel(spec, shape.blocks, 1, 1, shape.threads, 1, 1, (unsigned)lds_bytes, st, args, nullptr));
    } else launch_own();
    s.timers["fill_reads"].stop(st);
    HIP_CHECK(hipGetLastError());
}
// k_fill_reads: persistent waves, one workgroup per CU slot; MASK = quads per quality row (screened draws on the LDS image planned by
// pack_tables) or 0 (double precision from HBM: the reference path the tests compare with)
// they return the order of the raw arrays' rows: nullptr = row i is item i, else row i is item perm[i] (binned by tile)
template <uint32_t MASK, bool VAR, bool BINNED>
static const uint32_t *launch_fill_kernel(rsq_sim &s, const Fragment *frags, uint64_t n_pairs, uint64_t adapter_first, const RawLayout &raw, hipStream_t st, const FragmentVar *fvars) {
    FillBins bins{};
    if (BINNED)
        bins = build_fill_bins(s, n_pairs, s.dev.n_tiles, st, [&](uint16_t *keys, uint32_t *hist) {
            hipLaunchKernelGGL(k_pair_tiles, dim3(cdiv(n_pairs, kBinBlock)), dim3(kBinBlock), 0, st, s.dev, frags, fvars, n_pairs, adapter_first, keys, hist);
        }, frags, fvars);
    const size_t lds_bytes = fill_lds_bytes(s, MASK != 0, BINNED, &k_fill_reads<MASK, VAR, BINNED>);
    const FillShape shape = fill_shape(s, lds_bytes, n_pairs, 2, fill_block(VAR));
    uint32_t *sizes = s.cur->sizes.as<uint32_t>(), *counters = nullptr;
    RawLayout raw_arg = raw;
    void *args[] = {&s.dev, &s.names, &frags, &n_pairs, &adapter_first, &raw_arg, &sizes, &counters, &fvars, &bins};
    launch_read_kernel(s, st, shape, lds_bytes, 8, spec_kernel(s, SpecKind::kReads, MASK, VAR, BINNED), args, counters, [&] {
        hipLaunchKernelGGL((k_fill_reads<MASK, VAR, BINNED>), dim3(shape.blocks), dim3(shape.threads), lds_bytes, st, s.dev, s.names, frags, n_pairs, adapter_first, raw, sizes, counters, fvars,
                           bins);
    });
    return bins.perm;
}
template <uint32_t MASK, bool VAR = false>
static const uint32_t *launch_fill_mask(rsq_sim &s, const Fragment *frags, uint64_t n_pairs, uint64_t adapter_first, const RawLayout &raw, hipStream_t st, const FragmentVar *fvars = nullptr) {
    if constexpr (MASK != 0)
        if (fill_is_binned(s)) return launch_fill_kernel<MASK, VAR, true>(s, frags, n_pairs, adapter_first, raw, st, fvars);
    return launch_fill_kernel<MASK, VAR, false>(s, frags, n_pairs, adapter_first, raw, st, fvars);
}
template <uint32_t MASK, bool BINNED, bool PACKED>
static const uint32_t *launch_records_kernel(rsq_sim &s, const RecordJob &job, const uint8_t *seg_dev, uint64_t n, const RawLayout &raw, hipStream_t st) {
    FillBins bins{};
    if (BINNED)
        bins = build_fill_bins(s, n, 2 * s.dev.n_tiles, st, [&](uint16_t *keys, uint32_t *hist) {
            hipLaunchKernelGGL(k_record_tiles, dim3(cdiv(n, kBinBlock)), dim3(kBinBlock), 0, st, s.dev, seg_dev, job.first_index, n, keys, hist);
        });
    const size_t lds_bytes = fill_lds_bytes(s, MASK != 0, BINNED, &k_fill_records<MASK, BINNED, PACKED>);
    const FillShape shape = fill_shape(s, lds_bytes, n, 1, kFillBlockWalk);
    const uint32_t blocks = shape.blocks;
#if defined(RSQ_TRACE_FILL)
    const size_t counter_bytes = 16 + 32 * (size_t)blocks;
#else
    const size_t counter_bytes = 8;
#endif
    uint32_t *counters = nullptr;
    RecordJob job_arg = job;
    RawLayout raw_arg = raw;
    void *args[] = {&s.dev, &job_arg, &raw_arg, &counters, &bins};
    // (the variant's `var` flag names the packed records here)
    launch_read_kernel(s, st, shape, lds_bytes, counter_bytes, spec_kernel(s, SpecKind::kRecords, MASK, PACKED, BINNED), args, counters, [&] {
        hipLaunchKernelGGL((k_fill_records<MASK, BINNED, PACKED>), dim3(blocks), dim3(shape.threads), lds_bytes, st, s.dev, job, raw, counters, bins);
    });
#if defined(RSQ_TRACE_FILL)
    {
        std::vector<uint64_t> t(2 + 4 * (size_t)blocks);
        HIP_CHECK(hipMemcpyAsync(t.data(), s.cur->fill_counters.as<uint64_t>(), t.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        uint64_t first = ~0ull, last_start = 0, last_end = 0, stage = 0, run = 0;
        for (uint32_t b = 0; b < blocks; ++b) {
            first = std::min(first, t[2 + 4 * b]);
            last_start = std::max(last_start, t[2 + 4 * b]);
            last_end = std::max(last_end, t[4 + 4 * b]);
            stage += t[3 + 4 * b] - t[2 + 4 * b];
            run += t[4 + 4 * b] - t[3 + 4 * b];
        }
        if (getenv("RSQ_TRACE_WORKGROUPS")) {                      // workgroup: start + duration until its last wave ended (us), chunks it ran
            std::string line;
            for (uint32_t b = 0; b < blocks; ++b) {
                line += " " + std::to_string(b) + ":" + std::to_string((t[2 + 4 * b] - first) / 100) + "+" + std::to_string((t[4 + 4 * b] - t[2 + 4 * b]) / 100) + "/" + std::to_string(t[5 + 4 * b]);
            }
            fprintf(stderr, "trace_fill workgroup:start+duration(us)/chunks:%s\n", line.c_str());
        }
        fprintf(stderr, "trace_fill: %u workgroups of %u threads, %llu items: last start %.1f us after the first, last end %.1f us; image staged in %.1f us, chunks %.1f us (means; 100 MHz clock)\n", blocks,
                shape.threads, (unsigned long long)n, (last_start - first) / 100.0, (last_end - first) / 100.0, stage / 100.0 / blocks, run / 100.0 / blocks);
    }
#endif
    return bins.perm;
}
template <uint32_t MASK>
static const uint32_t *launch_records_mask(rsq_sim &s, const RecordJob &job, const uint8_t *seg_dev, uint64_t n, const RawLayout &raw, hipStream_t st) {
    if constexpr (MASK != 0)
        if (fill_is_binned(s)) return job.codes ? launch_records_kernel<MASK, true, true>(s, job, seg_dev, n, raw, st) : launch_records_kernel<MASK, true, false>(s, job, seg_dev, n, raw, st);
    return job.codes ? launch_records_kernel<MASK, false, true>(s, job, seg_dev, n, raw, st) : launch_records_kernel<MASK, false, false>(s, job, seg_dev, n, raw, st);
}
// The read kernels are instantiated for 0 quads and for every entry of kQualityQuads: f(std::integral_constant<uint32_t, Q>) for the Q that equals `mask`
template <class F, size_t... I>
static const uint32_t *with_fill_mask(uint32_t mask, const char *kernel, F &&f, std::index_sequence<I...>) {
    const uint32_t *order = nullptr;
    auto tried = [&](auto q) { return mask == q() && (order = f(q), true); };
    if (!(tried(std::integral_constant<uint32_t, 0u>{}) || ... || tried(std::integral_constant<uint32_t, kQualityQuads[I]>{})))
        throw Error(std::string("no ") + kernel + " instantiation for " + std::to_string(mask) + " quads");
    return order;
}
template <class F>
static const uint32_t *with_fill_mask(rsq_sim &s, const char *kernel, F &&f) {
    return with_fill_mask(effective_fill_mask(s.dev.lds.mask, s.force_fill_mode), kernel, f, std::make_index_sequence<sizeof(kQualityQuads) / sizeof(kQualityQuads[0])>{});
}
static const uint32_t *launch_fill_reads(rsq_sim &s, const Fragment *frags, uint64_t n_pairs, uint64_t adapter_first, const RawLayout &raw, hipStream_t st,
                              const FragmentVar *fvars = nullptr) {
    const bool var = frags && s.has_variants;            // with variants the error walk is per lane state
    return with_fill_mask(s, "k_fill_reads", [&](auto q) {
        if (var) return launch_fill_mask<decltype(q)::value, true>(s, frags, n_pairs, adapter_first, raw, st, fvars);
        return launch_fill_mask<decltype(q)::value>(s, frags, n_pairs, adapter_first, raw, st);
    });
}
static const uint32_t *launch_fill_records(rsq_sim &s, const RecordJob &job, const uint8_t *seg_dev, uint64_t n, const RawLayout &raw, hipStream_t st) {
    return with_fill_mask(s, "k_fill_records", [&](auto q) { return launch_records_mask<decltype(q)::value>(s, job, seg_dev, n, raw, st); });
}

// a text writer (one wave of 64 lanes per workgroup, rsq_format.h WaveImage): K<true> when the raw rows have an order (binned by tile), else K<false>
template <class K, class... A>
static void launch_text_waves(K with_order, K in_order, const uint32_t *row_order, dim3 grid, uint32_t lds, hipStream_t st, A... args) {
    hipLaunchKernelGGL(row_order ? with_order : in_order, grid, dim3(64), lds, st, args...);
}

// ---- the stages of one (sub-)range; they work on the simulator's current workspace (s.cur)
// What a pairs call was given, built once by its C entry point: the two files' FASTQ buffers, the caller's stream, and where truth alignments and fragments go
struct PairsCall {
    struct Out {
        char *dst = nullptr;
        size_t cap = 0, *len = nullptr;
        uint64_t room() const { return dst ? cap : 0; }      // what a kernel may write: nothing without a buffer
        size_t bytes() const { return len ? *len : 0; }      // what the call came to (a sorted run's flush has no FASTQ outputs)
    };
    Out r1, r2;
    hipStream_t st = nullptr;
    Out truth;             // the caller's SAM or BAM buffer.  kNoTruth: the call launches no kernel of rsq_sam.h; else it launches the kernels of one format
    // kBam: BAM records (rsq_bam.h BamFormat) in place of SAM text (SamFormat).  kSortedBam: those of a sorted run (rsq_bamsort.h): the parts write to its staging buffer, sorted_finish to `truth`
    enum Truth { kNoTruth, kSam, kBam, kSortedBam } kind = kNoTruth;
    rsq_fragment *frags_out = nullptr;      // rsq_sim_pairs*: the fragments themselves
    size_t frags_cap = 0;
    bool has_truth() const { return kind != kNoTruth; }
    bool bam() const { return kind >= kBam; }
    bool sorted() const { return kind == kSortedBam; }
    std::string need() const { return "output buffers too small: need " + std::to_string(r1.bytes()) + " and " + std::to_string(r2.bytes()) + " bytes"; }
};
// What the stages of one part work on: its pairs (fragments on the device, or adapter-only pairs when frags == nullptr) and, once reads_stage has run, their reads
struct Part {
    const Fragment *frags;
    const FragmentVar *fvars;      // variants of any kind (variants_mode 2), else nullptr
    uint64_t n_pairs, adapter_first;
    uint32_t part;
    RawLayout raw;
    const uint32_t *row_order;
};
// reads of the part's pairs into the raw arrays and their record sizes
static void reads_stage(rsq_sim &s, Part &p, hipStream_t st) {
    p.raw = raw_layout(s, 2 * p.n_pairs);
    s.cur->sizes.reserve(2 * p.n_pairs * 4 + 16);
    if (p.frags && (p.fvars || s.dev.meth_ptr)) {                    // both mates' templates written out first
        s.cur->templates.reserve(2 * p.n_pairs * s.template_words * 8 + 16);
        p.raw.templates = s.cur->templates.as<uint64_t>();
        p.raw.template_words = s.template_words;
    }
    if (p.frags && s.dev.meth_ptr && !p.fvars) {                     // --methylation: CTConversion of both mates' templates
        hipLaunchKernelGGL(k_methylation_templates, dim3(cdiv(2 * p.n_pairs, 256)), dim3(256), 0, st, s.dev, p.frags, p.n_pairs, p.raw);
        HIP_CHECK(hipGetLastError());
    }
    if (p.frags && p.fvars) {                                        // variants of any kind: the templates with the allele's variants
        s.timers["variant_templates"].start(st);
        hipLaunchKernelGGL(k_variant_templates, dim3(cdiv(2 * p.n_pairs, 256)), dim3(256), 0, st, s.dev, p.frags, p.fvars, p.n_pairs, p.raw);
        s.timers["variant_templates"].stop(st);
        HIP_CHECK(hipGetLastError());
    }
    p.row_order = launch_fill_reads(s, p.frags, p.n_pairs, p.adapter_first, p.raw, st, p.fvars);
}
// FASTQ text of the pairs of reads_stage: their offsets continue at totals[2 * part] / [2 * part + 1] (bytes of text in front of this part, per
// file), where the part ends goes to totals[2 * (part + 1)] / [.. + 1].  The kernel refuses to write past the caller's capacity.
static void text_stage(rsq_sim &s, const PairsCall &call, const Part &p, hipStream_t st) {
    rsq_sim::Workspace &w = *s.cur;
    const uint64_t n_pairs = p.n_pairs;
    w.off_r1.reserve((n_pairs + 1) * 8);
    w.off_r2.reserve((n_pairs + 1) * 8);
    uint64_t *totals = s.totals.as<uint64_t>();
    s.timers["scan"].start(st);
    // both files' record sizes in one set of launches; the call's longest record (the next call's image size, below) comes out of the tile sums' pass
    exclusive_scans(s, ScanArrays{{w.sizes.as<uint32_t>(), w.sizes.as<uint32_t>() + n_pairs}, {w.off_r1.as<uint64_t>(), w.off_r2.as<uint64_t>()},
                                  {totals + 2 * p.part, totals + 2 * p.part + 1}, {totals + 2 * (p.part + 1), totals + 2 * (p.part + 1) + 1}},
                    2, n_pairs, st, s.longest_record.as<uint32_t>());
    s.timers["scan"].stop(st);
    // the wave's LDS image: sized by the longest record of the call before (the first call takes room for records of 480 bytes); binned rows have a slot per
    // record, each with its own alignment.  This call's longest record goes to totals' last word for the next one.
    const uint32_t lds = format_lds_bytes(s.format_record_bytes, p.row_order != nullptr);
    s.timers["format_write"].start(st);
    launch_text_waves(k_format_write<true>, k_format_write<false>, p.row_order, dim3(cdiv(n_pairs, kFormatRecords), 2), lds, st, s.dev, s.names, p.frags, n_pairs, p.adapter_first, p.raw,
                      w.off_r1.as<uint64_t>(), w.off_r2.as<uint64_t>(), call.r1.dst, call.r2.dst, call.r1.room(), call.r2.room(), p.fvars, p.row_order, lds);
    s.timers["format_write"].stop(st);
    HIP_CHECK(hipGetLastError());
}
// The truth records of the pairs of reads_stage in one format, behind their text_stage on the same stream (it reads the FASTQ offsets' totals: nothing is written
// unless all three outputs fit so far).  Offsets continue at sam_totals[part]; where the part ends goes to sam_totals[part + 1].  A format has its own side array,
// timer keys and image size; sizes, offsets and totals live in the same buffers (a call writes one kind).
// A sorted run's part (rsq_bamsort.h): its records go to the staging buffer behind the held ones and the parts in front.  The part's bytes are known on the
// device only and the writer must not run past the buffer, so the host reads them here (the stream is idle afterwards: one wait per part, on a path whose
// call ends with a wait anyway).  A buffer that has to grow grows with its contents kept, and at once to what the whole call will need if its other parts are
// like this one, so a call copies what it kept at most once; the next call of the run finds the room.
static char *sorted_stage_room(rsq_sim &s, uint64_t n_pairs, uint32_t part, hipStream_t st, uint64_t &cap) {
    rsq_sim::BamSorted &b = s.bam_sorted;
    uint64_t ends[2];                                                // the bytes of the call's records in front of this part, and with it
    HIP_CHECK(hipMemcpyAsync(ends, s.sam_totals.as<uint64_t>() + part, 16, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t bytes = b.held_bytes + ends[1] + 32u, entries = b.n_held + 2u * (b.call_pairs + n_pairs);
    const uint64_t left = b.call_parts > part + 1u ? b.call_parts - (part + 1u) : 0u;          // parts still to come
    if (bytes > b.stage[b.cur].bytes()) {
        const uint64_t whole = bytes + (ends[1] - ends[0]) * left;
        b.stage[b.cur].reserve_keeping(whole + whole / 8u, b.held_bytes + ends[0], st);
    }
    if (entries * sizeof(BamDirEntry) > b.dir[b.cur].bytes()) {
        const uint64_t whole = entries + 2u * n_pairs * left;
        b.dir[b.cur].reserve_keeping((whole + whole / 8u) * sizeof(BamDirEntry), (b.n_held + 2u * b.call_pairs) * sizeof(BamDirEntry), st);
    }
    cap = b.stage[b.cur].bytes() - 32u - b.held_bytes;
    return b.stage[b.cur].as<char>() + b.held_bytes;
}
// the directory entries of a sorted run's part, behind its records
template <class Pair>
static void sorted_directory(rsq_sim &s, const Part &p, hipStream_t st) {
    rsq_sim::BamSorted &b = s.bam_sorted;
    s.timers["bam_sort_keys"].start(st);
    hipLaunchKernelGGL(k_bam_sort_keys<Pair>, dim3(cdiv(p.n_pairs, 256)), dim3(256), 0, st, p.frags, p.n_pairs, p.row_order, s.cur->bam_side.as<Pair>(), s.cur->off_sam.as<uint64_t>(),
                       b.held_bytes, b.dir[b.cur].as<BamDirEntry>() + b.n_held + 2u * b.call_pairs, s.dev.n_seqs, b.prev_cut, b.plan.pos_bits, b.out_of_order.as<uint32_t>());
    s.timers["bam_sort_keys"].stop(st);
    HIP_CHECK(hipGetLastError());
    b.call_pairs += p.n_pairs;
}
template <class Format>
static void truth_stage(rsq_sim &s, const PairsCall &call, const Part &p, hipStream_t st) {
    using Pair = typename Format::Pair;
    constexpr bool bam = Format::kBam;
    const char *sizes_timer = bam ? "bam_sizes" : "sam_sizes", *write_timer = bam ? "bam_write" : "sam_write";
    rsq_sim::Workspace &w = *s.cur;
    DevBuf &side = bam ? w.bam_side : w.sam_side;
    const uint64_t n_pairs = p.n_pairs;
    w.sam_sizes.reserve(n_pairs * 4 + 16);
    w.off_sam.reserve((n_pairs + 1) * 8);
    side.reserve(n_pairs * sizeof(Pair) + 16);
    uint64_t *totals = s.sam_totals.as<uint64_t>();
    char *dst = call.truth.dst;
    uint64_t cap = call.truth.room();
    s.timers[sizes_timer].start(st);
    hipLaunchKernelGGL(k_truth_sizes<Format>, dim3(cdiv(n_pairs, 256)), dim3(256), 0, st, s.dev, s.names, p.frags, n_pairs, p.adapter_first, p.raw, p.row_order, side.as<Pair>(),
                       w.sam_sizes.as<uint32_t>(), p.fvars);
    s.timers[sizes_timer].stop(st);
    exclusive_scan(s, w.sam_sizes.as<uint32_t>(), n_pairs, w.off_sam.as<uint64_t>(), st, totals + p.part, totals + p.part + 1, s.sam_longest.as<uint32_t>());
    const uint32_t lds = sam_lds_bytes(bam ? s.bam_pair_bytes : s.sam_pair_bytes, p.row_order != nullptr);
    if (call.sorted()) dst = sorted_stage_room(s, n_pairs, p.part, st, cap);      // (the caller's buffer takes the sorted records: sorted_finish)
    s.timers[write_timer].start(st);
    launch_text_waves(k_truth_write<Format, true>, k_truth_write<Format, false>, p.row_order, dim3(cdiv(n_pairs, kSamPairs)), lds, st, s.dev, s.names, p.frags, n_pairs, p.adapter_first, p.raw,
                      side.as<Pair>(), w.off_sam.as<uint64_t>(), dst, cap, w.off_r1.as<uint64_t>() + n_pairs, w.off_r2.as<uint64_t>() + n_pairs, call.r1.room(), call.r2.room(), p.row_order,
                      lds, p.fvars);
    s.timers[write_timer].stop(st);
    HIP_CHECK(hipGetLastError());
    if constexpr (bam)
        if (call.sorted()) sorted_directory<Pair>(s, p, st);
}
// The part's truth records in the call's format.  A reference with variants (accepted only with rsq_sim_truth_variants): the formats in reference coordinates.
// rsq_sim_truth_md (mapped pairs only: an adapter-only call's records carry no such tags): the same four with the tags.  The formats without variants never see a
// FragmentVar: a part has them only with variants_mode 2, which rsq_pack.h sets only with variants (its loader of a packed reference trusts the file for that).
static void sam_stage(rsq_sim &s, const PairsCall &call, const Part &p, hipStream_t st) {
    using Stage = void (*)(rsq_sim &, const PairsCall &, const Part &, hipStream_t);
    static const Stage stage[2][2][2] = {{{truth_stage<SamFormat>, truth_stage<BamFormat>}, {truth_stage<SamVarFormat>, truth_stage<BamVarFormat>}},
                                         {{truth_stage<SamMdFormat>, truth_stage<BamMdFormat>}, {truth_stage<SamVarMdFormat>, truth_stage<BamVarMdFormat>}}};
    if (s.truth_alleles) return (call.bam() ? truth_stage<BamAlleleFormat> : truth_stage<SamAlleleFormat>)(s, call, p, st);      // (never with truth_md: truth_refusal)
    stage[s.truth_md && p.frags][s.has_variants][call.bam()](s, call, p, st);
}
static void reset_call_timers(rsq_sim &s) {
    for (auto &t : s.timers) t.second.reset();
}
// The frame of a pairs call, around its `parts` parts.  begin_call: the totals the parts' offsets continue from.  finish_call: the bytes of text and of truth
// records, the variant walk's error flag, the image sizes of the next call; the call's streams are idle afterwards.  `mapped`: pairs from the reference, whose
// walk can fail and whose longest record sizes the next FASTQ image.  An adapter-only call never updated format_record_bytes and must not begin to.
static void begin_call(rsq_sim &s, const PairsCall &call, uint32_t parts, hipStream_t text_stream) {
    s.totals.reserve((size_t)(parts + 1) * 16 + 16);
    s.longest_record.reserve(8);
    HIP_CHECK(hipMemsetAsync(s.totals.as<uint64_t>(), 0, 16, text_stream));
    HIP_CHECK(hipMemsetAsync(s.longest_record.as<uint32_t>(), 0, 4, text_stream));
    if (!call.has_truth()) return;
    s.sam_totals.reserve((size_t)(parts + 1) * 8 + 16);
    s.sam_longest.reserve(8);
    HIP_CHECK(hipMemsetAsync(s.sam_totals.as<uint64_t>(), 0, 8, text_stream));
    HIP_CHECK(hipMemsetAsync(s.sam_longest.as<uint32_t>(), 0, 4, text_stream));
}
static int finish_call(rsq_sim &s, const PairsCall &call, uint32_t parts, bool mapped, hipStream_t text_stream) {
    rsq_sim::Mailbox &m = *s.mailbox;
    if (call.has_truth()) {
        HIP_CHECK(hipMemcpyAsync(&m.truth_bytes, s.sam_totals.as<uint64_t>() + parts, 8, hipMemcpyDeviceToHost, text_stream));
        HIP_CHECK(hipMemcpyAsync(&m.truth_longest, s.sam_longest.as<uint32_t>(), 4, hipMemcpyDeviceToHost, text_stream));
    }
    m.walk_error = 0;
    if (mapped && s.has_variants) HIP_CHECK(hipMemcpyAsync(&m.walk_error, s.dev.walk_error, 4, hipMemcpyDeviceToHost, text_stream));
    static_assert(offsetof(rsq_sim::Mailbox, r2_bytes) == offsetof(rsq_sim::Mailbox, r1_bytes) + 8, "one copy fills both");
    HIP_CHECK(hipMemcpyAsync(&m.r1_bytes, s.totals.as<uint64_t>() + 2 * parts, 16, hipMemcpyDeviceToHost, text_stream));
    HIP_CHECK(hipMemcpyAsync(&m.longest_record, s.longest_record.as<uint32_t>(), 4, hipMemcpyDeviceToHost, text_stream));
    HIP_CHECK(hipStreamSynchronize(text_stream));
    *call.r1.len = m.r1_bytes;
    *call.r2.len = m.r2_bytes;
    int rc = RSQ_OK;
    if (m.walk_error) {
        HIP_CHECK(hipMemsetAsync(s.dev.walk_error, 0, 4, text_stream));
        HIP_CHECK(hipStreamSynchronize(text_stream));
        g_last_error = kWalkErrorMessage;
        rc = RSQ_EINVAL;
    } else if (*call.r1.len > call.r1.cap || *call.r2.len > call.r2.cap || !call.r1.dst || !call.r2.dst) {
        g_last_error = call.need();
        rc = RSQ_ENOSPC;
    }
    if (call.has_truth() && m.truth_longest) (call.bam() ? s.bam_pair_bytes : s.sam_pair_bytes) = m.truth_longest + 16u;
    if (call.has_truth() && !call.sorted()) {                        // (a sorted run's staging buffer always fits; what the caller's must hold is known after the sort: sorted_finish)
        const uint64_t bytes = *call.truth.len = m.truth_bytes;
        if (rc == RSQ_ENOSPC || (rc == RSQ_OK && (bytes > call.truth.cap || !call.truth.dst))) {
            g_last_error = call.need() + " of FASTQ text and " + std::to_string(bytes) + (call.bam() ? " of BAM records" : " of SAM text");
            rc = RSQ_ENOSPC;
        }
    }
    if (mapped && (rc == RSQ_OK || rc == RSQ_ENOSPC) && m.longest_record) s.format_record_bytes = m.longest_record + 8u;      // for the next call's text stage
    return rc;
}

// reads + FASTQ text of adapter-only pairs (Simulator::SimulateAdapterOnlyPairs, Simulator.cpp:2359-2382): one part on the caller's stream
static int adapter_only_pairs(rsq_sim &s, const PairsCall &call, uint64_t n_pairs, uint64_t adapter_first) {
    HIP_CHECK(hipSetDevice(s.device));
    *call.r1.len = *call.r2.len = 0;
    if (call.has_truth()) *call.truth.len = 0;
    if (!n_pairs) return RSQ_OK;
    reset_call_timers(s);
    s.cur = &s.ws[0];
    begin_call(s, call, 1, call.st);
    Part p{nullptr, nullptr, n_pairs, adapter_first, 0};
    reads_stage(s, p, call.st);
    text_stage(s, call, p, call.st);
    if (call.has_truth()) sam_stage(s, call, p, call.st);
    return finish_call(s, call, 1, false, call.st);
}

// The sieve of one block range on the current workspace: attempt 0 is launched without waiting; collect() waits for it, and if a list overflowed
// repeats the pass with the exact sizes (capacities come from the expected number of passing cells + 6 sigma, so that is rare).
struct SieveRun {
    uint32_t block_lo = 0, block_hi = 0;
    uint64_t n_slots = 0, cand_cap = 0, hit_cap = 0, total = 0, n_cands = 0;
    uint32_t n_hits = 0;
    const SlotInfo *slot_table = nullptr;
};
static void sieve_attempt(rsq_sim &s, SieveRun &r, int attempt, rsq_sim::Mailbox::Sieve &mail, hipStream_t st) {
    rsq_sim::Workspace &w = *s.cur;
    const int vm = s.variants_mode;
    if (r.cand_cap >= (1ull << 32)) throw Error("more than 2^32 sieve candidates in one call: use smaller block ranges");
    w.cands.reserve(r.cand_cap * sizeof(SieveCand));
    w.pairs_of.reserve(r.cand_cap * 4 + 16);
    w.pair_off.reserve((r.cand_cap + 1) * 8);
    if (vm) w.hits.reserve(r.hit_cap * sizeof(SieveHit));
    else w.cell_info.reserve(r.cand_cap * 4 + 16);
    HIP_CHECK(hipMemsetAsync(w.hit_count.as<uint32_t>(), 0, 4, st));
    s.timers["sieve"].start(st);
    const uint32_t block_lo = r.block_lo, block_hi = r.block_hi;
    const uint64_t n_slots = r.n_slots, cand_cap = r.cand_cap;
    const dim3 ggrid(cdiv(n_slots, kSieveBlock)), gblock(kSieveBlock);
    // the gap walk on LDS copies of the group's tables where they fit (k_sieve_gaps_lds), else on the tables in memory
    const size_t lds_bytes = (size_t)(s.dev.insert_to - s.dev.insert_from) * kSieveLdsPerLength;
    const bool in_lds = s.opt.sieve_lds != 0 && lds_bytes <= (s.opt.sieve_lds_bytes > 0 ? (size_t)s.opt.sieve_lds_bytes : kSieveLdsLimit);
    const dim3 lgrid(cdiv(ggrid.x, kSieveTilesPerGroup));
    const SlotInfo *slot_table = r.slot_table;
    auto gaps = [&](auto vm_tag, auto fill_tag, uint32_t *counts, const uint64_t *cand_off, SieveCand *cands) {
        constexpr int kVm = decltype(vm_tag)::value;
        constexpr bool kFill = decltype(fill_tag)::value;
        if (in_lds)
            hipLaunchKernelGGL((k_sieve_gaps_lds<kVm, kFill>), lgrid, gblock, lds_bytes, st, s.dev, block_lo, block_hi, (uint32_t)n_slots, counts, cand_off, cands, cand_cap, slot_table);
        else
            hipLaunchKernelGGL((k_sieve_gaps<kVm, kFill>), ggrid, gblock, 0, st, s.dev, block_lo, block_hi, (uint32_t)n_slots, counts, cand_off, cands, cand_cap, slot_table);
    };
    using Vm0 = std::integral_constant<int, 0>;
    using Vm2 = std::integral_constant<int, 2>;
    if (!attempt) {
        if (2 == vm) {
            w.slot_table.reserve(n_slots * sizeof(SlotInfo) + 16);
            s.timers["slot_table"].start(st);
            hipLaunchKernelGGL(k_slot_table, dim3(block_hi - block_lo), dim3(256), 0, st, s.dev, block_lo, w.slot_table.as<SlotInfo>());
            s.timers["slot_table"].stop(st);
            slot_table = r.slot_table = w.slot_table.as<SlotInfo>();
        }
        s.timers["sieve_screen"].start(st);
        if (2 == vm) gaps(Vm2{}, std::false_type{}, w.counts.as<uint32_t>(), nullptr, nullptr);
        else gaps(Vm0{}, std::false_type{}, w.counts.as<uint32_t>(), nullptr, nullptr);
        s.timers["sieve_screen"].stop(st);
        exclusive_scan(s, w.counts.as<uint32_t>(), n_slots, w.offsets.as<uint64_t>(), st);
    }
    s.timers[in_lds ? "sieve_gaps_lds" : "sieve_gaps_mem"].mark();                    // which walk the call took (rsq_sim_last_kernel_launches)
    if (2 == vm) gaps(Vm2{}, std::true_type{}, nullptr, w.offsets.as<uint64_t>(), w.cands.as<SieveCand>());
    else gaps(Vm0{}, std::true_type{}, nullptr, w.offsets.as<uint64_t>(), w.cands.as<SieveCand>());
    const dim3 fgrid(cdiv(cand_cap, kSieveBlock)), fblock(kSieveBlock);
    // the kept surrounding-bias tracks where they cover every start and end of the call's blocks; else the candidate kernel computes the factors as before
    BiasTracks tracks{nullptr, nullptr, 0, 0};
    if (0 == vm && s.sieve_tracks.hi > s.sieve_tracks.lo) {
        auto global_of_block = [&](uint32_t b) { return s.seq_base_off[s.block_seq[b]] + (uint64_t)(b - s.first_block[s.block_seq[b]]) * kBlockSize; };
        const uint64_t first = global_of_block(block_lo), last = std::min<uint64_t>(s.total_ref_size, global_of_block(block_hi - 1u) + kBlockSize + s.dev.insert_to);
        if (first >= s.sieve_tracks.lo && last <= s.sieve_tracks.hi)
            tracks = BiasTracks{s.sieve_tracks.start_bias.as<double>(), s.sieve_tracks.end_bias.as<double>(), s.sieve_tracks.lo, s.sieve_tracks.hi};
    }
    if (0 == vm) s.timers[tracks.hi > tracks.lo ? "sieve_tracks" : "sieve_tracks_off"].mark();      // which of the two the call took (rsq_sim_last_kernel_launches)
#define RSQ_FINISH(VM, CAP)                                                                                                                                   \
    hipLaunchKernelGGL((k_sieve_finish<VM, CAP>), fgrid, fblock, 0, st, s.dev, block_lo, block_hi, (uint32_t)n_slots, w.offsets.as<uint64_t>(), w.cands.as<SieveCand>(),  \
                       cand_cap, w.pairs_of.as<uint32_t>(), w.hits.as<SieveHit>(), (uint32_t)std::min<uint64_t>(r.hit_cap, 0xFFFFFFFFull), w.hit_count.as<uint32_t>(), slot_table, \
                       w.cell_info.as<uint32_t>(), tracks)
    if (2 == vm && s.num_alleles <= 8) RSQ_FINISH(2, 8);        // few alleles: the cell's (allele, strand) slots stay in registers
    else if (2 == vm) RSQ_FINISH(2, kMaxDevAlleles);
    else if (1 == vm) RSQ_FINISH(1, 8);                         // allele copies exist for at most eight alleles
    else RSQ_FINISH(0, 1);
#undef RSQ_FINISH
    s.timers["sieve"].stop(st);
    HIP_CHECK(hipGetLastError());
    exclusive_scan(s, w.pairs_of.as<uint32_t>(), cand_cap, w.pair_off.as<uint64_t>(), st);
    HIP_CHECK(hipMemcpyAsync(&mail.total, w.pair_off.as<uint64_t>() + cand_cap, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&mail.n_hits, w.hit_count.as<uint32_t>(), 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&mail.n_cands, w.offsets.as<uint64_t>() + n_slots, 8, hipMemcpyDeviceToHost, st));
}
// (a range without start position slots launches nothing: r.n_slots and r.total stay 0)
static void sieve_launch(rsq_sim &s, SieveRun &r, uint32_t block_lo, uint32_t block_hi, rsq_sim::Mailbox::Sieve &mail, hipStream_t st) {
    rsq_sim::Workspace &w = *s.cur;
    const int vm = s.variants_mode;
    r = SieveRun{};
    r.block_lo = block_lo;
    r.block_hi = block_hi;
    r.n_slots = (uint64_t)(block_hi - block_lo) * kBlockSize;
    if (2 == vm && block_hi > block_lo) {                            // plus the starts inside inserted bases of these blocks
        uint32_t ptr[2];
        HIP_CHECK(hipMemcpy(&ptr[0], s.dev.block_extra_ptr + block_lo, 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&ptr[1], s.dev.block_extra_ptr + block_hi, 4, hipMemcpyDeviceToHost));
        r.n_slots += ptr[1] - ptr[0];
    }
    if (!r.n_slots) return;
    if (r.n_slots >= (1ull << 32) - kSieveBlock)                     // slot indices are 32 bits wide inside one call
        throw Error("block range too large for one call: at most " + std::to_string(((1ull << 32) - kSieveBlock) / kBlockSize - 1) + " blocks");
    w.counts.reserve(r.n_slots * 4 + 16);
    w.offsets.reserve((r.n_slots + 1) * 8);
    w.hit_count.reserve(8);
    // capacity of the candidate list: the cells expected to pass the zero threshold plus six standard deviations; of the hit list:
    // cells with fragments <= candidates (with variants a cell has one record per two chosen (allele, strand) slots)
    const double expected_cands = s.expected_passing * (double)r.n_slots;
    r.cand_cap = std::max<uint64_t>(w.cands.bytes() / sizeof(SieveCand), (uint64_t)(expected_cands + 6.0 * sqrt(expected_cands + 1.0)) + 65536);
    r.hit_cap = std::max<uint64_t>(w.hits.bytes() / sizeof(SieveHit), 0 == vm ? r.cand_cap : r.cand_cap + r.cand_cap / 4);
    sieve_attempt(s, r, 0, mail, st);
}
static void sieve_collect(rsq_sim &s, SieveRun &r, rsq_sim::Mailbox::Sieve &mail, hipStream_t st) {
    for (int attempt = 0;; ++attempt) {
        HIP_CHECK(hipStreamSynchronize(st));
        r.total = mail.total;
        r.n_hits = mail.n_hits;
        r.n_cands = mail.n_cands;
        if (r.n_cands <= r.cand_cap && r.n_hits <= r.hit_cap) return;
        if (attempt >= 2) throw Error("sieve lists overflowed three times");
        // the candidate count is exact; the hit count is exact once the candidates fit, before that it is scaled up with them
        const double grow = r.n_cands > r.cand_cap ? (double)r.n_cands / (double)r.cand_cap : 1.0;
        if (r.n_hits > r.hit_cap || grow > 1.0) r.hit_cap = std::max<uint64_t>(r.hit_cap, (uint64_t)((double)r.n_hits * grow * 1.25) + 65536);
        r.cand_cap = std::max(r.cand_cap, r.n_cands + 65536);
        sieve_attempt(s, r, attempt + 1, mail, st);
    }
}
static void sieve_emit(rsq_sim &s, const SieveRun &r, hipStream_t st) {
    rsq_sim::Workspace &w = *s.cur;
    w.frags.reserve(r.total * sizeof(Fragment) + 16);
    s.timers["sieve_emit"].start(st);
    if (2 == s.variants_mode) {
        w.fvars.reserve(r.total * sizeof(FragmentVar) + 16);
        hipLaunchKernelGGL(k_sieve_emit<2>, dim3(cdiv(r.n_hits, 256)), dim3(256), 0, st, s.dev, r.block_lo, r.block_hi, w.hits.as<SieveHit>(), r.n_hits, w.offsets.as<uint64_t>(),
                           w.pair_off.as<uint64_t>(), w.frags.as<Fragment>(), w.fvars.as<FragmentVar>(), w.slot_table.as<SlotInfo>());
    } else if (1 == s.variants_mode)                                // allele copies: the hit list (a cell may have several records), slots as without variants
        hipLaunchKernelGGL(k_sieve_emit<1>, dim3(cdiv(r.n_hits, 256)), dim3(256), 0, st, s.dev, r.block_lo, r.block_hi, w.hits.as<SieveHit>(), r.n_hits, w.offsets.as<uint64_t>(),
                           w.pair_off.as<uint64_t>(), w.frags.as<Fragment>(), (FragmentVar *)nullptr, (const SlotInfo *)nullptr);
    else
        hipLaunchKernelGGL(k_sieve_emit<0>, dim3(cdiv(r.n_cands, 256)), dim3(256), 0, st, s.dev, r.block_lo, r.block_hi, (const SieveHit *)nullptr, (uint32_t)r.n_cands,
                           w.offsets.as<uint64_t>(), w.pair_off.as<uint64_t>(), w.frags.as<Fragment>(), (FragmentVar *)nullptr, (const SlotInfo *)nullptr, w.cands.as<SieveCand>(),
                           w.pairs_of.as<uint32_t>(), w.cell_info.as<uint32_t>());
    s.timers["sieve_emit"].stop(st);
    HIP_CHECK(hipGetLastError());
}

// SimulateFromGivenBlock + CreateReads + Output for the blocks [block_lo, block_hi) (Simulator.cpp:2249-2357, 634-721, 215-230).  Blocks are independent
// (:2384-2401), so a range can be cut into `parts` sub-ranges that move through three stages -- sieve, reads, FASTQ text -- on three streams: the read
// kernel owns every CU while it runs (160 KB of LDS, all vector registers), so nothing overlaps IT; the sieve of part k + 1 and the text of part k run side
// by side behind it.  That does not pay (pairs_parts), so a call is one part unless option overlap asks for more; what stays is the stage structure.
//   reads(k) waits for: fragments of part k (sieve stream), the text of part k - 2 (same workspace);
//   sieve(k + 1) waits for: reads(k) launched and done (else it would only take CUs from it), the text of part k - 1 (same workspace);
//   text(k) waits for reads(k).
// The host meets the sieve once per part (list sizes decide the next launches), everything else is ordered by events.
static uint32_t pairs_parts(const rsq_sim &s, uint32_t n_blocks) {
    // Measured (bench workload, 10 M pairs): 1 part 81.6 ms per step, 2 parts 83.0, 4 parts 84.3, 8 parts 87.7 -- the sieve's candidate kernel and the
    // formatter both live on the memory system (gathers in the 24 MB surrounding table; 15 GB of raw arrays and text), so side by side each takes nearly as long
    // as the two in a row, and every part adds a read-kernel tail.  One part unless asked (option overlap = n, tests).
    const int64_t opt = s.opt.overlap;
    if (s.keeps_part()) return 1u;                                   // an open run (depth, stats) takes the call's part once its return code is known (runs_take): the part's arrays must still be there
    return opt > 0 ? (uint32_t)std::min<int64_t>(opt, std::max<uint32_t>(n_blocks, 1u)) : 1u;
}
// what rsq_sim_pairs and rsq_sim_job_generate ask of a block range before anything is sized from it
static int check_block_range(const rsq_sim &s, uint32_t block_lo, uint32_t block_hi) {
    if (!s.prepared || !s.has_ref) {
        g_last_error = "rsq_sim_prepare with a reference must run before rsq_sim_pairs";
        return RSQ_ESTATE;
    }
    if (block_lo < 1 || block_hi > s.total_blocks + 1 || block_lo > block_hi) {
        g_last_error = "block range outside [1, total_blocks]";
        return RSQ_EINVAL;
    }
    if (block_lo < block_hi && (block_lo < s.prepared_lo || block_hi > s.prepared_hi)) {       // a sharded pre-pass finished the tracks of the rank's own blocks only
        g_last_error = "blocks [" + std::to_string(block_lo) + ", " + std::to_string(block_hi) + ") lie outside the range the sharded pre-pass prepared on this simulator, [" +
                       std::to_string(s.prepared_lo) + ", " + std::to_string(s.prepared_hi) + ")";
        return RSQ_ESTATE;
    }
    return RSQ_OK;
}
static int sim_pairs(rsq_sim &s, const PairsCall &call, uint32_t block_lo, uint32_t block_hi, uint64_t *n_pairs) {
    if (const int rc = check_block_range(s, block_lo, block_hi)) return rc;
    HIP_CHECK(hipSetDevice(s.device));
    *n_pairs = 0;
    *call.r1.len = *call.r2.len = 0;
    if (call.has_truth()) *call.truth.len = 0;
    s.kept.have = false;
    if (block_lo == block_hi) return RSQ_OK;
    reset_call_timers(s);
    const uint32_t parts = pairs_parts(s, block_hi - block_lo);
    // one part: everything on the caller's stream; more: the reads stay there, sieve and text get their own
    const hipStream_t st = call.st, s_reads = st, s_sieve = parts > 1 ? s.side[0] : st, s_text = parts > 1 ? s.side[1] : st;
    if (parts > 1) {                                                 // the side streams begin where the caller's stream is
        HIP_CHECK(hipEventRecord(s.ev_call, st));
        HIP_CHECK(hipStreamWaitEvent(s_sieve, s.ev_call, 0));
        HIP_CHECK(hipStreamWaitEvent(s_text, s.ev_call, 0));
    }
    begin_call(s, call, parts, s_text);
    struct Abort {                                                   // an error in the middle: nothing of the call may still run when it returns
        bool armed = true;
        ~Abort() {
            if (armed) (void)hipDeviceSynchronize();
        }
    } abort_guard;
    auto part_range = [&](uint32_t k) {
        const uint64_t n = block_hi - block_lo;
        return std::pair<uint32_t, uint32_t>(block_lo + (uint32_t)(n * k / parts), block_lo + (uint32_t)(n * (k + 1) / parts));
    };
    SieveRun run[2];
    s.cur = &s.ws[0];
    sieve_launch(s, run[0], part_range(0).first, part_range(0).second, s.mailbox->sieve[0], s_sieve);
    uint64_t total_pairs = 0;
    static_assert(sizeof(rsq_fragment) == sizeof(Fragment), "ABI fragment layout");
    for (uint32_t k = 0; k < parts; ++k) {
        const uint32_t p = k & 1u;
        s.cur = &s.ws[p];
        SieveRun &r = run[p];
        if (r.n_slots) sieve_collect(s, r, s.mailbox->sieve[p], s_sieve);
        const uint64_t n = r.total;
        Part part{nullptr, nullptr, n, 0, k};
        if (n) {
            sieve_emit(s, r, s_sieve);
            part.frags = s.cur->frags.as<Fragment>();
            part.fvars = 2 == s.variants_mode ? s.cur->fvars.as<FragmentVar>() : nullptr;
            if (call.frags_out) {
                if (call.frags_cap < total_pairs + n) {
                    g_last_error = "fragment buffer too small: need at least " + std::to_string(total_pairs + n) + " records";
                    return RSQ_ENOSPC;
                }
                HIP_CHECK(hipMemcpyAsync(call.frags_out + total_pairs, part.frags, n * sizeof(Fragment), hipMemcpyDeviceToDevice, s_sieve));
            }
            if (parts > 1) {
                HIP_CHECK(hipEventRecord(s.ev_emit, s_sieve));
                HIP_CHECK(hipStreamWaitEvent(s_reads, s.ev_emit, 0));
                if (k >= 2) HIP_CHECK(hipStreamWaitEvent(s_reads, s.cur->text_done, 0));       // the raw arrays of this workspace were last read by text(k - 2)
            }
            reads_stage(s, part, s_reads);
            if (parts > 1) {
                HIP_CHECK(hipEventRecord(s.ev_fill, s_reads));
                HIP_CHECK(hipStreamWaitEvent(s_text, s.ev_fill, 0));
            }
            text_stage(s, call, part, s_text);
            if (call.has_truth()) sam_stage(s, call, part, s_text);
            if (s.keeps_part()) s.kept = rsq_sim::KeptPart{true, part.frags, part.fvars, part.n_pairs, part.raw, part.row_order};      // (one part: pairs_parts)
        } else {                                                     // no pairs in this part: its text ends where it begins
            HIP_CHECK(hipMemcpyAsync(s.totals.as<uint64_t>() + 2 * (k + 1), s.totals.as<uint64_t>() + 2 * k, 16, hipMemcpyDeviceToDevice, s_text));
            if (call.has_truth()) HIP_CHECK(hipMemcpyAsync(s.sam_totals.as<uint64_t>() + k + 1, s.sam_totals.as<uint64_t>() + k, 8, hipMemcpyDeviceToDevice, s_text));
        }
        if (parts > 1) HIP_CHECK(hipEventRecord(s.cur->text_done, s_text));
        total_pairs += n;
        if (k + 1 < parts) {                                         // the next part's sieve, on the other workspace
            s.cur = &s.ws[p ^ 1u];
            if (n) HIP_CHECK(hipStreamWaitEvent(s_sieve, s.ev_fill, 0));
            if (k >= 1) HIP_CHECK(hipStreamWaitEvent(s_sieve, s.cur->text_done, 0));
            sieve_launch(s, run[p ^ 1u], part_range(k + 1).first, part_range(k + 1).second, s.mailbox->sieve[p ^ 1u], s_sieve);
        }
    }
    *n_pairs = total_pairs;
    const int rc = total_pairs ? finish_call(s, call, parts, true, s_text) : (int)RSQ_OK;      // (no pairs at all: the lengths stay 0, nothing to wait for but the sieves)
    if (parts > 1)                                                   // the caller's stream continues behind the whole call
        for (hipStream_t side : {s_sieve, s_text}) HIP_CHECK(hipStreamSynchronize(side));
    HIP_CHECK(hipStreamSynchronize(st));
    abort_guard.armed = false;
    return rc;
}

// The open runs take the pairs of a call that has returned RSQ_OK -- and of no other, so a call repeated after RSQ_ENOSPC counts its pairs once: the call was one
// part, whose fragments and raw arrays still lie in the workspace (rsq_sim::KeptPart).  The stream is idle afterwards (the next call may reuse the arrays on another).
static void depth_take(rsq_sim &s, const rsq_sim::KeptPart &k, hipStream_t st) {
    rsq_sim::Depth &d = s.depth;
    const dim3 grid((uint32_t)cdiv(2u * k.n_pairs, 256)), block(256);
    s.timers["depth_add"].start(st);
    if (s.has_variants) hipLaunchKernelGGL(k_depth_add<true>, grid, block, 0, st, s.dev, k.frags, k.fvars, k.n_pairs, k.raw, k.row_order, d.diff.as<uint32_t>(), d.bad.as<uint32_t>());
    else hipLaunchKernelGGL(k_depth_add<false>, grid, block, 0, st, s.dev, k.frags, k.fvars, k.n_pairs, k.raw, k.row_order, d.diff.as<uint32_t>(), d.bad.as<uint32_t>());
    s.timers["depth_add"].stop(st);
}
// The rows kernel's geometry is rsq_stats.h's stats_rows_geometry; options stats_chunk, stats_slab and stats_groups replace its three choices.
static void stats_take(rsq_sim &s, const rsq_sim::KeptPart &k, hipStream_t st) {
    const StatsLayout &y = s.stats.lay;
    uint64_t *counts = s.stats.counts.as<uint64_t>();
    const bool skew = s.opt.stats_form != 1;
    if (2u * k.n_pairs >= (1ull << 32)) throw Error("more than 2^32 reads in one call: a workgroup of the report's kernels counts in 32 bits (use smaller block ranges)");
    if (y.lmax) {
        const StatsRowsGeometry geo = stats_rows_geometry(y.lmax, y.len[0], y.len[1], y.Q, skew, s.read_stride / 4u, s.n_cu, k.n_pairs, s.opt.stats_chunk, s.opt.stats_slab, s.opt.stats_groups);
        const StatsRowsPlan &plan = geo.plan;
        const uint32_t lds = geo.lds, groups = geo.groups, units = plan.units[0] + plan.units[1];
        if (lds > 64u * 1024u) throw Error("the simulation report's image of " + std::to_string(plan.chunk) + " positions does not fit the LDS (option stats_chunk, or a profile with more than 250 quality values)");
        if (units) {
            s.timers["stats_rows"].start(st);
            if (skew) hipLaunchKernelGGL(k_stats_rows<true>, dim3(groups), dim3(kStatsRowsBlock), lds, st, k.raw.seq, k.raw.qual, k.raw.meta, k.raw.pitch, k.n_pairs, y, plan, counts);
            else hipLaunchKernelGGL(k_stats_rows<false>, dim3(groups), dim3(kStatsRowsBlock), lds, st, k.raw.seq, k.raw.qual, k.raw.meta, k.raw.pitch, k.n_pairs, y, plan, counts);
            s.timers["stats_rows"].stop(st);
        }
    }
    const uint32_t grid = (uint32_t)std::min<uint64_t>(cdiv(2u * k.n_pairs, kStatsMatesBlock), s.opt.stats_groups > 0 ? (uint64_t)s.opt.stats_groups : 4ull * s.n_cu);
    s.timers["stats_mates"].start(st);
    if (s.has_variants) hipLaunchKernelGGL(k_stats_mates<true>, dim3(grid), dim3(kStatsMatesBlock), y.image_words * 4u, st, s.dev, k.frags, k.fvars, k.n_pairs, k.raw, k.row_order, y, counts);
    else hipLaunchKernelGGL(k_stats_mates<false>, dim3(grid), dim3(kStatsMatesBlock), y.image_words * 4u, st, s.dev, k.frags, k.fvars, k.n_pairs, k.raw, k.row_order, y, counts);
    s.timers["stats_mates"].stop(st);
}
static void pileup_take(rsq_sim &s, const rsq_sim::KeptPart &k, hipStream_t st) {
    rsq_sim::Pileup &u = s.pileup;
    const dim3 grid((uint32_t)cdiv(2u * k.n_pairs, 256)), block(256);
    const uint32_t strands = u.sets > 1u ? 1u : 0u;
    s.timers["pileup_add"].start(st);
    if (s.has_variants)
        hipLaunchKernelGGL(k_pileup_add<true>, grid, block, 0, st, s.dev, k.frags, k.fvars, k.n_pairs, k.raw, k.row_order, u.planes.as<uint32_t>(), u.words, strands, u.bad.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_pileup_add<false>, grid, block, 0, st, s.dev, k.frags, k.fvars, k.n_pairs, k.raw, k.row_order, u.planes.as<uint32_t>(), u.words, strands, u.bad.as<uint32_t>());
    s.timers["pileup_add"].stop(st);
}
static void runs_take(rsq_sim &s, hipStream_t st) {
    rsq_sim::KeptPart &k = s.kept;
    if (!k.have || !k.n_pairs) return;
    k.have = false;
    if (s.depth.open) depth_take(s, k, st);
    if (s.stats.open) stats_take(s, k, st);
    if (s.pileup.open) pileup_take(s, k, st);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));
}
// what a depth run refuses of the calls that simulate: pairs after rsq_sim_depth_finish
static bool depth_refusal(const rsq_sim &s) {
    if (s.pileup.open && s.pileup.finished) {
        g_last_error = "the pileup run is finished (rsq_sim_pileup_finish): rsq_sim_pileup_end must run before more pairs are simulated";
        return true;
    }
    if (!s.depth.open || !s.depth.finished) return false;
    g_last_error = "the depth run is finished (rsq_sim_depth_finish): rsq_sim_depth_end must run before more pairs are simulated";
    return true;
}
static bool depth_refuses_job(const rsq_sim &s, const char *call) {
    if (s.stats.open) {
        g_last_error = std::string(call) + ": a stats run is open (rsq_sim_stats_begin); the job calls are not counted in the simulation report";
        return true;
    }
    if (s.pileup.open) {
        g_last_error = std::string(call) + ": a pileup run is open (rsq_sim_pileup_begin); the job calls do not accumulate the pileup";
        return true;
    }
    if (!s.depth.open) return false;
    g_last_error = std::string(call) + ": a depth run is open (rsq_sim_depth_begin); the job calls do not accumulate depth";
    return true;
}

// The end of a sorted call (rsq_bamsort.h), behind its parts -- or, at the flush, over the held records alone: the sort of the directory's keys, the cut, and,
// when every buffer of the call fits, the gather into the caller's buffer (call.truth) and the index material.  Until then nothing of the run's state has changed
// (the held records and their entries lie untouched in front of the call's), so a call that ends with RSQ_ENOSPC can be repeated.  rc: what the parts came to.
static int sorted_finish(rsq_sim &s, const PairsCall &call, int rc, uint64_t cut, uint32_t block_hi) {
    rsq_sim::BamSorted &b = s.bam_sorted;
    const hipStream_t st = call.st;
    const uint64_t n = b.n_held + 2u * b.call_pairs;
    *call.truth.len = b.call_records = b.call_mapped = 0;
    if (n >= (1ull << 32)) throw Error("more than 2^32 BAM records in one sorted call: use smaller block ranges");
    if (!n) {
        if (rc == RSQ_OK) {
            b.prev_cut = cut;
            b.next_block = block_hi;
        }
        return rc;
    }
    s.cur = &s.ws[0];                                                // (the scans' scratch)
    const BamDirEntry *dir = b.dir[b.cur].as<BamDirEntry>();
    const uint32_t tiles = (uint32_t)cdiv(n, kBamSortTile), blocks = (uint32_t)cdiv(n, 256);
    for (int k = 0; k < 2; ++k) {
        b.keys[k].reserve(n * 8u);
        b.idx[k].reserve(n * 4u);
    }
    b.hist.reserve((size_t)tiles * kBamSortBins * 4u);
    b.hist_at.reserve(((size_t)tiles * kBamSortBins + 1u) * 8u);
    b.sizes.reserve(n * 4u);
    b.at.reserve((n + 1u) * 8u);
    b.result.reserve(64);
    uint64_t *const sort_keys[2] = {b.keys[0].as<uint64_t>(), b.keys[1].as<uint64_t>()};
    uint32_t *const sort_idx[2] = {b.idx[0].as<uint32_t>(), b.idx[1].as<uint32_t>()};
    s.timers["bam_sort"].start(st);
    hipLaunchKernelGGL(k_bam_sort_init, dim3(blocks), dim3(256), 0, st, dir, n, sort_keys[0], sort_idx[0]);
    const int from = bam_sort_passes(sort_keys, sort_idx, n, b.plan, b.hist.as<uint32_t>(), b.hist_at.as<uint64_t>(),
                                     [&](const uint32_t *in, uint64_t count, uint64_t *out) { exclusive_scan(s, in, count, out, st); }, st);
    const uint64_t *keys = b.keys[from].as<uint64_t>();
    const uint32_t *idx = b.idx[from].as<uint32_t>();
    hipLaunchKernelGGL(k_bam_sorted_sizes, dim3(blocks), dim3(256), 0, st, dir, idx, n, b.sizes.as<uint32_t>());
    exclusive_scan(s, b.sizes.as<uint32_t>(), n, b.at.as<uint64_t>(), st);
    hipLaunchKernelGGL(k_bam_cut, dim3(1), dim3(1), 0, st, keys, n, cut, bam_unmapped_key(s.dev.n_seqs), b.at.as<uint64_t>(), b.out_of_order.as<uint32_t>(), b.result.as<uint64_t>());
    s.timers["bam_sort"].stop(st);
    HIP_CHECK(hipGetLastError());
    uint64_t r[6];
    HIP_CHECK(hipMemcpyAsync(r, b.result.as<uint64_t>(), sizeof r, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t n_final = r[0], mapped = r[1], final_bytes = r[2], mapped_bytes = r[3], all_bytes = r[4];
    if (r[5]) {
        g_last_error = "sorted BAM: " + std::to_string(r[5]) + " records lie below the cut of the call before or outside their sequence: the stream would not be sorted";
        return RSQ_EINVAL;
    }
    *call.truth.len = final_bytes;
    b.call_records = n_final;
    b.call_mapped = mapped;
    if (rc == RSQ_ENOSPC || (rc == RSQ_OK && (final_bytes > call.truth.cap || (!call.truth.dst && final_bytes)))) {
        g_last_error = call.need() + " of FASTQ text and " + std::to_string(final_bytes) + " of sorted BAM records";
        return RSQ_ENOSPC;
    }
    if (rc != RSQ_OK) return rc;
    const int other = b.cur ^ 1;
    const uint64_t n_held = n - n_final, held_bytes = all_bytes - final_bytes;
    b.stage[other].reserve(held_bytes + 32u);
    b.dir[other].reserve(n_held * sizeof(BamDirEntry) + 8u);
    s.timers["bam_gather"].start(st);
    hipLaunchKernelGGL(k_bam_gather, dim3((uint32_t)cdiv(n, 16)), dim3(256), 0, st, dir, idx, b.at.as<uint64_t>(), n, n_final, b.stage[b.cur].as<char>(), call.truth.dst, b.stage[other].as<char>(),
                       b.dir[other].as<BamDirEntry>());
    s.timers["bam_gather"].stop(st);
    HIP_CHECK(hipGetLastError());
    if (mapped) {                                                    // the index material of the call's mapped final records
        b.flags.reserve(mapped * 4u);
        b.run_of.reserve((mapped + 1u) * 8u);
        s.timers["bam_index"].start(st);
        hipLaunchKernelGGL(k_bam_index_flags, dim3((uint32_t)cdiv(mapped, 256)), dim3(256), 0, st, dir, idx, b.at.as<uint64_t>(), mapped, b.stream_at, b.window_first.as<uint64_t>(),
                           b.windows.as<unsigned long long>(), b.flags.as<uint32_t>());
        exclusive_scan(s, b.flags.as<uint32_t>(), mapped, b.run_of.as<uint64_t>(), st);
        uint64_t n_runs = 0;
        HIP_CHECK(hipMemcpyAsync(&n_runs, b.run_of.as<uint64_t>() + mapped, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        b.runs.reserve(n_runs * sizeof(BamRunStart));
        hipLaunchKernelGGL(k_bam_index_runs, dim3((uint32_t)cdiv(mapped, 256)), dim3(256), 0, st, dir, idx, b.at.as<uint64_t>(), mapped, b.stream_at, b.flags.as<uint32_t>(),
                           b.run_of.as<uint64_t>(), b.runs.as<BamRunStart>());
        s.timers["bam_index"].stop(st);
        HIP_CHECK(hipGetLastError());
        std::vector<BamRunStart> starts(n_runs);
        HIP_CHECK(hipMemcpyAsync(starts.data(), b.runs.as<BamRunStart>(), n_runs * sizeof(BamRunStart), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        b.index.add_runs(starts.data(), starts.size(), b.stream_at + mapped_bytes);
    }
    HIP_CHECK(hipStreamSynchronize(st));
    b.cur = other;
    b.n_held = n_held;
    b.held_bytes = held_bytes;
    b.stream_at += final_bytes;
    b.prev_cut = cut == kBamCutAll ? b.prev_cut : cut;
    b.next_block = block_hi;
    return RSQ_OK;
}

// The reads' bases and qualities as rows of out_stride bytes (word-aligned): sixteen lanes copy a row, a word each per step -- 64 bytes of a row in one store
// instruction, where a lane per row wrote four bytes into each of 64 rows (10 ms per 8 M records of 150 bases).  Bytes past read_len inside the last word
// are zero in the raw arrays.
__global__ void __launch_bounds__(256) k_error_model_rows(RawLayout raw, uint64_t n, uint8_t *seq_out, uint8_t *qual_out, uint32_t out_stride) {
    const uint64_t row = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    if (row >= n) return;
    const uint64_t i = raw.item_of(row);
    const uint32_t read_len = raw.meta[row].read_len, nb = read_len < out_stride ? read_len : out_stride;
    const WordColumn seq = raw.seq_of(row), qual = raw.qual_of(row);
    uint32_t *so = reinterpret_cast<uint32_t *>(seq_out + i * out_stride), *qo = reinterpret_cast<uint32_t *>(qual_out + i * out_stride);
    for (uint32_t w = threadIdx.x & 15u; 4u * w < nb; w += 16u) {
        so[w] = seq.at(w);
        qo[w] = qual.at(w);
    }
}

// CIGAR strings and per-read scalars of the error-model-only mode (and the rows when they are not word-aligned)
__global__ void k_error_model_out(RawLayout raw, uint64_t n, uint8_t *seq_out, uint8_t *qual_out, uint32_t out_stride, uint16_t *read_len_out, uint16_t *num_errors_out,
                                  uint16_t *tile_out, char *cigar_out, uint32_t cigar_stride, uint32_t *overflow) {
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const uint64_t i = raw.item_of(row);
    const ReadMeta m = raw.meta[row];
    read_len_out[i] = m.read_len;
    num_errors_out[i] = m.num_errors;
    tile_out[i] = m.tile_id;
    const uint32_t nb = m.read_len < out_stride ? m.read_len : out_stride;
    const WordColumn seq = raw.seq_of(row), qual = raw.qual_of(row);
    if ((out_stride | (uint32_t)(uintptr_t)seq_out | (uint32_t)(uintptr_t)qual_out) & 3u)        // (word-aligned rows are copied by k_error_model_rows)
        for (uint32_t k = 0; k < nb; ++k) {
            seq_out[i * out_stride + k] = (uint8_t)(seq.at(k >> 2) >> (8u * (k & 3u)));
            qual_out[i * out_stride + k] = (uint8_t)(qual.at(k >> 2) >> (8u * (k & 3u)));
        }
    if (m.cigar_chars + 1u > cigar_stride || m.read_len > out_stride) {
        *overflow = 1;
        cigar_out[i * cigar_stride] = 0;
        return;
    }
    TextSink t{cigar_out + i * cigar_stride, 0};
    cigar_replay(raw.ops_of(row), m, t);
    t.ch(0);
}

}  // namespace rsq

// ================================================================================================= C ABI
// (a seqToIllumina record whose fragment length the profile's tables do not hold: check_fragment_lengths)
struct FragmentLengthOutside : rsq::Error {
    using rsq::Error::Error;
};
template <class F>
static int guard(F &&f) {
    try {
        return f();
    } catch (const HipError &e) {
        g_last_error = e.what();
        return RSQ_EHIP;
    } catch (const FragmentLengthOutside &e) {
        g_last_error = e.what();
        return RSQ_EIO;
    } catch (const Error &e) {
        g_last_error = e.what();
        return RSQ_EINVAL;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return RSQ_EINVAL;
    }
}
#define REQUIRE(cond, msg)          \
    do {                            \
        if (!(cond)) {              \
            g_last_error = msg;     \
            return RSQ_EINVAL;      \
        }                           \
    } while (0)

extern "C" {

const char *rsq_last_error(void) { return g_last_error.c_str(); }
const char *rsq_last_warning(void) { return g_last_warning.c_str(); }
const char *rsq_version(void) { return "reseq_amd 0.1 (gfx950)"; }
int rsq_set_option(const char *name, int64_t value) {
    REQUIRE(name, "null argument");
    if (set_option(name, value)) return RSQ_OK;
    g_last_error = std::string("unknown option '") + name + "' (options: " + option_names() + ")";
    return RSQ_EINVAL;
}
int rsq_get_option(const char *name, int64_t *value) {
    REQUIRE(name && value, "null argument");
    if (get_option(name, value)) return RSQ_OK;
    g_last_error = std::string("unknown option '") + name + "' (options: " + option_names() + ")";
    return RSQ_EINVAL;
}

int rsq_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_last_error = "no HIP device visible; this library has no CPU fallback";
        return RSQ_ENODEV;
    }
    return n;
}

// Which blocks a worker simulates (Simulator.cpp:2384-2401 hands blocks to threads one by one from a counter; here every worker owns a contiguous range, so that the
// workers' texts in worker order are the single run's): ranges balanced by expected pairs per block.  The one rule for the `reseq` command line's device threads and
// the N-process launcher (reseq_amd/sharding.py partition_blocks states the same arithmetic in the same order; tests/test_abi.py compares them).
int rsq_partition_blocks(uint32_t total_blocks, uint32_t workers, const double *weights, uint32_t *bounds) {
    REQUIRE(workers >= 1 && bounds && (weights || !total_blocks), "null argument or no worker");
    double total = 0.0;
    for (uint32_t b = 0; b < total_blocks; ++b) total += weights[b];
    bounds[0] = 1;
    double acc = 0.0;
    uint32_t b = 0;
    for (uint32_t r = 1; r < workers; ++r) {
        const double target = total * (double)r / (double)workers;
        while (b < total_blocks && acc + weights[b] / 2 <= target) acc += weights[b++];
        bounds[r] = b + 1u;
    }
    bounds[workers] = total_blocks + 1u;
    return RSQ_OK;
}
int rsq_sim_block_weights(const rsq_sim *s, double *weights, size_t cap, uint32_t *n_blocks) {
    REQUIRE(s && n_blocks && (s->prepared || s->pre.planned) && s->has_ref, "a simulator with a reference after rsq_sim_prepare or rsq_sim_prepare_plan");
    *n_blocks = s->total_blocks;
    if (!weights) return RSQ_OK;
    if (cap < s->total_blocks) {
        g_last_error = "room for " + std::to_string(cap) + " weights, the job has " + std::to_string(s->total_blocks) + " blocks";
        return RSQ_ENOSPC;
    }
    size_t at = 0;
    for (uint32_t i = 0; i < s->dev.n_seqs; ++i)                   // a sequence's blocks share its reference bias; sequences shorter than the longest insert have none (:1159)
        for (uint32_t k = 0; k < s->n_blocks[i]; ++k) weights[at++] = s->ref_seq_bias[i];
    REQUIRE(at == s->total_blocks, "block counts do not add up");
    return RSQ_OK;
}

int rsq_profile_load_reseq(const char *stats_path, const char *ipf_path, double ipf_precision_percent, rsq_profile **out) {
    REQUIRE(stats_path && out, "null argument");
    REQUIRE(ipf_precision_percent > 0.0, "ipfPrecision must be positive.");      // main.cpp:776-779
    try {
        g_last_warning.clear();
        *out = new rsq_profile{Profile::load_archives(stats_path, ipf_path ? ipf_path : "", ipf_precision_percent / 100.0, &g_last_warning)};
        return RSQ_OK;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return RSQ_EIO;
    }
}
int rsq_profile_is_reseq_archive(const char *path, int *yes) {
    REQUIRE(path && yes, "null argument");
    *yes = Profile::is_archive(path) ? 1 : 0;
    return RSQ_OK;
}
int rsq_profile_load(const char *path, rsq_profile **out) {
    REQUIRE(path && out, "null argument");
    try {
        if (Profile::is_archive(path)) return rsq_profile_load_reseq(path, nullptr, 5.0, out);
        *out = new rsq_profile{Profile::load(path)};
        return RSQ_OK;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return RSQ_EIO;
    }
}
int rsq_profile_archive_layout(const char *stats_path, const char *ipf_path, char *out, size_t cap, size_t *need) {
    REQUIRE(stats_path && need && (out || !cap), "null argument");
    return guard([&] {
        const std::string text = Profile::archive_layout(stats_path, ipf_path ? ipf_path : "");
        *need = text.size() + 1;
        if (cap) {
            const size_t n = std::min(cap - 1, text.size());
            memcpy(out, text.data(), n);
            out[n] = 0;
        }
        return (int)RSQ_OK;
    });
}
int rsq_profile_save(const rsq_profile *p, const char *path) {
    REQUIRE(p && path, "null argument");
    try {
        p->p.save(path);
        return RSQ_OK;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return RSQ_EIO;
    }
}
int rsq_profile_save_reseq(const rsq_profile *p, const char *stats_path, const char *ipf_path, uint64_t creation_time) {
    REQUIRE(p && stats_path, "null argument");
    try {
        p->p.save_archives(stats_path, ipf_path ? ipf_path : "", creation_time ? creation_time : (uint64_t)time(nullptr));
        return RSQ_OK;
    } catch (const Error &e) {
        g_last_error = e.what();
        return RSQ_EINVAL;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return RSQ_EIO;
    }
}
void rsq_profile_free(rsq_profile *p) { delete p; }
int rsq_profile_change_error_rate(rsq_profile *p, double m) {
    REQUIRE(p && m > 0.0, "bad error multiplier");
    p->p.change_error_rate(m);
    return RSQ_OK;
}
int rsq_profile_remove_substitution_errors(rsq_profile *p) {
    REQUIRE(p, "null profile");
    p->p.remove_substitution_errors();
    return RSQ_OK;
}
int rsq_profile_remove_indel_errors(rsq_profile *p) {
    REQUIRE(p, "null profile");
    p->p.remove_indel_errors();
    return RSQ_OK;
}
int rsq_profile_max_read_length(const rsq_profile *p, uint32_t *out) {
    REQUIRE(p && out, "null argument");
    *out = (uint32_t)std::max(p->p.read_lengths[0].to(), p->p.read_lengths[1].to()) - 1;
    return RSQ_OK;
}
int rsq_profile_num_tiles(const rsq_profile *p, uint32_t *out) {
    REQUIRE(p && out, "null argument");
    *out = p->p.n_tiles();
    return RSQ_OK;
}

int rsq_profile_max_len_deletion(const rsq_profile *p, uint32_t *out) {
    REQUIRE(p && out, "null argument");
    *out = p->p.max_len_deletion;
    return RSQ_OK;
}
int rsq_profile_ref_seq_bias(const rsq_profile *p, double *out, size_t cap, size_t *n) {
    REQUIRE(p && n, "null argument");
    *n = p->p.ref_seq_bias.size();
    if (!out) return RSQ_OK;
    if (cap < *n) return RSQ_ENOSPC;
    memcpy(out, p->p.ref_seq_bias.data(), *n * sizeof(double));
    return RSQ_OK;
}
int rsq_ref_sequence_name(const rsq_ref *r, uint32_t seq, char *out, size_t cap) {
    REQUIRE(r && out && seq < r->r.codes.size(), "bad sequence id");
    const std::string name = r->r.first_part(seq);
    if (name.size() + 1 > cap) return RSQ_ENOSPC;
    memcpy(out, name.c_str(), name.size() + 1);
    return RSQ_OK;
}

// the header of the truth alignments (rsq_sim_pairs_sam): host code
int rsq_ref_sam_header(const rsq_ref *r, char *out, size_t cap, size_t *need) {
    REQUIRE(r && need, "null argument");
    std::string text = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n";
    for (uint32_t seq = 0; seq < r->r.codes.size(); ++seq) text += "@SQ\tSN:" + r->r.first_part(seq) + "\tLN:" + std::to_string(r->r.codes[seq].size()) + "\n";
    text += "@PG\tID:reseq_amd\tPN:reseq_amd\n";
    *need = text.size();
    if (!out || cap < text.size()) {
        g_last_error = "header buffer too small: need " + std::to_string(text.size()) + " bytes";
        return RSQ_ENOSPC;
    }
    memcpy(out, text.data(), text.size());
    if (cap > text.size()) out[text.size()] = 0;
    return RSQ_OK;
}

// the same header in front of the BAM records (rsq_sim_pairs_bam; SAM specification 4.2): magic, the text, the sequences' names and lengths; coordinate: of the
// sorted file (rsq_sim_pairs_bam_sorted), whose @HD line says so
int rsq_ref_bam_header(const rsq_ref *r, char *out, size_t cap, size_t *need) { return rsq_ref_bam_header_so(r, 0, out, cap, need); }
int rsq_ref_bam_header_so(const rsq_ref *r, int coordinate, char *out, size_t cap, size_t *need) {
    REQUIRE(r && need, "null argument");
    size_t text_len = 0;
    (void)rsq_ref_sam_header(r, nullptr, 0, &text_len);
    std::string text(text_len, '\0'), h = "BAM\1";
    if (const int rc = rsq_ref_sam_header(r, &text[0], text_len, &text_len)) return rc;
    if (coordinate) {                                                // the same text with another first line
        const std::string unsorted = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n";
        REQUIRE(text.compare(0, unsorted.size(), unsorted) == 0, "the SAM header does not begin with the @HD line rsq_ref_bam_header_so replaces");
        text = "@HD\tVN:1.6\tSO:coordinate\n" + text.substr(unsorted.size());
    }
    auto put32 = [&](uint32_t v) {
        for (int k = 0; k < 4; ++k) h += (char)((v >> (8 * k)) & 0xFFu);
    };
    put32((uint32_t)text.size());
    h += text;
    put32((uint32_t)r->r.codes.size());
    for (uint32_t seq = 0; seq < r->r.codes.size(); ++seq) {
        const std::string name = r->r.first_part(seq);
        put32((uint32_t)name.size() + 1u);
        h += name;
        h += '\0';
        put32((uint32_t)r->r.codes[seq].size());
    }
    *need = h.size();
    if (!out || cap < h.size()) {
        g_last_error = "header buffer too small: need " + std::to_string(h.size()) + " bytes";
        return RSQ_ENOSPC;
    }
    memcpy(out, h.data(), h.size());
    return RSQ_OK;
}

// ---- the alleles of a reference with variants as sequences of their own (rsq_alleles.h): lengths, the FASTA text's size and index, the truth headers that name them
// bases of every (sequence, allele): the sequence's, and per variant of the allele the bases of its replacement minus the one it replaces
static std::vector<uint64_t> allele_lengths(const rsq_ref &r) {
    const uint32_t na = r.variants.num_alleles;
    std::vector<uint64_t> len(r.r.codes.size() * na);
    for (size_t seq = 0; seq < r.r.codes.size(); ++seq) {
        std::vector<int64_t> n(na, (int64_t)r.r.codes[seq].size());
        for (const Variant &v : r.variants.by_seq[seq])
            for (uint32_t w = 0; w < 2u; ++w)
                for (uint64_t bits = v.allele[w]; bits; bits &= bits - 1u) {
                    const uint32_t a = 64u * w + (uint32_t)__builtin_ctzll(bits);
                    if (a < na) n[a] += (int64_t)v.var_seq.size() - 1;
                }
        for (uint32_t a = 0; a < na; ++a) len[seq * na + a] = (uint64_t)n[a];
    }
    return len;
}
static std::vector<std::string> first_parts(const rsq_ref &r) {
    std::vector<std::string> names;
    for (size_t seq = 0; seq < r.r.codes.size(); ++seq) names.push_back(r.r.first_part(seq));
    return names;
}
static int put_text(const std::string &text, const char *what, char *out, size_t cap, size_t *need) {
    *need = text.size();
    if (!out || cap < text.size()) {
        g_last_error = std::string(what) + " buffer too small: need " + std::to_string(text.size()) + " bytes";
        return RSQ_ENOSPC;
    }
    memcpy(out, text.data(), text.size());
    if (cap > text.size()) out[text.size()] = 0;
    return RSQ_OK;
}
#define REQUIRE_VARIANTS(r) REQUIRE((r)->has_variants, "the reference has no variants (rsq_ref_read_variants): it has no alleles to write")
int rsq_ref_allele_length(const rsq_ref *r, uint32_t seq, uint32_t allele, uint64_t *out) {
    REQUIRE(r && out, "null argument");
    REQUIRE_VARIANTS(r);
    REQUIRE(seq < r->r.codes.size() && allele < r->variants.num_alleles, "no such sequence or allele");
    int64_t n = (int64_t)r->r.codes[seq].size();
    for (const Variant &v : r->variants.by_seq[seq])
        if (v.in_allele(allele)) n += (int64_t)v.var_seq.size() - 1;
    *out = (uint64_t)n;
    return RSQ_OK;
}
int rsq_ref_alleles_fasta_size(const rsq_ref *r, uint64_t *bytes) {
    REQUIRE(r && bytes, "null argument");
    REQUIRE_VARIANTS(r);
    *bytes = allele_records(first_parts(*r), r->variants.num_alleles, allele_lengths(*r)).back().at;
    return RSQ_OK;
}
// samtools faidx's index of that text: NAME, LENGTH, OFFSET of the first base, bases per line, bytes per line
int rsq_ref_alleles_fai(const rsq_ref *r, char *out, size_t cap, size_t *need) {
    REQUIRE(r && need, "null argument");
    REQUIRE_VARIANTS(r);
    const std::vector<std::string> names = first_parts(*r);
    const uint32_t na = r->variants.num_alleles;
    const std::vector<AlleleRecord> rec = allele_records(names, na, allele_lengths(*r));
    std::string text;
    for (size_t m = 0; m + 1 < rec.size(); ++m)
        text += names[m / na] + "_allele" + std::to_string(m % na) + "\t" + std::to_string(rec[m].length) + "\t" + std::to_string(rec[m].at + rec[m].header) + "\t" + std::to_string(kFastaLine) + "\t" +
                std::to_string(kFastaLine + 1u) + "\n";
    return put_text(text, "index", out, cap, need);
}
// the headers of truth alignments in allele coordinates: the sequences are the records of that text, in its order
static int alleles_header(const rsq_ref *r, bool bam, char *out, size_t cap, size_t *need) {
    REQUIRE(r && need, "null argument");
    REQUIRE_VARIANTS(r);
    const std::vector<std::string> names = first_parts(*r);
    const uint32_t na = r->variants.num_alleles;
    const std::vector<uint64_t> len = allele_lengths(*r);
    std::string text = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n", entries;
    auto put32 = [](std::string &h, uint32_t v) {
        for (int k = 0; k < 4; ++k) h += (char)((v >> (8 * k)) & 0xFFu);
    };
    for (size_t m = 0; m < len.size(); ++m) {
        const std::string name = names[m / na] + "_allele" + std::to_string(m % na);
        if (!len[m]) {
            g_last_error = "allele " + name + " has no bases: a header cannot list a sequence of length 0";
            return RSQ_EINVAL;
        }
        text += "@SQ\tSN:" + name + "\tLN:" + std::to_string(len[m]) + "\n";
        put32(entries, (uint32_t)name.size() + 1u);
        entries += name;
        entries += '\0';
        put32(entries, (uint32_t)len[m]);
    }
    text += "@PG\tID:reseq_amd\tPN:reseq_amd\n";
    if (!bam) return put_text(text, "header", out, cap, need);
    std::string h = "BAM\1";
    put32(h, (uint32_t)text.size());
    h += text;
    put32(h, (uint32_t)len.size());
    h += entries;
    return put_text(h, "header", out, cap, need);
}
int rsq_ref_sam_header_alleles(const rsq_ref *r, char *out, size_t cap, size_t *need) { return alleles_header(r, false, out, cap, need); }
int rsq_ref_bam_header_alleles(const rsq_ref *r, char *out, size_t cap, size_t *need) { return alleles_header(r, true, out, cap, need); }

int rsq_ref_load_fasta(const char *path, rsq_ref **out) {
    REQUIRE(path && out, "null argument");
    try {
        *out = new rsq_ref{Reference::read_fasta(path)};
        return RSQ_OK;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return RSQ_EIO;
    }
}
int rsq_ref_replace_n(rsq_ref *r, uint64_t seed) {
    REQUIRE(r, "null reference");
    return guard([&] {
        r->r.replace_n(seed);
        return RSQ_OK;
    });
}
void rsq_ref_free(rsq_ref *r) { delete r; }
int rsq_ref_num_sequences(const rsq_ref *r, uint32_t *out) {
    REQUIRE(r && out, "null argument");
    *out = (uint32_t)r->r.codes.size();
    return RSQ_OK;
}
int rsq_ref_sequence_length(const rsq_ref *r, uint32_t seq, uint32_t *out) {
    REQUIRE(r && out && seq < r->r.codes.size(), "bad sequence id");
    *out = (uint32_t)r->r.codes[seq].size();
    return RSQ_OK;
}
int rsq_ref_read_variants(rsq_ref *r, const char *path) {
    REQUIRE(r && path, "null argument");
    try {
        std::vector<std::string> first;
        for (size_t i = 0; i < r->r.codes.size(); ++i) first.push_back(r->r.first_part(i));
        r->variants = read_variants(path, first, r->r.codes);
        r->has_variants = true;
        return RSQ_OK;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return RSQ_EIO;
    }
}
int rsq_ref_num_alleles(const rsq_ref *r, uint32_t *out) {
    REQUIRE(r && out, "null argument");
    *out = r->variants.num_alleles;
    return RSQ_OK;
}
int rsq_ref_num_variants(const rsq_ref *r, uint32_t seq, uint32_t *out) {
    REQUIRE(r && out && r->has_variants && seq < r->variants.by_seq.size(), "no variants loaded or bad sequence id");
    *out = (uint32_t)r->variants.by_seq[seq].size();
    return RSQ_OK;
}
int rsq_ref_get_variant(const rsq_ref *r, uint32_t seq, uint32_t index, uint32_t *position, char *var_seq, size_t var_seq_cap, uint64_t allele_bits[2]) {
    REQUIRE(r && position && var_seq && allele_bits && r->has_variants && seq < r->variants.by_seq.size() && index < r->variants.by_seq[seq].size(), "bad variant index");
    const Variant &v = r->variants.by_seq[seq][index];
    REQUIRE(v.var_seq.size() + 1 <= var_seq_cap, "var_seq buffer too small");
    *position = v.position;
    for (size_t k = 0; k < v.var_seq.size(); ++k) var_seq[k] = "ACGTN"[v.var_seq[k]];
    var_seq[v.var_seq.size()] = 0;
    allele_bits[0] = v.allele[0];
    allele_bits[1] = v.allele[1];
    return RSQ_OK;
}
int rsq_ref_write_fasta(const rsq_ref *r, const char *path) {
    REQUIRE(r && path, "null argument");
    try {
        std::string text;
        for (size_t i = 0; i < r->r.codes.size(); ++i) {
            text += '>';
            text += r->r.names[i];
            text += '\n';
            const std::vector<uint8_t> &c = r->r.codes[i];
            for (size_t k = 0; k < c.size(); k += 70) {               // SeqAn's default FASTA line length
                for (size_t j = k; j < std::min(c.size(), k + 70); ++j) text += "ACGTN"[c[j] < 4 ? c[j] : 4];
                text += '\n';
            }
        }
        write_text_file(path, text);
        return RSQ_OK;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return RSQ_EIO;
    }
}
int rsq_ref_get_codes(const rsq_ref *r, uint32_t seq, uint8_t *out, uint32_t len) {
    REQUIRE(r && out && seq < r->r.codes.size() && len == r->r.codes[seq].size(), "bad sequence id or length");
    memcpy(out, r->r.codes[seq].data(), len);
    return RSQ_OK;
}

int rsq_sim_create(const rsq_profile *p, const rsq_ref *ref, int device, rsq_sim **out) {
    REQUIRE(p && out, "null argument");
    int n = rsq_device_count();
    if (n < 0) return n;
    REQUIRE(device >= 0 && device < n, "device index out of range");
    std::unique_ptr<rsq_sim> s(new rsq_sim());
    int rc = guard([&] {
        HIP_CHECK(hipSetDevice(device));
        s->device = device;
        s->up.device = device;
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, device));
        s->n_cu = (uint32_t)prop.multiProcessorCount;
        s->arch = prop.gcnArchName;
        s->specialize = s->opt.specialize != 0;
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&s->mailbox), sizeof(rsq_sim::Mailbox), hipHostMallocDefault));
        for (hipStream_t &st : s->side) HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        for (rsq_sim::Workspace &w : s->ws) HIP_CHECK(hipEventCreateWithFlags(&w.text_done, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&s->ev_call, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&s->ev_fill, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&s->ev_emit, hipEventDisableTiming));
        s->force_fill_mode = (int)s->opt.fill_mode;
        s->prof = p->p;
        pack_tables(*s, s->up);
        g_last_warning = s->plan_note;
        pack_profile(*s, s->up);
        if (ref) pack_reference(*s, s->up, ref->r, ref->has_variants ? &ref->variants : nullptr);
        return RSQ_OK;
    });
    if (rc == RSQ_OK) *out = s.release();
    return rc;
}
// the switches again, as they stand now (a simulator otherwise keeps the copy it took when it was created): for a caller that changes a call-shaping switch --
// overlap, job_chunk_bytes, job_write_direct, host_gzip, fill_waves, the pre-pass switches -- between the calls of ONE simulator.  What was decided when the
// simulator was created (fill_mode, image_tiles, rate_rows, base_call_word, min_quality_quads, specialize: the packed tables and the compiled kernel) stays.
int rsq_sim_take_options(rsq_sim *s) {
    REQUIRE(s, "null argument");
    s->opt = options();
    return RSQ_OK;
}
void rsq_sim_free(rsq_sim *s) {
    if (s) {
        (void)hipSetDevice(s->device);
        if (s->mailbox) (void)hipHostFree(s->mailbox);
        for (hipStream_t st : s->side)
            if (st) (void)hipStreamDestroy(st);
        for (rsq_sim::Workspace &w : s->ws)
            if (w.text_done) (void)hipEventDestroy(w.text_done);
        for (hipEvent_t e : {s->ev_call, s->ev_fill, s->ev_emit})
            if (e) (void)hipEventDestroy(e);
    }
    delete s;
}

int rsq_sim_prepare(rsq_sim *s, uint64_t seed, uint64_t num_read_pairs, double coverage, int ref_bias_mode, const char *record_base_identifier, void *stream) {
    REQUIRE(s, "null simulator");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        DevicePrepass be(*s, stream);
        s->sieve_tracks.drop();
        prepare(*s, s->up, be, seed, num_read_pairs, coverage, ref_bias_mode, record_base_identifier);
        return RSQ_OK;
    });
}

// the sharded pre-pass: the drivers of rsq_prepass.h refuse calls made out of order
int rsq_sim_prepare_plan(rsq_sim *s, uint64_t seed, uint64_t num_read_pairs, double coverage, int ref_bias_mode, const char *record_base_identifier) {
    REQUIRE(s, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        s->sieve_tracks.drop();
        prepare_plan(*s, s->up, seed, num_read_pairs, coverage, ref_bias_mode, record_base_identifier);
        return RSQ_OK;
    });
}
int rsq_sim_bias_partials(rsq_sim *s, uint32_t block_lo, uint32_t block_hi, double *sums, double *maxes, size_t cap, size_t *n, void *stream) {
    REQUIRE(s && n, "null argument");
    REQUIRE(s->pre.planned, "rsq_sim_prepare_plan must run first");
    *n = (size_t)bias_chunks(s->pre.bias_plan);
    if (!sums && !maxes && !cap) return RSQ_OK;                     // the size query
    REQUIRE(sums && maxes && cap >= *n, "arrays too small");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        DevicePrepass be(*s, stream);
        prepare_bias_partials(*s, be, block_lo, block_hi, sums, maxes);
        return RSQ_OK;
    });
}
int rsq_sim_prepare_normalization(rsq_sim *s, const double *sums, const double *maxes, size_t n) {
    REQUIRE(s && sums && maxes, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        prepare_normalization(*s, s->up, sums, maxes, n);
        return RSQ_OK;
    });
}
int rsq_sim_prepare_sys_errors(rsq_sim *s, uint32_t block_lo, uint32_t block_hi, const uint32_t in_state[2], uint32_t out_state[2], void *stream) {
    REQUIRE(s && in_state && out_state, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        DevicePrepass be(*s, stream);
        prepare_sys_errors(*s, be, block_lo, block_hi, in_state, out_state);
        return RSQ_OK;
    });
}
int rsq_sim_prepare_finish(rsq_sim *s) {
    REQUIRE(s, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        DevicePrepass be(*s, nullptr);
        prepare_finish(*s, be);
        return RSQ_OK;
    });
}

int rsq_sim_get_sequence_lengths(const rsq_sim *s, uint32_t *out, size_t cap, uint32_t *n_sequences) {
    REQUIRE(s && n_sequences && s->has_ref, "null argument, or a simulator without a reference");
    *n_sequences = (uint32_t)s->seq_len.size();
    if (out && cap >= s->seq_len.size()) memcpy(out, s->seq_len.data(), s->seq_len.size() * sizeof(uint32_t));
    else if (out) {
        g_last_error = "room for " + std::to_string(cap) + " lengths, the reference has " + std::to_string(s->seq_len.size()) + " sequences";
        return RSQ_ENOSPC;
    }
    return RSQ_OK;
}
// Reference::ReferenceSequence (Reference.cpp:483-567) for one call, the way the kernels get a template: allele_template on the allele's coordinate map (variants of
// any kind), else FragmentSrc on the allele's copy of the packed reference.  One thread; flag 1: the stretch leaves the allele's sequence.
__global__ void k_reference_sequence(DevSim S, uint32_t seq, uint32_t allele, uint32_t pos, VarStart from, uint32_t n, bool reversed, uint64_t *tmpl, uint32_t words, uint32_t *flag) {
    if (threadIdx.x || blockIdx.x) return;
    if (2u == S.variants_loaded) {
        const AlleleView a = allele_view(S, seq, allele);
        const int64_t h = from.start_variant_pos ? a.begin_of(a.entries_before(a.r.v[from.first_variant_id].pos)) + from.start_variant_pos : a.to_allele(pos);
        if (reversed ? h < (int64_t)n : h + (int64_t)n > a.length()) {
            *flag = 1u;
            return;
        }
        allele_template(a, pos, from, n, reversed, tmpl, words);
        return;
    }
    FragmentSrc src;
    src.words = hap_words(S, allele);
    src.word_off = S.seq_word_off[seq];
    src.first = pos;
    src.len = n;
    src.reverse = reversed;
    src.sys_ = nullptr;
    src.converted = nullptr;
    src.gc_prefix = nullptr;
    for (uint32_t w = 0; w < words; ++w) tmpl[w] = 0;
    for (uint32_t k = 0; k < n; ++k) tmpl[k >> 5] |= (uint64_t)src.ref(k) << ((k & 31u) * 2u);
}
int rsq_sim_reference_sequence(rsq_sim *s, uint32_t seq, uint32_t start_pos, uint32_t frag_length, int reversed, int32_t first_variant_id, uint32_t first_variant_pos, uint32_t allele,
                               uint8_t *out, size_t cap) {
    REQUIRE(s && out && s->has_ref && seq < s->dev.n_seqs, "null argument, a simulator without a reference, or no such sequence");
    REQUIRE(allele < (s->has_variants ? s->num_alleles : 1u), "no such allele");
    REQUIRE(frag_length <= (1u << 20) && cap >= frag_length, "room for fewer bases than asked for (at most 2^20 per call)");
    const uint32_t L = s->seq_len[seq];
    REQUIRE(reversed ? start_pos <= L : start_pos < L || 0 == frag_length, "start position outside the sequence");
    if (2 != s->variants_mode)                                      // alleles as long as the reference (with coordinate maps the kernel checks against the allele's length)
        REQUIRE(reversed ? frag_length <= start_pos : frag_length <= L - start_pos, "the stretch asked for leaves the sequence");
    if (first_variant_pos) {
        REQUIRE(2 == s->variants_mode, "a start inside inserted bases needs variants with insertions");
        const uint32_t n_var = s->var_ptr[seq + 1] - s->var_ptr[seq];
        REQUIRE(first_variant_id >= 0 && (uint32_t)first_variant_id < n_var && first_variant_pos <= s->variants[s->var_ptr[seq] + first_variant_id].len,
                "first_variant does not name bases of a variant of this sequence");
    }
    if (!frag_length) return RSQ_OK;
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        const uint32_t words = (frag_length + 31u) / 32u;
        uint64_t *dev = nullptr;
        HIP_CHECK(hipMalloc(&dev, (size_t)(words + 1u) * sizeof(uint64_t)));
        std::vector<uint64_t> host(words + 1u, 0);
        hipError_t e = hipMemset(dev, 0, (size_t)(words + 1u) * sizeof(uint64_t));
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_reference_sequence, dim3(1), dim3(64), 0, nullptr, s->dev, seq, allele, start_pos, VarStart{first_variant_id, first_variant_pos}, frag_length, reversed != 0,
                               dev, words, reinterpret_cast<uint32_t *>(dev + words));
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(host.data(), dev, host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
        (void)hipFree(dev);
        HIP_CHECK(e);
        if (host[words]) {
            g_last_error = "the stretch asked for leaves the allele's sequence";
            return RSQ_EINVAL;
        }
        for (uint32_t k = 0; k < frag_length; ++k) out[k] = (uint8_t)((host[k >> 5] >> ((k & 31u) * 2u)) & 3u);
        return RSQ_OK;
    });
}
// bases of every (sequence, allele) of a simulator with variants: the sequence's length and the total shift of the allele's map (its sentinel)
static std::vector<int64_t> sim_allele_lengths(const rsq_sim &s) {
    std::vector<int64_t> length(s.seq_len.size() * s.num_alleles);
    for (size_t m = 0; m < length.size(); ++m) length[m] = (int64_t)s.seq_len[m / s.num_alleles] + s.allele_map[s.allele_map_ptr[m + 1] - 1u].shift;
    return length;
}
// Bytes [at, at + bytes) of the alleles' FASTA text (rsq_alleles.h) into device memory: one launch, whatever the piece and the destination's alignment
int rsq_sim_alleles_fasta(rsq_sim *s, uint64_t at, size_t bytes, char *dst_dev, void *stream) {
    REQUIRE(s && (dst_dev || !bytes), "null argument");
    REQUIRE(s->has_ref && s->has_variants, "rsq_sim_alleles_fasta needs a reference with variants (rsq_ref_read_variants): there are no alleles to write");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        hipStream_t st = (hipStream_t)stream;
        rsq_sim::AllelesText &text = s->alleles_text;
        if (!text.n) {
            const uint32_t na = s->num_alleles;
            const std::vector<int64_t> bases = sim_allele_lengths(*s);
            std::vector<uint64_t> length(bases.size());
            for (size_t m = 0; m < bases.size(); ++m) {
                if (bases[m] < 0 || bases[m] > 0xFFFFFFFFll) throw Error("rsq_sim_alleles_fasta: an allele of " + s->ref_first_names[m / na] + " has more than 2^32 bases");
                length[m] = (uint64_t)bases[m];
            }
            const std::vector<AlleleRecord> records = allele_records(s->ref_first_names, na, length);
            text.records.upload(records);
            text.bytes = records.back().at;
            text.n = (uint32_t)records.size() - 1u;
        }
        if (at > text.bytes || bytes > text.bytes - at)
            throw Error("rsq_sim_alleles_fasta: bytes " + std::to_string(at) + " to " + std::to_string(at + bytes) + " were asked for, the text has " + std::to_string(text.bytes));
        reset_call_timers(*s);
        if (!bytes) return RSQ_OK;
        const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(dst_dev) & 15u);
        const uint64_t tiles = (lead + (uint64_t)bytes + kTileBytes - 1u) / kTileBytes;
        if (tiles > 0x7FFFFFFFull) throw Error("rsq_sim_alleles_fasta: at most 2^45 bytes per call");
        Timer &timer = s->timers["alleles_fasta"];
        timer.start(st);
        hipLaunchKernelGGL(k_alleles_fasta, dim3((uint32_t)tiles), dim3(kTileLanes), 0, st, s->dev, s->names, text.records.as<AlleleRecord>(), text.n, at, (uint64_t)bytes, lead, dst_dev);
        timer.stop(st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
        return RSQ_OK;
    });
}
int rsq_sim_export_reference(rsq_sim *s, const char *path) {
    REQUIRE(s && path, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        HIP_CHECK(hipDeviceSynchronize());
        export_reference(*s, s->up, path);
        return RSQ_OK;
    });
}
int rsq_sim_import_reference(rsq_sim *s, const char *path) {
    REQUIRE(s && path, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        MappedFile m(path);
        s->sieve_tracks.drop();
        import_reference(*s, s->up, m.data, m.size, path);
        s->alleles_text.n = 0;
        return RSQ_OK;
    });
}
int rsq_sim_specialize(rsq_sim *s, int kind, int *specialized) {
    REQUIRE(s && specialized && (kind == 0 || kind == 1), "null argument, or a kind that is neither 0 (read pairs) nor 1 (seqToIllumina records)");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        const uint32_t mask = effective_fill_mask(s->dev.lds.mask, s->force_fill_mode);
        g_spec_note.clear();
        hipFunction_t fn = spec_kernel(*s, kind == 0 ? SpecKind::kReads : SpecKind::kRecords, mask, kind == 0 && s->has_variants, fill_is_binned(*s));
        if (kind == 1 && fn) fn = spec_kernel(*s, SpecKind::kRecords, mask, true, fill_is_binned(*s));      // and the kernel for records parsed on the device (packed codes)
        *specialized = fn != nullptr;
        if (!s->specialize) g_spec_note = "option specialize is 0: the library's own instantiation of the read kernel runs";
        else if (!mask) g_spec_note = "the read kernel draws in double precision from device memory (no table image): nothing to compile for the profile";
        g_last_warning = g_spec_note;
        return RSQ_OK;
    });
}
// host only: the plan of the profile packed into host memory (nothing is uploaded), then the compilation rsq_sim_specialize would do
int rsq_profile_compile_read_kernel(const rsq_profile *p, int kind, int with_variants, int binned, const char *arch, const char *out_path, size_t *code_bytes, double *seconds) {
    REQUIRE(p && arch && code_bytes && (kind == 0 || kind == 1), "null argument, or a kind that is neither 0 nor 1");
    struct HostArrays : Uploader {
        std::vector<std::unique_ptr<char[]>> owned;
        void *put_bytes(const void *data, size_t bytes) override {
            owned.emplace_back(new char[bytes + 8]);
            memcpy(owned.back().get(), data, bytes);
            return owned.back().get();
        }
        void *put_zeros(size_t bytes) override {
            owned.emplace_back(new char[bytes + 8]());
            return owned.back().get();
        }
        void write_bytes(void *dst, const void *src, size_t bytes) override { memcpy(dst, src, bytes); }
        void read_bytes(void *dst, const void *src, size_t bytes) override { memcpy(dst, src, bytes); }
    };
    int rc = guard([&] {
        HostArrays up;
        SimState s;
        s.prof = p->p;
        pack_tables(s, up);
        pack_profile(s, up);
        if (!s.dev.lds.mask) throw Error("the profile has no table image (" + s.plan_note + "): there is nothing to compile for it");
        const SpecVariant variant{kind == 0 ? SpecKind::kReads : SpecKind::kRecords, s.dev.lds.mask, kind == 0 && with_variants != 0, binned != 0 || s.dev.lds.binned != 0};
        const std::string path = out_path ? out_path : "";
        if (path.size() > 4 && path.compare(path.size() - 4, 4, ".hip") == 0) {        // the program itself (for `hipcc -I reseq_amd/csrc -g ...`: listings with source lines)
            const std::string program = spec_program(spec_literals(s.dev), variant);
            FILE *f = fopen(out_path, "wb");
            if (!f || fwrite(program.data(), 1, program.size(), f) != program.size()) throw Error(std::string("cannot write ") + out_path);
            fclose(f);
            *code_bytes = program.size();
            if (seconds) *seconds = 0.0;
            return RSQ_OK;
        }
        SpecCode c;
        std::string note;
        if (!spec_compile(s.dev, variant, arch, c, note)) throw Error(note);
        *code_bytes = c.code.size();
        if (seconds) *seconds = c.seconds;
        if (out_path && *out_path) {
            FILE *f = fopen(out_path, "wb");
            if (!f || fwrite(c.code.data(), 1, c.code.size(), f) != c.code.size()) throw Error(std::string("cannot write ") + out_path);
            fclose(f);
        }
        return RSQ_OK;
    });
    return rc;
}
int rsq_set_kernel_cache_dir(const char *path) {
    spec_cache_dir_override() = path ? path : "";
    spec_cache_dir_set() = true;
    return RSQ_OK;
}
int rsq_sim_get_fill_plan(const rsq_sim *s, uint32_t *quality_quads, uint32_t *image_tiles, uint32_t *image_bytes) {
    REQUIRE(s && quality_quads && image_tiles && image_bytes, "null argument");
    *quality_quads = effective_fill_mask(s->dev.lds.mask, s->force_fill_mode);
    *image_tiles = *quality_quads ? s->dev.lds.img_tiles : 0u;
    *image_bytes = *quality_quads ? s->dev.lds.total_words * 4u : 0u;
    return RSQ_OK;
}
int rsq_sim_get_info(const rsq_sim *s, rsq_sim_info *out) {
    REQUIRE(s && out && (s->prepared || s->pre.planned), "simulator not prepared");      // the counts are known from rsq_sim_prepare_plan on
    out->total_pairs = s->total_pairs;
    out->adapter_only_pairs = s->adapter_only_pairs;
    out->total_blocks = s->total_blocks;
    out->n_coverage_groups = s->n_groups;
    out->insert_to = s->dev.insert_to;
    out->sys_chain_passes = s->passes;
    out->bias_normalization = s->bias_normalization;
    return RSQ_OK;
}
int rsq_sim_get_thresholds(const rsq_sim *s, double *out, size_t n) {
    REQUIRE(s && out && s->prepared && n == s->thresholds.size(), "bad threshold buffer size");
    memcpy(out, s->thresholds.data(), n * 8);
    return RSQ_OK;
}
int rsq_sim_get_norm_by_len(const rsq_sim *s, double *out, size_t n) {
    REQUIRE(s && out && s->prepared && n == s->norm_by_len.size(), "bad buffer size");
    memcpy(out, s->norm_by_len.data(), n * 8);
    return RSQ_OK;
}
int rsq_sim_set_normalization(rsq_sim *s, double bias_normalization, const double *thresholds, size_t n) {
    REQUIRE(s && thresholds && s->prepared && n == s->thresholds.size(), "bad threshold buffer size");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        s->bias_normalization = bias_normalization;
        s->thresholds.assign(thresholds, thresholds + n);
        upload_normalization(*s, s->up);
        return RSQ_OK;
    });
}
static int download_sys(const rsq_sim *s, const uint16_t *src, uint8_t *dom_out, uint8_t *rate_out, uint32_t len) {
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        read_sys_track(const_cast<rsq_sim *>(s)->up, src, len, dom_out, rate_out);      // reading changes nothing of the simulator
        return RSQ_OK;
    });
}
int rsq_sim_get_sys_errors(const rsq_sim *s, int reverse_strand, uint32_t seq, uint8_t *dom_out, uint8_t *rate_out, uint32_t len) {
    REQUIRE(s && s->prepared && s->has_ref && seq < s->dev.n_seqs && len == s->seq_len[seq] && dom_out && rate_out, "bad arguments");
    REQUIRE(s->n_blocks[seq], "sequence is shorter than the longest insert length and is not simulated");
    REQUIRE(s->first_block[seq] >= s->prepared_lo && s->first_block[seq] + s->n_blocks[seq] <= s->prepared_hi,
            "the sequence's systematic errors were not (all) drawn on this simulator: the sharded pre-pass finishes the tracks of the rank's own blocks only");
    return download_sys(s, (reverse_strand ? s->sys_rev : s->sys_fwd) + s->seq_base_off[seq], dom_out, rate_out, len);
}
int rsq_sim_create_sys_error_profile(rsq_sim *s, uint64_t seed, const char *path, void *stream) {
    REQUIRE(s && path, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        DevicePrepass be(*s, stream);
        create_sys_error_profile(*s, s->up, be, seed, path);
        return RSQ_OK;
    });
}
int rsq_sim_read_sys_errors(rsq_sim *s, const char *path) {
    REQUIRE(s && path && s->prepared && s->has_ref, "rsq_sim_prepare with a reference must run before rsq_sim_read_sys_errors");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        apply_sys_error_records(*s, s->up, parse_sys_error_fastq(read_text_file(path)));
        build_variant_sys_errors(*s, s->up);                        // their error-region state follows the loaded rates
        s->prepared_lo = 1;                                         // the file holds the tracks of every sequence
        s->prepared_hi = s->total_blocks + 1;
        return RSQ_OK;
    });
}
int rsq_sim_read_methylation(rsq_sim *s, const char *path) {
    REQUIRE(s && path && s->has_ref, "a simulator with a reference is needed");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        pack_methylation(*s, s->up, read_methylation_file(path, s->ref_first_names, s->seq_len, s->num_alleles));
        return RSQ_OK;
    });
}
int rsq_sim_set_ref_bias_file(rsq_sim *s, const char *path) {
    REQUIRE(s && path, "null argument");
    s->ref_bias_file = path;
    return RSQ_OK;
}
int rsq_sim_get_ref_seq_bias(const rsq_sim *s, double *out, size_t n) {
    REQUIRE(s && out && (s->prepared || s->pre.planned) && n == s->ref_seq_bias.size(), "bad arguments");
    memcpy(out, s->ref_seq_bias.data(), n * sizeof(double));
    return RSQ_OK;
}
int rsq_sim_get_adapter_sys_errors(const rsq_sim *s, int seg, uint32_t adapter, uint8_t *dom_out, uint8_t *rate_out, uint32_t len) {
    REQUIRE(s && s->prepared && (seg == 0 || seg == 1) && adapter < s->prof.adapters[seg].n() && dom_out && rate_out, "bad arguments");
    const HostAdapters &a = s->prof.adapters[seg];
    REQUIRE(len == a.seq_ptr[adapter + 1] - a.seq_ptr[adapter], "bad adapter length");
    return download_sys(s, s->adapter_sys[seg] + a.seq_ptr[adapter], dom_out, rate_out, len);
}

// Truth alignments, as SAM text or (bam) as BAM records.  A reference with variants is refused unless the caller has chosen the coordinate system of the record
// (rsq_sim_truth_variants: reference coordinates, rsq_sam.h SamVarFormat).  What BAM cannot hold is refused as well, before anything is launched: l_read_name is a byte, so no QNAME may exceed 254 characters (the base
// identifier, the longest reference name, every number at its widest), and the bins cover 2^29 bases.
static bool truth_refusal(const rsq_sim &s, bool bam) {
    if (s.has_variants && !s.truth_variants && !s.truth_alleles) {
        g_last_error = std::string("truth alignments (") + (bam ? "BAM" : "SAM") + ") are not available for a reference with variants (rsq_ref_read_variants)";
        return true;
    }
    size_t longest_name = 0;
    uint32_t longest_seq = 0;
    for (const std::string &n : s.ref_first_names) longest_name = std::max(longest_name, n.size());
    for (const uint32_t l : s.seq_len) longest_seq = std::max(longest_seq, l);
    if (s.truth_alleles) {                                           // the records' sequences are the alleles
        if (s.truth_md) {
            g_last_error = "truth alignments in allele coordinates (rsq_sim_truth_alleles) do not carry NM:i and MD:Z: switch rsq_sim_truth_md off";
            return true;
        }
        const std::vector<int64_t> length = sim_allele_lengths(s);
        for (size_t m = 0; m < length.size(); ++m) {
            const std::string name = s.ref_first_names[m / s.num_alleles] + "_allele" + std::to_string(m % s.num_alleles);
            if (length[m] <= 0) {
                g_last_error = "truth alignments in allele coordinates (rsq_sim_truth_alleles): " + name + " has no bases";
                return true;
            }
            if (bam && length[m] > (int64_t)kBamMaxRefLen) {
                g_last_error = "truth alignments (BAM) in allele coordinates (rsq_sim_truth_alleles): " + name + " has " + std::to_string(length[m]) + " bases, more than the 2^29 that BAM's bins cover";
                return true;
            }
        }
    }
    if (!bam) return false;
    if (longest_seq > kBamMaxRefLen) {
        g_last_error = "truth alignments (BAM): a reference sequence of " + std::to_string(longest_seq) + " bases is longer than the 2^29 that BAM's bins cover";
        return true;
    }
    // "{base}{block}_{number}:{pos}:{name}:{pos}:{tile}:1337:1337" with 32-bit block and number and a 16-bit tile; "{base}0_{number}:0:Adapter:0:{tile}:1337:1337" with a 64-bit number
    // (a reference with variants, rsq_sim_truth_variants: "_allele{a}" behind the number)
    const size_t allele = s.has_variants && 1 < s.num_alleles ? 7 + digits_u32(s.num_alleles - 1) : 0;
    const size_t mapped = s.names.base_len + 10 + 1 + 10 + allele + 1 + 2 * (size_t)digits_u32(longest_seq) + 2 + longest_name + 1 + 5 + 10;
    const size_t adapter_only = s.names.base_len + 2 + 20 + 12 + 1 + 5 + 10;
    if (std::max(mapped, adapter_only) > kBamMaxQname) {
        g_last_error = "truth alignments (BAM): a read name could take " + std::to_string(std::max(mapped, adapter_only)) + " characters, BAM holds 254 (shorten the reference names or the base identifier)";
        return true;
    }
    return false;
}
int rsq_sim_truth_variants(rsq_sim *s, int on) {
    REQUIRE(s, "null argument");
    REQUIRE(!on || !s->truth_alleles, "rsq_sim_truth_variants: rsq_sim_truth_alleles has chosen allele coordinates for the truth alignments; a record has one coordinate system (switch that off first)");
    s->truth_variants = on != 0;
    return RSQ_OK;
}
int rsq_sim_truth_alleles(rsq_sim *s, int on) {
    REQUIRE(s, "null argument");
    if (!on) {
        s->truth_alleles = false;
        return RSQ_OK;
    }
    REQUIRE(!s->truth_variants, "rsq_sim_truth_alleles: rsq_sim_truth_variants has chosen reference coordinates for the truth alignments; a record has one coordinate system (switch that off first)");
    REQUIRE(s->has_ref && s->has_variants, "rsq_sim_truth_alleles needs a reference with variants (rsq_ref_read_variants): without them there are no alleles");
    if (s->depth.open) {
        g_last_error = "rsq_sim_truth_alleles cannot be switched on while a depth run is open (rsq_sim_depth_begin): depth is in reference coordinates";
        return RSQ_ESTATE;
    }
    if (s->pileup.open) {
        g_last_error = "rsq_sim_truth_alleles cannot be switched on while a pileup run is open (rsq_sim_pileup_begin): the pileup is in reference coordinates";
        return RSQ_ESTATE;
    }
    if (s->bam_sorted.open) {
        g_last_error = "rsq_sim_truth_alleles cannot change inside a sorted run (between rsq_sim_bam_sorted_begin and rsq_sim_bam_sorted_flush)";
        return RSQ_ESTATE;
    }
    s->truth_alleles = true;
    return RSQ_OK;
}
// NM:i and MD:Z behind every mapped truth record's tags (rsq_md.h).  The writer's image is sized by the longest pair of the call before: the first call with the
// tags gets room for them.
int rsq_sim_truth_md(rsq_sim *s, int on) {
    REQUIRE(s, "null argument");
    const bool want = on != 0;
    if (want == s->truth_md) return RSQ_OK;
    if (s->bam_sorted.open) {
        g_last_error = "rsq_sim_truth_md cannot change inside a sorted run (between rsq_sim_bam_sorted_begin and rsq_sim_bam_sorted_flush)";
        return RSQ_ESTATE;
    }
    s->truth_md = want;
    if (want) {
        s->sam_pair_bytes += 64;
        s->bam_pair_bytes += 48;
    }
    return RSQ_OK;
}
// ---- truth depth (rsq_depth.h; include/reseq_amd.h rsq_sim_depth_*)
#define REQUIRE_STATE(cond, msg)    \
    do {                            \
        if (!(cond)) {              \
            g_last_error = msg;     \
            return RSQ_ESTATE;      \
        }                           \
    } while (0)
int rsq_sim_depth_begin(rsq_sim *s) {
    REQUIRE(s, "null argument");
    REQUIRE_STATE(s->prepared && s->has_ref, "rsq_sim_prepare with a reference must run before rsq_sim_depth_begin");
    REQUIRE_STATE(!s->depth.open, "rsq_sim_depth_begin: a depth run is open already (rsq_sim_depth_end ends it)");
    REQUIRE(!s->truth_alleles, "rsq_sim_depth_begin: depth is in reference coordinates; rsq_sim_truth_alleles has chosen allele coordinates (switch that off first)");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        rsq_sim::Depth &d = s->depth;
        d.words = depth_words(s->total_ref_size, s->dev.n_seqs);
        d.diff.reserve(d.words * 4u);
        d.bad.reserve(8);
        HIP_CHECK(hipMemset(d.diff.as<void>(), 0, d.words * 4u));
        HIP_CHECK(hipMemset(d.bad.as<void>(), 0, 8));
        d.open = true;
        d.finished = false;
        d.bg_seq = 0xFFFFFFFFu;
        return (int)RSQ_OK;
    });
}
int rsq_sim_depth_finish(rsq_sim *s, void *stream) {
    REQUIRE(s, "null argument");
    REQUIRE_STATE(s->depth.open && !s->depth.finished, "rsq_sim_depth_finish: no depth run is open, or it is finished already");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        rsq_sim::Depth &d = s->depth;
        const hipStream_t st = (hipStream_t)stream;
        const uint32_t tiles = (uint32_t)(d.words / kDepthTile);
        reset_call_timers(*s);
        d.tile_sums.reserve((size_t)tiles * 4u + 16u);
        s->timers["depth_scan"].start(st);
        hipLaunchKernelGGL(k_depth_tile_sums, dim3(tiles), dim3(kDepthBlock), 0, st, d.diff.as<const uint32_t>(), d.tile_sums.as<uint32_t>());
        hipLaunchKernelGGL(k_depth_tiles, dim3(1), dim3(kDepthTilesBlock), 0, st, d.tile_sums.as<uint32_t>(), tiles);
        hipLaunchKernelGGL(k_depth_apply, dim3(tiles), dim3(kDepthBlock), 0, st, d.diff.as<uint32_t>(), d.tile_sums.as<const uint32_t>());
        s->timers["depth_scan"].stop(st);
        HIP_CHECK(hipGetLastError());
        uint32_t bad = 0;
        HIP_CHECK(hipMemcpyAsync(&bad, d.bad.as<uint32_t>(), 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        d.finished = true;
        if (bad) {
            g_last_error = "truth depth: " + std::to_string(bad) + " alignment elements lay outside their sequence and were left out";
            return (int)RSQ_EINVAL;
        }
        return (int)RSQ_OK;
    });
}
static int depth_window(const rsq_sim &s, const char *call, uint32_t seq, uint64_t lo, uint64_t hi) {
    if (!s.depth.open || !s.depth.finished) {
        g_last_error = std::string(call) + ": rsq_sim_depth_finish must have run (the array holds differences until then)";
        return RSQ_ESTATE;
    }
    if (seq >= s.seq_len.size() || lo > hi || hi > s.seq_len[seq]) {
        g_last_error = std::string(call) + ": no such sequence, or a window that is not inside it";
        return RSQ_EINVAL;
    }
    return RSQ_OK;
}
int rsq_sim_depth_counts(rsq_sim *s, uint32_t seq, uint64_t lo, uint64_t hi, uint32_t *depth_dev, void *stream) {
    REQUIRE(s, "null argument");
    if (const int rc = depth_window(*s, "rsq_sim_depth_counts", seq, lo, hi)) return rc;
    REQUIRE(depth_dev || lo == hi, "null argument");
    if (lo == hi) return RSQ_OK;
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        const hipStream_t st = (hipStream_t)stream;
        HIP_CHECK(hipMemcpyAsync(depth_dev, s->depth.diff.as<uint32_t>() + s->seq_base_off[seq] + seq + lo, (hi - lo) * 4u, hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return (int)RSQ_OK;
    });
}
int rsq_sim_depth_bedgraph(rsq_sim *s, uint32_t seq, uint64_t lo, uint64_t hi, char *dst_dev, size_t cap, size_t *len, uint64_t *n_lines, void *stream) {
    REQUIRE(s && len && n_lines, "null argument");
    *len = 0;
    *n_lines = 0;
    if (const int rc = depth_window(*s, "rsq_sim_depth_bedgraph", seq, lo, hi)) return rc;
    rsq_sim::Depth &d = s->depth;
    REQUIRE_STATE(lo == 0 || (seq == d.bg_seq && lo == d.bg_next),
                  "rsq_sim_depth_bedgraph: the pieces of a sequence are contiguous and rising from 0 -- this one does not continue the piece before it");
    const uint32_t carry = lo ? d.bg_carry : 0u;                      // where the run that is open at lo began
    const uint64_t n = hi - lo;
    auto done = [&](uint32_t new_carry) {
        d.bg_seq = seq;
        d.bg_next = hi;
        d.bg_carry = new_carry;
        return (int)RSQ_OK;
    };
    if (!n) return done(carry);
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        const hipStream_t st = (hipStream_t)stream;
        reset_call_timers(*s);
        s->cur = &s->ws[0];                                             // (the scans' scratch)
        const uint32_t *depths = d.diff.as<const uint32_t>() + s->seq_base_off[seq] + seq;
        const uint32_t name_len = (uint32_t)s->ref_first_names[seq].size();
        d.flags.reserve(n * 4u + 16u);
        d.rank.reserve((n + 1u) * 8u);
        s->timers["depth_lines"].start(st);
        hipLaunchKernelGGL(k_depth_ends, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, st, depths, s->seq_len[seq], (uint32_t)lo, n, d.flags.as<uint32_t>());
        exclusive_scan(*s, d.flags.as<uint32_t>(), n, d.rank.as<uint64_t>(), st);
        s->timers["depth_lines"].stop(st);
        uint64_t lines = 0;
        HIP_CHECK(hipMemcpyAsync(&lines, d.rank.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (!lines) return done(carry);                                  // one run covers the piece and goes on
        d.ends.reserve(lines * 4u + 16u);
        d.sizes.reserve(lines * 4u + 16u);
        d.offsets.reserve((lines + 1u) * 8u);
        s->timers["depth_lines"].start(st);
        hipLaunchKernelGGL(k_depth_run_ends, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, st, d.flags.as<const uint32_t>(), d.rank.as<const uint64_t>(), (uint32_t)lo, n, d.ends.as<uint32_t>());
        hipLaunchKernelGGL(k_depth_line_sizes, dim3((uint32_t)cdiv(lines, 256)), dim3(256), 0, st, depths, d.ends.as<const uint32_t>(), lines, carry, name_len, d.sizes.as<uint32_t>());
        exclusive_scan(*s, d.sizes.as<uint32_t>(), lines, d.offsets.as<uint64_t>(), st);
        s->timers["depth_lines"].stop(st);
        HIP_CHECK(hipGetLastError());
        uint64_t bytes = 0;
        uint32_t last_end = 0;
        HIP_CHECK(hipMemcpyAsync(&bytes, d.offsets.as<uint64_t>() + lines, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(&last_end, d.ends.as<uint32_t>() + (lines - 1u), 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        *len = bytes;
        *n_lines = lines;
        if (bytes > cap || !dst_dev) {                                   // nothing written, the carried start unchanged: the call can be repeated
            g_last_error = "bedGraph buffer too small: need " + std::to_string(bytes) + " bytes";
            return (int)RSQ_ENOSPC;
        }
        const uint32_t lds = depth_lds_bytes(name_len);
        s->timers["depth_text"].start(st);
        hipLaunchKernelGGL(k_depth_text, dim3((uint32_t)cdiv(lines, kDepthLines)), dim3(64), lds, st, s->names, seq, depths, d.ends.as<const uint32_t>(), carry, lines,
                           d.offsets.as<const uint64_t>(), dst_dev, lds);
        s->timers["depth_text"].stop(st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
        return done(last_end);
    });
}
int rsq_sim_depth_end(rsq_sim *s) {
    REQUIRE(s, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        rsq_sim::Depth &d = s->depth;
        for (DevBuf *b : {&d.diff, &d.bad, &d.tile_sums, &d.flags, &d.rank, &d.ends, &d.sizes, &d.offsets}) b->release();
        d.open = d.finished = false;
        d.words = 0;
        return (int)RSQ_OK;
    });
}

// ---- simulation report (rsq_stats.h; include/reseq_amd.h rsq_sim_stats_*)
static_assert(RSQ_STATS_PAIRS == kStPairs && RSQ_STATS_STRAND == kStStrand && RSQ_STATS_TILE == kStTile && RSQ_STATS_FRAGMENT_LENGTH == kStFragmentLength &&
                  RSQ_STATS_READ_LENGTH == kStReadLength && RSQ_STATS_ERRORS_PER_READ == kStErrorsPerRead && RSQ_STATS_BASE_QUALITY == kStBaseQuality &&
                  RSQ_STATS_BASE_CALL == kStBaseCall && RSQ_STATS_INSERTION == kStInsertion && RSQ_STATS_DELETION == kStDeletion && RSQ_STATS_ADAPTER == kStAdapter &&
                  RSQ_STATS_TAIL == kStTail && RSQ_STATS_MISMATCH == kStMismatch && RSQ_STATS_BAD == kStBad && RSQ_STATS_COUNT == kStTables,
              "the ABI's table ids are rsq_stats.h's");
// Q: one more than the largest quality value the profile's quality tables can draw (their outcome values)
static uint32_t stats_quality_values(const rsq_sim &s) {
    uint32_t top = 0;
    for (const HostTable &t : s.prof.quality)
        for (const uint32_t v : t.par0) top = std::max(top, v);
    return top + 1u;
}
int rsq_sim_stats_begin(rsq_sim *s) {
    REQUIRE(s, "null argument");
    REQUIRE_STATE(s->prepared && s->has_ref, "rsq_sim_prepare with a reference must run before rsq_sim_stats_begin");
    REQUIRE_STATE(!s->stats.open, "rsq_sim_stats_begin: a stats run is open already (rsq_sim_stats_end ends it)");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        rsq_sim::Stats &t = s->stats;
        const uint32_t Q = stats_quality_values(*s);
        if (Q > 256u) throw Error("the simulation report: quality values beyond 255 do not fit a character");
        t.lay = stats_layout(s->dev.read_lengths[0].to, s->dev.read_lengths[1].to, s->dev.insert_to, Q, s->dev.n_tiles, s->dev.phred_offset);
        if ((uint64_t)t.lay.image_words * 4u > kStatsMatesLds) throw Error("the simulation report: the per-cycle tables of reads this long do not fit the LDS");
        t.counts.reserve((size_t)t.lay.words * 8u + 16u);
        HIP_CHECK(hipMemset(t.counts.as<void>(), 0, (size_t)t.lay.words * 8u));
        t.open = true;
        return (int)RSQ_OK;
    });
}
int rsq_sim_stats_layout(const rsq_sim *s, rsq_stats_layout *layout) {
    REQUIRE(s && layout, "null argument");
    REQUIRE_STATE(s->stats.open, "rsq_sim_stats_layout: no stats run is open (rsq_sim_stats_begin)");
    const StatsLayout &y = s->stats.lay;
    *layout = rsq_stats_layout{};
    layout->words = y.words;
    layout->read_length[0] = y.len[0];
    layout->read_length[1] = y.len[1];
    layout->insert_to = y.F;
    layout->n_quality = y.Q;
    layout->n_tiles = y.T;
    layout->phred_offset = y.phred;
    for (uint32_t t = 0; t < kStTables; ++t) layout->table[t] = rsq_stats_table{y.off[t], y.segments(t), t == kStBaseQuality || t == kStBaseCall ? 2u : 1u, {y.dim0(t), y.dim1(t)}};
    return RSQ_OK;
}
int rsq_sim_stats_counts(rsq_sim *s, uint64_t *host, size_t cap_words, void *stream) {
    REQUIRE(s && host, "null argument");
    REQUIRE_STATE(s->stats.open, "rsq_sim_stats_counts: no stats run is open (rsq_sim_stats_begin)");
    const StatsLayout &y = s->stats.lay;
    if (cap_words < y.words) {
        g_last_error = "stats buffer too small: need " + std::to_string(y.words) + " words";
        return RSQ_ENOSPC;
    }
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        const hipStream_t st = (hipStream_t)stream;
        HIP_CHECK(hipMemcpyAsync(host, s->stats.counts.as<uint64_t>(), (size_t)y.words * 8u, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        g_last_warning.clear();
        if (host[y.off[kStBad]])
            g_last_warning = "simulation report: " + std::to_string(host[y.off[kStBad]]) + " values were out of range (a quality, a base code, or a CIGAR element outside its read) and are counted under RSQ_STATS_BAD only";
        return (int)RSQ_OK;
    });
}
int rsq_sim_stats_end(rsq_sim *s) {
    REQUIRE(s, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        s->stats.counts.release();
        s->stats.open = false;
        return (int)RSQ_OK;
    });
}

// ---- truth pileup (rsq_pileup.h; include/reseq_amd.h rsq_sim_pileup_*)
static_assert(kPileupPlanes == RSQ_PILEUP_COLUMNS, "the ABI's row is rsq_pileup.h's");
int rsq_sim_pileup_begin(rsq_sim *s, uint32_t flags) {
    REQUIRE(s, "null argument");
    REQUIRE_STATE(s->prepared && s->has_ref, "rsq_sim_prepare with a reference must run before rsq_sim_pileup_begin");
    REQUIRE_STATE(!s->pileup.open, "rsq_sim_pileup_begin: a pileup run is open already (rsq_sim_pileup_end ends it)");
    REQUIRE(!s->truth_alleles, "rsq_sim_pileup_begin: the pileup is in reference coordinates; rsq_sim_truth_alleles has chosen allele coordinates (switch that off first)");
    REQUIRE(!(flags & ~RSQ_PILEUP_STRANDS), "rsq_sim_pileup_begin: unknown flags");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        rsq_sim::Pileup &u = s->pileup;
        u.sets = flags & RSQ_PILEUP_STRANDS ? 2u : 1u;
        u.words = depth_words(s->total_ref_size, s->dev.n_seqs);
        const uint64_t bytes = (uint64_t)u.sets * kPileupPlanes * u.words * 4u;
        try {
            u.planes.reserve(bytes);
        } catch (const std::exception &e) {
            u.words = 0;
            throw Error("rsq_sim_pileup_begin: the run needs " + std::to_string(bytes) + " bytes of device memory (" + std::to_string(4u * kPileupPlanes * u.sets) +
                        " per reference base): " + e.what());
        }
        u.bad.reserve(8);
        HIP_CHECK(hipMemset(u.planes.as<void>(), 0, bytes));
        HIP_CHECK(hipMemset(u.bad.as<void>(), 0, 8));
        u.open = true;
        u.finished = false;
        return (int)RSQ_OK;
    });
}
int rsq_sim_pileup_finish(rsq_sim *s, void *stream) {
    REQUIRE(s, "null argument");
    REQUIRE_STATE(s->pileup.open && !s->pileup.finished, "rsq_sim_pileup_finish: no pileup run is open, or it is finished already");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        rsq_sim::Pileup &u = s->pileup;
        const hipStream_t st = (hipStream_t)stream;
        const uint32_t tiles = (uint32_t)(u.words / kDepthTile);
        reset_call_timers(*s);
        u.tile_sums.reserve((size_t)tiles * 4u + 16u);
        for (uint32_t set = 0; set < u.sets; ++set) {                   // plane 0 of every strand set: differences -> depths
            uint32_t *plane = u.planes.as<uint32_t>() + (uint64_t)set * kPileupPlanes * u.words;
            s->timers["pileup_scan"].start(st);
            hipLaunchKernelGGL(k_depth_tile_sums, dim3(tiles), dim3(kDepthBlock), 0, st, (const uint32_t *)plane, u.tile_sums.as<uint32_t>());
            hipLaunchKernelGGL(k_depth_tiles, dim3(1), dim3(kDepthTilesBlock), 0, st, u.tile_sums.as<uint32_t>(), tiles);
            hipLaunchKernelGGL(k_depth_apply, dim3(tiles), dim3(kDepthBlock), 0, st, plane, u.tile_sums.as<const uint32_t>());
            s->timers["pileup_scan"].stop(st);
        }
        HIP_CHECK(hipGetLastError());
        uint32_t bad = 0;
        HIP_CHECK(hipMemcpyAsync(&bad, u.bad.as<uint32_t>(), 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        u.finished = true;
        if (bad) {
            g_last_error = "truth pileup: " + std::to_string(bad) + " alignment elements lay outside their sequence and were left out";
            return (int)RSQ_EINVAL;
        }
        return (int)RSQ_OK;
    });
}
static int pileup_window(const rsq_sim &s, const char *call, uint32_t seq, uint64_t lo, uint64_t hi) {
    if (!s.pileup.open || !s.pileup.finished) {
        g_last_error = std::string(call) + ": rsq_sim_pileup_finish must have run (plane 0 holds differences until then)";
        return RSQ_ESTATE;
    }
    if (seq >= s.seq_len.size() || lo > hi || hi > s.seq_len[seq]) {
        g_last_error = std::string(call) + ": no such sequence, or a window that is not inside it";
        return RSQ_EINVAL;
    }
    return RSQ_OK;
}
int rsq_sim_pileup_counts(rsq_sim *s, uint32_t seq, uint64_t lo, uint64_t hi, uint32_t *rows_dev, void *stream) {
    REQUIRE(s, "null argument");
    if (const int rc = pileup_window(*s, "rsq_sim_pileup_counts", seq, lo, hi)) return rc;
    REQUIRE(rows_dev || lo == hi, "null argument");
    if (lo == hi) return RSQ_OK;
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        const hipStream_t st = (hipStream_t)stream;
        const rsq_sim::Pileup &u = s->pileup;
        const uint64_t n = hi - lo;
        reset_call_timers(*s);
        s->timers["pileup_rows"].start(st);
        hipLaunchKernelGGL(k_pileup_rows, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, st, u.planes.as<const uint32_t>() + s->seq_base_off[seq] + seq, u.words, u.sets,
                           s->dev.ref_words + s->seq_word_off[seq], (uint32_t)lo, n, rows_dev);
        s->timers["pileup_rows"].stop(st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
        return (int)RSQ_OK;
    });
}
int rsq_sim_pileup_text(rsq_sim *s, uint32_t seq, uint64_t lo, uint64_t hi, uint32_t flags, char *dst_dev, size_t cap, size_t *len, uint64_t *n_lines, void *stream) {
    REQUIRE(s && len && n_lines, "null argument");
    *len = 0;
    *n_lines = 0;
    if (const int rc = pileup_window(*s, "rsq_sim_pileup_text", seq, lo, hi)) return rc;
    REQUIRE(!(flags & ~RSQ_PILEUP_ALL), "rsq_sim_pileup_text: unknown flags");
    const uint64_t n = hi - lo;
    if (!n) return RSQ_OK;
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        const hipStream_t st = (hipStream_t)stream;
        rsq_sim::Pileup &u = s->pileup;
        reset_call_timers(*s);
        s->cur = &s->ws[0];                                             // (the scan's scratch)
        const uint32_t *at = u.planes.as<const uint32_t>() + s->seq_base_off[seq] + seq;
        const uint64_t *ref_words = s->dev.ref_words + s->seq_word_off[seq];
        const uint32_t name_len = (uint32_t)s->ref_first_names[seq].size();
        u.flags.reserve(n * 4u + 16u);
        u.sizes.reserve(n * 4u + 16u);
        u.rank.reserve((n + 1u) * 8u);
        u.at_pos.reserve((n + 1u) * 8u);
        s->timers["pileup_lines"].start(st);
        hipLaunchKernelGGL(k_pileup_lines, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, st, at, u.words, u.sets, ref_words, (uint32_t)lo, n, flags & RSQ_PILEUP_ALL ? 1u : 0u, name_len,
                           u.flags.as<uint32_t>(), u.sizes.as<uint32_t>());
        exclusive_scans(*s, ScanArrays{{u.flags.as<const uint32_t>(), u.sizes.as<const uint32_t>()}, {u.rank.as<uint64_t>(), u.at_pos.as<uint64_t>()}, {nullptr, nullptr}, {nullptr, nullptr}}, 2, n, st);
        s->timers["pileup_lines"].stop(st);
        uint64_t lines = 0, bytes = 0;
        HIP_CHECK(hipMemcpyAsync(&lines, u.rank.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(&bytes, u.at_pos.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        *len = bytes;
        *n_lines = lines;
        if (!lines) return (int)RSQ_OK;
        if (bytes > cap || !dst_dev) {                                   // nothing written: the call can be repeated
            g_last_error = "pileup text buffer too small: need " + std::to_string(bytes) + " bytes";
            return (int)RSQ_ENOSPC;
        }
        u.line_pos.reserve(lines * 4u + 16u);
        u.offsets.reserve((lines + 1u) * 8u);
        s->timers["pileup_lines"].start(st);
        hipLaunchKernelGGL(k_pileup_place, dim3((uint32_t)cdiv(n + 1u, 256)), dim3(256), 0, st, u.flags.as<const uint32_t>(), u.rank.as<const uint64_t>(), u.at_pos.as<const uint64_t>(),
                           (uint32_t)lo, n, u.line_pos.as<uint32_t>(), u.offsets.as<uint64_t>());
        s->timers["pileup_lines"].stop(st);
        const uint32_t lds = pileup_lds_bytes(name_len, u.sets);
        s->timers["pileup_text"].start(st);
        hipLaunchKernelGGL(k_pileup_text, dim3((uint32_t)cdiv(lines, kPileupLines)), dim3(64), lds, st, s->names, seq, at, u.words, u.sets, ref_words, u.line_pos.as<const uint32_t>(), lines,
                           u.offsets.as<const uint64_t>(), dst_dev, lds);
        s->timers["pileup_text"].stop(st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
        return (int)RSQ_OK;
    });
}
int rsq_sim_pileup_end(rsq_sim *s) {
    REQUIRE(s, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        rsq_sim::Pileup &u = s->pileup;
        for (DevBuf *b : {&u.planes, &u.bad, &u.tile_sums, &u.flags, &u.sizes, &u.rank, &u.at_pos, &u.line_pos, &u.offsets}) b->release();
        u.open = u.finished = false;
        u.words = 0;
        return (int)RSQ_OK;
    });
}

// the entry points of the pairs calls
static int pairs_call(rsq_sim *s, const PairsCall &call, uint32_t block_lo, uint32_t block_hi, uint64_t *n_pairs) {
    REQUIRE(s && call.r1.len && call.r2.len && (call.truth.len || !call.has_truth()) && n_pairs, "null argument");
    if (call.has_truth() && truth_refusal(*s, call.bam())) return RSQ_EINVAL;
    if (depth_refusal(*s)) return RSQ_ESTATE;
    return guard([&] {
        const int rc = sim_pairs(*s, call, block_lo, block_hi, n_pairs);
        if (rc == RSQ_OK && s->keeps_part()) runs_take(*s, call.st);
        return rc;
    });
}
int rsq_sim_pairs(rsq_sim *s, uint32_t block_lo, uint32_t block_hi, char *r1_dev, size_t r1_cap, size_t *r1_len, char *r2_dev, size_t r2_cap, size_t *r2_len,
                  uint64_t *n_pairs, rsq_fragment *frags_dev, size_t frags_cap, void *stream) {
    return pairs_call(s, PairsCall{{r1_dev, r1_cap, r1_len}, {r2_dev, r2_cap, r2_len}, (hipStream_t)stream, {}, PairsCall::kNoTruth, frags_dev, frags_cap}, block_lo, block_hi, n_pairs);
}
int rsq_sim_pairs_sam(rsq_sim *s, uint32_t block_lo, uint32_t block_hi, char *r1_dev, size_t r1_cap, size_t *r1_len, char *r2_dev, size_t r2_cap, size_t *r2_len, char *sam_dev,
                      size_t sam_cap, size_t *sam_len, uint64_t *n_pairs, rsq_fragment *frags_dev, size_t frags_cap, void *stream) {
    return pairs_call(s, PairsCall{{r1_dev, r1_cap, r1_len}, {r2_dev, r2_cap, r2_len}, (hipStream_t)stream, {sam_dev, sam_cap, sam_len}, PairsCall::kSam, frags_dev, frags_cap}, block_lo, block_hi, n_pairs);
}
int rsq_sim_pairs_bam(rsq_sim *s, uint32_t block_lo, uint32_t block_hi, char *r1_dev, size_t r1_cap, size_t *r1_len, char *r2_dev, size_t r2_cap, size_t *r2_len, char *bam_dev,
                      size_t bam_cap, size_t *bam_len, uint64_t *n_pairs, rsq_fragment *frags_dev, size_t frags_cap, void *stream) {
    return pairs_call(s, PairsCall{{r1_dev, r1_cap, r1_len}, {r2_dev, r2_cap, r2_len}, (hipStream_t)stream, {bam_dev, bam_cap, bam_len}, PairsCall::kBam, frags_dev, frags_cap}, block_lo, block_hi, n_pairs);
}

// ---- the truth BAM sorted by coordinate (rsq_bamsort.h; include/reseq_amd.h rsq_sim_bam_sorted_*)
int rsq_sim_bam_sorted_begin(rsq_sim *s, uint64_t first_record_offset) {
    REQUIRE(s, "null argument");
    if (!s->prepared || !s->has_ref) {
        g_last_error = "rsq_sim_prepare with a reference must run before rsq_sim_bam_sorted_begin";
        return RSQ_ESTATE;
    }
    REQUIRE(!s->truth_alleles, "rsq_sim_bam_sorted_begin: a sorted run is not available in allele coordinates (rsq_sim_truth_alleles): the records of one sequence's alleles arrive "
                               "interleaved, so no record could be handed out before the sequence ends");
    if (truth_refusal(*s, true)) return RSQ_EINVAL;
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        rsq_sim::BamSorted &b = s->bam_sorted;
        uint32_t longest = 0;
        for (const uint32_t l : s->seq_len) longest = std::max(longest, l);
        b.active = true;
        b.open = true;
        b.stream_at = first_record_offset;
        b.next_block = 0;
        b.prev_cut = 0;
        b.plan = bam_sort_plan(s->dev.n_seqs, longest);
        b.cur = 0;
        b.n_held = b.held_bytes = b.call_pairs = 0;
        b.index.begin(s->seq_len);
        b.window_first.upload(b.index.window_first);
        b.windows.reserve(b.index.windows.size() * 8u + 8u);
        HIP_CHECK(hipMemset(b.windows.as<void>(), 0xFF, b.index.windows.size() * 8u));
        b.out_of_order.reserve(8);
        b.result.reserve(64);
        return (int)RSQ_OK;
    });
}
int rsq_sim_pairs_bam_sorted(rsq_sim *s, uint32_t block_lo, uint32_t block_hi, char *r1_dev, size_t r1_cap, size_t *r1_len, char *r2_dev, size_t r2_cap, size_t *r2_len, char *bam_dev,
                             size_t bam_cap, size_t *bam_len, uint64_t *n_pairs, uint64_t *n_records, rsq_fragment *frags_dev, size_t frags_cap, void *stream) {
    REQUIRE(s && r1_len && r2_len && bam_len && n_pairs && n_records, "null argument");
    if (truth_refusal(*s, true)) return RSQ_EINVAL;
    if (depth_refusal(*s)) return RSQ_ESTATE;
    rsq_sim::BamSorted &b = s->bam_sorted;
    *r1_len = *r2_len = *bam_len = 0;
    *n_pairs = *n_records = 0;
    if (!b.active) {
        g_last_error = "rsq_sim_bam_sorted_begin must run before rsq_sim_pairs_bam_sorted";
        return RSQ_ESTATE;
    }
    if (const int rc = check_block_range(*s, block_lo, block_hi)) return rc;
    if (b.next_block && block_lo != b.next_block) {
        g_last_error = "sorted BAM: the calls of a run are contiguous and rising -- this one must begin at block " + std::to_string(b.next_block) + ", not at " + std::to_string(block_lo);
        return RSQ_ESTATE;
    }
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        const hipStream_t st = (hipStream_t)stream;
        reset_call_timers(*s);
        b.call_pairs = 0;
        b.call_parts = block_hi > block_lo ? pairs_parts(*s, block_hi - block_lo) : 1u;
        HIP_CHECK(hipMemsetAsync(b.out_of_order.as<uint32_t>(), 0, 4, st));
        HIP_CHECK(hipStreamSynchronize(st));                         // (a pipelined call's parts run on other streams)
        const PairsCall call{{r1_dev, r1_cap, r1_len}, {r2_dev, r2_cap, r2_len}, st, {bam_dev, bam_cap, bam_len}, PairsCall::kSortedBam, frags_dev, frags_cap};
        const int rc = sim_pairs(*s, call, block_lo, block_hi, n_pairs);
        if (rc != RSQ_OK && rc != RSQ_ENOSPC) return rc;
        if (rc == RSQ_ENOSPC && !*n_pairs) return rc;                // the fragment buffer was too small: the call ended in the middle of its parts, no size is known yet
        const uint64_t cut = bam_cut_key(block_hi, s->total_blocks, s->dev.n_seqs, s->block_seq.data(), s->first_block.data(), kBlockSize);
        const int end = sorted_finish(*s, call, rc, cut, block_hi);
        *n_records = b.call_records;
        if (end == RSQ_OK && s->keeps_part()) runs_take(*s, st);        // (the run's state has moved on: the call will not be repeated)
        return end;
    });
}
int rsq_sim_bam_sorted_flush(rsq_sim *s, char *bam_dev, size_t bam_cap, size_t *bam_len, uint64_t *n_mapped, uint64_t *n_unmapped, void *stream) {
    REQUIRE(s && bam_len && n_mapped && n_unmapped, "null argument");
    rsq_sim::BamSorted &b = s->bam_sorted;
    *bam_len = 0;
    *n_mapped = *n_unmapped = 0;
    if (!b.active) {
        g_last_error = "rsq_sim_bam_sorted_begin must run before rsq_sim_bam_sorted_flush";
        return RSQ_ESTATE;
    }
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        const hipStream_t st = (hipStream_t)stream;
        reset_call_timers(*s);
        b.call_pairs = 0;
        HIP_CHECK(hipMemsetAsync(b.out_of_order.as<uint32_t>(), 0, 4, st));
        const PairsCall call{{}, {}, st, {bam_dev, bam_cap, bam_len}, PairsCall::kSortedBam};        // a sorted call without parts or FASTQ outputs
        const int rc = sorted_finish(*s, call, RSQ_OK, kBamCutAll, b.next_block);
        *n_mapped = b.call_mapped;
        *n_unmapped = b.call_records - b.call_mapped;
        if (rc == RSQ_OK) b.open = false;
        return rc;
    });
}
int rsq_sim_bam_sorted_index(rsq_sim *s, const uint64_t *block_u, const uint64_t *block_c, size_t n_blocks, uint64_t n_no_coor, char *out, size_t cap, size_t *need) {
    REQUIRE(s && need && block_u && block_c && n_blocks, "null argument");
    rsq_sim::BamSorted &b = s->bam_sorted;
    if (!b.active) {
        g_last_error = "rsq_sim_bam_sorted_begin must run before rsq_sim_bam_sorted_index";
        return RSQ_ESTATE;
    }
    REQUIRE(block_u[0] == 0 && std::is_sorted(block_u, block_u + n_blocks) && std::is_sorted(block_c, block_c + n_blocks), "the block table begins at offset 0 and rises");
    for (size_t k = 0; k + 1 < n_blocks; ++k) REQUIRE(block_u[k + 1] - block_u[k] <= 65536, "a BGZF block holds at most 64 KiB: the block table is not this file's");
    REQUIRE(block_u[n_blocks - 1] >= b.stream_at, "the block table ends in front of the run's last record: its last entry is the end-of-file member");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        HIP_CHECK(hipMemcpy(b.index.windows.data(), b.windows.as<void>(), b.index.windows.size() * 8u, hipMemcpyDeviceToHost));
        const std::string bytes = bam_bai_bytes(b.index, block_u, block_c, n_blocks, n_no_coor);
        *need = bytes.size();
        if (!out || cap < bytes.size()) {
            g_last_error = "index buffer too small: need " + std::to_string(bytes.size()) + " bytes";
            return (int)RSQ_ENOSPC;
        }
        memcpy(out, bytes.data(), bytes.size());
        return (int)RSQ_OK;
    });
}

// ---- a rank's share, generated once and kept (include/reseq_amd.h rsq_sim_job_*)
constexpr size_t kJobChunkBytes = (size_t)2 << 30, kJobSliceBytes = (size_t)32 << 20;
int rsq_sim_job_generate(rsq_sim *s, uint32_t block_lo, uint32_t block_hi, uint32_t batch_blocks, uint64_t *n_pairs, uint64_t *r1_bytes, uint64_t *r2_bytes, void *stream) {
    REQUIRE(s && n_pairs && r1_bytes && r2_bytes, "null argument");
    *n_pairs = *r1_bytes = *r2_bytes = 0;
    if (depth_refuses_job(*s, "rsq_sim_job_generate")) return RSQ_ESTATE;
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        rsq_sim::JobText &job = s->job;
        job.clear();
        if (const int rc = check_block_range(*s, block_lo, block_hi)) return rc;      // before anything is sized from the range (block_hi - block_lo is unsigned)
        const size_t chunk_bytes = s->opt.job_chunk_bytes > 0 ? (size_t)s->opt.job_chunk_bytes : kJobChunkBytes;
        // about 12 M pairs per call, at least 2000 blocks: a call is a round of launches with a tail behind each, and a longer call shares it among more pairs --
        // the Drosophila-sized job runs at 154 M pairs/s in calls of 2.4 M pairs and at 179 M in one call of 14.5 M, the human-sized one at a tenth of its size
        // at 119 and 139 M (profiles/r05_i_other_configs.json); 12 M pairs take about 20 GB of the 288 for workspace and text
        if (!batch_blocks)
            batch_blocks = (uint32_t)std::min(400000.0, std::max(2000.0, 12e6 * (double)s->total_blocks / (double)std::max<uint64_t>(1, s->total_pairs)));
        // bytes per block a call is given room for: the largest seen so far; before the first call 400 bytes per read (2 x 150 characters, an id of 60 to 90) at the
        // job's pair density
        const double prior = 400.0 * (double)s->total_pairs / (double)std::max<uint32_t>(1, s->total_blocks);
        double per_block[2] = {prior, prior};
        auto room = [&](int f) { return job.chunks[f].empty() ? (size_t)0 : job.chunks[f].back()->bytes() - job.used[f].back(); };
        // arrays: the whole range in one when memory allows (option job_chunk_bytes unset), else pieces of 2 GiB
        size_t free_bytes = 0, total_bytes = 0;
        HIP_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
        const size_t whole = (size_t)(prior * (double)(block_hi - block_lo) * 1.1) + ((size_t)64 << 20);
        const size_t first_chunk = s->opt.job_chunk_bytes > 0 ? chunk_bytes : (2 * whole + ((size_t)8 << 30) < free_bytes ? std::max(whole, chunk_bytes) : chunk_bytes);
        auto new_chunk = [&](int f, size_t at_least) {
            job.chunks[f].emplace_back(new DevBuf());
            job.chunks[f].back()->reserve(std::max(job.chunks[f].size() == 1 ? first_chunk : chunk_bytes, at_least));
            job.used[f].push_back(0);
        };
        for (uint32_t lo = block_lo; lo < block_hi; lo += batch_blocks) {
            const uint32_t hi = (uint32_t)std::min<uint64_t>(block_hi, (uint64_t)lo + batch_blocks);
            for (int f = 0; f < 2; ++f) {
                const size_t expect = (size_t)(per_block[f] * (hi - lo) * 1.15) + 65536;
                if (room(f) < expect) new_chunk(f, expect);
            }
            for (int attempt = 0;; ++attempt) {
                size_t len[2] = {0, 0};
                uint64_t n = 0;
                char *dst[2];
                for (int f = 0; f < 2; ++f) dst[f] = job.chunks[f].back()->as<char>() + job.used[f].back();
                const int rc = sim_pairs(*s, PairsCall{{dst[0], room(0), &len[0]}, {dst[1], room(1), &len[1]}, (hipStream_t)stream}, lo, hi, &n);
                if (rc == RSQ_ENOSPC && attempt < 2) {              // the estimate was too small (the first call has none): arrays for what the call asked
                    for (int f = 0; f < 2; ++f)
                        if (len[f] > room(f)) new_chunk(f, len[f] + len[f] / 16 + 65536);
                    continue;
                }
                if (rc != RSQ_OK) return rc;
                for (int f = 0; f < 2; ++f) {
                    job.used[f].back() += len[f];
                    job.bytes[f] += len[f];
                    per_block[f] = std::max(per_block[f], (double)len[f] / (double)(hi - lo));
                }
                *n_pairs += n;
                break;
            }
        }
        *r1_bytes = job.bytes[0];
        *r2_bytes = job.bytes[1];
        job.complete = true;
        return (int)RSQ_OK;
    });
}
int rsq_sim_job_free(rsq_sim *s) {
    REQUIRE(s, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        s->job.clear();
        return (int)RSQ_OK;
    });
}
int rsq_sim_job_write(rsq_sim *s, const char *r1_path, uint64_t r1_offset, const char *r2_path, uint64_t r2_offset, uint32_t threads_per_file) {
    REQUIRE(s && r1_path, "null argument");
    if (depth_refuses_job(*s, "rsq_sim_job_write")) return RSQ_ESTATE;
    return guard([&] {
        const rsq_sim::JobText &job = s->job;
        if (!job.complete) {
            g_last_error = "rsq_sim_job_write: there is no generated text (rsq_sim_job_generate has not run to its end on this simulator, or rsq_sim_job_free has released it)";
            return (int)RSQ_ESTATE;
        }
        if (!r2_path && job.bytes[1]) throw Error("rsq_sim_job_write: the job has text for a second file, but no second path was given");
        const int n_files = r2_path ? 2 : 1;                  // one file: the text of seqToIllumina records kept by rsq_sim_error_model_file
        if (job.is_packed) {                                  // compressed in host memory already (rsq_sim_job_compress): plain writes at the offsets
            const char *names[2] = {r1_path, r2_path};
            const uint64_t at[2] = {r1_offset, r2_offset};
            for (int f = 0; f < n_files; ++f) {
                const int fd = open(names[f], O_WRONLY | O_CREAT, 0644);
                if (fd < 0) throw Error(std::string("cannot open '") + names[f] + "' for writing: " + strerror(errno));
                for (size_t done = 0; done < job.packed[f].size();) {
                    const ssize_t w = pwrite(fd, job.packed[f].data() + done, std::min<size_t>(job.packed[f].size() - done, (size_t)1 << 30), (off_t)(at[f] + done));
                    if (w < 0 && errno == EINTR) continue;
                    if (w <= 0) {
                        close(fd);
                        throw Error(std::string("writing '") + names[f] + "' failed: " + (w < 0 ? strerror(errno) : "no space"));
                    }
                    done += (size_t)w;
                }
                if (close(fd) != 0) throw Error(std::string("closing '") + names[f] + "' failed: " + strerror(errno));
            }
            return (int)RSQ_OK;
        }
        const uint32_t T = threads_per_file ? std::min(threads_per_file, 64u) : 1u;
        const char *paths[2] = {r1_path, r2_path};
        const uint64_t offsets[2] = {r1_offset, r2_offset};
        int fds[2] = {-1, -1};
        // Buffered pwrite()s into ONE file take the inode's lock one after the other, so more threads per file do not help on tmpfs or ext4 (measured on /dev/shm, 23 GB:
        // 1 thread per file 12.9 GB/s, 4 threads 7.5, 8 threads 7.2); copying into a shared mapping of the pre-sized file avoids that lock but pays a page fault per
        // 4 KB (6.4 GB/s however many threads) -- profiles/r03_e_*.  One thread per file is the default; file systems with concurrent direct I/O may want more.
        for (int f = 0; f < n_files; ++f) {
            fds[f] = open(paths[f], O_WRONLY | O_CREAT, 0644);
            if (fds[f] < 0) {
                if (f) close(fds[0]);
                throw Error(std::string("cannot open '") + paths[f] + "' for writing: " + strerror(errno));
            }
        }
        std::atomic<bool> failed{false};
        std::mutex message_mutex;
        std::string message;
        auto fail = [&](const std::string &m) {
            std::lock_guard<std::mutex> lock(message_mutex);
            if (!failed.exchange(true)) message = m;
        };
        // Option job_write_direct: the file is also opened with O_DIRECT, and what lies on whole blocks of the file (kDirectAlign) bypasses the page cache: writers of
        // ONE file then do not take turns on its inode (buffered writes into one file serialise there however many ranks write, profiles/r03_g_*).  A rank's byte
        // range begins and ends anywhere, so its head and tail up to the next block boundary go through the buffered descriptor.  Falls back to buffered writes
        // when the file system refuses O_DIRECT (tmpfs does).
        constexpr uint64_t kDirectAlign = 4096;
        int direct_fds[2] = {-1, -1};
        if (s->opt.job_write_direct)
            for (int f = 0; f < n_files; ++f) direct_fds[f] = open(paths[f], O_WRONLY | O_DIRECT);
        // thread t of file f writes bytes [bytes * t / T, bytes * (t + 1) / T) of the file's text: pieces of at most 32 MB, the copy of one overlapping the write of the one before
        auto work = [&](int f, uint32_t t) {
            try {
                HIP_CHECK(hipSetDevice(s->device));
                const uint64_t begin = job.bytes[f] * t / T, end = job.bytes[f] * (t + 1) / T;
                if (begin == end) return;
                struct Staging {                                    // released however the thread leaves (a failed pwrite or HIP call throws)
                    hipStream_t st = nullptr;
                    char *host[2] = {nullptr, nullptr};
                    ~Staging() {
                        if (st) (void)hipStreamSynchronize(st);     // a copy still in flight must not land in freed memory
                        for (char *h : host)
                            if (h) (void)hipHostFree(h);
                        if (st) (void)hipStreamDestroy(st);
                    }
                } staging;
                HIP_CHECK(hipStreamCreateWithFlags(&staging.st, hipStreamNonBlocking));
                for (char *&h : staging.host) HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&h), kJobSliceBytes, hipHostMallocDefault));      // page-aligned: fit for O_DIRECT
                hipStream_t st = staging.st;
                char *const *host = staging.host;
                struct Piece {
                    uint64_t at;                                    // place in the file's text
                    size_t n;
                    bool direct;
                };
                std::vector<Piece> pieces;
                {
                    const uint64_t file_begin = offsets[f] + begin, file_end = offsets[f] + end;      // in the file
                    uint64_t a = file_begin;
                    const bool direct = direct_fds[f] >= 0;
                    if (direct && a % kDirectAlign) {               // the head up to the first block boundary
                        const uint64_t to = std::min(file_end, (a / kDirectAlign + 1) * kDirectAlign);
                        pieces.push_back(Piece{a - offsets[f], (size_t)(to - a), false});
                        a = to;
                    }
                    const uint64_t whole_end = direct ? std::max(a, file_end / kDirectAlign * kDirectAlign) : file_end;
                    for (; a < whole_end; a += std::min<uint64_t>(kJobSliceBytes, whole_end - a)) pieces.push_back(Piece{a - offsets[f], (size_t)std::min<uint64_t>(kJobSliceBytes, whole_end - a), direct});
                    if (a < file_end) pieces.push_back(Piece{a - offsets[f], (size_t)(file_end - a), false});      // the tail behind the last whole block
                }
                // the text lies in a list of device arrays: a piece may reach over the end of one
                auto copy = [&](size_t i) {
                    uint64_t chunk_at = 0, at = pieces[i].at;
                    size_t left = pieces[i].n, put = 0;
                    for (size_t c = 0; c < job.chunks[f].size() && left; ++c) {
                        const uint64_t c_end = chunk_at + job.used[f][c];
                        if (at < c_end) {
                            const size_t n = (size_t)std::min<uint64_t>(left, c_end - at);
                            HIP_CHECK(hipMemcpyAsync(host[i & 1] + put, job.chunks[f][c]->as<char>() + (at - chunk_at), n, hipMemcpyDeviceToHost, st));
                            at += n, put += n, left -= n;
                        }
                        chunk_at = c_end;
                    }
                    if (left) throw Error("internal: a piece of the job's text lies outside its arrays");
                };
                if (!pieces.empty()) copy(0);
                for (size_t i = 0; i < pieces.size() && !failed; ++i) {
                    HIP_CHECK(hipStreamSynchronize(st));
                    if (i + 1 < pieces.size()) copy(i + 1);
                    size_t done = 0;
                    const int fd = pieces[i].direct ? direct_fds[f] : fds[f];
                    while (done < pieces[i].n) {
                        const ssize_t w = pwrite(fd, host[i & 1] + done, pieces[i].n - done, (off_t)(offsets[f] + pieces[i].at + done));
                        if (w < 0 && errno == EINTR) continue;
                        if (w <= 0) throw Error(std::string("writing '") + paths[f] + "' failed: " + (w < 0 ? strerror(errno) : "no space"));
                        done += (size_t)w;
                        if (pieces[i].direct && done < pieces[i].n && done % kDirectAlign) throw Error(std::string("writing '") + paths[f] + "': a direct write stopped inside a block");
                    }
                }
                HIP_CHECK(hipStreamSynchronize(st));
            } catch (const std::exception &e) {
                fail(e.what());
            }
        };
        std::vector<std::thread> pool;
        for (int f = 0; f < n_files; ++f)
            for (uint32_t t = 0; t < T; ++t) pool.emplace_back(work, f, t);
        for (std::thread &t : pool) t.join();
        for (int f = 0; f < n_files; ++f) {
            if (direct_fds[f] >= 0) close(direct_fds[f]);
            if (close(fds[f]) != 0) fail(std::string("closing '") + paths[f] + "' failed: " + strerror(errno));
        }
        if (failed) throw Error(message);
        return (int)RSQ_OK;
    });
}

// ------------------------------------------------------------------------------------------------ gzip on the device (rsq_deflate.h)
// The code of a call: the symbol counts of a sample of its pieces (k_gzip_pieces<true>), the code built on the host (gz::build_codes), uploaded.
static void gzip_code_of(rsq_sim &s, const uint8_t *text, size_t n, hipStream_t st) {
    const uint64_t n_pieces = cdiv(n, gz::kPiece);
    const uint32_t stride = gz::sample_stride(n_pieces);
    s.gz_hist.reserve(2 * (gz::kLitLen + gz::kDist) * 4);           // the sample walked both ways: by FASTQ lines, and densely (gz::dense_pays decides)
    s.gz_codes.reserve(sizeof(gz::Codes));
    uint32_t *lines = s.gz_hist.as<uint32_t>(), *dense = lines + gz::kLitLen + gz::kDist;
    HIP_CHECK(hipMemsetAsync(lines, 0, 2 * (gz::kLitLen + gz::kDist) * 4, st));
    const dim3 grid((uint32_t)cdiv(n_pieces, stride)), block(gz::kThreads);
    const int64_t route = s.opt.gzip_route;                          // < 0: the sample decides; 0 / > 0: by lines / dense whatever it says (only that route's sample is taken)
    if (route <= 0)
        hipLaunchKernelGGL((gz::k_gzip_pieces<true, gz::kProbeStep>), grid, block, 0, st, text, (uint64_t)n, stride, (const gz::Codes *)nullptr, (uint8_t *)nullptr, (uint32_t *)nullptr, lines);
    if (route != 0)
        hipLaunchKernelGGL((gz::k_gzip_pieces<true, gz::kDenseStep>), grid, block, 0, st, text, (uint64_t)n, stride, (const gz::Codes *)nullptr, (uint8_t *)nullptr, (uint32_t *)nullptr, dense);
    HIP_CHECK(hipGetLastError());
    uint32_t hist[2][gz::kLitLen + gz::kDist];
    HIP_CHECK(hipMemcpyAsync(hist, lines, sizeof hist, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    s.gz_dense = route < 0 ? gz::dense_pays(hist[0], hist[1]) : route > 0;
    gz::Codes codes = gz::build_codes(hist[s.gz_dense ? 1 : 0]);
    codes.dense = s.gz_dense ? 1u : 0u;
    HIP_CHECK(hipMemcpyAsync(s.gz_codes.as<char>(), &codes, sizeof codes, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                             // `codes` leaves scope
}
// text[0, n) of device memory as gzip members behind each other in out (device memory, room for out_cap bytes): stretches of at most kGzipStretch pieces (option gzip_stretch: of so many) go through
// the slots (compress, store what did not fit, scan the sizes, move the members into place).  *out_len = the bytes of all members; more than out_cap: nothing
// useful is in out, RSQ_ENOSPC.  with_code: the call's code is taken from this text first (else the caller has set it: several arrays of one job share a code).
constexpr uint64_t kGzipStretch = 8192;                              // pieces per pass: 535 MB of text, as much again in slots
static int gzip_device(rsq_sim &s, const uint8_t *text, size_t n, uint8_t *out, size_t out_cap, size_t *out_len, bool with_code, hipStream_t st) {
    *out_len = 0;
    if (!n) return RSQ_OK;
    if (with_code && !(s.gz_keep_code && s.gz_have_code)) {
        gzip_code_of(s, text, n, st);
        s.gz_have_code = true;
    }
    const uint64_t n_pieces = cdiv(n, gz::kPiece);
    const uint64_t stretch = std::min<uint64_t>(n_pieces, s.opt.gzip_stretch > 0 ? (uint64_t)s.opt.gzip_stretch : kGzipStretch);
    s.gz_slots.reserve(stretch * gz::kSlot);
    s.gz_sizes.reserve(stretch * 4);
    s.gz_at.reserve((stretch + 1) * 8);
    s.gz_total.reserve(8);
    size_t total = 0;
    for (uint64_t first = 0; first < n_pieces; first += stretch) {
        const uint32_t pieces = (uint32_t)std::min<uint64_t>(stretch, n_pieces - first);
        const uint8_t *t = text + first * gz::kPiece;
        const uint64_t bytes = std::min<uint64_t>((uint64_t)pieces * gz::kPiece, n - first * gz::kPiece);
        s.timers["gzip"].start(st);
        if (s.gz_dense)
            hipLaunchKernelGGL((gz::k_gzip_pieces<false, gz::kDenseStep>), dim3(pieces), dim3(gz::kThreads), 0, st, t, bytes, 1u, s.gz_codes.as<gz::Codes>(), s.gz_slots.as<uint8_t>(),
                               s.gz_sizes.as<uint32_t>(), (uint32_t *)nullptr);
        else
            hipLaunchKernelGGL((gz::k_gzip_pieces<false, gz::kProbeStep>), dim3(pieces), dim3(gz::kThreads), 0, st, t, bytes, 1u, s.gz_codes.as<gz::Codes>(), s.gz_slots.as<uint8_t>(),
                               s.gz_sizes.as<uint32_t>(), (uint32_t *)nullptr);
        hipLaunchKernelGGL(gz::k_gzip_stored, dim3(pieces), dim3(gz::kThreads), 0, st, t, bytes, s.gz_slots.as<uint8_t>(), s.gz_sizes.as<uint32_t>());
        exclusive_scan(s, s.gz_sizes.as<uint32_t>(), pieces, s.gz_at.as<uint64_t>(), st, nullptr, s.gz_total.as<uint64_t>());
        uint64_t stretch_bytes = 0;
        HIP_CHECK(hipMemcpyAsync(&stretch_bytes, s.gz_total.as<uint64_t>(), 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (total + stretch_bytes <= out_cap)
            hipLaunchKernelGGL(gz::k_gzip_compact, dim3(pieces), dim3(256), 0, st, s.gz_slots.as<uint8_t>(), s.gz_sizes.as<uint32_t>(), s.gz_at.as<uint64_t>(), out + total);
        s.timers["gzip"].stop(st);
        HIP_CHECK(hipGetLastError());
        total += stretch_bytes;
    }
    HIP_CHECK(hipStreamSynchronize(st));
    *out_len = total;
    if (total > out_cap) {
        g_last_error = "output buffer too small: the members need " + std::to_string(total) + " bytes";
        return RSQ_ENOSPC;
    }
    return RSQ_OK;
}
int rsq_sim_gzip_keep_code(rsq_sim *s, int keep) {
    REQUIRE(s, "null argument");
    s->gz_keep_code = keep != 0;
    s->gz_have_code = false;
    return RSQ_OK;
}
// The member that ends a BGZF file (SAM specification 4.1.2: an empty block, 28 bytes): bgzip / htslib warn about a file without it.  It is a complete gzip member of no
// text, so gzip, zlib and SeqAn read the file as before.  Whoever finishes a file of device-made members appends it.
size_t rsq_gzip_eof_member(char *out, size_t cap) {
    static const unsigned char kEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (out && cap >= sizeof kEof) memcpy(out, kEof, sizeof kEof);
    return sizeof kEof;
}
size_t rsq_gzip_bound(size_t text_len) { return (size_t)cdiv(text_len, gz::kPiece) * (gz::kHeaderBytes + 5u + gz::kTrailerBytes) + text_len; }
int rsq_sim_gzip_device(rsq_sim *s, const char *text_dev, size_t text_len, char *out_dev, size_t out_cap, size_t *out_len, void *stream) {
    REQUIRE(s && out_len && (text_dev || !text_len) && (out_dev || !out_cap), "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(s->device));
        reset_call_timers(*s);
        return gzip_device(*s, reinterpret_cast<const uint8_t *>(text_dev), text_len, reinterpret_cast<uint8_t *>(out_dev), out_cap, out_len, true, (hipStream_t)stream);
    });
}
// the kept text of a job on the device: every array of text becomes an array of members (the first array's sample gives the code of the file); the text is released
static void job_compress_on_device(rsq_sim &s, hipStream_t st) {
    rsq_sim::JobText &job = s.job;
    reset_call_timers(s);
    const bool kept = s.gz_keep_code;                                 // a job's text is of one kind: the first array's sample gives the code of all of them
    if (!kept) (void)rsq_sim_gzip_keep_code(&s, 1);
    struct Restore {
        rsq_sim &s;
        bool kept;
        ~Restore() {
            if (!kept) (void)rsq_sim_gzip_keep_code(&s, 0);
        }
    } restore{s, kept};
    for (int f = 0; f < 2; ++f) {
        uint64_t packed_bytes = 0;
        for (size_t c = 0; c < job.chunks[f].size(); ++c) {
            const size_t n = job.used[f][c];
            if (!n) continue;
            const uint8_t *text = job.chunks[f][c]->as<uint8_t>();
            // members need a third of the text or less; an array of that size first, the bound if the text is of another kind (the call then runs again)
            std::unique_ptr<DevBuf> packed(new DevBuf());
            size_t len = 0;
            packed->reserve(n / 2 + ((size_t)1 << 20));
            int rc = gzip_device(s, text, n, packed->as<uint8_t>(), packed->bytes(), &len, true, st);
            if (rc == RSQ_ENOSPC) {
                packed.reset(new DevBuf());
                packed->reserve(rsq_gzip_bound(n));
                rc = gzip_device(s, text, n, packed->as<uint8_t>(), packed->bytes(), &len, false, st);
            }
            if (rc != RSQ_OK) throw Error("compressing the job's text on the device failed: " + g_last_error);
            std::unique_ptr<DevBuf> fitted(new DevBuf());             // an array of the members' size (the first was sized by guess)
            fitted->reserve(len);
            HIP_CHECK(hipMemcpyAsync(fitted->as<char>(), packed->as<char>(), len, hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));
            packed = std::move(fitted);
            job.chunks[f][c] = std::move(packed);                     // the text's array is released
            job.used[f][c] = len;
            packed_bytes += len;
        }
        job.bytes[f] = packed_bytes;
    }
    s.gz_slots.release();                                             // the slots are as large as the text was: not kept beyond the call
}

// The kept text as gzip members (rsq_textio.h ParallelGzip: 1 MB of text each, compressed by a pool of threads) in host memory; the device arrays are released.
// A file of concatenated members is a gzip file: ranks exchange their COMPRESSED sizes and write their members at the offsets like plain text.
int rsq_sim_job_compress(rsq_sim *s, uint64_t *r1_bytes, uint64_t *r2_bytes) {
    REQUIRE(s && r1_bytes && r2_bytes, "null argument");
    if (depth_refuses_job(*s, "rsq_sim_job_compress")) return RSQ_ESTATE;
    return guard([&] {
        rsq_sim::JobText &job = s->job;
        if (!job.complete || job.is_packed || job.device_packed) {
            g_last_error = "rsq_sim_job_compress: there is no generated text, or it has been compressed already";
            return (int)RSQ_ESTATE;
        }
        HIP_CHECK(hipSetDevice(s->device));
        if (!s->opt.host_gzip) {                                   // on the device: the members stay in device memory, rsq_sim_job_write / _job_read serve them like text
            job_compress_on_device(*s, nullptr);
            job.device_packed = true;
            *r1_bytes = job.bytes[0];
            *r2_bytes = job.bytes[1];
            return (int)RSQ_OK;
        }
        s2i::CopyStream st;
        s2i::Pinned host[2];
        for (auto &h : host) h.ensure(kJobSliceBytes);
        for (int f = 0; f < 2; ++f) {
            textio::ParallelGzip gz;
            gz.open_memory(job.packed[f]);
            // the text lies in a list of device arrays; slices of kJobSliceBytes, the copy of one under the compression of the one before
            struct Slice {
                size_t chunk, at, n;
            };
            std::vector<Slice> slices;
            for (size_t c = 0; c < job.chunks[f].size(); ++c)
                for (size_t at = 0; at < job.used[f][c]; at += kJobSliceBytes) slices.push_back(Slice{c, at, std::min<size_t>(kJobSliceBytes, job.used[f][c] - at)});
            auto copy = [&](size_t i) { HIP_CHECK(hipMemcpyAsync(host[i & 1].p, job.chunks[f][slices[i].chunk]->as<char>() + slices[i].at, slices[i].n, hipMemcpyDeviceToHost, st.st)); };
            if (!slices.empty()) copy(0);
            for (size_t i = 0; i < slices.size(); ++i) {
                HIP_CHECK(hipStreamSynchronize(st.st));
                if (i + 1 < slices.size()) copy(i + 1);
                gz.write(host[i & 1].chars(), slices[i].n);
            }
            if (!gz.close()) throw Error("compressing the job's text failed");
            job.chunks[f].clear();
            job.used[f].clear();
            job.bytes[f] = job.packed[f].size();
        }
        job.is_packed = true;
        *r1_bytes = job.bytes[0];
        *r2_bytes = job.bytes[1];
        return (int)RSQ_OK;
    });
}

// a stretch of the kept text into device memory of the caller (what a rank contributes to one round of a gather of the output)
int rsq_sim_job_read(rsq_sim *s, int file, uint64_t at, size_t bytes, char *dst_dev, void *stream) {
    REQUIRE(s && (file == 0 || file == 1) && (dst_dev || !bytes), "null argument, or a file that is neither 0 nor 1");
    if (depth_refuses_job(*s, "rsq_sim_job_read")) return RSQ_ESTATE;
    return guard([&] {
        const rsq_sim::JobText &job = s->job;
        if (job.is_packed) {
            g_last_error = "rsq_sim_job_read: the text has been compressed into host memory (rsq_sim_job_compress); a gather works on the plain text";
            return (int)RSQ_ESTATE;
        }
        if (!job.complete) {
            g_last_error = "rsq_sim_job_read: there is no generated text (rsq_sim_job_generate has not run to its end on this simulator, or rsq_sim_job_free has released it)";
            return (int)RSQ_ESTATE;
        }
        if (at > job.bytes[file] || bytes > job.bytes[file] - at) {
            g_last_error = "rsq_sim_job_read: bytes [" + std::to_string(at) + ", " + std::to_string(at + bytes) + ") lie outside the file's " + std::to_string(job.bytes[file]) + " bytes of text";
            return (int)RSQ_EINVAL;
        }
        HIP_CHECK(hipSetDevice(s->device));
        uint64_t chunk_at = 0;
        size_t left = bytes, put = 0;
        for (size_t c = 0; c < job.chunks[file].size() && left; ++c) {            // the text lies in a list of device arrays
            const uint64_t c_end = chunk_at + job.used[file][c];
            if (at < c_end) {
                const size_t n = (size_t)std::min<uint64_t>(left, c_end - at);
                HIP_CHECK(hipMemcpyAsync(dst_dev + put, job.chunks[file][c]->as<char>() + (at - chunk_at), n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
                at += n, put += n, left -= n;
            }
            chunk_at = c_end;
        }
        HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        return (int)RSQ_OK;
    });
}

// the adapter-only entry points
static int adapter_only_call(rsq_sim *s, const PairsCall &call, uint64_t first, uint64_t n) {
    REQUIRE(s && call.r1.len && call.r2.len && (call.truth.len || !call.has_truth()) && s->prepared, "simulator not prepared");
    if (call.has_truth() && truth_refusal(*s, call.bam())) return RSQ_EINVAL;
    return guard([&] { return adapter_only_pairs(*s, call, n, first); });
}
int rsq_sim_adapter_only_pairs(rsq_sim *s, uint64_t first, uint64_t n, char *r1_dev, size_t r1_cap, size_t *r1_len, char *r2_dev, size_t r2_cap, size_t *r2_len,
                               void *stream) {
    return adapter_only_call(s, PairsCall{{r1_dev, r1_cap, r1_len}, {r2_dev, r2_cap, r2_len}, (hipStream_t)stream}, first, n);
}
int rsq_sim_adapter_only_pairs_sam(rsq_sim *s, uint64_t first, uint64_t n, char *r1_dev, size_t r1_cap, size_t *r1_len, char *r2_dev, size_t r2_cap, size_t *r2_len, char *sam_dev,
                                   size_t sam_cap, size_t *sam_len, void *stream) {
    return adapter_only_call(s, PairsCall{{r1_dev, r1_cap, r1_len}, {r2_dev, r2_cap, r2_len}, (hipStream_t)stream, {sam_dev, sam_cap, sam_len}, PairsCall::kSam}, first, n);
}
int rsq_sim_adapter_only_pairs_bam(rsq_sim *s, uint64_t first, uint64_t n, char *r1_dev, size_t r1_cap, size_t *r1_len, char *r2_dev, size_t r2_cap, size_t *r2_len, char *bam_dev,
                                   size_t bam_cap, size_t *bam_len, void *stream) {
    return adapter_only_call(s, PairsCall{{r1_dev, r1_cap, r1_len}, {r2_dev, r2_cap, r2_len}, (hipStream_t)stream, {bam_dev, bam_cap, bam_len}, PairsCall::kBam}, first, n);
}

// A profile with several read lengths draws a record's read length from tables over the fragment length (draw_read_length): a length outside them ends the call
// with the words of the reference's Vect::at (Vect.hpp:196-221 prints them before it throws) -- RSQ_EIO, nothing simulated
static void check_fragment_lengths(rsq_sim *s, uint64_t n, const uint8_t *seg_dev, const uint32_t *frag_len_dev, hipStream_t st) {
    FragmentRange range{{0u, 0u}, {0xFFFFFFFFu, 0xFFFFFFFFu}};
    bool any = false;
    for (int seg = 0; seg < 2; ++seg) {
        const DevReadLengths &rl = s->dev.read_lengths[seg];
        if (rl.fixed) continue;
        any = true;
        range.lo[seg] = std::max((uint32_t)s->insert_lengths_from, rl.row_first);
        range.hi[seg] = std::min(s->dev.insert_to, rl.row_first + rl.rows);
    }
    if (!any) return;
    s->cur->rec_count.reserve(16);
    uint32_t *flag = s->cur->rec_count.as<uint32_t>() + 2;            // (words 0 and 1 are the partition's counts)
    uint32_t &mail = s->mailbox->bad_fragment;
    mail = 0xFFFFFFFFu;
    HIP_CHECK(hipMemcpyAsync(flag, &mail, 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_fragment_range, dim3(cdiv(n, 256)), dim3(256), 0, st, seg_dev, frag_len_dev, n, range, flag);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(&mail, flag, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const uint32_t bad = mail;
    if (bad == 0xFFFFFFFFu) return;
    uint32_t fl = 0;
    uint8_t seg = 0;
    HIP_CHECK(hipMemcpy(&fl, frag_len_dev + bad, 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(&seg, seg_dev + bad, 1, hipMemcpyDeviceToHost));
    const DevReadLengths &rl = s->dev.read_lengths[seg ? 1 : 0];
    const bool in_insert_lengths = fl >= s->insert_lengths_from && fl < s->dev.insert_to;
    const uint64_t from = in_insert_lengths ? rl.row_first : s->insert_lengths_from, to = in_insert_lengths ? (uint64_t)rl.row_first + rl.rows : s->dev.insert_to;
    throw FragmentLengthOutside("record " + std::to_string(bad) + " of the call: Called index " + std::to_string(fl) + " range is from " + std::to_string(from) + " to " + std::to_string(to) +
                                " (the fragment length has no entry in the profile's " + (in_insert_lengths ? "read lengths by fragment length" : "insert lengths") + ")");
}

// the records' reads into the raw arrays: partition by template segment, k_fill_records
// (rec_at / rec_len: records of their own lengths at their own offsets of arrays of array_bytes bytes, read_len = the longest; nullptr: n x read_len bytes)
static RawLayout error_model_fill(rsq_sim *s, uint64_t first_index, uint64_t n, uint32_t read_len, const uint8_t *seqs_dev, const uint8_t *seg_dev, const uint32_t *frag_len_dev,
                                  const uint8_t *dom_dev, const uint8_t *rate_dev, hipStream_t st, const uint32_t *rec_at = nullptr, const uint32_t *rec_len = nullptr,
                                  uint32_t array_bytes = 0, bool fresh_timers = true, const uint16_t *codes = nullptr) {
    // a template longer than the profile's reads needs a wider op buffer than the one sized at create time
    const uint32_t need_ops = (s->rmax + read_len + s->max_adapter + 4u + 15u) / 16u;
    if (need_ops > s->ops_stride) s->ops_stride = need_ops;
    if (n >= 0xFFFFFFFFull) throw Error("at most 2^32-1 records per call");
    s->cur = &s->ws[0];
    if (fresh_timers) reset_call_timers(*s);
    check_fragment_lengths(s, n, seg_dev, frag_len_dev, st);
    RawLayout raw = raw_layout(*s, n);
    // partition the records by template segment: the read kernel's workgroups hold one segment's tables in LDS (binned by tile: build_fill_bins)
    if (!fill_is_binned(*s)) {
        s->cur->rec_flags.reserve(n * 4 + 16);
        s->cur->rec_index.reserve(n * 4 + 16);
        s->cur->rec_count.reserve(8);
        s->cur->offsets.reserve((n + 1) * 8);
        const dim3 rgrid(cdiv(n, 256)), rblock(256);
        hipLaunchKernelGGL(k_record_flags, rgrid, rblock, 0, st, seg_dev, n, s->cur->rec_flags.as<uint32_t>());
        exclusive_scan(*s, s->cur->rec_flags.as<uint32_t>(), n, s->cur->offsets.as<uint64_t>(), st);
        hipLaunchKernelGGL(k_record_partition, rgrid, rblock, 0, st, seg_dev, n, s->cur->offsets.as<uint64_t>(), s->cur->rec_index.as<uint32_t>(), s->cur->rec_count.as<uint32_t>());
        HIP_CHECK(hipGetLastError());
    }
    const RecordJob job{first_index, read_len, seqs_dev, dom_dev, rate_dev, frag_len_dev, s->cur->rec_index.as<uint32_t>(), s->cur->rec_count.as<uint32_t>(), n, rec_at, rec_len, array_bytes, codes};
    raw.order = launch_fill_records(*s, job, seg_dev, n, raw, st);
    return raw;
}

int rsq_sim_error_model(rsq_sim *s, uint64_t first_index, uint64_t n, uint32_t read_len, const uint8_t *seqs_dev, const uint8_t *seg_dev, const uint32_t *frag_len_dev,
                        const uint8_t *dom_dev, const uint8_t *rate_dev, uint8_t *seq_out_dev, uint8_t *qual_out_dev, uint32_t out_stride, uint16_t *read_len_out_dev,
                        uint16_t *num_errors_out_dev, uint16_t *tile_out_dev, char *cigar_out_dev, uint32_t cigar_stride, void *stream) {
    REQUIRE(s && s->prepared, "simulator not prepared");
    REQUIRE(seqs_dev && seg_dev && frag_len_dev && dom_dev && rate_dev && seq_out_dev && qual_out_dev && read_len_out_dev && num_errors_out_dev && tile_out_dev && cigar_out_dev,
            "null device pointer");
    if (!n) return RSQ_OK;
    return guard([&] {
        hipStream_t st = (hipStream_t)stream;
        HIP_CHECK(hipSetDevice(s->device));
        const RawLayout raw = error_model_fill(s, first_index, n, read_len, seqs_dev, seg_dev, frag_len_dev, dom_dev, rate_dev, st);
        s->cur->scan_total.reserve(8);
        HIP_CHECK(hipMemsetAsync(s->cur->scan_total.as<uint32_t>(), 0, 4, st));
        if (!((out_stride | (uint32_t)(uintptr_t)seq_out_dev | (uint32_t)(uintptr_t)qual_out_dev) & 3u))
            hipLaunchKernelGGL(k_error_model_rows, dim3(cdiv(n * 16, 256)), dim3(256), 0, st, raw, n, seq_out_dev, qual_out_dev, out_stride);
        hipLaunchKernelGGL(k_error_model_out, dim3(cdiv(n, 64)), dim3(64), 0, st, raw, n, seq_out_dev, qual_out_dev, out_stride, read_len_out_dev, num_errors_out_dev,
                           tile_out_dev, cigar_out_dev, cigar_stride, s->cur->scan_total.as<uint32_t>());
        HIP_CHECK(hipGetLastError());
        uint32_t overflow = 0;
        HIP_CHECK(hipMemcpyAsync(&overflow, s->cur->scan_total.as<uint32_t>(), 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (overflow) {
            g_last_error = "out_stride or cigar_stride too small for at least one record";
            return (int)RSQ_ENOSPC;
        }
        return (int)RSQ_OK;
    });
}

// the FASTQ text of the records in the raw arrays: sizes, scan, text; *text_len = the bytes needed (RSQ_ENOSPC, nothing written, if text_cap is smaller)
static int error_model_text(rsq_sim *s, const RawLayout &raw, uint64_t n, const RecordIds &ids, char *text_dev, size_t text_cap, size_t *text_len, hipStream_t st) {
    s->cur->sizes.reserve(n * 4 + 16);
    s->cur->off_r1.reserve((n + 1) * 8);
    s->timers["format_write"].start(st);
    hipLaunchKernelGGL(k_record_text_sizes, dim3(cdiv(n, 256)), dim3(256), 0, st, raw, n, ids, s->cur->sizes.as<uint32_t>());
    // the waves' LDS image is sized by the longest record of the call before (this call's goes to longest_record for the next one, out of the scan's first pass)
    s->longest_record.reserve(8);
    HIP_CHECK(hipMemsetAsync(s->longest_record.as<uint32_t>(), 0, 4, st));
    exclusive_scan(*s, s->cur->sizes.as<uint32_t>(), n, s->cur->off_r1.as<uint64_t>(), st, nullptr, nullptr, s->longest_record.as<uint32_t>());
    const uint32_t lds = format_lds_bytes(s->record_text_bytes, raw.order != nullptr);
    launch_text_waves(k_record_text_waves<true>, k_record_text_waves<false>, raw.order, dim3(cdiv(n, kFormatRecords)), lds, st, raw, n, ids, s->cur->off_r1.as<uint64_t>(), text_dev,
                      (uint64_t)text_cap, lds);
    s->timers["format_write"].stop(st);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(&s->mailbox->text_bytes, s->cur->off_r1.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&s->mailbox->text_longest, s->longest_record.as<uint32_t>(), 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    *text_len = s->mailbox->text_bytes;
    if (s->mailbox->text_longest) s->record_text_bytes = s->mailbox->text_longest + 8u;
    if (*text_len > text_cap) {
        g_last_error = "text buffer too small: need " + std::to_string(*text_len) + " bytes";
        return (int)RSQ_ENOSPC;
    }
    return (int)RSQ_OK;
}

int rsq_sim_error_model_fastq(rsq_sim *s, uint64_t first_index, uint64_t n, uint32_t read_len, const uint8_t *seqs_dev, const uint8_t *seg_dev, const uint32_t *frag_len_dev,
                              const uint8_t *dom_dev, const uint8_t *rate_dev, const char *ids_dev, const uint64_t *id_off_dev, char *text_dev, size_t text_cap,
                              size_t *text_len, void *stream) {
    REQUIRE(s && s->prepared, "simulator not prepared");
    REQUIRE(seqs_dev && seg_dev && frag_len_dev && dom_dev && rate_dev && ids_dev && id_off_dev && text_len && (text_dev || !text_cap), "null pointer");
    *text_len = 0;
    if (!n) return RSQ_OK;
    return guard([&] {
        hipStream_t st = (hipStream_t)stream;
        HIP_CHECK(hipSetDevice(s->device));
        const RawLayout raw = error_model_fill(s, first_index, n, read_len, seqs_dev, seg_dev, frag_len_dev, dom_dev, rate_dev, st);
        return error_model_text(s, raw, n, RecordIds{ids_dev, id_off_dev, nullptr, nullptr}, text_dev, text_cap, text_len, st);
    });
}

// the reference's complaint about a malformed record (Simulator.cpp:2423-2485; rec = the record's text from its '>' on)
static std::string record_message(const std::vector<uint8_t> &rec) {
    std::vector<uint8_t> scratch[3];
    for (auto &v : scratch) v.resize(rec.size() + 8);
    fasta::RecordFields f{0, 0, 0, 0};
    const fasta::RecordError e = fasta::parse_record(rec.data(), rec.size(), fasta::ByteArrays{scratch[0].data(), scratch[1].data(), scratch[2].data()}, f);
    const size_t line_end = (size_t)fasta::find_byte(rec.data(), 1, rec.size(), '\n');
    size_t header_len = line_end - 1;
    if (header_len && rec[line_end - 1] == '\r') --header_len;
    const std::string header(reinterpret_cast<const char *>(rec.data()) + 1, header_len);
    size_t L = 0;                                            // the template's length: as parse_record counts it
    for (size_t p = line_end + 1; p < rec.size(); ++p)
        if (rec[p] != '\n' && !(rec[p] == '\r' && (p + 1 == rec.size() || rec[p + 1] == '\n'))) ++L;
    size_t end = header_len > 2 * L + 2 ? header_len - 2 * L - 3 : 0;
    while (end && header[end] != ' ') --end;
    switch (e) {
        case fasta::kTooShort: return "Read description is too short to contain systematic error information and a sequence id: " + header;
        case fasta::kErrorSeparators: return "The two systematic error entries are not separated by a semicolon from themselves or the rest of the ReSeq information: " + header;
        case fasta::kNoId: return "No sequence id found that is separated by a space from the ReSeq information: " + header;
        case fasta::kSegment: return std::string("Template segment is ") + header[end + 1] + " not 1 or 2: " + header;
        case fasta::kSegmentSeparator: return "The template segment and fragment length are not separated by a semicolon: " + header;
        case fasta::kFragmentLength: {
            const size_t fl_at = end + 3, fl_end = header_len - 2 * L - 2;
            return "Fragment length '" + (fl_end > fl_at ? header.substr(fl_at, fl_end - fl_at) : std::string()) + "' is not a pure integer: " + header;
        }
        case fasta::kContainsN: return "input sequences must not contain N: " + header.substr(0, end);
        default: return "malformed record: " + header;
    }
}

int rsq_sim_error_model_fasta(rsq_sim *s, uint64_t first_index, const char *text_dev, size_t text_len, int final, char *out_dev, size_t out_cap, size_t *out_len,
                              uint64_t *n_records, size_t *consumed, void *stream) {
    REQUIRE(s && s->prepared, "simulator not prepared");
    REQUIRE(out_len && n_records && consumed && (text_dev || !text_len) && (out_dev || !out_cap), "null pointer");
    REQUIRE(text_len < 0xFFFFFFF0ull, "a block of FASTA text has to be shorter than 4 GB");
    *out_len = 0;
    *n_records = 0;
    *consumed = 0;
    if (!text_len) return RSQ_OK;
    return guard([&] {
        hipStream_t st = (hipStream_t)stream;
        HIP_CHECK(hipSetDevice(s->device));
        s->cur = &s->ws[0];
        rsq_sim::Workspace &w = *s->cur;
        const uint8_t *text = reinterpret_cast<const uint8_t *>(text_dev);
        // the record starts: counts per tile, their scan, the starts in input order
        const uint32_t n_tiles = cdiv(text_len, fasta::kTileBytes);
        auto roomy = [](size_t bytes) { return bytes + bytes / 8 + 64; };          // blocks differ by a few percent: grow once
        w.fa_counts.reserve(roomy((size_t)n_tiles * 4));
        w.fa_first.reserve(roomy(((size_t)n_tiles + 1) * 8));
        w.fa_summary.reserve(64);
        const dim3 tgrid(cdiv(n_tiles, fasta::kStartsBlock / 64u)), tblock(fasta::kStartsBlock);
        hipLaunchKernelGGL(fasta::k_fasta_count, tgrid, tblock, 0, st, text, (uint64_t)text_len, n_tiles, w.fa_counts.as<uint32_t>());
        exclusive_scan(*s, w.fa_counts.as<uint32_t>(), n_tiles, w.fa_first.as<uint64_t>(), st);
        rsq_sim::Mailbox &mail = *s->mailbox;
        HIP_CHECK(hipMemcpyAsync(&mail.fasta_starts, w.fa_first.as<uint64_t>() + n_tiles, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const uint64_t starts = mail.fasta_starts;
        if (starts >= 0xFFFFFFFFull) throw Error("more than 2^32 records in one block of text");
        w.fa_at.reserve(roomy((starts + 1) * 4));
        hipLaunchKernelGGL(fasta::k_fasta_starts, tgrid, tblock, 0, st, text, (uint64_t)text_len, n_tiles, w.fa_first.as<uint64_t>(), w.fa_at.as<uint32_t>());
        // a block that is not the input's last leaves its last record to the caller: its end is not known yet
        const uint32_t n = (uint32_t)(final || !starts ? starts : starts - 1);
        w.fa_len.reserve(roomy((size_t)n * 4));
        w.fa_id_len.reserve(roomy((size_t)n * 4));
        w.fa_frag_len.reserve(roomy((size_t)n * 4));
        w.fa_seg.reserve(roomy(n));
        w.fa_codes.reserve(roomy(2 * (text_len + 8)));                // a half-word per byte of text: a record's codes lie at its own offset
        uint32_t *summary = w.fa_summary.as<uint32_t>();
        mail.fasta_summary = {0u, 0xFFFFFFFFu, 0u, 0u};
        HIP_CHECK(hipMemcpyAsync(summary, &mail.fasta_summary, 16, hipMemcpyHostToDevice, st));
        // text in front of the first record: [0, at[0]) -- at[0] = text_len without any record
        HIP_CHECK(hipMemcpyAsync(&mail.fasta_lead_end, w.fa_at.as<uint32_t>(), 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(&mail.fasta_last_start, w.fa_at.as<uint32_t>() + (starts ? starts - 1 : 0), 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const uint32_t lead_end = mail.fasta_lead_end, last_start = mail.fasta_last_start;
        reset_call_timers(*s);
        s->timers["parse_records"].start(st);
        const fasta::Records rec{w.fa_at.as<uint32_t>(), w.fa_len.as<uint32_t>(), w.fa_id_len.as<uint32_t>(), w.fa_frag_len.as<uint32_t>(), w.fa_seg.as<uint8_t>()};
        if (lead_end) hipLaunchKernelGGL(fasta::k_fasta_lead, dim3(std::min(1024u, cdiv(lead_end, 256))), dim3(256), 0, st, text, lead_end, summary);
        if (n) {
            // per launch like fill_lds_bytes: function attributes belong to the device the call runs on, and a process may hold simulators on several
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&fasta::k_fasta_records), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fasta::kStageBytes));
            hipLaunchKernelGGL(fasta::k_fasta_records, dim3(cdiv(n, fasta::kRecordsBlock)), dim3(fasta::kRecordsBlock), fasta::kStageBytes, st, text, n, rec, w.fa_codes.as<uint16_t>(), summary,
                               s->opt.fasta_no_stage ? 0u : fasta::kStageBytes);
        }
        s->timers["parse_records"].stop(st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(&mail.fasta_summary, summary, 16, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const uint32_t longest = mail.fasta_summary.longest, first_bad = mail.fasta_summary.first_bad;
        if (mail.fasta_summary.stray_text) {
            g_last_error = "sequence data without a header line in the input";
            return (int)RSQ_EIO;
        }
        if (first_bad != 0xFFFFFFFFu) {
            uint32_t span[2];
            HIP_CHECK(hipMemcpy(span, w.fa_at.as<uint32_t>() + first_bad, 8, hipMemcpyDeviceToHost));
            std::vector<uint8_t> record(span[1] - span[0]);
            HIP_CHECK(hipMemcpy(record.data(), text + span[0], record.size(), hipMemcpyDeviceToHost));
            g_last_error = record_message(record);
            return (int)RSQ_EIO;
        }
        *consumed = final ? text_len : (starts ? last_start : 0);      // no record starts in a block that is not the last: nothing consumed, the caller hands in more
        *n_records = n;
        if (!n) return (int)RSQ_OK;
        const RawLayout raw = error_model_fill(s, first_index, n, longest, nullptr, w.fa_seg.as<uint8_t>(), w.fa_frag_len.as<uint32_t>(), nullptr, nullptr, st, w.fa_at.as<uint32_t>(),
                                               w.fa_len.as<uint32_t>(), (uint32_t)text_len + 8u, false, w.fa_codes.as<uint16_t>());
        return error_model_text(s, raw, n, RecordIds{text_dev, nullptr, w.fa_at.as<uint32_t>(), w.fa_id_len.as<uint32_t>()}, out_dev, out_cap, out_len, st);
    });
}

int rsq_sim_error_model_file(rsq_sim *s, const char *input_path, const char *output_path, const rsq_error_model_file_options *options, uint64_t *n_records,
                             uint64_t *out_bytes) {
    REQUIRE(s && s->prepared, "simulator not prepared");
    REQUIRE(n_records && out_bytes, "null argument");
    *n_records = 0;
    *out_bytes = 0;
    return guard([&] {
        using namespace s2i;
        const auto t_start = Clock::now();
        rsq_error_model_file_options opt{};
        if (options) opt = *options;
        HIP_CHECK(hipSetDevice(s->device));
        const unsigned hw = std::thread::hardware_concurrency();
        // reader threads of a plain file: one copies 6-9 GB/s out of the page cache
        const uint32_t n_readers = opt.read_threads ? opt.read_threads : std::max(1u, std::min(hw > 3 ? hw - 3 : 1u, 6u));
        const size_t block_bytes = (size_t)std::min<uint32_t>(1u << 20, opt.block_kb ? opt.block_kb : 48u << 10) << 10;
        uint32_t batch_blocks = opt.batch_blocks ? opt.batch_blocks : 8u;
        while (batch_blocks > 1 && batch_blocks * block_bytes > ((size_t)3 << 30)) --batch_blocks;      // a call takes less than 4 GB of text
        uint64_t plain_size = 0;
        FileDescriptor plain;
        SequentialIn seq_in;
        if (input_path) plain.fd = open_plain_file(input_path, plain_size);
        if (plain.fd < 0) {
            if (opt.from || opt.to) throw Error("a byte range needs an input file that can be read at offsets (not compressed, not a pipe)");
            if (!seq_in.open(input_path)) {
                g_last_error = std::string("Could not open '") + input_path + "' for reading.";
                return (int)RSQ_EIO;
            }
        }
        const uint64_t to = std::min(opt.to ? opt.to : plain_size, plain_size), from = std::min(opt.from, to);
        Fault fault;
        OutPipe out(s->device, fault);
        rsq_sim::JobText &job = s->job;
        // a .gz output: every call's text becomes gzip members on the device (rsq_deflate.h) and the members go down the link and into the file as they are -- a third
        // of the bytes, and no host thread compresses (option host_gzip: zlib behind the writer, as before round 5)
        const bool gz_on_device = output_path && textio::has_suffix(output_path, ".gz") && !s->opt.host_gzip;
        DevBuf call_text;
        // the first call's sample gives the code of the whole file -- of THIS file: the caller's setting (and no code of this file's) is what later calls find
        struct RestoreCode {
            rsq_sim *s;
            bool on, kept;
            ~RestoreCode() {
                if (on) (void)rsq_sim_gzip_keep_code(s, kept ? 1 : 0);
            }
        } restore_code{s, gz_on_device, s->gz_keep_code};
        if (gz_on_device) (void)rsq_sim_gzip_keep_code(s, 1);
        if (opt.keep_text) {                                  // the text stays in device memory, as rsq_sim_job_generate keeps a rank's share of the pairs' text
            if (output_path) throw Error("keep_text and an output path exclude each other");
            job.clear();
        } else if (gz_on_device && !opt.from && !opt.to) {     // a whole file of device-made members ends like a BGZF file (a share of a job: whoever ends the file does it)
            char eof[32];
            out.tail.assign(eof, rsq_gzip_eof_member(eof, sizeof eof));
        }
        if (!opt.keep_text && !out.open(output_path, gz_on_device)) {
            g_last_error = std::string("Could not open '") + output_path + "' for writing.";
            return (int)RSQ_EIO;
        }
        auto room = [&] { return job.chunks[0].empty() ? (size_t)0 : job.chunks[0].back()->bytes() - job.used[0].back(); };
        auto new_chunk = [&](size_t bytes) {
            job.chunks[0].push_back(std::make_unique<DevBuf>());
            job.chunks[0].back()->reserve(std::max<size_t>(bytes, (size_t)256 << 20));
            job.used[0].push_back(0);
        };
        InPipe in(s->device, block_bytes, plain.fd >= 0 ? n_readers : 1, fault);
        if (plain.fd >= 0) in.start_file(plain.fd, from, to, n_readers);
        else in.start_stream(seq_in);
        // the records' read kernel for this profile, while the readers fetch the first blocks (a second of compilation the first time a profile is used)
        (void)spec_kernel(*s, SpecKind::kRecords, effective_fill_mask(s->dev.lds.mask, s->force_fill_mode), true, fill_is_binned(*s));
        CopyStream st;
        DevBuf joined[2];                                     // the text of a call: what the call before left over (it lies in the other one), then the blocks
        int next_joined = 0;
        const char *rest = nullptr;                           // the start of a record whose end the next block holds
        size_t rest_len = 0;
        uint64_t records = 0, next_report = 0, calls = 0;
        StageTime t_wait, t_join, t_call;
        double at_first_block = 0;
        int rc = RSQ_OK;
        bool last = false;
        for (uint64_t b = 0; rc == RSQ_OK && !last;) {
            auto t0 = Clock::now();
            InPipe::Slot *slot = in.take(b);
            t_wait.add(t0);
            if (!slot) break;                                 // a side has failed: `fault` says why
            if (!b) at_first_block = seconds_since(t_start);
            t0 = Clock::now();
            DevBuf &j = joined[next_joined];
            next_joined ^= 1;
            j.reserve(rest_len + batch_blocks * block_bytes + 16);
            char *text = j.as<char>();
            st.copy(text, rest, rest_len, hipMemcpyDeviceToDevice);
            size_t len = rest_len;
            for (uint32_t k = 0; slot; ++k) {
                st.copy(text + len, slot->dev.as<char>(), slot->len, hipMemcpyDeviceToDevice);
                len += slot->len;
                last = slot->last;
                in.release(b++);
                slot = last || k + 1 == batch_blocks ? nullptr : in.take(b, false);
            }
            t_join.add(t0);
            t0 = Clock::now();
            DevBuf *o = opt.keep_text ? nullptr : out.begin();
            if (!o && !opt.keep_text) break;
            size_t out_len = 0, used = 0;
            uint64_t n = 0;
            for (int attempt = 0; attempt < 2; ++attempt) {
                const size_t want = std::max(out_len + out_len / 8, len + len / 8) + 4096;
                char *dst;
                size_t cap;
                if (opt.keep_text) {
                    if (room() < (attempt ? out_len : want)) new_chunk(want);
                    dst = job.chunks[0].back()->as<char>() + job.used[0].back();
                    cap = room();
                } else {
                    DevBuf &to = gz_on_device ? call_text : *o;
                    to.reserve(want);
                    dst = to.as<char>();
                    cap = to.bytes();
                }
                rc = rsq_sim_error_model_fasta(s, opt.first_record + records, text, len, last ? 1 : 0, dst, cap, &out_len, &n, &used, st.st);
                if (rc != RSQ_ENOSPC) break;
            }
            if (rc == RSQ_OK && gz_on_device && out_len) {
                size_t packed = 0;
                o->reserve(out_len / 2 + ((size_t)1 << 20));
                rc = gzip_device(*s, call_text.as<uint8_t>(), out_len, o->as<uint8_t>(), o->bytes(), &packed, true, st.st);
                if (rc == RSQ_ENOSPC) {
                    o->reserve(rsq_gzip_bound(out_len));
                    rc = gzip_device(*s, call_text.as<uint8_t>(), out_len, o->as<uint8_t>(), o->bytes(), &packed, false, st.st);
                }
                out_len = packed;
            }
            t_call.add(t0);
            if (rc != RSQ_OK) break;                          // g_last_error holds the reason (the reference's complaint about a record: RSQ_EIO)
            ++calls;
            if (opt.keep_text) {
                job.used[0].back() += out_len;
                job.bytes[0] += out_len;
            } else if (out_len) out.submit(out_len);
            records += n;                                     // first_record + records = the index of the next record in the input (it selects the records' random streams)
            rest = text + used;
            rest_len = len - used;
            if (opt.progress && records >= next_report) {
                opt.progress(records, opt.user);
                next_report = records + 1000000;
            }
        }
        const double t_loop = seconds_since(t_start);
        if (rc != RSQ_OK) fault.raise(g_last_error);
        in.join();
        out.close();
        if (opt.trace && opt.trace_cap)
            snprintf(opt.trace, opt.trace_cap,
                     "first block on the device %.3f s into the call; the simulator side took %.3f s for %llu records in %llu calls: waiting for blocks %.3f, putting blocks together "
                     "%.3f, device calls %.3f (of these waiting for a free output buffer %.3f); readers (summed over %u threads): reading %.3f, uploads %.3f, waiting for a slot %.3f; "
                     "downloads %.3f (+ %.3f waiting for a free buffer); writing %.3f",
                     at_first_block, t_loop, (unsigned long long)records, (unsigned long long)calls, t_wait.s(), t_join.s(), t_call.s(), out.t_dev.s(), (unsigned)in.readers.size(),
                     in.t_read.s(), in.t_upload.s(), in.t_slot.s(), out.t_download.s(), out.t_stage.s(), out.t_write.s());
        if (fault.set) {
            if (opt.keep_text) job.clear();
            g_last_error = fault.what;
            return rc != RSQ_OK ? rc : (int)RSQ_EIO;
        }
        *n_records = records;
        *out_bytes = opt.keep_text ? job.bytes[0] : out.bytes + out.tail.size();
        job.complete = opt.keep_text != 0;
        return (int)RSQ_OK;
    });
}

int rsq_fasta_count_records(const char *path, uint64_t from, uint64_t to, uint32_t threads, uint64_t *n_starts, uint64_t *first_start) {
    REQUIRE(path && n_starts && first_start, "null argument");
    return guard([&] {
        s2i::count_records(path, from, to, threads, n_starts, first_start);
        return (int)RSQ_OK;
    });
}

int rsq_sim_last_kernel_ms(const rsq_sim *s, const char *kernel, double *ms) {
    REQUIRE(s && kernel && ms, "null argument");
    auto it = s->timers.find(kernel);
    REQUIRE(it != s->timers.end() && it->second.launches(), "unknown kernel name or kernel not launched in the last call");
    *ms = it->second.ms();
    return RSQ_OK;
}
int rsq_sim_last_kernel_launches(const rsq_sim *s, const char *kernel, uint32_t *launches) {
    REQUIRE(s && kernel && launches, "null argument");
    auto it = s->timers.find(kernel);
    *launches = it == s->timers.end() ? 0u : (uint32_t)it->second.launches();
    return RSQ_OK;
}

int rsq_dev_alloc(int device, size_t bytes, void **out_dev) {
    REQUIRE(out_dev, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipMalloc(out_dev, bytes ? bytes : 8));
        return RSQ_OK;
    });
}
int rsq_dev_free(int device, void *dev) {
    return guard([&] {
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipFree(dev));
        return RSQ_OK;
    });
}
int rsq_dev_upload(int device, void *dst_dev, const void *src, size_t bytes) {
    return guard([&] {
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipMemcpy(dst_dev, src, bytes, hipMemcpyHostToDevice));
        return RSQ_OK;
    });
}
int rsq_host_alloc(size_t bytes, void **out_host) {
    REQUIRE(out_host, "null argument");
    return guard([&] {
        HIP_CHECK(hipHostMalloc(out_host, bytes ? bytes : 8, hipHostMallocDefault));
        return RSQ_OK;
    });
}
int rsq_host_free(void *host) {
    return guard([&] {
        if (host) HIP_CHECK(hipHostFree(host));
        return RSQ_OK;
    });
}
// device memory to its place in a file: slices through two page-locked buffers, the copy of one under the write of the one before (the writer of a gathered output)
int rsq_dev_pwrite(int device, const void *src_dev, size_t bytes, const char *path, uint64_t offset) {
    REQUIRE(path && (src_dev || !bytes), "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(device));
        struct Staging {
            hipStream_t st = nullptr;
            char *host[2] = {nullptr, nullptr};
            int fd = -1;
            ~Staging() {
                if (st) (void)hipStreamSynchronize(st);
                for (char *h : host)
                    if (h) (void)hipHostFree(h);
                if (st) (void)hipStreamDestroy(st);
                if (fd >= 0) close(fd);
            }
        } g;
        g.fd = open(path, O_WRONLY | O_CREAT, 0644);
        if (g.fd < 0) throw Error(std::string("cannot open '") + path + "' for writing: " + strerror(errno));
        constexpr size_t kSlice = (size_t)16 << 20;
        HIP_CHECK(hipStreamCreateWithFlags(&g.st, hipStreamNonBlocking));
        for (char *&h : g.host) HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&h), std::min(kSlice, std::max<size_t>(bytes, 1)), hipHostMallocDefault));
        const char *src = static_cast<const char *>(src_dev);
        const size_t n_slices = (bytes + kSlice - 1) / kSlice;
        auto copy = [&](size_t i) { HIP_CHECK(hipMemcpyAsync(g.host[i & 1], src + i * kSlice, std::min(kSlice, bytes - i * kSlice), hipMemcpyDeviceToHost, g.st)); };
        if (n_slices) copy(0);
        for (size_t i = 0; i < n_slices; ++i) {
            HIP_CHECK(hipStreamSynchronize(g.st));
            if (i + 1 < n_slices) copy(i + 1);
            const size_t n = std::min(kSlice, bytes - i * kSlice);
            for (size_t done = 0; done < n;) {
                const ssize_t w = pwrite(g.fd, g.host[i & 1] + done, n - done, (off_t)(offset + i * kSlice + done));
                if (w < 0 && errno == EINTR) continue;
                if (w <= 0) throw Error(std::string("writing '") + path + "' failed: " + (w < 0 ? strerror(errno) : "no space"));
                done += (size_t)w;
            }
        }
        const int fd = g.fd;
        g.fd = -1;
        if (close(fd) != 0) throw Error(std::string("closing '") + path + "' failed: " + strerror(errno));
        return RSQ_OK;
    });
}
int rsq_dev_download(int device, void *dst, const void *src_dev, size_t bytes) {
    return guard([&] {
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipMemcpy(dst, src_dev, bytes, hipMemcpyDeviceToHost));
        return RSQ_OK;
    });
}
// streams of the caller's own (the CLI's reader, simulator and writer sides each work on one): copies on them return when they are done and leave
// the other streams alone -- the plain calls above go through the null stream, which waits for every other one
int rsq_stream_create(int device, void **out_stream) {
    REQUIRE(out_stream, "null argument");
    return guard([&] {
        HIP_CHECK(hipSetDevice(device));
        hipStream_t st = nullptr;
        HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        *out_stream = st;
        return RSQ_OK;
    });
}
int rsq_stream_destroy(int device, void *stream) {
    return guard([&] {
        HIP_CHECK(hipSetDevice(device));
        if (stream) HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
        return RSQ_OK;
    });
}
int rsq_dev_copy_on(int device, void *dst, const void *src, size_t bytes, int kind, void *stream) {
    REQUIRE(kind >= 0 && kind <= 2 && (dst || !bytes) && (src || !bytes), "kind is 0 (host to device), 1 (device to host) or 2 (device to device)");
    return guard([&] {
        HIP_CHECK(hipSetDevice(device));
        static const hipMemcpyKind kinds[3] = {hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice};
        if (bytes) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, kinds[kind], (hipStream_t)stream));
        HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        return RSQ_OK;
    });
}

}  // extern "C"
