// philox_steps_trial.cpp -- TEST-ONLY: philox() and Stream::step of reseq_amd/csrc/rsq_core.h, the random words every draw of every kernel starts from, written to a
// file word by word -- portable_trial.cpp's scheme: one source, two programs.  Built by a host compiler it runs the host forms (tests/test_philox_words.py: against
// a Philox4x32-10 written in the test and against the oracle's); built by hipcc for the library's architecture it runs them inside kernels
// (tests/test_philox_steps_gpu.py: word for word the same).
//   philox_steps_trial words <inputs> <results>      records of six words (seed low, seed high, c0, c1, c2, c3) -> philox()'s four words each; on the device one
//                                                    lane per record, so the seeds differ between the lanes of a wave: the form without a barrier, which every caller
//                                                    but the read kernel's step takes
//   philox_steps_trial steps <inputs> <results>      jobs of six words (seed low, seed high, c3base, first step, steps, lanes) followed by three words (c0, c1, c2) per
//                                                    lane -> for every choice of kChoices in turn, for every lane, Stream::step(first step + t) for t = 0 .. steps - 1,
//                                                    four words each.  On the device the job is one launch of one workgroup: the seed is the kernel's argument
//                                                    (wave-uniform, as the read kernel's is), the steps are a LOOP inside the kernel (so the compiler places the round
//                                                    keys as it does in the read kernel's step loop), and only the first `lanes` threads are active (partial waves).
// kChoices: where the round keys pass through RSQ_KEEP_IN_SGPR (philox's KEYS_FROM) -- every choice the tree uses (none: kKeysAhead; the read
// kernels' step: kKeysFromStep, rsq_reads.h), every round, all but the first, and the last round alone.  The words do not depend on it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_reads.h"

using namespace rsq;

constexpr int kChoices[] = {kKeysAhead, kKeysFromStep, 0, 1, kPhiloxRounds - 1};
constexpr uint32_t kBlock = 192u, kStepsMax = 4096u;                   // three waves: 129 lanes leave the third with one
struct Record {
    uint32_t seed_lo, seed_hi, c0, c1, c2, c3;
};
struct Job {
    uint32_t seed_lo, seed_hi, c3base, first, steps, lanes;
};
struct Lane {
    uint32_t c0, c1, c2;
};
RSQ_HD uint64_t seed_of(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }
template <int KEYS>
RSQ_HD void lane_steps(uint64_t seed, const Job &job, const Lane &l, Words *out) {
    const Stream st{seed, l.c0, l.c1, l.c2, job.c3base};
    for (uint32_t t = 0; t < job.steps; ++t) out[t] = st.template step<KEYS>(job.first + t);
}

#if RSQ_DEVICE_BUILD
#define CHECK(call)                                                                          \
    do {                                                                                     \
        const hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                              \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                       \
            return 3;                                                                        \
        }                                                                                    \
    } while (0)
__global__ void __launch_bounds__(64) k_words(const Record *__restrict__ in, uint32_t n, Words *__restrict__ out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i < n) out[i] = philox(seed_of(in[i].seed_lo, in[i].seed_hi), in[i].c0, in[i].c1, in[i].c2, in[i].c3);
}
template <int KEYS>
__global__ void __launch_bounds__(kBlock) k_steps(uint64_t seed, Job job, const Lane *__restrict__ lanes, Words *__restrict__ out) {
    if (threadIdx.x < job.lanes) lane_steps<KEYS>(seed, job, lanes[threadIdx.x], out + (size_t)threadIdx.x * job.steps);
}
static int run_words(const std::vector<Record> &in, Words *out) {
    Record *d_in = nullptr;
    Words *d_out = nullptr;
    CHECK(hipMalloc(&d_in, in.size() * sizeof(Record)));
    CHECK(hipMalloc(&d_out, in.size() * sizeof(Words)));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * sizeof(Record), hipMemcpyHostToDevice));
    k_words<<<(uint32_t)((in.size() + 63u) / 64u), 64>>>(d_in, (uint32_t)in.size(), d_out);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(out, d_out, in.size() * sizeof(Words), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    return 0;
}
template <int KEYS>
static int run_steps(const Job &job, const std::vector<Lane> &lanes, Words *out) {
    Lane *d_lanes = nullptr;
    Words *d_out = nullptr;
    const size_t n_out = (size_t)job.lanes * job.steps;
    CHECK(hipMalloc(&d_lanes, lanes.size() * sizeof(Lane)));
    CHECK(hipMalloc(&d_out, n_out * sizeof(Words)));
    CHECK(hipMemcpy(d_lanes, lanes.data(), lanes.size() * sizeof(Lane), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xA5, n_out * sizeof(Words)));
    k_steps<KEYS><<<1, kBlock>>>(seed_of(job.seed_lo, job.seed_hi), job, d_lanes, d_out);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(out, d_out, n_out * sizeof(Words), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_lanes));
    CHECK(hipFree(d_out));
    return 0;
}
#else
static int run_words(const std::vector<Record> &in, Words *out) {
    for (size_t i = 0; i < in.size(); ++i) out[i] = philox(seed_of(in[i].seed_lo, in[i].seed_hi), in[i].c0, in[i].c1, in[i].c2, in[i].c3);
    return 0;
}
template <int KEYS>
static int run_steps(const Job &job, const std::vector<Lane> &lanes, Words *out) {
    for (uint32_t l = 0; l < job.lanes; ++l) lane_steps<KEYS>(seed_of(job.seed_lo, job.seed_hi), job, lanes[l], out + (size_t)l * job.steps);
    return 0;
}
#endif

template <int... KEYS>
static int run_choices(const Job &job, const std::vector<Lane> &lanes, FILE *f) {
    std::vector<Words> out((size_t)job.lanes * job.steps);             // at exactly their size, so that the sanitizer sees a word beside them
    int rc = 0;
    ((rc = rc ? rc : run_steps<KEYS>(job, lanes, out.data()), rc = rc ? rc : (fwrite(out.data(), sizeof(Words), out.size(), f) == out.size() ? 0 : 2)), ...);
    return rc;
}

int main(int argc, char **argv) {
    if (argc != 4 || (strcmp(argv[1], "words") && strcmp(argv[1], "steps"))) return fprintf(stderr, "usage: philox_steps_trial words|steps <inputs> <results>\n"), 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return perror(argv[2]), 2;
    FILE *g = fopen(argv[3], "wb");
    if (!g) return perror(argv[3]), 2;
    size_t n = 0;
    if (!strcmp(argv[1], "words")) {
        std::vector<Record> in;
        Record rec;
        while (fread(&rec, sizeof rec, 1, f) == 1) in.push_back(rec);
        if (in.empty()) return fprintf(stderr, "no records\n"), 2;
        std::vector<Words> out(in.size());
        if (const int rc = run_words(in, out.data())) return rc;
        if (fwrite(out.data(), sizeof(Words), out.size(), g) != out.size()) return 2;
        n = in.size();
    } else {
        Job job;
        while (fread(&job, sizeof job, 1, f) == 1) {
            if (job.lanes < 1u || job.lanes > kBlock || job.steps < 1u || job.steps > kStepsMax) return fprintf(stderr, "job %zu: %u lanes, %u steps\n", n, job.lanes, job.steps), 2;
            std::vector<Lane> lanes(job.lanes);
            if (fread(lanes.data(), sizeof(Lane), lanes.size(), f) != lanes.size()) return fprintf(stderr, "job %zu: short\n", n), 2;
            static_assert(sizeof(kChoices) / sizeof(kChoices[0]) == 5, "the list below");
            if (const int rc = run_choices<kChoices[0], kChoices[1], kChoices[2], kChoices[3], kChoices[4]>(job, lanes, g)) return rc;
            ++n;
        }
    }
    fclose(f);
    return fclose(g) == 0 ? (printf("%zu records\n", n), 0) : 2;
}
