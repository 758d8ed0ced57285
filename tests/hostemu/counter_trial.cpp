// counter_trial.cpp -- TEST-ONLY: counter_add of reseq_amd/csrc/rsq_portable.h (the one primitive that adds into device memory other workgroups add to as well:
// rsq_depth.h's array of differences) evaluated over a table of inputs, the results written to a file -- portable_trial.cpp's scheme for this primitive.
//   counter_trial <inputs> <results>
// One source, two programs.  Built by a host compiler (tests/test_portable_counter.py: g++ with -fsanitize=address,undefined) it runs the host form; built by hipcc
// for the library's architecture it runs the device form, and the test requires of both the words its own definition gives.
// <inputs>: records of two words (first, v); <results>: four words per record.  Lane l of 64 adds v rotated left by l to counter (first + l) % 4 of four counters,
// which keep what earlier records left: the counters after each record.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_portable.h"

using namespace rsq;

struct In {
    uint32_t first, v;
};
struct Out {
    uint32_t r[4];
};
constexpr uint32_t kCounters = 4, kLanes = 64;
RSQ_HD uint32_t rotate_left(uint32_t v, uint32_t n) { return (v << (n & 31u)) | (v >> ((32u - n) & 31u)); }
RSQ_HD void counter_add_lane(const In &in, uint32_t lane, uint32_t *counters) { counter_add(counters + ((in.first + lane) & (kCounters - 1u)), rotate_left(in.v, lane)); }

#if RSQ_DEVICE_BUILD
#define CHECK(call)                                                                          \
    do {                                                                                     \
        const hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                              \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                       \
            return 3;                                                                        \
        }                                                                                    \
    } while (0)
// record i by the lanes of workgroup i % gridDim.x, one launch per record (the launches of a stream run in order): the additions cross workgroups
__global__ void __launch_bounds__(64) k_counter_add(In rec, uint32_t *counters) {
    if (threadIdx.x < kLanes / gridDim.x) counter_add_lane(rec, blockIdx.x * (kLanes / gridDim.x) + threadIdx.x, counters);
}
static int run(const std::vector<In> &in, std::vector<Out> &out) {
    uint32_t *d_counters = nullptr;
    CHECK(hipMalloc(&d_counters, kCounters * 4u));
    CHECK(hipMemset(d_counters, 0, kCounters * 4u));
    for (size_t i = 0; i < in.size(); ++i) {
        k_counter_add<<<i & 1u ? 4 : 1, 64>>>(in[i], d_counters);      // one workgroup of 64 lanes, or four of 16
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(out[i].r, d_counters, kCounters * 4u, hipMemcpyDeviceToHost));
    }
    CHECK(hipFree(d_counters));
    return 0;
}
#else
static int run(const std::vector<In> &in, std::vector<Out> &out) {
    uint32_t *counters = (uint32_t *)calloc(kCounters, 4);             // at exactly their size, so that the sanitizer sees a word beside them
    for (size_t i = 0; i < in.size(); ++i) {
        for (uint32_t lane = 0; lane < kLanes; ++lane) counter_add_lane(in[i], lane, counters);
        for (uint32_t w = 0; w < kCounters; ++w) out[i].r[w] = counters[w];
    }
    free(counters);
    return 0;
}
#endif

int main(int argc, char **argv) {
    if (argc != 3) return fprintf(stderr, "usage: counter_trial <inputs> <results>\n"), 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 2;
    std::vector<In> in;
    In rec;
    while (fread(&rec, sizeof rec, 1, f) == 1) in.push_back(rec);
    fclose(f);
    std::vector<Out> out(in.size(), Out{{0u, 0u, 0u, 0u}});
    if (const int rc = run(in, out)) return rc;
    f = fopen(argv[2], "wb");
    if (!f) return perror(argv[2]), 2;
    const bool ok = fwrite(out.data(), sizeof(Out), out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? (printf("%zu records\n", in.size()), 0) : 2;
}
