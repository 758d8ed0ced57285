// xor3_trial.cpp -- TEST-ONLY: xor3 and RSQ_KEEP_IN_SGPR of reseq_amd/csrc/rsq_portable.h (what Philox's rounds are made of, rsq_core.h) evaluated over a table of
// inputs, the results written to a file -- portable_trial.cpp's scheme for these two.
//   xor3_trial <inputs> <results>
// One source, two programs.  Built by a host compiler (tests/test_portable_xor3.py: g++ with -fsanitize=address,undefined) it runs the host forms; built by hipcc
// for the library's architecture it runs the device forms, and the test requires of both the words its own definition gives.
// <inputs>: records of three words (a, b, c).  <results>: for every number of active lanes of kLanes in turn, for every record, for every active lane l four words:
//   xor3(a + l, b ^ l * 0x01000193, c rotated left by l)      -- lane 0 has the record's own triple
//   a passed through RSQ_KEEP_IN_SGPR                         -- wave-uniform on the device: the record is the kernel's argument-addressed, lane-independent load
//   a passed through it four times with 0x9E3779B9 added behind each pass (the form of Philox's round keys)
//   l
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_portable.h"

using namespace rsq;

struct In {
    uint32_t a, b, c;
};
struct Out {
    uint32_t r[4];
};
constexpr uint32_t kLanes[] = {1u, 63u, 64u, 65u}, kBlock = 128u;      // whole and partial waves; 65: a second wave with one lane
RSQ_HD uint32_t rotate_left(uint32_t v, uint32_t n) { return (v << (n & 31u)) | (v >> ((32u - n) & 31u)); }
RSQ_HD Out trial(const In &in, uint32_t lane) {
    uint32_t kept = in.a, chain = in.a;
    RSQ_KEEP_IN_SGPR(kept);
    for (int r = 0; r < 4; ++r) {
        RSQ_KEEP_IN_SGPR(chain);
        chain += 0x9E3779B9u;
    }
    return Out{{xor3(in.a + lane, in.b ^ (lane * 0x01000193u), rotate_left(in.c, lane)), kept, chain, lane}};
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
// one workgroup; the first `lanes` threads are active and walk all records: out[(i * lanes + l)]
__global__ void __launch_bounds__(kBlock) k_xor3(const In *__restrict__ in, uint32_t n, uint32_t lanes, Out *__restrict__ out) {
    if (threadIdx.x >= lanes) return;
    for (uint32_t i = 0; i < n; ++i) out[(size_t)i * lanes + threadIdx.x] = trial(in[i], threadIdx.x);
}
static int run(const std::vector<In> &in, uint32_t lanes, Out *out) {
    In *d_in = nullptr;
    Out *d_out = nullptr;
    const size_t n_out = in.size() * lanes;
    CHECK(hipMalloc(&d_in, in.size() * sizeof(In)));
    CHECK(hipMalloc(&d_out, n_out * sizeof(Out)));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * sizeof(In), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xA5, n_out * sizeof(Out)));
    k_xor3<<<1, kBlock>>>(d_in, (uint32_t)in.size(), lanes, d_out);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(out, d_out, n_out * sizeof(Out), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    return 0;
}
#else
static int run(const std::vector<In> &in, uint32_t lanes, Out *out) {
    for (size_t i = 0; i < in.size(); ++i)
        for (uint32_t lane = 0; lane < lanes; ++lane) out[i * lanes + lane] = trial(in[i], lane);
    return 0;
}
#endif

int main(int argc, char **argv) {
    if (argc != 3) return fprintf(stderr, "usage: xor3_trial <inputs> <results>\n"), 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 2;
    std::vector<In> in;
    In rec;
    while (fread(&rec, sizeof rec, 1, f) == 1) in.push_back(rec);
    fclose(f);
    if (in.empty()) return fprintf(stderr, "no records\n"), 2;
    f = fopen(argv[2], "wb");
    if (!f) return perror(argv[2]), 2;
    bool ok = true;
    for (const uint32_t lanes : kLanes) {
        std::vector<Out> out(in.size() * lanes, Out{{0u, 0u, 0u, 0u}});      // at exactly their size, so that the sanitizer sees a word beside them
        if (const int rc = run(in, lanes, out.data())) return fclose(f), rc;
        ok = ok && fwrite(out.data(), sizeof(Out), out.size(), f) == out.size();
    }
    return fclose(f) == 0 && ok ? (printf("%zu records\n", in.size()), 0) : 2;
}
