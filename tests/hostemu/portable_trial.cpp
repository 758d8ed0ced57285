// portable_trial.cpp -- TEST-ONLY: every primitive of reseq_amd/csrc/rsq_portable.h evaluated over a table of inputs, the results written to a file.
//   portable_trial <inputs> <results>
// One source, two programs.  Built by a host compiler (tests/test_portable.py: g++ with -fsanitize=address,undefined) it runs the host forms, and the test
// compares every result with a definition of its own.  Built by hipcc for the library's architecture (tests/test_portable_gpu.py) it runs the device forms in
// one kernel of one workgroup, and the test requires the host program's results, word for word.
// <inputs>: records of eight words (operation, six arguments, a spare); <results>: four words per record.  The table is tests/portable_table.py's.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_portable.h"

using namespace rsq;

enum Op : uint32_t {
    kBaseLetters, kComplementLetters, kBamNibbles, kPermBytes, kByteReverse, kBamPack, kAlignBytes, kBytesAt,      // bytes
    kDivSmall, kPopcount64, kLowestSetBit64, kBitReverse32, kBitReverse64, kClampFromZero,                         // integers
    kFma2, kFma1, kMulAdd2,                                                                                        // single precision
    kLoad64Align1, kLoad64Align2, kLoad128Align2, kLoad32Align1, kLoad32Align4, kLoad64Align1Lds,                  // loads from the 64-byte buffers
    kStore64Align1, kImageOr, kWaveAny,                                                                            // those with a state or a wave: in the table's order
    kOps
};
struct In {
    uint32_t op, a[6], spare;
};
struct Out {
    uint32_t r[4];
};
struct __attribute__((packed, aligned(2))) Eight {      // as FragmentSrc::rate_total has it (rsq_reads.h)
    uint64_t a, b;
};
constexpr uint32_t kBufBytes = 64, kImageWords = 4, kLanes = 64;
RSQ_HD uint8_t buf_byte(uint32_t i) { return (uint8_t)(i * 37u + 11u); }      // what the buffers hold
RSQ_HD float as_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
RSQ_HD uint32_t as_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
RSQ_HD Out out64(uint64_t x) { return Out{{(uint32_t)x, (uint32_t)(x >> 32), 0u, 0u}}; }
RSQ_HD bool is_pure(uint32_t op) { return op < kStore64Align1; }
RSQ_HD uint32_t rotate_left(uint32_t v, uint32_t n) { return (v << (n & 31u)) | (v >> ((32u - n) & 31u)); }

// bytes a record reads or writes in a buffer, and the alignment it promises; 0: none
inline uint32_t access_bytes(uint32_t op, uint32_t &align) {
    switch (op) {
    case kLoad64Align1: case kLoad64Align1Lds: case kStore64Align1: align = 1; return 8;
    case kLoad64Align2: align = 2; return 8;
    case kLoad128Align2: align = 2; return 16;
    case kLoad32Align1: align = 1; return 4;
    case kLoad32Align4: align = 4; return 4;
    default: align = 1; return 0;
    }
}

// a record without a state: buf and lds are kBufBytes bytes of buf_byte
RSQ_HD Out eval_pure(const In &in, const uint8_t *buf, const RSQ_LDS uint8_t *lds) {
    const uint32_t *a = in.a;
    const uint64_t x = ((uint64_t)a[1] << 32) | a[0];
    Float2 p, q, s;
    p.x = as_float(a[0]), p.y = as_float(a[1]), q.x = as_float(a[2]), q.y = as_float(a[3]), s.x = as_float(a[4]), s.y = as_float(a[5]);
    switch (in.op) {
    case kBaseLetters: return Out{{base_letters(a[0]), 0u, 0u, 0u}};
    case kComplementLetters: return Out{{sam_complement_letters(a[0]), 0u, 0u, 0u}};
    case kBamNibbles: return Out{{bam_nibbles(a[0], a[1] != 0u), 0u, 0u, 0u}};
    case kPermBytes: return Out{{perm_bytes(a[0], a[1], a[2]) & ~a[3], 0u, 0u, 0u}};      // a[3]: the bytes whose selector is outside the contract
    case kByteReverse: return Out{{sam_byte_reverse(a[0]), 0u, 0u, 0u}};
    case kBamPack: return Out{{bam_pack(a[0], a[1]), 0u, 0u, 0u}};
    case kAlignBytes: return Out{{align_bytes(a[0], a[1], a[2]), 0u, 0u, 0u}};
    case kBytesAt: return Out{{bytes_at(a[0], a[1], a[2]), 0u, 0u, 0u}};
    case kDivSmall: return Out{{div_small(a[0], a[1]), 0u, 0u, 0u}};
    case kPopcount64: return Out{{popcount64(x), 0u, 0u, 0u}};
    case kLowestSetBit64: return Out{{lowest_set_bit64(x), 0u, 0u, 0u}};
    case kBitReverse32: return Out{{bit_reverse32(a[0]), 0u, 0u, 0u}};
    case kBitReverse64: return out64(bit_reverse64(x));
    case kClampFromZero: return Out{{(uint32_t)clamp_from_zero((int32_t)a[0], (int32_t)a[1]), 0u, 0u, 0u}};
    case kFma2: {
        const Float2 r = fma2(p, q, s);
        return Out{{as_bits(r.x), as_bits(r.y), 0u, 0u}};
    }
    case kFma1: return Out{{as_bits(fma1(p.x, q.x, s.x)), 0u, 0u, 0u}};
    case kMulAdd2: {                                   // Float2's own operators: two roundings (the programs are built with -ffp-contract=off, like everything that includes the header)
        const Float2 r = p * q + s;
        return Out{{as_bits(r.x), as_bits(r.y), 0u, 0u}};
    }
    case kLoad64Align1: return out64(load_as<uint64_t, 1>(buf + a[0]));
    case kLoad64Align2: return out64(load_as<uint64_t, 2>(buf + a[0]));
    case kLoad128Align2: {
        const Eight e = load_as<Eight, 2>(buf + a[0]);
        return Out{{(uint32_t)e.a, (uint32_t)(e.a >> 32), (uint32_t)e.b, (uint32_t)(e.b >> 32)}};
    }
    case kLoad32Align1: return Out{{load_as<uint32_t, 1>(buf + a[0]), 0u, 0u, 0u}};
    case kLoad32Align4: return Out{{load_as<uint32_t, 4>(buf + a[0]), 0u, 0u, 0u}};
    case kLoad64Align1Lds: return out64(load_as<uint64_t, 1>(lds + a[0]));
    default: return Out{{0xDEADBEEFu, in.op, 0u, 0u}};
    }
}
// kStore64Align1: the word (a[1], a[2]) stored at byte a[0] of the zeroed scratch buffer -> the eight bytes there, and the sum of all the buffer's bytes
RSQ_HD Out eval_store(const In &in, uint8_t *scratch) {
    store_as<uint64_t, 1>(scratch + in.a[0], ((uint64_t)in.a[2] << 32) | in.a[1]);
    uint64_t back = 0;
    uint32_t sum = 0;
    for (uint32_t j = 0; j < 8u; ++j) back |= (uint64_t)scratch[in.a[0] + j] << (8u * j);
    for (uint32_t j = 0; j < kBufBytes; ++j) sum += scratch[j], scratch[j] = 0;
    return Out{{(uint32_t)back, (uint32_t)(back >> 32), sum, 0u}};
}
// kImageOr: lane l of 64 ORs a[1] rotated left by l into word (a[0] + l) % 4 of the image (which keeps what earlier records left) -> the image afterwards
RSQ_HD void image_or_lane(const In &in, uint32_t lane, RSQ_LDS uint32_t *image) { image_or(image + ((in.a[0] + lane) & (kImageWords - 1u)), rotate_left(in.a[1], lane)); }
// kWaveAny: lanes 0 .. a[2] - 1 are there, lane l with the predicate bit l of (a[1] : a[0]) -> what wave_any tells lane 0

#if RSQ_DEVICE_BUILD
#define CHECK(call)                                                                          \
    do {                                                                                     \
        const hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                              \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                       \
            return 3;                                                                        \
        }                                                                                    \
    } while (0)
__global__ void __launch_bounds__(256) k_portable(const In *in, Out *out, uint32_t n, const uint8_t *buf, uint8_t *scratch) {
    __shared__ uint64_t s_lds[kBufBytes / 8u];
    __shared__ uint32_t s_image[kImageWords];
    RSQ_LDS uint8_t *lds = (RSQ_LDS uint8_t *)s_lds;
    RSQ_LDS uint32_t *image = (RSQ_LDS uint32_t *)s_image;
    const uint32_t tid = threadIdx.x;
    if (tid < kBufBytes) lds[tid] = buf_byte(tid);
    if (tid < kImageWords) image[tid] = 0u;
    __syncthreads();
    for (uint32_t i = 0; i < n; ++i) {                                   // in.op is the same for every thread: the barriers below are met by all
        const In rec = in[i];
        if (is_pure(rec.op)) {
            if (i % blockDim.x == tid) out[i] = eval_pure(rec, buf, lds);
        } else if (rec.op == kStore64Align1) {
            if (tid == 0u) out[i] = eval_store(rec, scratch);
        } else if (rec.op == kImageOr) {
            if (tid < kLanes) image_or_lane(rec, tid, image);
            __syncthreads();
            if (tid < kImageWords) out[i].r[tid] = image[tid];
            __syncthreads();
        } else if (rec.op == kWaveAny) {
            if (tid < rec.a[2]) {                                        // a[2] <= 64: part of the first wave
                const bool p = ((((uint64_t)rec.a[1] << 32) | rec.a[0]) >> tid) & 1u;
                const bool any = wave_any(p);
                if (tid == 0u) out[i] = Out{{any ? 1u : 0u, 0u, 0u, 0u}};
            }
        }
    }
}
static int run(const std::vector<In> &in, std::vector<Out> &out) {
    uint8_t pattern[kBufBytes];
    for (uint32_t i = 0; i < kBufBytes; ++i) pattern[i] = buf_byte(i);
    In *d_in = nullptr;
    Out *d_out = nullptr;
    uint8_t *d_buf = nullptr, *d_scratch = nullptr;
    CHECK(hipMalloc(&d_in, in.size() * sizeof(In)));
    CHECK(hipMalloc(&d_out, in.size() * sizeof(Out)));
    CHECK(hipMalloc(&d_buf, kBufBytes));
    CHECK(hipMalloc(&d_scratch, kBufBytes));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * sizeof(In), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0, in.size() * sizeof(Out)));
    CHECK(hipMemcpy(d_buf, pattern, kBufBytes, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_scratch, 0, kBufBytes));
    k_portable<<<1, 256>>>(d_in, d_out, (uint32_t)in.size(), d_buf, d_scratch);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, in.size() * sizeof(Out), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_buf));
    CHECK(hipFree(d_scratch));
    return 0;
}
#else
static int run(const std::vector<In> &in, std::vector<Out> &out) {
    // the buffers at exactly their size, so that the sanitizer sees a byte read or written beside them
    uint8_t *buf = (uint8_t *)malloc(kBufBytes), *lds = (uint8_t *)malloc(kBufBytes), *scratch = (uint8_t *)calloc(kBufBytes, 1);
    uint32_t *image = (uint32_t *)calloc(kImageWords, 4);
    for (uint32_t i = 0; i < kBufBytes; ++i) buf[i] = lds[i] = buf_byte(i);
    for (size_t i = 0; i < in.size(); ++i) {
        const In &rec = in[i];
        if (is_pure(rec.op)) out[i] = eval_pure(rec, buf, lds);
        else if (rec.op == kStore64Align1) out[i] = eval_store(rec, scratch);
        else if (rec.op == kImageOr) {
            for (uint32_t lane = 0; lane < kLanes; ++lane) image_or_lane(rec, lane, image);
            for (uint32_t w = 0; w < kImageWords; ++w) out[i].r[w] = image[w];
        } else if (rec.op == kWaveAny) {                                 // the host's wave is one lane: the lanes in turn, any of them
            bool any = false;
            for (uint32_t lane = 0; lane < rec.a[2]; ++lane) any = any || wave_any(((((uint64_t)rec.a[1] << 32) | rec.a[0]) >> lane) & 1u);
            out[i] = Out{{any ? 1u : 0u, 0u, 0u, 0u}};
        }
    }
    free(buf), free(lds), free(scratch), free(image);
    return 0;
}
#endif

int main(int argc, char **argv) {
    if (argc != 3) return fprintf(stderr, "usage: portable_trial <inputs> <results>\n"), 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 2;
    std::vector<In> in;
    In rec;
    while (fread(&rec, sizeof rec, 1, f) == 1) in.push_back(rec);
    fclose(f);
    // nothing outside the buffers is touched, whatever the table says: checked here, before anything runs
    for (size_t i = 0; i < in.size(); ++i) {
        uint32_t align = 1;
        const uint32_t bytes = access_bytes(in[i].op, align);
        const bool bad = in[i].op >= kOps || (bytes && (in[i].a[0] > kBufBytes - bytes || in[i].a[0] % align)) || (in[i].op == kWaveAny && (in[i].a[2] < 1u || in[i].a[2] > kLanes));
        if (bad) return fprintf(stderr, "record %zu: operation %u with argument %u is outside what this program runs\n", i, in[i].op, in[i].a[0]), 2;
    }
    std::vector<Out> out(in.size(), Out{{0u, 0u, 0u, 0u}});
    if (const int rc = run(in, out)) return rc;
    f = fopen(argv[2], "wb");
    if (!f) return perror(argv[2]), 2;
    const bool ok = fwrite(out.data(), sizeof(Out), out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? (printf("%zu records\n", in.size()), 0) : 2;
}
