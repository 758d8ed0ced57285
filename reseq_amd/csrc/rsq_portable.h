// rsq_portable.h -- everything that differs between the builds of the kernels' headers, and nothing else.
//
// The headers serve four settings: hipcc's device pass (the library's kernels), hipcc's host pass, hiprtc (a read kernel compiled at run time for one profile,
// rsq_spec.h: device pass only, no C library headers) and a host compiler (tests/hostemu: the kernels' own RSQ_HD functions run on the CPU against the oracle).
// The host emulation is only sound if every function that does one thing on the device and another on the host does the SAME thing in both places.  Those
// functions all live here, each with its domain stated and -- on the host -- asserted; tests/hostemu/portable_trial.cpp runs every one of them over a fixed table
// of inputs on the host (tests/test_portable.py: against definitions written in the test) and on the device (tests/test_portable_gpu.py: word for word the
// host's results).  The other headers name neither build: they call these.
#pragma once
#if defined(__HIPCC_RTC__)
// hiprtc's built-in header has the fixed-width types and the device's math
using __hip_internal::int32_t;
using __hip_internal::int64_t;
using __hip_internal::uint16_t;
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
using __hip_internal::uint8_t;
typedef unsigned long uintptr_t;
#define RSQ_DEVICE_BUILD 1
#define RSQ_HD __host__ __device__ __forceinline__
#elif defined(__HIPCC__)
#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <hip/hip_runtime.h>
#define RSQ_DEVICE_BUILD 1
#define RSQ_HD __host__ __device__ __forceinline__
#else
#include <assert.h>
#include <math.h>
#include <stdint.h>
#define RSQ_DEVICE_BUILD 0
#define RSQ_HD inline
#endif

// RSQ_DEVICE_BUILD: the compiler knows __global__ (it fences off the kernels).  RSQ_ON_DEVICE: this pass makes device code (it chooses between a builtin and its
// host form, below and nowhere else but for the host-only counters of rsq_reads.h).
#if defined(__HIP_DEVICE_COMPILE__)
#define RSQ_ON_DEVICE 1
#else
#define RSQ_ON_DEVICE 0
#endif
// the device pass of a compiler that knows v_bitop3_b32, for a target that has it (xor3 below; every other build takes the plain form)
#define RSQ_HAS_BITOP3 0
#if RSQ_ON_DEVICE && defined(__gfx950__) && defined(__has_builtin)
#if __has_builtin(__builtin_amdgcn_bitop3_b32)
#undef RSQ_HAS_BITOP3
#define RSQ_HAS_BITOP3 1
#endif
#endif

// ------------------------------------------------------------------------------------------------ attributes and macros
#if RSQ_ON_DEVICE
#define RSQ_LDS __attribute__((address_space(3)))                // a pointer into the workgroup's LDS (ds_ instructions, 32-bit addresses); the host: plain memory
#define RSQ_NOINLINE __device__ __noinline__                     // a function that stays a call
#define RSQ_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)    // the instruction scheduler moves nothing across
#define RSQ_KEEP_IN_VGPR(x) asm volatile("" : "+v"(x))           // the value is formed here, in a vector register: the compiler folds it into nothing earlier
#define RSQ_KEEP_IN_SGPR(x) asm volatile("" : "+s"(x))           // the same for a WAVE-UNIFORM 32-bit value, in a scalar register: what is computed from it is computed behind this point, not ahead of the loop
#define RSQ_UNROLL _Pragma("unroll")                           // where only the device wants the loop unrolled
#define RSQ_DOMAIN(cond) ((void)0)
#else
#define RSQ_LDS
#define RSQ_NOINLINE inline
#define RSQ_SCHED_BARRIER() ((void)0)
#define RSQ_KEEP_IN_VGPR(x) ((void)0)
#define RSQ_KEEP_IN_SGPR(x) ((void)0)
#define RSQ_UNROLL
#define RSQ_DOMAIN(cond) assert(cond)                            // the stated domain of a primitive: outside it the two builds may differ
#endif

namespace rsq {

// ------------------------------------------------------------------------------------------------ any lane of the wave
// true if the predicate holds for any lane of the wave that is here (the host: the caller's own): a wave-uniform branch around work that no lane needs.  The
// wave's ballot of a predicate is the compare's own result (s_and with exec), where __any() takes an int.  (The read kernel's loops had the ballot as a macro, the
// text writers __any() as image_any: the compiler makes the same instructions of both in every kernel -- DESIGN_LOG.md section 25 -- so there is one form.)
RSQ_HD bool wave_any(bool p) {
#if RSQ_ON_DEVICE
    return __builtin_amdgcn_ballot_w64(p) != 0ull;
#else
    return p;
#endif
}

// ------------------------------------------------------------------------------------------------ bytes
// v_perm_b32: byte k of the result is byte s of the eight bytes (hi : lo), s = byte k of `sel`; lo holds bytes 0-3, hi bytes 4-7.
// Domain, byte by byte: s = 0..7.  A selector byte outside it spoils byte k of the result and no other (the instruction gives 8..15 meanings of their own -- sign
// bytes and constants -- which nothing here relies on; the host form gives 0).  That cannot be an assertion: the selectors of the table lookups below are DATA, and
// a row's last word carries whatever lies behind its last code, which the callers mask out of the result (tests/hostemu/text_trial.cpp fills it with 0xA5).
RSQ_HD uint32_t perm_bytes(uint32_t hi, uint32_t lo, uint32_t sel) {
#if RSQ_ON_DEVICE
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t s = (sel >> (8u * k)) & 0xFFu;
        if (s < 8u) out |= ((uint32_t)(both >> (8u * s)) & 0xFFu) << (8u * k);
    }
    return out;
#endif
}
// v_alignbyte_b32: the four bytes of (hi : lo) from byte n on, i.e. (hi : lo) >> 8 n.  Domain: n = 0..3 (the instruction takes n modulo 4).
RSQ_HD uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t n) {
#if RSQ_ON_DEVICE
    return __builtin_amdgcn_alignbyte(hi, lo, n);
#else
    RSQ_DOMAIN(n < 4u);
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * n));
#endif
}
// the same up to a whole word: at = 0..4 (4: hi itself).  One byte permute whose selector depends on `at` alone (a caller with a fixed phase computes it once).
RSQ_HD uint32_t bytes_at(uint32_t hi, uint32_t lo, uint32_t at) {
    RSQ_DOMAIN(at <= 4u);
    return perm_bytes(hi, lo, 0x03020100u + at * 0x01010101u);
}
// What the text and BAM writers make of them.  Four base codes, one per byte (0..3 ACGT, 4 N; domain 0..7 byte by byte, 5..7 are N as well), become
RSQ_HD uint32_t base_letters(uint32_t codes) { return perm_bytes(0x4E4E4E4Eu, 0x54474341u, codes); }                  // the letters "ACGT", 'N'
RSQ_HD uint32_t sam_complement_letters(uint32_t codes) { return perm_bytes(0x4E4E4E4Eu, 0x41434754u, codes); }        // the complements' letters "TGCA", 'N'
RSQ_HD uint32_t bam_nibbles(uint32_t codes, bool complement) { return perm_bytes(0x0F0F0F0Fu, complement ? 0x01020408u : 0x08040201u, codes); }      // BAM's 4-bit codes (N: 15), of the bases or of their complements
RSQ_HD uint32_t sam_byte_reverse(uint32_t w) { return perm_bytes(0u, w, 0x00010203u); }
// eight 4-bit codes, one per byte of (n1 : n0) -> four bytes, the earlier code of a pair in the high nibble
RSQ_HD uint32_t bam_pack(uint32_t n0, uint32_t n1) {
    const uint32_t x0 = (n0 << 4) | (n0 >> 8), x1 = (n1 << 4) | (n1 >> 8);      // bytes 0 and 2 hold the pairs (0, 1) and (2, 3)
    return perm_bytes(x1, x0, 0x06040200u);
}

// ------------------------------------------------------------------------------------------------ bits
RSQ_HD uint32_t popcount64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
RSQ_HD uint32_t lowest_set_bit64(uint64_t x) {                   // index of the lowest set bit.  Domain: x != 0
    RSQ_DOMAIN(x != 0ull);
    return (uint32_t)__builtin_ctzll(x);
}
// bit k of the result is bit 31 - k (63 - k) of x
RSQ_HD uint32_t bit_reverse32(uint32_t x) {
#if defined(__clang__)
    return __builtin_bitreverse32(x);
#else
    uint32_t r = 0;
    for (uint32_t i = 0; i < 32u; ++i) r |= ((x >> i) & 1u) << (31u - i);
    return r;
#endif
}
RSQ_HD uint64_t bit_reverse64(uint64_t x) {
#if defined(__clang__)
    return __builtin_bitreverse64(x);
#else
    return ((uint64_t)bit_reverse32((uint32_t)x) << 32) | bit_reverse32((uint32_t)(x >> 32));
#endif
}
// a ^ b ^ c: one v_bitop3_b32 (truth table 0x96, three-input parity) where the target has it -- the compiler pairs the xors up into two instructions by itself.  Any
// words.  (Its table and its two programs are its own: tests/hostemu/xor3_trial.cpp, tests/test_portable_xor3.py, with RSQ_KEEP_IN_SGPR.)
RSQ_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if RSQ_HAS_BITOP3
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96u);
#else
    return a ^ b ^ c;
#endif
}
// min(max(d, 0), last): d held between 0 and last >= 0 (a median of three on the device)
RSQ_HD int32_t clamp_from_zero(int32_t d, int32_t last) {
#if defined(__clang__)
    return __builtin_elementwise_min(__builtin_elementwise_max(d, 0), last);
#else
    const int32_t low = d < 0 ? 0 : d;
    return low < last ? low : last;
#endif
}

// ------------------------------------------------------------------------------------------------ loads and stores below the type's alignment
// A T at an address that is a multiple of ALIGN only (ALIGN <= alignof(T); T trivially copyable).  The device does such a load with one instruction (amdhsa:
// unaligned access is on), the host copies the bytes.  Domain: p is a multiple of ALIGN.  The second pair: the same from and to LDS.
template <class T, uint32_t ALIGN>
RSQ_HD T load_as(const void *p) {
#if RSQ_ON_DEVICE
    typedef T __attribute__((aligned(ALIGN))) Under;
    return *reinterpret_cast<const Under *>(p);
#else
    RSQ_DOMAIN((uintptr_t)p % ALIGN == 0u);
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
#endif
}
template <class T, uint32_t ALIGN>
RSQ_HD void store_as(void *p, const T &v) {
#if RSQ_ON_DEVICE
    typedef T __attribute__((aligned(ALIGN))) Under;
    *reinterpret_cast<Under *>(p) = v;
#else
    RSQ_DOMAIN((uintptr_t)p % ALIGN == 0u);
    __builtin_memcpy(p, &v, sizeof(T));
#endif
}
#if RSQ_ON_DEVICE
template <class T, uint32_t ALIGN>
RSQ_HD T load_as(const RSQ_LDS void *p) {
    typedef T __attribute__((aligned(ALIGN))) Under;
    return *reinterpret_cast<const RSQ_LDS Under *>(p);
}
#endif
// v ORed into a word of a zeroed image in LDS that other lanes OR into as well (rsq_format.h): ds_or_b32 without return.  The host: one lane at a time.
RSQ_HD void image_or(RSQ_LDS uint32_t *w, uint32_t v) {
#if RSQ_ON_DEVICE
    __hip_atomic_fetch_or(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    store_as<uint32_t, 1>(w, load_as<uint32_t, 1>(w) | v);
#endif
}

// v added modulo 2^32 to a counter in device memory that lanes of any workgroup add to as well (rsq_depth.h): a global atomic add whose result nobody reads.  The
// host: one lane at a time.  Domain: p is a multiple of four.  (Its table and its two programs are its own: tests/hostemu/counter_trial.cpp,
// tests/test_portable_counter.py -- the host form against the meaning stated here, the device form word for word the same.)
RSQ_HD void counter_add(uint32_t *p, uint32_t v) {
#if RSQ_ON_DEVICE
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    RSQ_DOMAIN((uintptr_t)p % 4u == 0u);
    *p += v;
#endif
}

// ------------------------------------------------------------------------------------------------ arithmetic
// x / d. Domain: x < 2^24, 1 <= d, a quotient below 2^17 (the percentages: at most 65535 + d / 2 over d).  The device has no integer division: the compiler's
// sequence for a 32-bit one is about 28 instructions.  Here: both operands are exact in single precision, the product with the reciprocal (1 ulp) is off by less than
// 2^17 * 2^-22 of the true quotient, so its integer part is the quotient or one beside it, and the remainder says which.
RSQ_HD uint32_t div_small(uint32_t x, uint32_t d) {
#if RSQ_ON_DEVICE
    uint32_t q = (uint32_t)((float)x * __builtin_amdgcn_rcpf((float)d));
    const int32_t r = (int32_t)(x - q * d);
    if (r < 0) --q;
    else if ((uint32_t)r >= d) ++q;
    return q;
#else
    RSQ_DOMAIN(x < (1u << 24) && d >= 1u && x / d < (1u << 17));
    return x / d;
#endif
}
// a pair of floats: v_pk_mul_f32 / v_pk_add_f32 on the device
#if RSQ_ON_DEVICE
typedef float Float2 __attribute__((ext_vector_type(2)));
#else
struct Float2 {
    float x, y;
};
inline Float2 operator*(const Float2 &a, const Float2 &b) { return Float2{a.x * b.x, a.y * b.y}; }
inline Float2 operator+(const Float2 &a, const Float2 &b) { return Float2{a.x + b.x, a.y + b.y}; }
#endif
// a * b + c with one rounding: v_pk_fma_f32 / v_fma_f32 on the device, the correctly rounded fmaf on the host (the emulation decides as the device does).  The
// headers are built with -ffp-contract=off, so a multiply and an add written apart stay apart in every build.
RSQ_HD Float2 fma2(const Float2 &a, const Float2 &b, const Float2 &c) {
#if RSQ_ON_DEVICE
    return __builtin_elementwise_fma(a, b, c);
#else
    return Float2{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y)};
#endif
}
RSQ_HD float fma1(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

}  // namespace rsq
