// rsq_scan.h -- the exclusive prefix sum the sieve and the record partition place their output by (library only):
//   k_scan_tile_sums, k_scan_tiles, k_scan_apply, and scan_launch, the three launches of one scan
// tests/hostemu/kernel_trial.cpp runs these kernels alone, through scan_launch, on inputs no simulation makes (tests/test_kernel_trial_gpu.py).
#pragma once
#include "rsq_types.h"

namespace rsq {

#if RSQ_DEVICE_BUILD
// ------------------------------------------------------------------------------------------------ scans
// exclusive prefix sum of uint32 counts into uint64 offsets (n+1 entries: offsets[n] = total); three launches, which serve up to two arrays of the same
// length at once (grid.y: the two FASTQ files' record sizes of a call).
// A tile is 4096 elements, a wave's quarter of it four rounds of 256: in round k lane l holds the four elements from 256 k + 4 l on -- one 16-byte load where the
// array is aligned, a wave's loads and stores next to each other in memory.  Inside a wave the sums travel by shuffles; LDS carries four numbers per workgroup.
constexpr uint32_t kScanBlock = 256;
constexpr uint32_t kScanPer = 16;             // elements per thread
constexpr uint32_t kScanTile = kScanBlock * kScanPer;
constexpr uint32_t kScanRounds = kScanPer / 4u, kScanWaves = kScanBlock / 64u, kScanWaveSpan = 64u * kScanPer;

struct ScanArrays {                           // [1]: unused by a launch with grid.y == 1
    const uint32_t *in[2];
    uint64_t *out[2];                         // n + 1 offsets
    const uint64_t *init[2];                  // what lies in front of the whole array (nullptr: 0)
    uint64_t *total[2];
};

// four consecutive elements from `at` on, zero behind n; `aligned`: the array begins on a 16-byte boundary (`at` is a multiple of four)
__device__ __forceinline__ uint4 scan_load4(const uint32_t *in, uint64_t at, uint64_t n, bool aligned) {
    if (at + 4u <= n) {
        if (aligned) return *reinterpret_cast<const uint4 *>(in + at);
        return uint4{in[at], in[at + 1u], in[at + 2u], in[at + 3u]};
    }
    uint4 v{0u, 0u, 0u, 0u};
    if (at < n) v.x = in[at];
    if (at + 1u < n) v.y = in[at + 1u];
    if (at + 2u < n) v.z = in[at + 2u];
    return v;
}
__device__ __forceinline__ uint64_t scan_shfl_up(uint64_t v, uint32_t d) {
    return (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)v, d, 64) | ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64) << 32);
}
__device__ __forceinline__ uint64_t scan_shfl(uint64_t v, int from) {
    return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, from, 64) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), from, 64) << 32);
}
__device__ __forceinline__ uint64_t scan_shfl_xor(uint64_t v, uint32_t d) {
    return (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)v, (int)d, 64) | ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)d, 64) << 32);
}

// the tiles' sums, [array][tile]; `longest` (nullptr: not wanted): the largest element of all arrays, one atomic per workgroup
__global__ void __launch_bounds__(kScanBlock) k_scan_tile_sums(ScanArrays a, uint64_t n, uint64_t *tile_sums, uint32_t *longest) {
    __shared__ uint64_t s_sum[kScanWaves];
    __shared__ uint32_t s_max[kScanWaves];
    const uint32_t *in = a.in[blockIdx.y];
    const bool aligned = 0u == (reinterpret_cast<uintptr_t>(in) & 15u);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)wave * kScanWaveSpan + 4u * lane;
    uint64_t acc = 0;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanRounds; ++k) {
        const uint4 v = scan_load4(in, base + 256u * k, n, aligned);
        acc += (uint64_t)v.x + v.y + v.z + v.w;
        m = max(max(m, v.x), max(max(v.y, v.z), v.w));
    }
    for (uint32_t d = 32; d; d >>= 1) {
        acc += scan_shfl_xor(acc, d);
        m = max(m, (uint32_t)__shfl_xor((int)m, (int)d, 64));
    }
    if (0u == lane) {
        s_sum[wave] = acc;
        s_max[wave] = m;
    }
    __syncthreads();
    if (0u == threadIdx.x) {
        uint64_t sum = 0;
        uint32_t mx = 0;
        for (uint32_t w = 0; w < kScanWaves; ++w) {
            sum += s_sum[w];
            mx = max(mx, s_max[w]);
        }
        tile_sums[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
        if (longest && mx) atomicMax(longest, mx);
    }
}
// one workgroup per array: every thread adds up a stretch of tiles, the stretches' sums are scanned in LDS, then every thread turns its stretch into
// exclusive prefixes (thousands of tiles for a batch of 10 M pairs: a single serial thread took a millisecond)
constexpr uint32_t kScanTilesBlock = 1024;
__global__ void __launch_bounds__(kScanTilesBlock) k_scan_tiles(ScanArrays a, uint64_t *all_tile_sums, uint32_t n_tiles) {
    __shared__ uint64_t s[kScanTilesBlock];
    uint64_t *tile_sums = all_tile_sums + (uint64_t)blockIdx.x * n_tiles;
    const uint64_t *init = a.init[blockIdx.x];
    const uint64_t first = init ? *init : 0u;
    const uint32_t per = (n_tiles + kScanTilesBlock - 1u) / kScanTilesBlock, lo = min(threadIdx.x * per, n_tiles), hi = lo + per < n_tiles ? lo + per : n_tiles;
    uint64_t acc = 0;
    for (uint32_t i = lo; i < hi; ++i) acc += tile_sums[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t d = 1; d < kScanTilesBlock; d <<= 1) {              // inclusive scan of the stretches' sums
        const uint64_t v = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = first + s[threadIdx.x] - acc;                      // what lies in front of this thread's stretch
    for (uint32_t i = lo; i < hi; ++i) {
        const uint64_t v = tile_sums[i];
        tile_sums[i] = run;
        run += v;
    }
    if (threadIdx.x == kScanTilesBlock - 1u) *a.total[blockIdx.x] = first + s[threadIdx.x];
}
__global__ void __launch_bounds__(kScanBlock) k_scan_apply(ScanArrays a, uint64_t n, const uint64_t *tile_sums) {
    __shared__ uint64_t s_wave[kScanWaves];
    const uint32_t *in = a.in[blockIdx.y];
    uint64_t *out = a.out[blockIdx.y];
    const bool aligned = 0u == (reinterpret_cast<uintptr_t>(in) & 15u), out_aligned = 0u == (reinterpret_cast<uintptr_t>(out) & 15u);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)wave * kScanWaveSpan + 4u * lane;
    uint4 v[kScanRounds];
    uint64_t before[kScanRounds];                                   // of the wave's span: what lies in front of this lane's four elements of round k
    uint64_t run = 0;                                               // the rounds before
#pragma unroll
    for (uint32_t k = 0; k < kScanRounds; ++k) v[k] = scan_load4(in, base + 256u * k, n, aligned);
#pragma unroll
    for (uint32_t k = 0; k < kScanRounds; ++k) {
        const uint64_t mine = (uint64_t)v[k].x + v[k].y + v[k].z + v[k].w;
        uint64_t incl = mine;                                       // inclusive scan over the lanes
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t t = scan_shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        before[k] = run + incl - mine;
        run += scan_shfl(incl, 63);                                 // the round's sum, from the last lane
    }
    if (0u == lane) s_wave[wave] = run;                             // the span's sum (the same in every lane)
    __syncthreads();
    uint64_t front = tile_sums[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) front += s_wave[w];
#pragma unroll
    for (uint32_t k = 0; k < kScanRounds; ++k) {
        const uint64_t at = base + 256u * k;
        uint64_t o = front + before[k];
        if (at + 4u <= n && out_aligned) {                          // 32 bytes on a 16-byte boundary (`at` is a multiple of four)
            *reinterpret_cast<ulonglong2 *>(out + at) = ulonglong2{o, o + v[k].x};
            o += (uint64_t)v[k].x + v[k].y;
            *reinterpret_cast<ulonglong2 *>(out + at + 2u) = ulonglong2{o, o + v[k].z};
        } else {
            if (at < n) out[at] = o;
            o += v[k].x;
            if (at + 1u < n) out[at + 1u] = o;
            o += v[k].y;
            if (at + 2u < n) out[at + 2u] = o;
            o += v[k].z;
            if (at + 3u < n) out[at + 3u] = o;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = *a.total[blockIdx.y];
}
// The three launches of a scan of `arrays` (1 or 2) arrays of n elements each: a.total[0 .. arrays) are set, tile_sums has arrays * (tiles + 1) words with
// tiles = ceil(n / kScanTile), longest as in k_scan_tile_sums.  n >= 1: a grid of no tiles is not launched, so out[0] and *total would stay unwritten.
inline void scan_launch(const ScanArrays &a, uint32_t arrays, uint64_t n, uint64_t *tile_sums, hipStream_t st, uint32_t *longest) {
    const uint32_t tiles = (uint32_t)((n + kScanTile - 1u) / kScanTile);
    hipLaunchKernelGGL(k_scan_tile_sums, dim3(tiles, arrays), dim3(kScanBlock), 0, st, a, n, tile_sums, longest);
    hipLaunchKernelGGL(k_scan_tiles, dim3(arrays), dim3(kScanTilesBlock), 0, st, a, tile_sums, tiles);
    hipLaunchKernelGGL(k_scan_apply, dim3(tiles, arrays), dim3(kScanBlock), 0, st, a, n, (const uint64_t *)tile_sums);
}
#endif

}  // namespace rsq
