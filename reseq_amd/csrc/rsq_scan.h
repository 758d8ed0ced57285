// rsq_scan.h -- the exclusive prefix sum the sieve and the record partition place their output by (library only):
//   k_scan_tile_sums, k_scan_tiles, k_scan_apply
#pragma once
#include "rsq_types.h"

namespace rsq {

#if RSQ_DEVICE_BUILD
// ------------------------------------------------------------------------------------------------ scans
// exclusive prefix sum of uint32 counts into uint64 offsets (n+1 entries: offsets[n] = total); three launches.
constexpr uint32_t kScanBlock = 256;
constexpr uint32_t kScanPer = 8;              // elements per thread
constexpr uint32_t kScanTile = kScanBlock * kScanPer;

__global__ void k_scan_tile_sums(const uint32_t *in, uint64_t n, uint64_t *tile_sums) {
    __shared__ uint64_t s[kScanBlock];
    uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer, acc = 0;
    for (uint32_t i = 0; i < kScanPer; ++i)
        if (base + i < n) acc += in[base + i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t d = kScanBlock / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = s[0];
}
// one workgroup: every thread adds up a stretch of tiles, the stretches' sums are scanned in LDS, then every thread turns its stretch into
// exclusive prefixes (tens of thousands of tiles for a batch of 10 M pairs: a single serial thread took a millisecond)
constexpr uint32_t kScanTilesBlock = 1024;
// `init`: what lies in front of the whole array (nullptr: 0) -- the offsets of a sub-range continue where the sub-range in front of it ended
__global__ void __launch_bounds__(kScanTilesBlock) k_scan_tiles(uint64_t *tile_sums, uint32_t n_tiles, uint64_t *total, const uint64_t *init) {
    __shared__ uint64_t s[kScanTilesBlock];
    const uint64_t first = init ? *init : 0u;
    const uint32_t per = (n_tiles + kScanTilesBlock - 1u) / kScanTilesBlock, lo = threadIdx.x * per, hi = lo + per < n_tiles ? lo + per : n_tiles;
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
    if (threadIdx.x == kScanTilesBlock - 1u) *total = first + s[threadIdx.x];
}
__global__ void k_scan_apply(const uint32_t *in, uint64_t n, const uint64_t *tile_sums, const uint64_t *total, uint64_t *out) {
    __shared__ uint64_t s[kScanBlock];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
    uint32_t v[kScanPer];
    uint64_t acc = 0;
    for (uint32_t i = 0; i < kScanPer; ++i) {
        v[i] = base + i < n ? in[base + i] : 0u;
        acc += v[i];
    }
    s[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t d = 1; d < kScanBlock; d <<= 1) {                 // Hillis-Steele inclusive scan of the per-thread sums
        uint64_t t = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    uint64_t run = tile_sums[blockIdx.x] + s[threadIdx.x] - acc;
    for (uint32_t i = 0; i < kScanPer; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = *total;
}
#endif

}  // namespace rsq
