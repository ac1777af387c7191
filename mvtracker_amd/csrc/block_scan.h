// The order-preserving compaction's scan (mvt_query_pool in query_sample.hip, mvt_voxel_emit in cloud_prep.hip): count per
// workgroup, THIS scan over the counts in one workgroup, scatter.  Integer arithmetic throughout, so the prefix is the same in any
// order of addition.
#pragma once
#include "common.h"

namespace {

constexpr int SCAN_WG = 256;  // threads of the one workgroup (4 waves)

// Exclusive prefix sum of v over the SCAN_WG threads of the workgroup (thread order); total = the sum of all.  lds: 4 words.
__device__ __forceinline__ unsigned long long wg_excl_scan_u64(unsigned long long v, unsigned long long* lds, unsigned long long& total) {
  typedef unsigned long long u64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    unsigned lo = __shfl_up((unsigned)inc, o, 64), hi = __shfl_up((unsigned)(inc >> 32), o, 64);
    if (lane >= o) inc += ((u64)hi << 32) | lo;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  u64 woff = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < SCAN_WG / 64; ++w) {
    if (w < wave) woff += lds[w];
    total += lds[w];
  }
  __syncthreads();  // lds may be reused at once
  return woff + inc - v;
}

// One workgroup of SCAN_WG threads: block_counts[nb] -> exclusive prefix in place, the total to *count.  Thread t owns the contiguous
// chunk [t * chunk, (t + 1) * chunk), chunk = ceil(nb / SCAN_WG).  The body of each file's own __global__ kernel.
__device__ __forceinline__ void block_counts_scan(int* __restrict__ block_counts, int nb, int chunk, int* __restrict__ count) {
  typedef unsigned long long u64;
  __shared__ u64 s_scan[SCAN_WG / 64];
  const int b0 = threadIdx.x * chunk;  // (< nb + SCAN_WG, and nb = ceil(P / 256) < 2^23 for the P < 2^31 both entries take)
  u64 sum = 0;
  for (int j = 0; j < chunk; ++j)
    if (b0 + j < nb) sum += (u64)block_counts[b0 + j];
  u64 total;
  u64 off = wg_excl_scan_u64(sum, s_scan, total);
  for (int j = 0; j < chunk; ++j)
    if (b0 + j < nb) {
      const int c = block_counts[b0 + j];
      block_counts[b0 + j] = (int)off;
      off += (u64)c;
    }
  if (threadIdx.x == 0) *count = (int)total;
}

}  // namespace
