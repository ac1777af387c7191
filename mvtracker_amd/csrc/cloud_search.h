// The self-search's shared pieces (cloud_clean.hip, cloud_prep.hip): the tile layout of ONE cloud, the ring of a tile, and the lower
// bounds of d2 against a box, all with the scan's arithmetic fma(dz,dz,fma(dy,dy,dx*dx)) on per-axis gaps, every rounding step of
// which is monotonic, so a bound never exceeds the d2 of a pair it covers.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float inf_f() { return __int_as_float(0x7f800000); }
__device__ __forceinline__ float nan_f() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ bool finite3(const f32x4& p) { return fabsf(p[0]) < inf_f() && fabsf(p[1]) < inf_f() && fabsf(p[2]) < inf_f(); }

// Point of lane `lane` of tile `tile` of ONE cloud: mvt_tile_aabb's tile_point with a single image per cloud.
__device__ __forceinline__ int clean_tile_point(int tile, int lane, int grid_w) {
  if (grid_w == 0) return tile * 64 + lane;
  const unsigned tpr = (unsigned)grid_w >> 3;
  const unsigned ty = (unsigned)tile / tpr, tx = (unsigned)tile - ty * tpr;
  return (int)((ty * 8 + (lane >> 3)) * grid_w + tx * 8 + (lane & 7));
}

// Is tile t in the ring of tile t0 (t0 itself included)?  Pass 0 visits exactly these tiles and pass 1 exactly the others.
__device__ __forceinline__ bool in_ring(int t, int t0, int grid_w) {
  if (grid_w == 0) return t - t0 <= 2 && t0 - t <= 2;
  const int tpr = grid_w >> 3;
  const int ty = t / tpr, tx = t - ty * tpr, ty0 = t0 / tpr, tx0 = t0 - ty0 * tpr;
  return ty - ty0 <= 1 && ty0 - ty <= 1 && tx - tx0 <= 1 && tx0 - tx <= 1;
}

__device__ __forceinline__ float gap_d2(float dx, float dy, float dz) { return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx))); }

// lower bound of d2 between a point of box [qlo, qhi] and a point of box [lo, hi]
__device__ __forceinline__ float box_box_d2(const f32x4& qlo, const f32x4& qhi, const f32x4& lo, const f32x4& hi) {
  const float dx = fmaxf(fmaxf(lo[0] - qhi[0], qlo[0] - hi[0]), 0.f);
  const float dy = fmaxf(fmaxf(lo[1] - qhi[1], qlo[1] - hi[1]), 0.f);
  const float dz = fmaxf(fmaxf(lo[2] - qhi[2], qlo[2] - hi[2]), 0.f);
  return gap_d2(dx, dy, dz);
}

// lower bound of d2 between the point q and a point of box [lo, hi] (the existing scan's tile bound)
__device__ __forceinline__ float point_box_d2(const f32x4& q, const f32x4& lo, const f32x4& hi) {
  const float dx = fmaxf(fmaxf(lo[0] - q[0], q[0] - hi[0]), 0.f);
  const float dy = fmaxf(fmaxf(lo[1] - q[1], q[1] - hi[1]), 0.f);
  const float dz = fmaxf(fmaxf(lo[2] - q[2], q[2] - hi[2]), 0.f);
  return gap_d2(dx, dy, dz);
}

inline bool aligned(const void* p, size_t a) { return p && ((uintptr_t)p % a) == 0; }

}  // namespace
