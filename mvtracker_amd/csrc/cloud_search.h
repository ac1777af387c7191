// The cloud searches' shared pieces (cloud_clean.hip, cloud_prep.hip, cloud_cluster.hip, cloud_align.hip): the tile layout of ONE
// cloud, the ring of a tile, the lower bounds of d2 against a box, all with the scan's arithmetic fma(dz,dz,fma(dy,dy,dx*dx)) on
// per-axis gaps, every rounding step of which is monotonic, so a bound never exceeds the d2 of a pair it covers; and walk_cloud, the
// one walk over a cloud's group boxes, tile boxes and points that the self-searches run (cleaning, normals, clustering; the
// alignment's search of OTHER clouds keeps its own copy in cloud_align.hip, see there).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float inf_f() { return __int_as_float(0x7f800000); }
__device__ __forceinline__ float nan_f() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ bool finite3(const f32x4& p) { return fabsf(p[0]) < inf_f() && fabsf(p[1]) < inf_f() && fabsf(p[2]) < inf_f(); }

// Point of lane `lane` of tile `tile` of ONE cloud: mvt_tile_aabb's tile_point with a single image per cloud.
__device__ __forceinline__ int cloud_tile_point(int tile, int lane, int grid_w) {
  if (grid_w == 0) return tile * 64 + lane;
  const unsigned tpr = (unsigned)grid_w >> 3;
  const unsigned ty = (unsigned)tile / tpr, tx = (unsigned)tile - ty * tpr;
  return (int)((ty * 8 + (lane >> 3)) * grid_w + tx * 8 + (lane & 7));
}

// Is tile t in the ring of tile t0 (t0 itself included)?  VISIT_RING visits exactly these tiles and VISIT_REST exactly the others.
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

// ------------------------------------------------------------------------------------------------------------------- the walk
// One candidate cloud: its points and the boxes of mvt_tile_aabb / mvt_tile_group_aabb.
struct cloud_view {
  const float* __restrict__ xyz;   // [P][4]
  const float* __restrict__ box;   // [ntiles][8]: lo, hi; word 3 = the tile's number of finite points
  const float* __restrict__ gbox;  // [(ntiles + 63) / 64][8], the same of every 64 tiles
  long long P;
  int ntiles, grid_w;
};

// Cloud `cloud` of a launch's clouds of P points each, stored one after the other.
__device__ __forceinline__ cloud_view cloud_of(const float* xyz, const float* box, const float* gbox, long long cloud, long long P, int ntiles,
                                               int grid_w) {
  const int ng = (ntiles + 63) >> 6;
  return {xyz + cloud * P * 4, box + cloud * ntiles * 8, gbox + cloud * ng * 8, P, ntiles, grid_w};
}

// Which tiles a walk visits.  A self-search walks twice: the ring of the query's own tile first, without any box cull, which gives
// every query a bound, then the rest.
enum { VISIT_RING = 0, VISIT_REST = 1 };

// What a visitor need not say.  skip_empty: a group or tile whose box counts no finite point (word 3) is dropped before any load
// of its points.
struct walk_defaults {
  static constexpr bool skip_empty = false;
  __device__ __forceinline__ bool tile_ok(int) const { return true; }
  __device__ __forceinline__ void end_tile() {}
};

// The walk of one wave, ONE QUERY PER LANE (q; a lane without a query holds NaNs), over the cloud c: groups of 64 tiles, 64 at a
// time, then the tiles of every group kept, then the points of every tile kept, loaded one per lane and broadcast lane by lane
// (v_readlane); groups, tiles and points each in ascending order.  [qlo, qhi] is the box of the wave's queries, `tile` the queries'
// own tile (VISIT_RING / VISIT_REST), `visit` wave-uniform.  The visitor v (walk_defaults and):
//   bound()          the lane's bound: no candidate with d2 ABOVE it matters to the lane; -inf when it has nothing left to find.
//                    It may only shrink.
//   tile_ok(t)       may the lane's tile t hold anything of interest, whatever its box?
//   candidate(i, p)  once per loaded tile, in the lanes whose point of the tile exists: the point p, its index i.  Does it take
//                    part?  What else the visitor needs of it, it loads here, beside the point's own load, and keeps.
//   visit(j, i, d2)  lane j's point takes part and lies d2 from this lane's query (NaN for a NaN query).  i is THIS lane's index
//                    of the tile: what belongs to lane j's point, that or what the visitor kept, it reads with readlane(., j).
//   end_tile()       after the points of a tile.
// A box is culled only when its distance EXCEEDS the bound, !(lb > bound): a point exactly at the bound is still seen (it can win
// a tie by its index), and a NaN never culls.  Groups and tiles are tested box to box against the wave's largest bound, then the
// tile point to box per query.
template <class V>
__device__ __forceinline__ void walk_cloud(const cloud_view& c, const f32x4& q, const f32x4& qlo, const f32x4& qhi, int tile, int visit, V& v) {
  const int lane = threadIdx.x & 63;
  const int ng = (c.ntiles + 63) >> 6;
  const bool cull = visit != VISIT_RING;
  for (int gb = 0; gb < ng; gb += 64) {
    // this lane's bound, and the wave's largest (-inf: the lane / the wave has nothing left to find)
    float mine = v.bound();
    float tmax = wave_max(mine);
    bool gnear = gb + lane < ng;
    if ((V::skip_empty || cull) && gnear) {
      const float* gp = c.gbox + (long long)(gb + lane) * 8;
      const f32x4 glo = *reinterpret_cast<const f32x4*>(gp);
      if (V::skip_empty) gnear = glo[3] > 0.f;  // a group without a finite point: none of its tiles is looked at
      if (cull && gnear) gnear = !(box_box_d2(qlo, qhi, glo, *reinterpret_cast<const f32x4*>(gp + 4)) > tmax);
    }
    unsigned long long gmask = __ballot(gnear);
    while (gmask) {
      const int tb = (gb + __builtin_ctzll(gmask)) * 64;
      gmask &= gmask - 1;
      const int t = tb + lane;
      bool tnear = t < c.ntiles && in_ring(t, tile, c.grid_w) == (visit == VISIT_RING);
      if (tnear) tnear = v.tile_ok(t);
      if ((V::skip_empty || cull) && tnear) {
        const float* bp = c.box + (long long)t * 8;
        const f32x4 blo = *reinterpret_cast<const f32x4*>(bp);
        if (V::skip_empty) tnear = blo[3] > 0.f;  // a tile without a finite point is never loaded (its box is lo = +inf, hi = -inf)
        if (cull && tnear) tnear = !(box_box_d2(qlo, qhi, blo, *reinterpret_cast<const f32x4*>(bp + 4)) > tmax);
      }
      unsigned long long tmask = __ballot(tnear);
      while (tmask) {
        const int tt = tb + __builtin_ctzll(tmask);
        tmask &= tmask - 1;
        // per query: can the tile hold a point within this lane's bound?
        const float* bp = c.box + (long long)tt * 8;
        const float lbq = point_box_d2(q, *reinterpret_cast<const f32x4*>(bp), *reinterpret_cast<const f32x4*>(bp + 4));
        if (!__ballot(mine > -inf_f() && !(lbq > mine))) continue;
        const int ci = cloud_tile_point(tt, lane, c.grid_w);
        f32x4 p = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};
        bool take = false;
        if (ci < c.P) {
          p = *reinterpret_cast<const f32x4*>(c.xyz + (long long)ci * 4);
          take = v.candidate(ci, p);
        }
        unsigned long long cm = __ballot(take);
        while (cm) {
          const int j = __builtin_ctzll(cm);
          cm &= cm - 1;
          const float cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p[0]), j));
          const float cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p[1]), j));
          const float cz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p[2]), j));
          v.visit(j, ci, gap_d2(cx - q[0], cy - q[1], cz - q[2]));
        }
        v.end_tile();
        mine = v.bound();
      }
      tmax = wave_max(mine);  // (bounds only shrink: the group mask taken with the older value stays valid)
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- host side
inline bool aligned(const void* p, size_t a) { return p && ((uintptr_t)p % a) == 0; }

// C clouds of P points, a point list (grid 0 x 0) or organised as grid_w x grid_h in whole 8x8 patches: what every search takes.
inline bool cloud_shape_ok(int C, long long P, int grid_w, int grid_h) {
  return C > 0 && C <= 65535 && P > 0 && P < (1ll << 31) - 64 &&
         ((grid_w == 0 && grid_h == 0) || (grid_w > 0 && grid_h > 0 && grid_w % 8 == 0 && grid_h % 8 == 0 && P == (long long)grid_w * grid_h));
}

// workgroups of 256 threads of a grid-strided kernel over `total` elements
inline unsigned strided_blocks(long long total) {
  const long long b = mvt_cdiv(total, 256);
  return (unsigned)(b > 8192 ? 8192 : b);
}

}  // namespace
