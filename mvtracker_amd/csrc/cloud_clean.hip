// Depth cleaning: statistical and radius outlier removal of every (view, frame) cloud (reference: the demo's --clean_pointcloud,
// utils/visualizer_rerun.py _clean_point_cloud_with_open3d -> Open3D remove_statistical_outlier / remove_radius_outlier).
//
// clean_points - depth maps read in place -> one organised cloud per (view, frame), padded to whole 8x8 patches; a pixel that is
//                not valid (or whose point is not finite, or lies outside the sphere crop) becomes a NaN point.
// clean_search - the self-search: every point of a cloud is a query against that same cloud.  A wave owns one tile of 64 points,
//                ONE QUERY PER LANE; candidate tiles are loaded one float4 per lane and their points are broadcast lane by lane
//                (v_readlane), so a candidate step is 3 subtracts + 3 multiply-adds + 1 compare for 64 queries at once.
//                  statistical: a query keeps the K smallest d2 seen so far in its own LDS column (list[k][lane], conflict free) with
//                  the largest of them as its bound; a candidate below the bound replaces the largest entry and the column is
//                  rescanned for the new one.  Only the MULTISET of the K smallest d2 matters for the mean distance (equal d2 give
//                  equal terms), so no indices are kept and a tie at the K-th place needs no rule.
//                  radius: a counter per query, stopped at min_points + 1.
//                Walk (walk_cloud, cloud_search.h): pass 0 visits the query tile and the ring around it (3x3 patches, or tiles t-2..t+2 of a point list), which
//                gives every query a bound; pass 1 visits the rest through the group boxes and tile boxes of mvt_tile_group_aabb /
//                mvt_tile_aabb.  A box is skipped only when its distance exceeds the current bound: box to box (the query tile's
//                own box, against the largest bound of the wave) for groups and tiles, then point to box per query; all with the
//                scan's arithmetic fma(dz,dz,fma(dy,dy,dx*dx)) on per-axis gaps, every rounding step of which is monotonic, so the
//                bound never exceeds the d2 of a pair it covers.  The result does not depend on the point order.
//                Every loop is bounded by the tile count; nothing waits on another wave; a wave touches its own LDS columns only.
// clean_mask   - one workgroup per cloud: M, mu, sigma and the threshold in fp64 (thread-strided sums, a fixed shuffle tree, the
//                four waves in order: the same bits in every run), then the keep mask.
#include "cloud_search.h"

namespace {

constexpr int CS_WG = 128;  // threads per workgroup of the search (2 waves): K * 512 bytes of LDS, 32 KiB at K = 64
constexpr int CM_WG = 256;  // (block_sum_f64 adds up four waves)

__global__ __launch_bounds__(256) void clean_points_kernel(const float* __restrict__ depths, const float* __restrict__ conf,
                                                           const float* __restrict__ kinv, const float* __restrict__ einv, int V, int T, int t0,
                                                           int nt, int H, int W, int Hp, int Wp, float conf_thresh, int use_sphere, float sx,
                                                           float sy, float sz, float sr2, float* __restrict__ xyz) {
  const long long total = (long long)V * nt * Hp * Wp;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % Wp);
    const long long r = i / Wp;
    const int y = (int)(r % Hp);
    const int c = (int)(r / Hp);  // cloud = v * nt + (t - t0)
    const int v = c / nt, t = t0 + (c - v * nt);
    f32x4 o = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};
    if (x < W && y < H) {
      const long long cam = (long long)v * T + t;
      const long long src = (cam * H + y) * W + x;
      const float d = depths[src];
      if (d > 0.f && d < inf_f() && (conf ? conf[src] > conf_thresh : true)) {
        const f32x4 p = mvt_unproject_point(kinv + cam * 9, einv + cam * 12, x, y, 1.0f, d);
        bool ok = finite3(p);
        if (use_sphere) ok = ok && gap_d2(p[0] - sx, p[1] - sy, p[2] - sz) < sr2;  // |X - centre|^2 < radius^2, the scan's d2
        if (ok) o = p;
      }
    }
    *reinterpret_cast<f32x4*>(xyz + i * 4) = o;
  }
}

// What a query keeps during the walk.  MODE 0 (statistical): the K smallest d2 in its LDS column, the largest of them (+inf until K
// are found) as the bound.  MODE 1 (radius): a counter stopped at cap, r2 as the bound until then.
template <int MODE>
struct clean_visitor : walk_defaults {
  float* list;  // entry k of this lane's query: list[k * 64]
  int K, cap;
  float r2;
  bool valid;
  float thr;
  int maxpos, cnt;
  __device__ __forceinline__ clean_visitor(float* list_, int K_, float r2_, int cap_, bool valid_)
      : list(list_), K(K_), cap(cap_), r2(r2_), valid(valid_), thr(inf_f()), maxpos(0), cnt(0) {}
  __device__ __forceinline__ float bound() const { return MODE == 0 ? (valid ? thr : -inf_f()) : ((valid && cnt < cap) ? r2 : -inf_f()); }
  __device__ __forceinline__ bool candidate(int, const f32x4& p) const { return finite3(p); }  // NaN points take no part
  __device__ __forceinline__ void visit(int, int, float d2) {
    if (MODE == 0) {
      if (d2 < thr) {
        list[maxpos * 64] = d2;
        float m = -1.f;
        int mp = 0;
        for (int k = 0; k < K; ++k) {
          const float v = list[k * 64];
          if (v > m) {
            m = v;
            mp = k;
          }
        }
        thr = m;
        maxpos = mp;
      }
    } else {
      cnt += d2 < r2 ? 1 : 0;
    }
  }
  __device__ __forceinline__ void end_tile() {
    if (MODE == 1) cnt = cnt < cap ? cnt : cap;
  }
};

// MODE 0: statistical (a_out), MODE 1: radius (c_out).  One wave per (cloud, tile); lane = query.
template <int MODE>
__global__ __launch_bounds__(CS_WG) void clean_search_kernel(const float* __restrict__ xyz, long long P, int ntiles, int grid_w, int K, float r2,
                                                             int cap, const float* __restrict__ box, const float* __restrict__ gbox,
                                                             float* __restrict__ a_out, int* __restrict__ c_out) {
  extern __shared__ float lds[];  // [waves][K][64] (MODE 0)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * (CS_WG / 64) + wave;
  if (tile >= ntiles) return;  // (wave-uniform; the kernel has no workgroup barrier)
  const long long cloud = blockIdx.y;
  const cloud_view cv = cloud_of(xyz, box, gbox, cloud, P, ntiles, grid_w);
  float* list = lds + wave * K * 64 + lane;  // entry k of this lane's query: list[k * 64]

  const int qi = cloud_tile_point(tile, lane, grid_w);
  f32x4 q = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};
  if (qi < P) q = *reinterpret_cast<const f32x4*>(cv.xyz + (long long)qi * 4);
  const bool valid = finite3(q);
  if (!__ballot(valid)) {  // nothing to search for
    if (qi < P) {
      if (MODE == 0) a_out[cloud * P + qi] = nan_f();
      else c_out[cloud * P + qi] = -1;
    }
    return;
  }
  if (MODE == 0)
    for (int k = 0; k < K; ++k) list[k * 64] = inf_f();
  const f32x4 qlo = *reinterpret_cast<const f32x4*>(cv.box + (long long)tile * 8), qhi = *reinterpret_cast<const f32x4*>(cv.box + (long long)tile * 8 + 4);

  clean_visitor<MODE> vis(list, K, r2, cap, valid);
  for (int pass = 0; pass < 2; ++pass) walk_cloud(cv, q, qlo, qhi, tile, pass == 0 ? VISIT_RING : VISIT_REST, vis);

  if (MODE == 0) {
    // mean of the distances in ascending order of d2, fp64; entries still +inf were never found (fewer than K points in the cloud)
    double sum = 0.0;
    int kk = 0;
    for (int r = 0; r < K; ++r) {
      float m = inf_f();
      int mp = -1;
      for (int k = 0; k < K; ++k) {
        const float v = list[k * 64];
        if (v < m) {
          m = v;
          mp = k;
        }
      }
      if (mp >= 0) {
        sum += sqrt((double)m);
        ++kk;
        list[mp * 64] = inf_f();
      }
    }
    if (qi < P) a_out[cloud * P + qi] = (valid && kk > 0) ? (float)(sum / (double)kk) : nan_f();
  } else {
    if (qi < P) c_out[cloud * P + qi] = valid ? vis.cnt : -1;
  }
}

// One workgroup per cloud.  state[cloud] = {M, mu, sigma, thr} (doubles); keep[cloud][P].
__global__ __launch_bounds__(CM_WG) void clean_mask_kernel(const float* __restrict__ a, const int* __restrict__ c, long long P, int mode,
                                                           double std_ratio, int min_points, double* __restrict__ state,
                                                           unsigned char* __restrict__ keep) {
  __shared__ double s_red[CM_WG / 64];
  const long long base = (long long)blockIdx.x * P;
  double* st = state + (long long)blockIdx.x * 4;
  if (mode == 1) {
    double m = 0.0;
    for (long long i = threadIdx.x; i < P; i += CM_WG) {
      const int ci = c[base + i];
      m += ci >= 0 ? 1.0 : 0.0;
      keep[base + i] = ci > min_points ? 1 : 0;
    }
    m = block_sum_f64(m, s_red);
    if (threadIdx.x == 0) {
      st[0] = m;
      st[1] = st[2] = st[3] = 0.0;
    }
    return;
  }
  double m = 0.0, s = 0.0;
  for (long long i = threadIdx.x; i < P; i += CM_WG) {
    const float ai = a[base + i];
    m += ai == ai ? 1.0 : 0.0;  // (a NaN marks a point that is not valid)
    s += ai > 0.f ? (double)ai : 0.0;
  }
  m = block_sum_f64(m, s_red);  // (an integer below 2^31: exact)
  s = block_sum_f64(s, s_red);
  const double mu = m > 0.0 ? s / m : 0.0;
  double q = 0.0;
  for (long long i = threadIdx.x; i < P; i += CM_WG) {
    const float ai = a[base + i];
    if (ai > 0.f) {
      const double d = (double)ai - mu;
      q += d * d;
    }
  }
  q = block_sum_f64(q, s_red);
  const double sigma = m > 1.0 ? sqrt(q / (m - 1.0)) : 0.0;
  const double thr = mu + std_ratio * sigma;
  for (long long i = threadIdx.x; i < P; i += CM_WG) {
    const float ai = a[base + i];
    keep[base + i] = (m > 1.0 && ai > 0.f && (double)ai < thr) ? 1 : 0;
  }
  if (threadIdx.x == 0) {
    st[0] = m;
    st[1] = mu;
    st[2] = sigma;
    st[3] = thr;
  }
}

}  // namespace

extern "C" int mvt_clean_points(const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T, int t0, int nt, int H,
                                int W, float conf_thresh, const float* sphere, float* xyz, void* stream) {
  MVT_REQUIRE(aligned(depths, 4) && (conf == nullptr || aligned(conf, 4)) && aligned(kinv, 4) && aligned(einv, 4) && aligned(xyz, 16));
  MVT_REQUIRE(V > 0 && T > 0 && t0 >= 0 && nt > 0 && t0 <= T - nt && H > 0 && W > 0 && H <= (1 << 15) && W <= (1 << 15));
  const int Hp = (H + 7) & ~7, Wp = (W + 7) & ~7;
  MVT_REQUIRE((long long)Hp * Wp < (1ll << 31) && (long long)V * nt <= 65535);
  float sx = 0.f, sy = 0.f, sz = 0.f, sr2 = 0.f;
  if (sphere) {  // 4 floats on the HOST: centre, radius
    MVT_REQUIRE(sphere[3] > 0.f && sphere[3] < INFINITY && sphere[0] == sphere[0] && sphere[1] == sphere[1] && sphere[2] == sphere[2]);
    sx = sphere[0], sy = sphere[1], sz = sphere[2], sr2 = sphere[3] * sphere[3];
  }
  const long long total = (long long)V * nt * Hp * Wp;
  hipLaunchKernelGGL(clean_points_kernel, dim3(strided_blocks(total)), dim3(256), 0, mvt_stream(stream), depths, conf, kinv, einv, V, T, t0,
                     nt, H, W, Hp, Wp, conf_thresh, sphere ? 1 : 0, sx, sy, sz, sr2, xyz);
  return mvt_launch_status();
}

extern "C" int mvt_clean_search(const float* xyz, int C, long long P, int grid_w, int grid_h, int mode, int K, float radius, int min_points,
                                const float* tile_box, const float* group_box, float* a_out, int* c_out, void* stream) {
  MVT_REQUIRE(aligned(xyz, 16) && aligned(tile_box, 16) && aligned(group_box, 16));
  MVT_REQUIRE(cloud_shape_ok(C, P, grid_w, grid_h));
  const int ntiles = (int)((P + 63) / 64);
  const dim3 grid((unsigned)mvt_cdiv(ntiles, CS_WG / 64), (unsigned)C);
  if (mode == MVT_CLEAN_STATISTICAL) {
    MVT_REQUIRE(aligned(a_out, 4) && K >= 1 && K <= MVT_CLEAN_MAX_K);
    hipLaunchKernelGGL(clean_search_kernel<0>, grid, dim3(CS_WG), (size_t)K * CS_WG * sizeof(float), mvt_stream(stream), xyz, P, ntiles, grid_w, K,
                       0.f, 0, tile_box, group_box, a_out, (int*)nullptr);
  } else {
    MVT_REQUIRE(mode == MVT_CLEAN_RADIUS && aligned(c_out, 4) && radius > 0.f && radius < INFINITY && min_points >= 0 && min_points < (1 << 30));
    hipLaunchKernelGGL(clean_search_kernel<1>, grid, dim3(CS_WG), 0, mvt_stream(stream), xyz, P, ntiles, grid_w, 0, radius * radius,
                       min_points + 1, tile_box, group_box, (float*)nullptr, c_out);
  }
  return mvt_launch_status();
}

extern "C" int mvt_clean_mask(const float* a, const int* c, int C, long long P, int mode, float std_ratio, int min_points, double* state,
                              unsigned char* keep, void* stream) {
  MVT_REQUIRE(C > 0 && P > 0 && P < (1ll << 31) && aligned(state, 8) && keep != nullptr);
  MVT_REQUIRE((mode == MVT_CLEAN_STATISTICAL && aligned(a, 4) && std_ratio == std_ratio && std_ratio > -INFINITY && std_ratio < INFINITY) ||
              (mode == MVT_CLEAN_RADIUS && aligned(c, 4) && min_points >= 0));
  hipLaunchKernelGGL(clean_mask_kernel, dim3((unsigned)C), dim3(CM_WG), 0, mvt_stream(stream), a, c, P, mode == MVT_CLEAN_RADIUS ? 1 : 0,
                     (double)std_ratio, min_points, state, keep);
  return mvt_launch_status();
}
