// Reprojection check: a z-buffered render of the other views' points into a camera, and photometric / depth scores of the render
// against the camera's own frame (reference: conversions/droid/reproject_depth_into_videos.py render_dense_pointcloud and
// conversions/droid/debug/compare_photometric_error.py compute_mse / compute_psnr / compute_mae / compute_ssim).
//
// splat   - the scatter: one thread per source point (a pixel of a source view's depth map, unprojected with the arithmetic of
//           mvt_clean_points, or a row of a point list), a loop over the target cameras.  The projection is fp64 with every product,
//           sum and quotient rounded on its own (no fused multiply-add), so numpy gives the same bits; the pixel keeps the minimum of
//           the 64-bit key (bits of (float)z) << 32 | source index through ONE unsigned 64-bit atomicMin per point and pixel: the
//           nearest point, the lowest index among equal depths, whatever the order of arrival.  Every address is checked against the
//           image before the atomic; a sprite is clipped to it.
// resolve - per target pixel: key -> index, depth and the colour gathered from the source frame (or the list's colours).
// score   - one workgroup per 16 x 16 tile: the two grey tiles with a 5-pixel halo (reflect-101) go to LDS, the horizontal pass of
//           the five blurred maps goes to LDS, the vertical pass and the SSIM map stay in registers; integer and fp64 sums per
//           workgroup (a fixed shuffle tree, the four waves in order) are written as one record per workgroup, and a second launch
//           adds the records of an image in an order fixed by their number.  No float atomics: the same bits in every run.
#include "cloud_search.h"

namespace {

typedef unsigned long long u64;

constexpr int RP_WG = 256;
constexpr int SC_TILE = 16, SC_HALO = 5, SC_SPAN = SC_TILE + 2 * SC_HALO;  // 26
constexpr int SC_WORDS = MVT_SCORE_WORDS;

struct rp_targets {
  int n;
  int view[MVT_REPROJECT_MAX_TARGETS];
};

struct sc_taps {
  double w[11];
};

// The rendering rule of include/mvtracker_hip.h: false when the point is not drawn into this camera.
__device__ __forceinline__ bool rp_project(const float* __restrict__ K, const float* __restrict__ E, float xf, float yf, float zf, double min_depth,
                                           int W, int H, int& u, int& v, unsigned& zbits) {
  // Plain operators under contract(off): the __dmul_rn / __dadd_rn of the HIP headers are inline `a * b` / `a + b` compiled under the
  // headers' own contraction mode, and the compiler fuses them after inlining (seen in the ISA); here it must not.
#pragma clang fp contract(off)
  const double x = (double)xf, y = (double)yf, z = (double)zf;
  double c[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) c[r] = (((double)E[4 * r] * x + (double)E[4 * r + 1] * y) + (double)E[4 * r + 2] * z) + (double)E[4 * r + 3];
  if (!(c[2] > min_depth)) return false;  // (a NaN depth fails too)
  const double uf = (c[0] * (double)K[0]) / c[2] + (double)K[2];
  const double vf = (c[1] * (double)K[4]) / c[2] + (double)K[5];
  if (!(fabs(uf) < 2147483648.0 && fabs(vf) < 2147483648.0)) return false;  // (not finite fails too)
  u = (int)uf;  // truncation toward zero: uf in (-1, 0) lands in column 0, as the reference's astype(int32)
  v = (int)vf;
  if (u < 0 || u >= W || v < 0 || v >= H) return false;
  zbits = __float_as_uint((float)c[2]);  // positive: the bits order as the values do
  return true;
}

__device__ __forceinline__ void rp_draw(u64* __restrict__ img, int W, int H, int u, int v, int rad, u64 key) {
  const int y0 = max(v - rad, 0), y1 = min(v + rad, H - 1), x0 = max(u - rad, 0), x1 = min(u + rad, W - 1);
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) atomicMin(img + (long long)y * W + x, key);
}

__global__ __launch_bounds__(RP_WG) void splat_depths_kernel(const float* __restrict__ depths, const float* __restrict__ conf,
                                                             const float* __restrict__ kinv, const float* __restrict__ einv, int V, int T, int t,
                                                             int H, int W, float conf_thresh, rp_targets tg, const float* __restrict__ intrs,
                                                             const float* __restrict__ extrs, int exclude_self, double min_depth, int rad,
                                                             u64* __restrict__ keys) {
  const long long HW = (long long)H * W, total = (long long)V * HW;
  const long long i = blockIdx.x * (long long)RP_WG + threadIdx.x;
  if (i >= total) return;
  const int sv = (int)(i / HW);
  const int pix = (int)(i - sv * HW);
  const int y = pix / W, x = pix - y * W;
  const long long cam = (long long)sv * T + t;
  const long long src = cam * HW + pix;
  const float d = depths[src];
  if (!(d > 0.f && d < inf_f() && (conf ? conf[src] > conf_thresh : true))) return;
  const f32x4 p = mvt_unproject_point(kinv + cam * 9, einv + cam * 12, x, y, 1.0f, d);
  if (!finite3(p)) return;
  for (int k = 0; k < tg.n; ++k) {
    if (exclude_self && tg.view[k] == sv) continue;
    int u, v;
    unsigned zb;
    if (rp_project(intrs + k * 9, extrs + k * 12, p[0], p[1], p[2], min_depth, W, H, u, v, zb))
      rp_draw(keys + k * HW, W, H, u, v, rad, ((u64)zb << 32) | (unsigned)i);
  }
}

__global__ __launch_bounds__(RP_WG) void splat_points_kernel(const float* __restrict__ points, long long M, int n_targets,
                                                             const float* __restrict__ intrs, const float* __restrict__ extrs, int H, int W,
                                                             double min_depth, int rad, u64* __restrict__ keys) {
  const long long i = blockIdx.x * (long long)RP_WG + threadIdx.x;
  if (i >= M) return;
  const float px = points[i * 3], py = points[i * 3 + 1], pz = points[i * 3 + 2];
  if (!(fabsf(px) < inf_f() && fabsf(py) < inf_f() && fabsf(pz) < inf_f())) return;
  const long long HW = (long long)H * W;
  for (int k = 0; k < n_targets; ++k) {
    int u, v;
    unsigned zb;
    if (rp_project(intrs + k * 9, extrs + k * 12, px, py, pz, min_depth, W, H, u, v, zb))
      rp_draw(keys + k * HW, W, H, u, v, rad, ((u64)zb << 32) | (unsigned)i);
  }
}

// An 8-bit channel value of a frame: the byte, or an fp32 value rounded to the nearest integer (ties to even) and clamped; NaN -> 0.
__device__ __forceinline__ int rp_channel(const void* __restrict__ img, long long off, int is_u8) {
  if (is_u8) return (int)reinterpret_cast<const unsigned char*>(img)[off];
  return (int)fminf(fmaxf(rintf(reinterpret_cast<const float*>(img)[off]), 0.f), 255.f);
}

__global__ __launch_bounds__(RP_WG) void resolve_kernel(const u64* __restrict__ keys, int n_targets, long long HW, const void* __restrict__ rgbs,
                                                        int rgb_u8, int T, int t, const unsigned char* __restrict__ colors,
                                                        long long limit, long long target_stride, int* __restrict__ index, float* __restrict__ depth,
                                                        unsigned char* __restrict__ color) {
  const long long i = blockIdx.x * (long long)RP_WG + threadIdx.x;
  if (i >= n_targets * HW) return;
  const long long k = i / HW, pix = i - k * HW;
  const u64 key = keys[i];
  const bool empty = key == ~0ull || (long long)(unsigned)key >= limit;  // (an index no splat wrote: keys that were never cleared)
  const int idx = empty ? -1 : (int)(unsigned)key;
  const long long o = k * target_stride * HW + pix;
  index[o] = idx;
  depth[o] = empty ? 0.f : __uint_as_float((unsigned)(key >> 32));
  unsigned char* co = color + k * target_stride * 3 * HW + pix;
  for (int c = 0; c < 3; ++c) {
    int val = 0;
    if (!empty) {
      if (colors) {
        val = colors[(long long)idx * 3 + c];
      } else {
        const long long sv = idx / HW, sp = idx - sv * HW;
        val = rp_channel(rgbs, ((sv * T + t) * 3 + c) * HW + sp, rgb_u8);
      }
    }
    co[c * HW] = (unsigned char)val;
  }
}

__device__ __forceinline__ int reflect101(int i, int n) {  // one reflection, then a clamp for the tile parts outside the image (unused there)
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}

// the integer twin of block_sum_f64 (common.h)
__device__ __forceinline__ u64 sc_block_sum(u64 v, u64* s_red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(RP_WG) void score_tiles_kernel(const void* __restrict__ a, int a_u8, const void* __restrict__ b, int b_u8,
                                                            const int* __restrict__ index, const float* __restrict__ depth,
                                                            const float* __restrict__ target_depth, int H, int W, double depth_tol, sc_taps taps,
                                                            u64* __restrict__ partial) {
  __shared__ float s_ga[SC_SPAN][SC_SPAN + 1], s_gb[SC_SPAN][SC_SPAN + 1];  // grey values 0..255: exact in fp32
  __shared__ double s_h[5][SC_SPAN][SC_TILE + 1];                           // the horizontal pass of x, y, xx, yy, xy
  __shared__ u64 s_red[RP_WG / 64];
  const long long HW = (long long)H * W;
  const int pair = blockIdx.z, tx0 = blockIdx.x * SC_TILE, ty0 = blockIdx.y * SC_TILE;
  const long long ia = (long long)pair * 3 * HW;
  for (int e = threadIdx.x; e < SC_SPAN * SC_SPAN; e += RP_WG) {
    const int r = e / SC_SPAN, c = e - r * SC_SPAN;
    const long long p = (long long)reflect101(ty0 - SC_HALO + r, H) * W + reflect101(tx0 - SC_HALO + c, W);
    // OpenCV's 8-bit BGR2GRAY: (4899 R + 9617 G + 1868 B + 8192) >> 14
    s_ga[r][c] = (float)((4899 * rp_channel(a, ia + p, a_u8) + 9617 * rp_channel(a, ia + HW + p, a_u8) + 1868 * rp_channel(a, ia + 2 * HW + p, a_u8) + 8192) >> 14);
    s_gb[r][c] = (float)((4899 * rp_channel(b, ia + p, b_u8) + 9617 * rp_channel(b, ia + HW + p, b_u8) + 1868 * rp_channel(b, ia + 2 * HW + p, b_u8) + 8192) >> 14);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < SC_SPAN * SC_TILE; e += RP_WG) {
    const int r = e / SC_TILE, c = e - r * SC_TILE;
    double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0, h4 = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const double x = (double)s_ga[r][c + k], y = (double)s_gb[r][c + k], w = taps.w[k];
      h0 += w * x;
      h1 += w * y;
      h2 += w * (x * x);
      h3 += w * (y * y);
      h4 += w * (x * y);
    }
    s_h[0][r][c] = h0, s_h[1][r][c] = h1, s_h[2][r][c] = h2, s_h[3][r][c] = h3, s_h[4][r][c] = h4;
  }
  __syncthreads();
  const int ly = threadIdx.x / SC_TILE, lx = threadIdx.x - ly * SC_TILE;
  const int y = ty0 + ly, x = tx0 + lx;
  const bool inside = y < H && x < W;
  u64 n_cov = 0, sse = 0, sae = 0, sse_c = 0, sae_c = 0, n_depth = 0, n_close = 0;
  double ssim = 0.0, ssim_c = 0.0, dsum = 0.0, dsum_c = 0.0;
  if (inside) {
    double m[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 11; ++k) acc += taps.w[k] * s_h[q][ly + k][lx];
      m[q] = acc;
    }
    const double mu1 = m[0], mu2 = m[1];
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
    const double C1 = 6.5025, C2 = 58.5225;
    ssim = ((2.0 * mu12 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
    const long long p = (long long)y * W + x, ip = (long long)pair * HW + p;
    for (int c = 0; c < 3; ++c) {
      const int d = rp_channel(a, ia + c * HW + p, a_u8) - rp_channel(b, ia + c * HW + p, b_u8);
      sse += (u64)(d * d);
      sae += (u64)(d < 0 ? -d : d);
    }
    if (index[ip] >= 0) {
      n_cov = 1, sse_c = sse, sae_c = sae, ssim_c = ssim;
      const float zt = target_depth[ip];
      if (zt > 0.f && zt < inf_f()) {
        const double dd = fabs((double)depth[ip] - (double)zt);
        n_depth = 1, dsum = dd;
        if (dd <= depth_tol) n_close = 1, dsum_c = dd;
      }
    }
  }
  double* s_redd = reinterpret_cast<double*>(s_red);
  n_cov = sc_block_sum(n_cov, s_red), sse = sc_block_sum(sse, s_red), sae = sc_block_sum(sae, s_red);
  sse_c = sc_block_sum(sse_c, s_red), sae_c = sc_block_sum(sae_c, s_red);
  n_depth = sc_block_sum(n_depth, s_red), n_close = sc_block_sum(n_close, s_red);
  ssim = block_sum_f64(ssim, s_redd), ssim_c = block_sum_f64(ssim_c, s_redd);
  dsum = block_sum_f64(dsum, s_redd), dsum_c = block_sum_f64(dsum_c, s_redd);
  if (threadIdx.x == 0) {
    const long long blk = ((long long)pair * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    u64* o = partial + blk * SC_WORDS;
    o[MVT_SCORE_N] = 0;  // (set by the sum)
    o[MVT_SCORE_COVERED] = n_cov, o[MVT_SCORE_SSE] = sse, o[MVT_SCORE_SAE] = sae, o[MVT_SCORE_SSE_COV] = sse_c, o[MVT_SCORE_SAE_COV] = sae_c;
    o[MVT_SCORE_SSIM] = (u64)__double_as_longlong(ssim), o[MVT_SCORE_SSIM_COV] = (u64)__double_as_longlong(ssim_c);
    o[MVT_SCORE_N_DEPTH] = n_depth, o[MVT_SCORE_N_CLOSE] = n_close;
    o[MVT_SCORE_DEPTH_SAE] = (u64)__double_as_longlong(dsum), o[MVT_SCORE_DEPTH_SAE_CLOSE] = (u64)__double_as_longlong(dsum_c);
    o[12] = o[13] = o[14] = o[15] = 0;
  }
}

__device__ __forceinline__ bool sc_word_is_double(int w) {
  return w == MVT_SCORE_SSIM || w == MVT_SCORE_SSIM_COV || w == MVT_SCORE_DEPTH_SAE || w == MVT_SCORE_DEPTH_SAE_CLOSE;
}

// One workgroup per pair: word w is summed by 16 threads (thread g takes records g, g + 16, .. ascending; the 16 sums are added
// for g = 0..15): an order fixed by the number of records.
__global__ __launch_bounds__(RP_WG) void score_sum_kernel(const u64* __restrict__ partial, int nblocks, long long HW, u64* __restrict__ out) {
  __shared__ u64 s_part[SC_WORDS][16];
  const int w = threadIdx.x >> 4, g = threadIdx.x & 15;
  const u64* p = partial + (long long)blockIdx.x * nblocks * SC_WORDS + w;
  const bool dbl = sc_word_is_double(w);
  u64 si = 0;
  double sd = 0.0;
  for (int r = g; r < nblocks; r += 16) {
    const u64 v = p[(long long)r * SC_WORDS];
    if (dbl) sd += __longlong_as_double((long long)v);
    else si += v;
  }
  s_part[w][g] = dbl ? (u64)__double_as_longlong(sd) : si;
  __syncthreads();
  if (g == 0) {
    u64 ti = 0;
    double td = 0.0;
    for (int q = 0; q < 16; ++q) {
      if (dbl) td += __longlong_as_double((long long)s_part[w][q]);
      else ti += s_part[w][q];
    }
    out[(long long)blockIdx.x * SC_WORDS + w] = w == MVT_SCORE_N ? (u64)HW : (dbl ? (u64)__double_as_longlong(td) : ti);
  }
}

inline bool rp_image_ok(int H, int W) { return H > 0 && W > 0 && H <= (1 << 15) && W <= (1 << 15); }
inline bool rp_render_ok(float min_depth, int splat) { return min_depth == min_depth && min_depth >= 0.f && min_depth < INFINITY && (splat == 1 || splat == 3 || splat == 5); }

}  // namespace

extern "C" int mvt_reproject_clear(unsigned long long* keys, long long n, void* stream) {
  MVT_REQUIRE(aligned(keys, 8) && n > 0);
  hipError_t e = hipMemsetAsync(keys, 0xFF, (size_t)n * sizeof(u64), mvt_stream(stream));
  return e == hipSuccess ? MVT_OK : MVT_ERR_HIP_BASE + (int)e;
}

extern "C" int mvt_reproject_splat_depths(const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T, int t, int H,
                                          int W, float conf_thresh, const int* target_views, int n_targets, const float* intrs, const float* extrs,
                                          int exclude_self, float min_depth, int splat, unsigned long long* keys, void* stream) {
  MVT_REQUIRE(aligned(depths, 4) && (conf == nullptr || aligned(conf, 4)) && aligned(kinv, 4) && aligned(einv, 4) && aligned(intrs, 4) &&
              aligned(extrs, 4) && aligned(keys, 8) && target_views != nullptr);
  MVT_REQUIRE(V > 0 && T > 0 && t >= 0 && t < T && rp_image_ok(H, W) && (long long)V * H * W < (1ll << 31));
  MVT_REQUIRE(n_targets >= 1 && n_targets <= MVT_REPROJECT_MAX_TARGETS && rp_render_ok(min_depth, splat));
  rp_targets tg;
  tg.n = n_targets;
  for (int k = 0; k < MVT_REPROJECT_MAX_TARGETS; ++k) tg.view[k] = -1;
  for (int k = 0; k < n_targets; ++k) {
    MVT_REQUIRE(target_views[k] >= 0 && target_views[k] < V);
    tg.view[k] = target_views[k];
  }
  const long long total = (long long)V * H * W;
  hipLaunchKernelGGL(splat_depths_kernel, dim3((unsigned)mvt_cdiv(total, RP_WG)), dim3(RP_WG), 0, mvt_stream(stream), depths, conf, kinv, einv, V, T, t,
                     H, W, conf_thresh, tg, intrs, extrs, exclude_self ? 1 : 0, (double)min_depth, splat / 2, keys);
  return mvt_launch_status();
}

extern "C" int mvt_reproject_splat_points(const float* points, long long M, int n_targets, const float* intrs, const float* extrs, int H, int W,
                                          float min_depth, int splat, unsigned long long* keys, void* stream) {
  MVT_REQUIRE(aligned(points, 4) && aligned(intrs, 4) && aligned(extrs, 4) && aligned(keys, 8));
  MVT_REQUIRE(M > 0 && M < (1ll << 31) && rp_image_ok(H, W) && (long long)H * W < (1ll << 31));
  MVT_REQUIRE(n_targets >= 1 && n_targets <= MVT_REPROJECT_MAX_TARGETS && rp_render_ok(min_depth, splat));
  hipLaunchKernelGGL(splat_points_kernel, dim3((unsigned)mvt_cdiv(M, RP_WG)), dim3(RP_WG), 0, mvt_stream(stream), points, M, n_targets, intrs, extrs, H,
                     W, (double)min_depth, splat / 2, keys);
  return mvt_launch_status();
}

extern "C" int mvt_reproject_resolve(const unsigned long long* keys, int n_targets, int H, int W, const void* rgbs, int rgb_u8, int V, int T, int t,
                                     const unsigned char* colors, long long M, long long target_stride, int* index, float* depth,
                                     unsigned char* color, void* stream) {
  MVT_REQUIRE(aligned(keys, 8) && aligned(index, 4) && aligned(depth, 4) && color != nullptr);
  MVT_REQUIRE(n_targets >= 1 && n_targets <= MVT_REPROJECT_MAX_TARGETS && rp_image_ok(H, W) && target_stride >= 1);
  if (colors) {  // the list form: indices are rows of colors [M][3]
    MVT_REQUIRE(rgbs == nullptr && M > 0 && M < (1ll << 31));
  } else {  // the clip form: indices are view * H * W + pixel of rgbs [V][T][3][H][W]
    MVT_REQUIRE(rgbs != nullptr && (rgb_u8 || aligned(rgbs, 4)) && V > 0 && T > 0 && t >= 0 && t < T && (long long)V * H * W < (1ll << 31));
  }
  const long long HW = (long long)H * W;
  hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)mvt_cdiv(n_targets * HW, RP_WG)), dim3(RP_WG), 0, mvt_stream(stream), keys, n_targets, HW, rgbs,
                     rgb_u8 ? 1 : 0, T, t, colors, colors ? M : (long long)V * HW, target_stride, index, depth, color);
  return mvt_launch_status();
}

extern "C" int mvt_photometric_blocks(int H, int W) {
  if (!rp_image_ok(H, W) || H < 6 || W < 6) return -1;
  return (int)(mvt_cdiv(H, SC_TILE) * mvt_cdiv(W, SC_TILE));
}

extern "C" int mvt_photometric_score(const void* a, int a_u8, const void* b, int b_u8, const int* index, const float* depth,
                                     const float* target_depth, int n, int H, int W, float depth_tol, unsigned long long* partial,
                                     unsigned long long* scores, void* stream) {
  MVT_REQUIRE(a != nullptr && b != nullptr && (a_u8 || aligned(a, 4)) && (b_u8 || aligned(b, 4)) && aligned(index, 4) && aligned(depth, 4) &&
              aligned(target_depth, 4) && aligned(partial, 8) && aligned(scores, 8));
  MVT_REQUIRE(n >= 1 && n <= 65535 && rp_image_ok(H, W) && H >= 6 && W >= 6 && depth_tol == depth_tol && depth_tol >= 0.f);
  sc_taps taps;
  double sum = 0.0;
  for (int i = 0; i < 11; ++i) sum += taps.w[i] = exp(-(double)((i - 5) * (i - 5)) / 4.5);  // GaussianBlur((11, 11), 1.5): sigma^2 = 2.25
  for (int i = 0; i < 11; ++i) taps.w[i] /= sum;
  const dim3 grid((unsigned)mvt_cdiv(W, SC_TILE), (unsigned)mvt_cdiv(H, SC_TILE), (unsigned)n);
  hipLaunchKernelGGL(score_tiles_kernel, grid, dim3(RP_WG), 0, mvt_stream(stream), a, a_u8 ? 1 : 0, b, b_u8 ? 1 : 0, index, depth, target_depth, H, W,
                     (double)depth_tol, taps, partial);
  int rc = mvt_launch_status();
  if (rc != MVT_OK) return rc;
  hipLaunchKernelGGL(score_sum_kernel, dim3((unsigned)n), dim3(RP_WG), 0, mvt_stream(stream), partial, (int)(grid.x * grid.y), (long long)H * W, scores);
  return mvt_launch_status();
}
