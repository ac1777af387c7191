// Motion masks ("Motion masks"): which pixels of a clip belong to the static background.
//
//   d_b      = ((|dc0| + |dc1|) + |dc2|) / 3.0f          fp32, frames b and b + 1, IEEE division
//   change   = max of d_b over b in [t - win, t + win - 1] n [0, T - 2] and over the (2r+1)^2 patch clipped to the image
//   static   = change < thresh
//
// Three entries.  mvt_motion_temporal walks the frames once, one lane per 4 adjacent pixels of a plane, with the previous frame's
// channel values in registers: it writes either every boundary's diff map or (win covering the whole clip) the running maximum
// alone, and the per-boundary sums of |dc0| + |dc1| + |dc2| as fp64 block partials.  mvt_motion_mask takes the temporal maximum
// while it stages a tile with its halo in LDS, then a separable (2r+1)^2 maximum (rows, then columns), the comparison, one mask
// byte per pixel and a static-pixel count per tile.  mvt_motion_report adds the partials in an order fixed by their number.
// Maxima propagate a NaN, as the reference's pooling does (a NaN diff makes its neighbourhood moving).  No atomics anywhere.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / MVT_WAVE;
constexpr int kTileW = MVT_MOTION_TILE_W, kTileH = MVT_MOTION_TILE_H;
constexpr int kRowsPerWave = kTileH / kWaves;
static_assert(kTileW == MVT_WAVE, "one lane per tile column");
static_assert(MVT_MOTION_BLOCK_PIXELS == 4 * kThreads, "four pixels per lane");

__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

// The maximum of q[k * stride] over k in [lo, hi], lo <= hi, four loads at a time (an index past hi repeats hi: the maximum does
// not mind) so that they are in flight together.
__device__ __forceinline__ float window_max(const float* q, long long stride, int lo, int hi) {
  float m = -INFINITY;
  for (int k = lo; k <= hi; k += 4) {
    const float a0 = q[k * stride], a1 = q[min(k + 1, hi) * stride], a2 = q[min(k + 2, hi) * stride], a3 = q[min(k + 3, hi) * stride];
    m = max_nan(m, max_nan(max_nan(a0, a1), max_nan(a2, a3)));
  }
  return m;
}

// Four adjacent pixels of one channel plane as fp32.  VEC: the group is whole and its address aligned (the entry checks both);
// otherwise element by element, pixels at or past `n` reading as 0.
template <bool U8, bool VEC>
__device__ __forceinline__ f32x4 load_px4(const void* plane, long long p, long long n) {
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (U8) {
    const unsigned char* s = static_cast<const unsigned char*>(plane);
    if (VEC) {
      const unsigned w = *reinterpret_cast<const unsigned*>(s + p);
      o[0] = (float)(w & 255u), o[1] = (float)((w >> 8) & 255u), o[2] = (float)((w >> 16) & 255u), o[3] = (float)(w >> 24);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (p + i < n) o[i] = (float)s[p + i];
    }
  } else {
    const float* s = static_cast<const float*>(plane);
    if (VEC) {
      o = *reinterpret_cast<const f32x4*>(s + p);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (p + i < n) o[i] = s[p + i];
    }
  }
  return o;
}

template <bool VEC>
__device__ __forceinline__ void store_px4(float* plane, long long p, long long n, const f32x4& v) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(plane + p) = v;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (p + i < n) plane[p + i] = v[i];
  }
}

struct px12 {
  f32x4 c[3];
};

template <bool U8, bool VEC>
__device__ __forceinline__ px12 load_frame(const void* rgbs, long long frame, long long hw, long long p, bool live) {
  px12 f;
  const long long esz = U8 ? 1 : 4;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f.c[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (live) f.c[c] = load_px4<U8, VEC>(static_cast<const char*>(rgbs) + (frame * 3 + c) * hw * esz, p, hw);
  }
  return f;
}

// grid (blocks per view, V).  rgbs (V, T, 3, H, W) planar; out: all_mode ? (V, H*W) the maximum over every boundary
//                                                                         : (V, T-1, H*W) every boundary's diff.
// partial ((v * gridDim.x + block), T-1) fp64: the block's sum of |dc0| + |dc1| + |dc2| per boundary.
template <bool U8, bool VEC>
__global__ __launch_bounds__(kThreads) void motion_temporal_kernel(const void* __restrict__ rgbs, int T, long long hw, int all_mode,
                                                                   float* __restrict__ out, double* __restrict__ partial) {
  __shared__ double red[2][kWaves];
  const int v = blockIdx.y;
  const long long p = ((long long)blockIdx.x * kThreads + threadIdx.x) * 4;
  const bool live = p < hw;
  const int lane = threadIdx.x & (MVT_WAVE - 1), wave = threadIdx.x / MVT_WAVE;
  const long long f0 = (long long)v * T;
  double* prow = partial + ((long long)v * gridDim.x + blockIdx.x) * (T - 1);
  px12 prev = load_frame<U8, VEC>(rgbs, f0, hw, p, live);
  px12 nxt = load_frame<U8, VEC>(rgbs, f0 + 1, hw, p, live);
  f32x4 run = {0.f, 0.f, 0.f, 0.f};  // (diffs are >= 0 or NaN)
  for (int b = 0; b + 1 < T; ++b) {
    const px12 cur = nxt;
    if (b + 2 < T) nxt = load_frame<U8, VEC>(rgbs, f0 + b + 2, hw, p, live);  // in flight over the arithmetic and the barrier below
    f32x4 d;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a = (fabsf(cur.c[0][i] - prev.c[0][i]) + fabsf(cur.c[1][i] - prev.c[1][i])) + fabsf(cur.c[2][i] - prev.c[2][i]);
      d[i] = a / 3.0f;  // correctly rounded: the build keeps hipcc's default IEEE fp32 division (no fast-math flag in build.py)
      run[i] = max_nan(run[i], d[i]);
      s += a;  // pixels past the plane read 0 in both frames
    }
    if (!all_mode && live) store_px4<VEC>(out + (f0 - v + b) * hw, p, hw, d);
    const double ws = wave_sum_f64((double)s);
    if (lane == 0) red[b & 1][wave] = ws;
    __syncthreads();  // one barrier per boundary: buffer b & 1 is next written at b + 2, behind the barrier of b + 1
    if (threadIdx.x == 0) prow[b] = ((red[b & 1][0] + red[b & 1][1]) + red[b & 1][2]) + red[b & 1][3];
    prev = cur;
  }
  if (all_mode && live) store_px4<VEC>(out + (long long)v * hw, p, hw, run);
}

// grid (tiles in x, tiles in y, images), images = V * T (win >= 1: image = v * T + t, src (V, T-1, H, W)) or V (win == 0: src
// (V, H, W), the mask of view v written to all T frames).  Dynamic LDS: ((kTileH + 2r) * (kTileW + 2r) + (kTileH + 2r) * kTileW)
// floats with r > 0, none with r == 0.  counts (image, tile) int32: static pixels of the tile.
__global__ __launch_bounds__(kThreads) void motion_mask_kernel(const float* __restrict__ src, int T, int H, int W, int win, int r, float thresh,
                                                               unsigned char* __restrict__ mask, int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int wcount[kWaves];
  const int lane = threadIdx.x & (MVT_WAVE - 1), wave = threadIdx.x / MVT_WAVE;
  const int img = blockIdx.z;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const long long hw = (long long)H * W;
  int v = img, t = 0, lo = 0, hi = 0;
  if (win > 0) {
    v = img / T, t = img - v * T;
    lo = max(0, t - win), hi = min(T - 2, t + win - 1);
  }
  const float* base = src + (win > 0 ? (long long)v * (T - 1) : (long long)v) * hw;  // boundary b of the view: base + b * hw
  const int iw = kTileW + 2 * r, ih = kTileH + 2 * r;
  float* in = lds;             // [ih][iw]: the temporal maximum, -inf outside the image
  float* rm = lds + ih * iw;   // [ih][kTileW]: row maxima
  if (r > 0) {
    for (int iy = wave; iy < ih; iy += kWaves) {
      const int gy = y0 - r + iy;
      for (int ix = lane; ix < iw; ix += MVT_WAVE) {
        const int gx = x0 - r + ix;
        float m = -INFINITY;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
          m = window_max(base + (long long)gy * W + gx, hw, lo, hi);
        }
        in[iy * iw + ix] = m;
      }
    }
    __syncthreads();
    for (int iy = wave; iy < ih; iy += kWaves) {
      rm[iy * kTileW + lane] = window_max(in + iy * iw + lane, 1, 0, 2 * r);
    }
    __syncthreads();
  }
  const int gx = x0 + lane;
  int n_static = 0;
#pragma unroll
  for (int j = 0; j < kRowsPerWave; ++j) {
    const int ty = wave * kRowsPerWave + j, gy = y0 + ty;
    const bool inside = gy < H && gx < W;
    float m = -INFINITY;
    if (r > 0) {
      m = window_max(rm + ty * kTileW + lane, kTileW, 0, 2 * r);
    } else if (inside) {
      m = window_max(base + (long long)gy * W + gx, hw, lo, hi);
    }
    const bool is_static = inside && m < thresh;
    n_static += __popcll(__ballot(is_static));
    if (inside) {
      const long long px = (long long)gy * W + gx;
      if (win > 0) {
        mask[(long long)img * hw + px] = is_static;
      } else {
        for (int f = 0; f < T; ++f) mask[((long long)v * T + f) * hw + px] = is_static;
      }
    }
  }
  if (lane == 0) wcount[wave] = n_static;
  __syncthreads();
  if (threadIdx.x == 0)
    counts[((long long)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((wcount[0] + wcount[1]) + wcount[2]) + wcount[3];
}

// grid (T - 1 + V * T).  Block i < T - 1: report[i] = the sum over `rows` partial rows of column i; block T - 1 + v * T + t: the
// static pixels of frame t of view v from `tiles` tile counts.  Thread k adds entries k, k + 256, ... in turn, then a fixed tree.
__global__ __launch_bounds__(kThreads) void motion_report_kernel(const double* __restrict__ partial, long long rows, const int* __restrict__ counts,
                                                                 int tiles, int T, int all_mode, double* __restrict__ report) {
  __shared__ double red[kThreads];
  const int i = blockIdx.x;
  double s = 0.0;
  if (i < T - 1) {
    for (long long k = threadIdx.x; k < rows; k += kThreads) s += partial[k * (T - 1) + i];
  } else {
    const int vt = i - (T - 1);
    const long long img = all_mode ? vt / T : vt;
    for (int k = threadIdx.x; k < tiles; k += kThreads) s += (double)counts[img * tiles + k];
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) report[i] = red[0];
}

bool shape_ok(int V, int T, int H, int W) {
  return V >= 1 && V <= 65535 && T >= 2 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) - 4 * kThreads && (long long)V * T <= 65535;
}

}  // namespace

extern "C" {

int mvt_motion_blocks(int H, int W) {
  if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31) - 4 * kThreads) return -1;
  return (int)mvt_cdiv((long long)H * W, MVT_MOTION_BLOCK_PIXELS);
}

int mvt_motion_tiles(int H, int W) {
  if (H < 1 || W < 1) return -1;
  const long long n = mvt_cdiv(W, kTileW) * mvt_cdiv(H, kTileH);
  return n < (1ll << 31) ? (int)n : -1;
}

int mvt_motion_temporal(const void* rgbs, int is_u8, int V, int T, int H, int W, int all_mode, float* out, double* partial, void* stream) {
  MVT_REQUIRE(rgbs && out && partial && shape_ok(V, T, H, W));
  MVT_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)partial & 7) == 0 && (is_u8 || ((uintptr_t)rgbs & 3) == 0));
  const long long hw = (long long)H * W;
  // whole, aligned groups of four: every plane starts at a multiple of hw elements from the base
  const bool vec = hw % 4 == 0 && ((uintptr_t)rgbs & (is_u8 ? 3 : 15)) == 0 && ((uintptr_t)out & 15) == 0;
  const dim3 grid((unsigned)mvt_cdiv(hw, MVT_MOTION_BLOCK_PIXELS), (unsigned)V);
  hipStream_t s = mvt_stream(stream);
  const int all = all_mode != 0;
  if (is_u8) {
    if (vec) motion_temporal_kernel<true, true><<<grid, kThreads, 0, s>>>(rgbs, T, hw, all, out, partial);
    else motion_temporal_kernel<true, false><<<grid, kThreads, 0, s>>>(rgbs, T, hw, all, out, partial);
  } else {
    if (vec) motion_temporal_kernel<false, true><<<grid, kThreads, 0, s>>>(rgbs, T, hw, all, out, partial);
    else motion_temporal_kernel<false, false><<<grid, kThreads, 0, s>>>(rgbs, T, hw, all, out, partial);
  }
  return mvt_launch_status();
}

int mvt_motion_mask(const float* src, int V, int T, int H, int W, int win, int r, float thresh, unsigned char* mask, int* counts,
                    void* stream) {
  MVT_REQUIRE(src && mask && counts && shape_ok(V, T, H, W));
  MVT_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)counts & 3) == 0);
  MVT_REQUIRE(win >= 0 && r >= 0 && r <= MVT_MOTION_MAX_RADIUS && thresh == thresh && fabsf(thresh) != INFINITY);
  const long long ty = mvt_cdiv(H, kTileH);
  MVT_REQUIRE(ty <= 65535 && mvt_motion_tiles(H, W) > 0);
  const dim3 grid((unsigned)mvt_cdiv(W, kTileW), (unsigned)ty, (unsigned)(win > 0 ? V * T : V));
  const size_t lds = r > 0 ? sizeof(float) * (size_t)(kTileH + 2 * r) * (size_t)(kTileW + 2 * r + kTileW) : 0;
  motion_mask_kernel<<<grid, kThreads, lds, mvt_stream(stream)>>>(src, T, H, W, win, r, thresh, mask, counts);
  return mvt_launch_status();
}

int mvt_motion_report(const double* partial, const int* counts, int V, int T, int H, int W, int all_mode, double* report, void* stream) {
  MVT_REQUIRE(partial && counts && report && shape_ok(V, T, H, W));
  MVT_REQUIRE(((uintptr_t)partial & 7) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)report & 7) == 0);
  const long long rows = (long long)V * mvt_motion_blocks(H, W);
  motion_report_kernel<<<(unsigned)(T - 1 + V * T), kThreads, 0, mvt_stream(stream)>>>(partial, rows, counts, mvt_motion_tiles(H, W), T, all_mode != 0,
                                                                                      report);
  return mvt_launch_status();
}

}  // extern "C"
