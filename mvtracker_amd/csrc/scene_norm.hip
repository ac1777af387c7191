// Scene normalisation (reference datasets/generic_scene_dataset.py:288-358 compute_auto_scene_normalization, datasets/utils.py:210-301
// transform_scene): an exact order statistic by radix select, the pool statistics of one frame (kept count, centroid, the z quantile
// that becomes the floor, the radius quantile), and the similarity transform X' = t + R (s X) applied to depths, extrinsics, query
// rows and track rows.  Everything summed across workgroups is an integer, or an fp64 sum taken in an order fixed by the problem
// size alone: two runs give the same bits.  No kernel waits on another workgroup; every loop is bounded by an argument.
#include "common.h"

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int SN_WG = 256;  // threads per workgroup of every kernel here (4 waves of 64)
constexpr int SN_BLOCKS = MVT_SCENE_BLOCKS;
constexpr u32 SN_SENTINEL = 0xFFFFFFFFu;  // key of a pixel that is not in the pool: the image of a NaN, above every real key

// words of the select workspace behind the 256 histogram bins
enum { WS_PREFIX = 256, WS_RANK = 257, WS_CNT_LE = 258, WS_MIN_GT = 259 };

// The monotone uint32 image of a float: a < b as floats <=> key(a) < key(b), and -0.0 (0x7FFFFFFF) < +0.0 (0x80000000).
__device__ __forceinline__ u32 fkey(u32 b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ u32 funkey(u32 k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

// (every thread of a 256-thread workgroup) a fresh select for rank k: empty histogram, empty prefix
__device__ __forceinline__ void sel_reset(u32* __restrict__ ws, u32 k) {
  ws[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    ws[WS_PREFIX] = 0;
    ws[WS_RANK] = k;
    ws[WS_CNT_LE] = 0;
    ws[WS_MIN_GT] = SN_SENTINEL;
  }
}

inline int sel_grid(long long n) {
  const long long b = mvt_cdiv(n, SN_WG * 4);
  return (int)(b < 1 ? 1 : (b > SN_BLOCKS ? SN_BLOCKS : b));
}

// ------------------------------------------------------------------------------------------------------------- radix select
// Four passes over the keys, 8 bits each from the top.  Pass p: a histogram of digit p of the keys whose higher digits equal the
// prefix chosen so far (LDS per workgroup, then integer adds into 256 global bins), and one workgroup that finds the bin holding
// the remaining rank, extends the prefix by that digit and lowers the rank by the bins before it.  After pass 3 the prefix is the key.
__global__ __launch_bounds__(SN_WG) void sel_init_kernel(u32* __restrict__ ws, u32 k) { sel_reset(ws, k); }

__global__ __launch_bounds__(SN_WG) void sel_hist_kernel(const u32* __restrict__ data, long long n, int is_float, int pass,
                                                         u32* __restrict__ ws) {
  __shared__ u32 s_hist[256];
  s_hist[threadIdx.x] = 0;
  const u32 prefix = ws[WS_PREFIX];
  const int shift = 24 - 8 * pass;
  const u32 mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
  __syncthreads();
  for (long long i = blockIdx.x * (long long)SN_WG + threadIdx.x; i < n; i += (long long)gridDim.x * SN_WG) {
    u32 k = data[i];
    if (is_float) k = fkey(k);
    if ((k & mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
  }
  __syncthreads();
  const u32 c = s_hist[threadIdx.x];
  if (c) atomicAdd(&ws[threadIdx.x], c);
}

__global__ __launch_bounds__(SN_WG) void sel_pick_kernel(u32* __restrict__ ws, int pass, float* __restrict__ out) {
  __shared__ u32 s_w[SN_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 c = ws[tid];
  const u32 rank = ws[WS_RANK], prefix = ws[WS_PREFIX];
  u32 inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();  // (also: every thread has read rank and prefix before one thread rewrites them)
  u32 woff = 0;
  for (int w = 0; w < wave; ++w) woff += s_w[w];
  const u32 excl = woff + inc - c;
  ws[tid] = 0;  // ready for the next pass
  if (c != 0 && rank >= excl && rank - excl < c) {  // exactly one thread, as the rank is below the number of keys
    const u32 p = prefix | ((u32)tid << (24 - 8 * pass));
    ws[WS_PREFIX] = p;
    ws[WS_RANK] = rank - excl;
    if (pass == 3 && out) out[0] = __uint_as_float(funkey(p));
  }
}

// With x = the selected key: how many keys are <= x, and the smallest key above x.  The next order statistic is x again when the
// count exceeds rank + 1, that smallest key otherwise.
__global__ __launch_bounds__(SN_WG) void sel_next_kernel(const u32* __restrict__ data, long long n, int is_float, u32* __restrict__ ws) {
  const u32 x = ws[WS_PREFIX];
  u32 cnt = 0, mn = SN_SENTINEL;
  for (long long i = blockIdx.x * (long long)SN_WG + threadIdx.x; i < n; i += (long long)gridDim.x * SN_WG) {
    u32 k = data[i];
    if (is_float) k = fkey(k);
    if (k <= x) ++cnt;
    else mn = k < mn ? k : mn;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    const u32 m2 = __shfl_xor(mn, o, 64);
    mn = m2 < mn ? m2 : mn;
  }
  if ((threadIdx.x & 63) == 0) {
    if (cnt) atomicAdd(&ws[WS_CNT_LE], cnt);
    if (mn != SN_SENTINEL) atomicMin(&ws[WS_MIN_GT], mn);
  }
}

void launch_select(const u32* data, long long n, int is_float, u32* ws, float* out, hipStream_t s) {
  const int grid = sel_grid(n);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(sel_hist_kernel, dim3(grid), dim3(SN_WG), 0, s, data, n, is_float, pass, ws);
    hipLaunchKernelGGL(sel_pick_kernel, dim3(1), dim3(SN_WG), 0, s, ws, pass, out);
  }
}

// ------------------------------------------------------------------------------------------------------------- pool statistics
struct SceneArgs {
  const float* depths;  // clip (V,T,1,H,W)
  const float* conf;    // same layout, or NULL
  const float* kinv;    // [V*T][9]
  const float* einv;    // [V*T][12]
  int V, T, t, H, W;
  float thr;
};

// Pixel i of the (V,H,W) raster of frame t: its view, its place in the clip, its depth and whether it is valid.
__device__ __forceinline__ bool scene_pixel(const SceneArgs& a, long long i, int& v, int& x, int& y, float& d) {
  x = (int)(i % a.W);
  const long long r = i / a.W;
  y = (int)(r % a.H);
  v = (int)(r / a.H);
  const long long src = (((long long)v * a.T + a.t) * a.H + y) * a.W + x;
  d = a.depths[src];
  return (a.conf ? a.conf[src] > a.thr : true) && d > 0.f;
}

__device__ __forceinline__ f32x4 scene_point(const SceneArgs& a, int v, int x, int y, float d) {
  const long long cam = (long long)v * a.T + a.t;
  return mvt_unproject_point(a.kinv + cam * 9, a.einv + cam * 12, x, y, 1.0f, d);
}

__device__ __forceinline__ u32 float_key(float f) { return fkey(__float_as_uint(f)); }

__global__ __launch_bounds__(SN_WG) void scene_init_kernel(long long* __restrict__ state, u32* __restrict__ ws, int* __restrict__ view_counts, int V) {
  if (threadIdx.x < MVT_SN_WORDS) state[threadIdx.x] = 0;
  for (int v = threadIdx.x; v < V; v += SN_WG) view_counts[v] = 0;
  sel_reset(ws, 0);
}

// Valid pixels of every view (ballot popcounts; a wave may straddle views), and the valid pixels whose depth is not finite.
__global__ __launch_bounds__(SN_WG) void scene_count_kernel(SceneArgs a, long long n, int* __restrict__ view_counts, long long* __restrict__ state) {
  const long long i = blockIdx.x * (long long)SN_WG + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const long long base = i - lane;  // (the same in every lane of the wave)
  if (base >= n) return;
  const long long hw = (long long)a.H * a.W;
  int v = 0, x, y;
  float d = 0.f;
  const bool valid = i < n && scene_pixel(a, i, v, x, y, d);
  const int v_lo = (int)(base / hw), v_hi = (int)((base + 63 < n ? base + 63 : n - 1) / hw);
  for (int vv = v_lo; vv <= v_hi; ++vv) {
    const u64 m = __ballot(valid && v == vv);
    if (lane == 0 && m) atomicAdd(&view_counts[vv], __popcll(m));
  }
  const u64 bad = __ballot(valid && !(d < INFINITY));
  if (lane == 0 && bad) atomicAdd(reinterpret_cast<u64*>(state) + MVT_SN_NONFINITE, (u64)__popcll(bad));
}

// keys[i] = the key of z of pixel i when its view is kept and it is valid, the sentinel otherwise; fp64 coordinate sums of this
// workgroup's kept pixels (grid-stride order, wave tree, then the four waves in order) -> partial[block][3]; kept count -> state.
__global__ __launch_bounds__(SN_WG) void scene_keys_z_kernel(SceneArgs a, long long n, int min_points, const int* __restrict__ view_counts,
                                                             u32* __restrict__ keys, double* __restrict__ partial, long long* __restrict__ state) {
  __shared__ double s_red[SN_WG / 64][3];
  double s[3] = {0.0, 0.0, 0.0};
  u32 cnt = 0;
  for (long long i = blockIdx.x * (long long)SN_WG + threadIdx.x; i < n; i += (long long)gridDim.x * SN_WG) {
    int v, x, y;
    float d;
    u32 key = SN_SENTINEL;
    if (scene_pixel(a, i, v, x, y, d) && view_counts[v] >= min_points) {
      const f32x4 p = scene_point(a, v, x, y, d);
      key = float_key(p[2]);
      s[0] += (double)p[0];
      s[1] += (double)p[1];
      s[2] += (double)p[2];
      ++cnt;
    }
    keys[i] = key;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) s[c] = wave_sum_f64(s[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) {
    for (int c = 0; c < 3; ++c) s_red[threadIdx.x >> 6][c] = s[c];
    if (cnt) atomicAdd(reinterpret_cast<u64*>(state) + MVT_SN_M, (u64)cnt);
  }
  __syncthreads();
  if (threadIdx.x < 3) partial[blockIdx.x * 3 + threadIdx.x] = (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
}

// torch.quantile's rank of a float32 tensor of M values: q * (M - 1) in fp32 (one rounded multiply), its floor and the fraction.
__device__ __forceinline__ u32 quantile_rank(float q, long long M, double& w) {
  w = 0.0;
  if (M <= 1) return 0;
  const float rf = __fmul_rn(q, (float)(M - 1));
  const float kb = floorf(rf);
  w = (double)(rf - kb);
  long long k = (long long)kb;
  k = k < 0 ? 0 : (k > M - 1 ? M - 1 : k);
  return (u32)k;
}

// One workgroup: centroid = sum of the partials (thread order, wave tree, waves in order) / M, and the select for the z quantile.
__global__ __launch_bounds__(SN_WG) void scene_centroid_kernel(const double* __restrict__ partial, int nb, float q_floor, long long* __restrict__ state,
                                                               u32* __restrict__ ws) {
  __shared__ double s_red[SN_WG / 64][3];
  __shared__ u32 s_rank;
  double s[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nb; b += SN_WG)
    for (int c = 0; c < 3; ++c) s[c] += partial[b * 3 + c];
  for (int c = 0; c < 3; ++c) s[c] = wave_sum_f64(s[c]);
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 3; ++c) s_red[threadIdx.x >> 6][c] = s[c];
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long M = state[MVT_SN_M];
    for (int c = 0; c < 3; ++c) {
      const double t = (s_red[0][c] + s_red[1][c]) + (s_red[2][c] + s_red[3][c]);
      st_f64(state, MVT_SN_CENTROID + c) = M > 0 ? t / (double)M : 0.0;
    }
    double w;
    const u32 k = quantile_rank(q_floor, M, w);
    state[MVT_SN_Z_RANK] = (long long)k;
    st_f64(state, MVT_SN_Z_WEIGHT) = w;
    s_rank = k;
  }
  __syncthreads();
  sel_reset(ws, s_rank);
}

// One workgroup, after a select and its sel_next pass: the two order statistics and the linear interpolation between them.
// which = 0: the z quantile and the floor, then (q_radius >= 0) the select for the radius quantile; which = 1: the radius quantile.
__global__ __launch_bounds__(SN_WG) void scene_quantile_kernel(long long* __restrict__ state, u32* __restrict__ ws, int which, float q_radius) {
  __shared__ u32 s_rank;
  if (threadIdx.x == 0) {
    const int w_lo = which ? MVT_SN_R_LO : MVT_SN_Z_LO, w_hi = which ? MVT_SN_R_HI : MVT_SN_Z_HI;
    const long long M = state[MVT_SN_M], kb = state[which ? MVT_SN_R_RANK : MVT_SN_Z_RANK];
    const double w = st_f64(state, which ? MVT_SN_R_WEIGHT : MVT_SN_Z_WEIGHT);
    const float lo = __uint_as_float(funkey(ws[WS_PREFIX]));
    const float hi = (kb + 1 >= M || (long long)ws[WS_CNT_LE] >= kb + 2) ? lo : __uint_as_float(funkey(ws[WS_MIN_GT]));
    const double q = (double)lo + w * ((double)hi - (double)lo);
    st_f64(state, w_lo) = (double)lo;
    st_f64(state, w_hi) = (double)hi;
    s_rank = 0;
    if (which == 0) {
      st_f64(state, MVT_SN_Z_QUANTILE) = q;
      st_f64(state, MVT_SN_FLOOR) = q - st_f64(state, MVT_SN_CENTROID + 2);
      if (q_radius >= 0.f) {
        double wr;
        s_rank = quantile_rank(q_radius, M, wr);
        state[MVT_SN_R_RANK] = (long long)s_rank;
        st_f64(state, MVT_SN_R_WEIGHT) = wr;
      }
    } else {
      st_f64(state, MVT_SN_R_QUANTILE) = q;
    }
  }
  __syncthreads();
  sel_reset(ws, s_rank);
}

// keys[i] <- the key of |p - centroid - (0, 0, floor)| (fp64, rounded to fp32 once) for the pixels of the pool, which the z keys mark.
__global__ __launch_bounds__(SN_WG) void scene_keys_r_kernel(SceneArgs a, long long n, u32* __restrict__ keys, const long long* __restrict__ state) {
  const double* f = reinterpret_cast<const double*>(state);
  const double cx = f[MVT_SN_CENTROID], cy = f[MVT_SN_CENTROID + 1], cz = f[MVT_SN_CENTROID + 2] + f[MVT_SN_FLOOR];
  for (long long i = blockIdx.x * (long long)SN_WG + threadIdx.x; i < n; i += (long long)gridDim.x * SN_WG) {
    if (keys[i] == SN_SENTINEL) continue;
    int v, x, y;
    float d;
    scene_pixel(a, i, v, x, y, d);
    const f32x4 p = scene_point(a, v, x, y, d);
    const double dx = (double)p[0] - cx, dy = (double)p[1] - cy, dz = (double)p[2] - cz;
    keys[i] = float_key((float)sqrt(dx * dx + dy * dy + dz * dz));
  }
}

// ------------------------------------------------------------------------------------------------------------- the transform
struct SceneXf {
  double s, R[9], t[3];
};

__global__ __launch_bounds__(SN_WG) void scale_kernel(const float* __restrict__ in, float* __restrict__ out, long long n4, long long n, double s) {
  const long long stride = (long long)gridDim.x * SN_WG, gid = blockIdx.x * (long long)SN_WG + threadIdx.x;
  for (long long i = gid; i < n4; i += stride) {
    const f32x4 v = reinterpret_cast<const f32x4*>(in)[i];
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (float)((double)v[c] * s);
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
  for (long long i = n4 * 4 + gid; i < n; i += stride) out[i] = (float)((double)in[i] * s);
}

// [Re | te] -> [Re | s te] [R^T | -R^T t; 0 1] = [Re R^T | s te - Re R^T t]: the rigid inverse in closed form.
__global__ __launch_bounds__(SN_WG) void extr_kernel(const float* __restrict__ in, float* __restrict__ out, int n, SceneXf x) {
  const int m = blockIdx.x * SN_WG + threadIdx.x;
  if (m >= n) return;
  double E[12];
  for (int j = 0; j < 12; ++j) E[j] = (double)in[(long long)m * 12 + j];
  double c[3];
  for (int k = 0; k < 3; ++k) c[k] = -(x.R[k] * x.t[0] + x.R[3 + k] * x.t[1] + x.R[6 + k] * x.t[2]);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      out[(long long)m * 12 + i * 4 + j] = (float)(E[i * 4] * x.R[j * 3] + E[i * 4 + 1] * x.R[j * 3 + 1] + E[i * 4 + 2] * x.R[j * 3 + 2]);
    out[(long long)m * 12 + i * 4 + 3] = (float)((E[i * 4] * c[0] + E[i * 4 + 1] * c[1] + E[i * 4 + 2] * c[2]) + x.s * E[i * 4 + 3]);
  }
}

// Rows of STRIDE floats whose last three are a point: X -> t + R (s X); a leading column (the query frame) is copied.
template <int STRIDE>
__global__ __launch_bounds__(SN_WG) void points_kernel(const float* __restrict__ in, float* __restrict__ out, long long n, SceneXf x) {
  for (long long r = blockIdx.x * (long long)SN_WG + threadIdx.x; r < n; r += (long long)gridDim.x * SN_WG) {
    const float* p = in + r * STRIDE;
    float* o = out + r * STRIDE;
    if (STRIDE == 4) o[0] = p[0];
    const double X = x.s * (double)p[STRIDE - 3], Y = x.s * (double)p[STRIDE - 2], Z = x.s * (double)p[STRIDE - 1];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[STRIDE - 3 + i] = (float)(x.t[i] + (x.R[i * 3] * X + x.R[i * 3 + 1] * Y + x.R[i * 3 + 2] * Z));
  }
}

inline bool aligned(const void* p, size_t a) { return p && ((uintptr_t)p % a) == 0; }

inline bool load_xf(const double* xf, SceneXf& x) {
  if (!xf) return false;
  x.s = xf[0];
  for (int i = 0; i < 9; ++i) x.R[i] = xf[1 + i];
  for (int i = 0; i < 3; ++i) x.t[i] = xf[10 + i];
  bool ok = x.s > 0.0 && x.s < INFINITY;
  for (int i = 1; i < 13; ++i) ok = ok && xf[i] == xf[i] && xf[i] > -INFINITY && xf[i] < INFINITY;
  return ok;
}

inline int row_grid(long long n) {
  const long long b = mvt_cdiv(n, SN_WG);
  return (int)(b > 4096 ? 4096 : b);
}

}  // namespace

extern "C" int mvt_select_kth(const float* values, long long n, long long k, float* out, void* workspace, void* stream) {
  MVT_REQUIRE(aligned(values, 4) && aligned(out, 4) && aligned(workspace, 4));
  MVT_REQUIRE(n >= 1 && n < (1ll << 31) && k >= 0 && k < n);
  hipStream_t s = mvt_stream(stream);
  u32* ws = (u32*)workspace;
  hipLaunchKernelGGL(sel_init_kernel, dim3(1), dim3(SN_WG), 0, s, ws, (u32)k);
  launch_select(reinterpret_cast<const u32*>(values), n, 1, ws, out, s);
  return mvt_launch_status();
}

extern "C" int mvt_scene_stats(const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T, int t, int H, int W,
                               float conf_thresh, int min_points, float q_floor, float q_radius, unsigned int* keys, double* partial,
                               int* iws, long long* state, void* stream) {
  MVT_REQUIRE(aligned(depths, 4) && (conf == nullptr || aligned(conf, 4)) && aligned(kinv, 4) && aligned(einv, 4));
  MVT_REQUIRE(aligned(keys, 4) && aligned(partial, 8) && aligned(iws, 4) && aligned(state, 8));
  MVT_REQUIRE(V > 0 && T > 0 && t >= 0 && t < T && H > 0 && W > 0 && (long long)V * H * W < (1ll << 31) && min_points >= 0);
  MVT_REQUIRE(q_floor >= 0.f && q_floor <= 1.f && q_radius <= 1.f);  // (q_radius < 0: no radius quantile)
  const long long n = (long long)V * H * W;
  const int nb = (int)(mvt_cdiv(n, SN_WG) > SN_BLOCKS ? SN_BLOCKS : mvt_cdiv(n, SN_WG));
  SceneArgs a = {depths, conf, kinv, einv, V, T, t, H, W, conf_thresh};
  u32* ws = (u32*)iws;
  int* view_counts = iws + MVT_SELECT_WS_WORDS;
  float* f_state = reinterpret_cast<float*>(state);
  hipStream_t s = mvt_stream(stream);
  hipLaunchKernelGGL(scene_init_kernel, dim3(1), dim3(SN_WG), 0, s, state, ws, view_counts, V);
  hipLaunchKernelGGL(scene_count_kernel, dim3((unsigned)mvt_cdiv(n, SN_WG)), dim3(SN_WG), 0, s, a, n, view_counts, state);
  hipLaunchKernelGGL(scene_keys_z_kernel, dim3(nb), dim3(SN_WG), 0, s, a, n, min_points, view_counts, keys, partial, state);
  hipLaunchKernelGGL(scene_centroid_kernel, dim3(1), dim3(SN_WG), 0, s, partial, nb, q_floor, state, ws);
  launch_select(keys, n, 0, ws, f_state + 2 * MVT_SN_Z_LO, s);
  hipLaunchKernelGGL(sel_next_kernel, dim3(sel_grid(n)), dim3(SN_WG), 0, s, keys, n, 0, ws);
  hipLaunchKernelGGL(scene_quantile_kernel, dim3(1), dim3(SN_WG), 0, s, state, ws, 0, q_radius);
  if (q_radius >= 0.f) {
    hipLaunchKernelGGL(scene_keys_r_kernel, dim3(nb), dim3(SN_WG), 0, s, a, n, keys, state);
    launch_select(keys, n, 0, ws, f_state + 2 * MVT_SN_R_LO, s);
    hipLaunchKernelGGL(sel_next_kernel, dim3(sel_grid(n)), dim3(SN_WG), 0, s, keys, n, 0, ws);
    hipLaunchKernelGGL(scene_quantile_kernel, dim3(1), dim3(SN_WG), 0, s, state, ws, 1, -1.0f);
  }
  return mvt_launch_status();
}

extern "C" int mvt_scene_apply(const float* depths, float* depths_out, long long n_depth, const float* extrs, float* extrs_out, int n_extr,
                               const float* queries, float* queries_out, long long n_query, const double* xf, void* stream) {
  SceneXf x;
  MVT_REQUIRE(load_xf(xf, x));
  MVT_REQUIRE(n_depth >= 0 && n_extr >= 0 && n_query >= 0 && n_query < (1ll << 31));
  MVT_REQUIRE(n_depth == 0 || (aligned(depths, 4) && aligned(depths_out, 4)));
  MVT_REQUIRE(n_extr == 0 || (aligned(extrs, 4) && aligned(extrs_out, 4)));
  MVT_REQUIRE(n_query == 0 || (aligned(queries, 4) && aligned(queries_out, 4)));
  hipStream_t s = mvt_stream(stream);
  if (n_depth > 0) {
    const long long n4 = (aligned(depths, 16) && aligned(depths_out, 16)) ? n_depth / 4 : 0;
    const long long b = mvt_cdiv(n4 > 0 ? n4 : n_depth, SN_WG);
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(SN_WG), 0, s, depths, depths_out, n4, n_depth, x.s);
  }
  if (n_extr > 0) hipLaunchKernelGGL(extr_kernel, dim3((unsigned)mvt_cdiv(n_extr, SN_WG)), dim3(SN_WG), 0, s, extrs, extrs_out, n_extr, x);
  if (n_query > 0) hipLaunchKernelGGL(points_kernel<4>, dim3(row_grid(n_query)), dim3(SN_WG), 0, s, queries, queries_out, n_query, x);
  return mvt_launch_status();
}

extern "C" int mvt_scene_tracks(const float* tracks, float* out, long long n_rows, const double* xf, void* stream) {
  SceneXf x;
  MVT_REQUIRE(load_xf(xf, x));
  MVT_REQUIRE(n_rows >= 1 && aligned(tracks, 4) && aligned(out, 4));
  hipLaunchKernelGGL(points_kernel<3>, dim3(row_grid(n_rows)), dim3(SN_WG), 0, mvt_stream(stream), tracks, out, n_rows, x);
  return mvt_launch_status();
}
