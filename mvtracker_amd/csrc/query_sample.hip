// Query sampling from depth (reference evaluation/evaluator_3dpt.py:286-388, kmeans_sample :42-59): the candidate pool of one
// frame (unprojection + confidence / cylinder test + order-preserving compaction) and k-means over it (greedy k-means++ seeding,
// Lloyd iterations).  Everything that is summed across lanes or workgroups is an INTEGER (fixed point), so results do not depend
// on the order of addition: two runs give the same bits.  No kernel waits on another workgroup; every loop is bounded by an argument.
#include "block_scan.h"

namespace {

typedef unsigned long long u64;

constexpr int QS_WG = 256;          // threads per workgroup of every kernel here
static_assert(QS_WG == SCAN_WG, "wg_excl_scan_u64 and block_counts_scan are written for this workgroup size");
constexpr int QS_TILE = 4 * QS_WG;  // points per tile of the k-means kernels (4 per lane)
constexpr int QS_MAX_K = MVT_KMEANS_MAX_K;
constexpr int QS_MAX_CAND = MVT_KMEANS_MAX_CAND;
constexpr int QS_MAX_BLOCKS = MVT_KMEANS_SEED_BLOCKS;
constexpr int QS_LDS_ACC_K = 1024;  // up to this k the per-centre sums are first added up in LDS (12 k + 32 k bytes <= 44 KiB)

// words of the k-means state (include/mvtracker_hip.h, MVT_KM_*)
enum { ST_LO = MVT_KM_LO, ST_HI = MVT_KM_HI, ST_SCALE = MVT_KM_SCALE, ST_SCALE2 = MVT_KM_SCALE2, ST_TOL = MVT_KM_TOL, ST_ITER = MVT_KM_ITER,
       ST_CONV = MVT_KM_CONVERGED, ST_EMPTY = MVT_KM_EMPTY, ST_INERTIA = MVT_KM_INERTIA, ST_INERTIA_ACC = MVT_KM_INERTIA_ACC,
       ST_SHIFT = MVT_KM_SHIFT, ST_POT = MVT_KM_POT, ST_CAND = MVT_KM_CAND };

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
  return v;
}

// ------------------------------------------------------------------------------------------------------------- candidate pool
struct PoolArgs {
  const float* depths;  // clip (V,T,1,H,W)
  const float* conf;    // same layout, or NULL
  const float* kinv;    // [V*T][9]
  const float* einv;    // [V*T][12]
  int V, T, t, H, W;
  float thr, x0, y0, r2, zmin, zmax;
  int inclusive;
};

// Pixel i of the (V,H,W) raster of frame t: its world point and whether the pool keeps it.  A NaN coordinate fails every test.
__device__ __forceinline__ bool pool_point(const PoolArgs& a, int i, f32x4& p) {
  const int x = i % a.W, r = i / a.W, y = r % a.H, v = r / a.H;
  const long long cam = (long long)v * a.T + a.t;
  const long long src = (cam * a.H + y) * a.W + x;
  const float d = a.depths[src];
  const bool valid = a.conf ? a.conf[src] > a.thr : d > 0.f;
  p = mvt_unproject_point(a.kinv + cam * 9, a.einv + cam * 12, x, y, 1.0f, d);
  const float dx = p[0] - a.x0, dy = p[1] - a.y0;
  const float r2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));  // x**2 + y**2 as torch rounds it: no fused multiply-add
  const bool inside = (a.inclusive ? r2 <= a.r2 : r2 < a.r2) && p[2] >= a.zmin && p[2] <= a.zmax;
  return valid && inside;
}

__global__ __launch_bounds__(QS_WG) void pool_count_kernel(PoolArgs a, int n, int* __restrict__ block_counts) {
  __shared__ int s_cnt[QS_WG / 64];
  const int i = blockIdx.x * QS_WG + threadIdx.x;
  f32x4 p;
  const bool keep = i < n && pool_point(a, i, p);
  const u64 m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(QS_WG) void pool_scan_kernel(int* __restrict__ block_counts, int nb, int chunk, int* __restrict__ count) {
  block_counts_scan(block_counts, nb, chunk, count);
}

__global__ __launch_bounds__(QS_WG) void pool_scatter_kernel(PoolArgs a, int n, const int* __restrict__ block_base, float* __restrict__ pool) {
  __shared__ int s_cnt[QS_WG / 64];
  const int i = blockIdx.x * QS_WG + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 p;
  const bool keep = i < n && pool_point(a, i, p);
  const u64 m = __ballot(keep);
  if (lane == 0) s_cnt[wave] = __popcll(m);
  __syncthreads();
  int base = block_base[blockIdx.x];  // <= the total, and base + (kept before me in this workgroup) < total <= n
  for (int w = 0; w < wave; ++w) base += s_cnt[w];
  if (keep) {
    const long long pos = base + __popcll(m & ((1ull << lane) - 1ull));
    pool[pos * 3] = p[0];
    pool[pos * 3 + 1] = p[1];
    pool[pos * 3 + 2] = p[2];
  }
}

// ------------------------------------------------------------------------------------------------------------- k-means: statistics
__device__ __forceinline__ float d2f(float px, float py, float pz, float cx, float cy, float cz) {
  const float dx = px - cx, dy = py - cy, dz = pz - cz;  // the direct form (no |a|^2 + |b|^2 - 2ab cancellation)
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// A squared distance in fixed point (truncated; scale2 is a power of two chosen so that M of them cannot overflow 63 bits).
__device__ __forceinline__ u64 q2(float d2, double scale2) { return (u64)((double)d2 * scale2); }

__global__ __launch_bounds__(QS_WG) void stats_minmax_kernel(const float* __restrict__ pts, long long M, double* __restrict__ part) {
  __shared__ float s_red[QS_WG / 64][6];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long long i = blockIdx.x * (long long)QS_WG + threadIdx.x; i < M; i += (long long)gridDim.x * QS_WG)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = pts[i * 3 + c];
      lo[c] = fminf(lo[c], v);
      hi[c] = fmaxf(hi[c], v);
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lo[c] = -wave_max(-lo[c]);
    hi[c] = wave_max(hi[c]);
  }
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 3; ++c) {
      s_red[threadIdx.x >> 6][c] = lo[c];
      s_red[threadIdx.x >> 6][3 + c] = hi[c];
    }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    part[blockIdx.x * 6 + c] = (double)fminf(fminf(s_red[0][c], s_red[1][c]), fminf(s_red[2][c], s_red[3][c]));
    part[blockIdx.x * 6 + 3 + c] = (double)fmaxf(fmaxf(s_red[0][3 + c], s_red[1][3 + c]), fmaxf(s_red[2][3 + c], s_red[3][3 + c]));
  }
}

// One wave: the bounding box and the two fixed-point scales.
__global__ __launch_bounds__(64) void stats_range_kernel(const double* __restrict__ part, int nb, long long M, long long* __restrict__ state) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < nb; b += 64)
    for (int c = 0; c < 3; ++c) {
      lo[c] = fmin(lo[c], part[b * 6 + c]);
      hi[c] = fmax(hi[c], part[b * 6 + 3 + c]);
    }
  for (int c = 0; c < 3; ++c)
    for (int o = 32; o > 0; o >>= 1) {
      lo[c] = fmin(lo[c], __shfl_xor(lo[c], o, 64));
      hi[c] = fmax(hi[c], __shfl_xor(hi[c], o, 64));
    }
  if (threadIdx.x == 0) {
    double ext = 0.0, diag2 = 0.0;
    for (int c = 0; c < 3; ++c) {
      st_f64(state, ST_LO + c) = lo[c];
      st_f64(state, ST_HI + c) = hi[c];
      ext = fmax(ext, hi[c] - lo[c]);
      diag2 += (hi[c] - lo[c]) * (hi[c] - lo[c]);
    }
    // per-value budget: 2^40 levels, fewer when M values of that size would pass 2^62 (so a sum stays below 2^63 with a factor 2 to spare)
    const double qmax = fmin(1099511627776.0, 4611686018427387904.0 / (double)M);
    const bool ok = ext > 0.0 && ext < INFINITY;
    st_f64(state, ST_SCALE) = ok ? ldexp(1.0, ilogb(qmax / ext)) : 1.0;      // (x - lo) * scale <= qmax
    st_f64(state, ST_SCALE2) = ok ? ldexp(1.0, ilogb(qmax / diag2)) : 1.0;   // d2 * scale2 <= qmax inside the box
  }
}

__global__ __launch_bounds__(QS_WG) void stats_moments_kernel(const float* __restrict__ pts, long long M, const long long* __restrict__ state,
                                                              double* __restrict__ part) {
  __shared__ double s_red[QS_WG / 64][6];
  double s[6] = {0, 0, 0, 0, 0, 0};
  const double lo[3] = {st_f64(state, ST_LO), st_f64(state, ST_LO + 1), st_f64(state, ST_LO + 2)};
  for (long long i = blockIdx.x * (long long)QS_WG + threadIdx.x; i < M; i += (long long)gridDim.x * QS_WG)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double d = (double)pts[i * 3 + c] - lo[c];
      s[c] += d;
      s[3 + c] += d * d;
    }
#pragma unroll
  for (int c = 0; c < 6; ++c) s[c] = wave_sum_f64(s[c]);
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 6; ++c) s_red[threadIdx.x >> 6][c] = s[c];
  __syncthreads();
  if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
}

// One wave: tol * mean per-coordinate variance (sklearn's _tolerance), and the counters of a fresh run.
__global__ __launch_bounds__(64) void stats_tol_kernel(const double* __restrict__ part, int nb, long long M, float tol, long long* __restrict__ state) {
  double s[6] = {0, 0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nb; b += 64)
    for (int c = 0; c < 6; ++c) s[c] += part[b * 6 + c];
  for (int c = 0; c < 6; ++c) s[c] = wave_sum_f64(s[c]);
  if (threadIdx.x == 0) {
    double var = 0.0;
    for (int c = 0; c < 3; ++c) {
      const double mean = s[c] / (double)M;
      var += fmax(s[3 + c] / (double)M - mean * mean, 0.0);
    }
    st_f64(state, ST_TOL) = (double)tol * var / 3.0;
    state[ST_ITER] = 0;
    state[ST_CONV] = 0;
    state[ST_EMPTY] = 0;
    st_f64(state, ST_INERTIA) = 0.0;
    state[ST_INERTIA_ACC] = 0;
    st_f64(state, ST_SHIFT) = 0.0;
    state[ST_POT] = 0;
  }
}

// ------------------------------------------------------------------------------------------------------------- k-means: seeding
__host__ __device__ inline u64 mix64(u64 z) {  // splitmix64's finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// Counter-based draw: 64 uniform bits that depend on (seed, step, candidate) alone.
__host__ __device__ inline u64 draw64(u64 seed, int step, int cand) { return mix64(mix64(seed) + ((u64)(unsigned)step << 8) + (u64)(unsigned)cand); }

__device__ __forceinline__ long long clamp_index(long long i, long long M) { return i < 0 ? 0 : (i >= M ? M - 1 : i); }

__global__ void seed_first_kernel(long long M, u64 seed, long long* __restrict__ state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) state[ST_CAND] = (long long)__umul64hi(draw64(seed, 0, 0), (u64)M);  // uniform in [0, M)
}

// Step `step` of the seeding, first launch: fold centre step-1 (the previous winner) into min_d2, then for every candidate c of this
// step the potential sum_i min(min_d2[i], |x_i - x_cand_c|^2) of this workgroup's points -> partials[c][block].  Workgroup b owns the
// tiles [b * tpb, (b + 1) * tpb).
__global__ __launch_bounds__(QS_WG) void seed_eval_kernel(const float* __restrict__ pts, long long M, float* __restrict__ min_d2,
                                                          const float* __restrict__ centres, int step, int ncand, int tpb,
                                                          u64* __restrict__ partials, const long long* __restrict__ state) {
  __shared__ float s_cand[QS_MAX_CAND * 3];
  __shared__ u64 s_red[QS_WG / 64][QS_MAX_CAND];
  const int tid = threadIdx.x;
  const double scale2 = st_f64(state, ST_SCALE2);
  if (tid < ncand) {
    const long long idx = clamp_index(state[ST_CAND + tid], M);
    for (int c = 0; c < 3; ++c) s_cand[tid * 3 + c] = pts[idx * 3 + c];
  }
  float vx = 0.f, vy = 0.f, vz = 0.f;
  if (step > 0) {
    vx = centres[(step - 1) * 3];
    vy = centres[(step - 1) * 3 + 1];
    vz = centres[(step - 1) * 3 + 2];
  }
  __syncthreads();
  u64 acc[QS_MAX_CAND];
#pragma unroll
  for (int c = 0; c < QS_MAX_CAND; ++c) acc[c] = 0;
  for (int tl = 0; tl < tpb; ++tl) {
    const long long base = ((long long)blockIdx.x * tpb + tl) * QS_TILE;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long i = base + e * QS_WG + tid;
      if (i < M) {
        const float px = pts[i * 3], py = pts[i * 3 + 1], pz = pts[i * 3 + 2];
        const float m = step > 0 ? fminf(min_d2[i], d2f(px, py, pz, vx, vy, vz)) : INFINITY;
        min_d2[i] = m;
#pragma unroll
        for (int c = 0; c < QS_MAX_CAND; ++c)
          if (c < ncand) acc[c] += q2(fminf(m, d2f(px, py, pz, s_cand[c * 3], s_cand[c * 3 + 1], s_cand[c * 3 + 2])), scale2);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < QS_MAX_CAND; ++c)
    if (c < ncand) {
      const u64 s = wave_sum_u64(acc[c]);
      if ((tid & 63) == 0) s_red[tid >> 6][c] = s;
    }
  __syncthreads();
  if (tid < ncand) partials[(long long)tid * gridDim.x + blockIdx.x] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
}

// Step `step`, second launch (one workgroup): the candidate with the lowest potential becomes centre `step`; then the nnext candidates
// of step + 1 are drawn with probability proportional to the updated min_d2 (D^2 sampling): a target in [0, potential), the
// workgroup of seed_eval whose prefix range holds it (binary search over the block prefix in LDS), the point inside that range.
__global__ __launch_bounds__(QS_WG) void seed_pick_kernel(const float* __restrict__ pts, long long M, const float* __restrict__ min_d2,
                                                          const u64* __restrict__ partials, int nblocks, int tpb, float* __restrict__ centres,
                                                          int step, int ncand, int nnext, u64 seed, long long* __restrict__ state) {
  __shared__ u64 s_prefix[QS_MAX_BLOCKS];
  __shared__ u64 s_red[QS_WG / 64];
  __shared__ u64 s_pot[QS_MAX_CAND];
  __shared__ u64 s_scan[QS_WG / 64];
  __shared__ long long s_found;
  __shared__ int s_w;
  const int tid = threadIdx.x;
  for (int c = 0; c < ncand; ++c) {
    u64 a = 0;
    for (int b = tid; b < nblocks; b += QS_WG) a += partials[(long long)c * nblocks + b];
    a = wave_sum_u64(a);
    if ((tid & 63) == 0) s_red[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) s_pot[c] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    __syncthreads();
  }
  if (tid == 0) {
    int w = 0;
    for (int c = 1; c < ncand; ++c)
      if (s_pot[c] < s_pot[w]) w = c;  // ties: the lowest candidate
    s_w = w;
  }
  __syncthreads();
  const int w = s_w;
  const u64 pot = s_pot[w];
  const long long iw = clamp_index(state[ST_CAND + w], M);
  const float wx = pts[iw * 3], wy = pts[iw * 3 + 1], wz = pts[iw * 3 + 2];
  if (tid == 0) {
    centres[step * 3] = wx;
    centres[step * 3 + 1] = wy;
    centres[step * 3 + 2] = wz;
    state[ST_POT] = (long long)pot;
  }
  __syncthreads();  // every thread has read its candidate index before the next ones are written
  if (nnext == 0) return;
  {  // exclusive prefix of the winner's block potentials
    const int chunk = (nblocks + QS_WG - 1) / QS_WG;
    const int b0 = tid * chunk;
    u64 sum = 0;
    for (int j = 0; j < chunk; ++j)
      if (b0 + j < nblocks) sum += partials[(long long)w * nblocks + b0 + j];
    u64 total;
    u64 off = wg_excl_scan_u64(sum, s_scan, total);
    for (int j = 0; j < chunk; ++j)
      if (b0 + j < nblocks) {
        s_prefix[b0 + j] = off;
        off += partials[(long long)w * nblocks + b0 + j];
      }
    __syncthreads();
  }
  const double scale2 = st_f64(state, ST_SCALE2);
  for (int t = 0; t < nnext; ++t) {
    const u64 r = draw64(seed, step + 1, t);
    long long idx = (long long)__umul64hi(r, (u64)M);  // potential 0 (every point is a centre already): a uniform draw
    if (tid == 0) s_found = -1;
    __syncthreads();
    if (pot > 0) {
      const u64 target = __umul64hi(r, pot);  // uniform in [0, pot)
      int lo = 0, hi = nblocks - 1;
      for (int it = 0; it < 13; ++it) {  // nblocks <= 4096: 12 halvings
        const int mid = (lo + hi + 1) >> 1;
        if (lo < hi) {
          if (s_prefix[mid] <= target) lo = mid;
          else hi = mid - 1;
        }
      }
      u64 rem = target - s_prefix[lo];
      for (int sub = 0; sub < tpb * 4; ++sub) {
        const long long i = (long long)lo * tpb * QS_TILE + (long long)sub * QS_WG + tid;
        u64 v = 0;
        if (i < M) v = q2(fminf(min_d2[i], d2f(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], wx, wy, wz)), scale2);
        u64 total;
        const u64 off = wg_excl_scan_u64(v, s_scan, total);
        if (rem < total) {  // (uniform: rem and total are the same in every thread)
          if (off <= rem && rem < off + v) s_found = i;
          break;
        }
        rem -= total;
      }
    }
    __syncthreads();
    if (s_found >= 0) idx = s_found;
    if (tid == 0) state[ST_CAND + t] = idx;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------- k-means: Lloyd
// acc [k][4] u64: fixed-point coordinate sums (offset from the box minimum, times scale) and the count of every centre.
template <int LDS_ACC>
__global__ __launch_bounds__(QS_WG) void assign_kernel(const float* __restrict__ pts, long long M, const float* __restrict__ centres, int k,
                                                       int* __restrict__ labels, u64* __restrict__ acc, long long* __restrict__ state,
                                                       int ntiles, int max_iter, int final_pass) {
  extern __shared__ u64 s_mem[];  // [k][4] u64 partial sums (LDS_ACC), then the centres [k][3] fp32
  if (!final_pass && (state[ST_CONV] != 0 || state[ST_ITER] >= max_iter)) return;  // (uniform: a finished run costs an empty launch)
  u64* s_acc = s_mem;
  float* s_c = reinterpret_cast<float*>(s_mem + (LDS_ACC ? (size_t)k * 4 : 0));
  const int tid = threadIdx.x;
  for (int j = tid; j < k * 3; j += QS_WG) s_c[j] = centres[j];
  if (LDS_ACC)
    for (int j = tid; j < k * 4; j += QS_WG) s_acc[j] = 0;
  const double lox = st_f64(state, ST_LO), loy = st_f64(state, ST_LO + 1), loz = st_f64(state, ST_LO + 2);
  const double scale = st_f64(state, ST_SCALE), scale2 = st_f64(state, ST_SCALE2);
  __syncthreads();
  u64 inertia = 0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    float px[4], py[4], pz[4], best[4];
    int bi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long i = (long long)tile * QS_TILE + e * QS_WG + tid;
      const bool in = i < M;
      px[e] = in ? pts[i * 3] : 0.f;
      py[e] = in ? pts[i * 3 + 1] : 0.f;
      pz[e] = in ? pts[i * 3 + 2] : 0.f;
      best[e] = INFINITY;
      bi[e] = 0;
    }
    for (int j = 0; j < k; ++j) {
      const float cx = s_c[j * 3], cy = s_c[j * 3 + 1], cz = s_c[j * 3 + 2];  // one address for the whole wave: an LDS broadcast
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = d2f(px[e], py[e], pz[e], cx, cy, cz);
        if (d < best[e]) {  // strict: a tie keeps the lower index
          best[e] = d;
          bi[e] = j;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long i = (long long)tile * QS_TILE + e * QS_WG + tid;
      if (i < M) {
        const int j = bi[e];
        labels[i] = j;
        const double dx = (double)px[e] - (double)s_c[j * 3], dy = (double)py[e] - (double)s_c[j * 3 + 1], dz = (double)pz[e] - (double)s_c[j * 3 + 2];
        inertia += (u64)((dx * dx + dy * dy + dz * dz) * scale2);
        const u64 qx = (u64)(((double)px[e] - lox) * scale), qy = (u64)(((double)py[e] - loy) * scale), qz = (u64)(((double)pz[e] - loz) * scale);
        u64* a = (LDS_ACC ? s_acc : acc) + (size_t)j * 4;
        atomicAdd(a, qx);
        atomicAdd(a + 1, qy);
        atomicAdd(a + 2, qz);
        atomicAdd(a + 3, 1ull);
      }
    }
  }
  inertia = wave_sum_u64(inertia);
  if ((tid & 63) == 0 && inertia != 0) atomicAdd(reinterpret_cast<u64*>(state) + ST_INERTIA_ACC, inertia);
  if (LDS_ACC) {
    __syncthreads();
    for (int j = tid; j < k; j += QS_WG)
      if (s_acc[j * 4 + 3] != 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) atomicAdd(acc + (size_t)j * 4 + c, s_acc[j * 4 + c]);
  }
}

// One workgroup.  centre = lo + sum / (count * scale) in fp64, stored as fp32; an empty cluster keeps its centre.  Then sklearn's
// stopping rule: sum of squared centre shifts <= tol * mean variance.  final_pass: the sums are those of the returned centres --
// report their inertia and empty clusters and change nothing else.
__global__ __launch_bounds__(QS_WG) void update_kernel(float* __restrict__ centres, int k, u64* __restrict__ acc, long long* __restrict__ state,
                                                       int max_iter, int final_pass) {
  __shared__ double s_shift[QS_WG / 64];
  __shared__ int s_empty[QS_WG / 64];
  if (!final_pass && (state[ST_CONV] != 0 || state[ST_ITER] >= max_iter)) return;
  const double scale = st_f64(state, ST_SCALE);
  double shift = 0.0;
  int empty = 0;
  for (int j = threadIdx.x; j < k; j += QS_WG) {
    const u64 cnt = acc[(size_t)j * 4 + 3];
    if (cnt == 0) ++empty;
    if (!final_pass) {
      if (cnt != 0)
        for (int c = 0; c < 3; ++c) {
          const float nv = (float)(st_f64(state, ST_LO + c) + (double)acc[(size_t)j * 4 + c] / ((double)cnt * scale));
          const double d = (double)nv - (double)centres[j * 3 + c];
          shift += d * d;
          centres[j * 3 + c] = nv;
        }
      for (int c = 0; c < 4; ++c) acc[(size_t)j * 4 + c] = 0;  // ready for the next assignment
    }
  }
  shift = wave_sum_f64(shift);
  for (int o = 32; o > 0; o >>= 1) empty += __shfl_xor(empty, o, 64);
  if ((threadIdx.x & 63) == 0) {
    s_shift[threadIdx.x >> 6] = shift;
    s_empty[threadIdx.x >> 6] = empty;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    state[ST_EMPTY] = s_empty[0] + s_empty[1] + s_empty[2] + s_empty[3];
    st_f64(state, ST_INERTIA) = (double)(u64)state[ST_INERTIA_ACC] / st_f64(state, ST_SCALE2);
    state[ST_INERTIA_ACC] = 0;
    if (!final_pass) {
      const double total = (s_shift[0] + s_shift[1]) + (s_shift[2] + s_shift[3]);
      st_f64(state, ST_SHIFT) = total;
      state[ST_ITER] += 1;
      if (total <= st_f64(state, ST_TOL)) state[ST_CONV] = 1;
    }
  }
}

inline bool aligned(const void* p, size_t a) { return p && ((uintptr_t)p % a) == 0; }

inline int seed_blocks(long long M, int* tpb) {
  const long long tiles = mvt_cdiv(M, QS_TILE);
  *tpb = (int)mvt_cdiv(tiles, QS_MAX_BLOCKS);
  return (int)mvt_cdiv(tiles, *tpb);
}

inline int stat_blocks(long long M) {
  const long long b = mvt_cdiv(M, QS_WG);
  return (int)(b > MVT_KMEANS_STAT_BLOCKS ? MVT_KMEANS_STAT_BLOCKS : b);
}

inline bool kmeans_args_ok(const float* pts, long long M, int k) {
  return aligned(pts, 4) && M >= 1 && M < (1ll << 31) && k >= 1 && k <= QS_MAX_K && (long long)k <= M;
}

int launch_assign(const float* pts, long long M, const float* centres, int k, int* labels, u64* acc, long long* state, int max_iter,
                  int final_pass, hipStream_t s) {
  const int ntiles = (int)mvt_cdiv(M, QS_TILE);
  const int grid = ntiles < 1024 ? ntiles : 1024;
  if (k <= QS_LDS_ACC_K)
    hipLaunchKernelGGL(assign_kernel<1>, dim3(grid), dim3(QS_WG), (size_t)k * 44, s, pts, M, centres, k, labels, acc, state, ntiles, max_iter,
                       final_pass);
  else
    hipLaunchKernelGGL(assign_kernel<0>, dim3(grid), dim3(QS_WG), (size_t)k * 12, s, pts, M, centres, k, labels, acc, state, ntiles, max_iter,
                       final_pass);
  return mvt_launch_status();
}

}  // namespace

extern "C" int mvt_query_pool(const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T, int t, int H,
                              int W, float conf_threshold, float x0, float y0, float radius_sq, float z_min, float z_max, int flags,
                              float* pool, int* count, int* block_counts, void* stream) {
  MVT_REQUIRE(aligned(depths, 4) && (conf == nullptr || aligned(conf, 4)) && aligned(kinv, 4) && aligned(einv, 4));
  MVT_REQUIRE(aligned(pool, 4) && aligned(count, 4) && aligned(block_counts, 4));
  MVT_REQUIRE(V > 0 && T > 0 && t >= 0 && t < T && H > 0 && W > 0 && (long long)V * H * W < (1ll << 31));
  MVT_REQUIRE((flags & ~MVT_POOL_RADIUS_INCLUSIVE) == 0);
  const int n = V * H * W;
  const int nb = (int)mvt_cdiv(n, QS_WG);
  PoolArgs a = {depths, conf, kinv, einv, V, T, t, H, W, conf_threshold, x0, y0, radius_sq, z_min, z_max, flags & MVT_POOL_RADIUS_INCLUSIVE};
  hipStream_t s = mvt_stream(stream);
  hipLaunchKernelGGL(pool_count_kernel, dim3(nb), dim3(QS_WG), 0, s, a, n, block_counts);
  hipLaunchKernelGGL(pool_scan_kernel, dim3(1), dim3(QS_WG), 0, s, block_counts, nb, (int)mvt_cdiv(nb, QS_WG), count);
  hipLaunchKernelGGL(pool_scatter_kernel, dim3(nb), dim3(QS_WG), 0, s, a, n, block_counts, pool);
  return mvt_launch_status();
}

extern "C" int mvt_kmeans_stats(const float* pts, long long M, float tol, double* partial, long long* state, void* stream) {
  MVT_REQUIRE(aligned(pts, 4) && aligned(partial, 8) && aligned(state, 8) && M >= 1 && M < (1ll << 31) && tol >= 0.f);
  const int nb = stat_blocks(M);
  hipStream_t s = mvt_stream(stream);
  hipLaunchKernelGGL(stats_minmax_kernel, dim3(nb), dim3(QS_WG), 0, s, pts, M, partial);
  hipLaunchKernelGGL(stats_range_kernel, dim3(1), dim3(64), 0, s, partial, nb, M, state);
  hipLaunchKernelGGL(stats_moments_kernel, dim3(nb), dim3(QS_WG), 0, s, pts, M, state, partial);
  hipLaunchKernelGGL(stats_tol_kernel, dim3(1), dim3(64), 0, s, partial, nb, M, tol, state);
  return mvt_launch_status();
}

extern "C" int mvt_kmeans_seed(const float* pts, long long M, int k, long long seed, float* min_d2, void* partials, float* centres,
                               long long* state, void* stream) {
  MVT_REQUIRE(kmeans_args_ok(pts, M, k) && aligned(min_d2, 4) && aligned(partials, 8) && aligned(centres, 4) && aligned(state, 8));
  int tpb;
  const int nblocks = seed_blocks(M, &tpb);
  int ntrials = 2;  // sklearn: 2 + int(log(k))
  for (double e = 2.718281828459045; e <= (double)k; e *= 2.718281828459045) ++ntrials;
  if (ntrials > QS_MAX_CAND) ntrials = QS_MAX_CAND;
  hipStream_t s = mvt_stream(stream);
  hipLaunchKernelGGL(seed_first_kernel, dim3(1), dim3(64), 0, s, M, (u64)seed, state);
  for (int step = 0; step < k; ++step) {
    const int ncand = step == 0 ? 1 : ntrials;
    hipLaunchKernelGGL(seed_eval_kernel, dim3(nblocks), dim3(QS_WG), 0, s, pts, M, min_d2, centres, step, ncand, tpb, (u64*)partials, state);
    hipLaunchKernelGGL(seed_pick_kernel, dim3(1), dim3(QS_WG), 0, s, pts, M, min_d2, (const u64*)partials, nblocks, tpb, centres, step, ncand,
                       step + 1 < k ? ntrials : 0, (u64)seed, state);
  }
  return mvt_launch_status();
}

extern "C" int mvt_kmeans_assign(const float* pts, long long M, const float* centres, int k, int* labels, void* acc, long long* state,
                                 int max_iter, int final_pass, void* stream) {
  MVT_REQUIRE(kmeans_args_ok(pts, M, k) && aligned(centres, 4) && aligned(labels, 4) && aligned(acc, 8) && aligned(state, 8) && max_iter >= 1);
  return launch_assign(pts, M, centres, k, labels, (u64*)acc, state, max_iter, final_pass ? 1 : 0, mvt_stream(stream));
}

extern "C" int mvt_kmeans_update(float* centres, int k, void* acc, long long* state, int max_iter, int final_pass, void* stream) {
  MVT_REQUIRE(aligned(centres, 4) && aligned(acc, 8) && aligned(state, 8) && k >= 1 && k <= QS_MAX_K && max_iter >= 1);
  hipLaunchKernelGGL(update_kernel, dim3(1), dim3(QS_WG), 0, mvt_stream(stream), centres, k, (u64*)acc, state, max_iter, final_pass ? 1 : 0);
  return mvt_launch_status();
}

extern "C" int mvt_kmeans_iterate(const float* pts, long long M, float* centres, int k, int* labels, void* acc, long long* state, int n_iters,
                                  int max_iter, void* stream) {
  MVT_REQUIRE(kmeans_args_ok(pts, M, k) && aligned(centres, 4) && aligned(labels, 4) && aligned(acc, 8) && aligned(state, 8));
  MVT_REQUIRE(max_iter >= 1 && n_iters >= 1 && n_iters <= 64);
  hipStream_t s = mvt_stream(stream);
  for (int it = 0; it < n_iters; ++it) {
    int rc = launch_assign(pts, M, centres, k, labels, (u64*)acc, state, max_iter, 0, s);
    if (rc != MVT_OK) return rc;
    hipLaunchKernelGGL(update_kernel, dim3(1), dim3(QS_WG), 0, s, centres, k, (u64*)acc, state, max_iter, 0);
  }
  return mvt_launch_status();
}
