// Mask queries ("Mask queries"): per-camera instance masks lifted to world space through depth, their per
// (view, frame, label) statistics, the "average distance" matching of the cameras' local ids into global object ids, the relabelled
// clip and the per-object candidate pools.  Everything that is summed across lanes or workgroups is an INTEGER (counts, and
// coordinates in fixed point with 20 fractional bits), so results do not depend on the order of addition: two runs give the same
// bits.  No float atomics.  No kernel waits on another workgroup; every loop is bounded by an argument.
#include "block_scan.h"

namespace {

typedef unsigned long long u64;

constexpr int MQ_WG = 256;  // threads per workgroup of every kernel here
static_assert(MQ_WG == SCAN_WG, "block_counts_scan is written for this workgroup size");
constexpr int MQ_L = MVT_MASK_LABELS;
constexpr int MQ_WORDS = MVT_MASK_STAT_WORDS;
constexpr int MQ_SPAN = 16 * MQ_WG;  // label bytes per workgroup of the statistics kernel: one 16-byte load per lane
enum { W_PIXELS = MVT_MASK_PIXELS, W_COUNT = MVT_MASK_COUNT, W_SUM = MVT_MASK_SUM, W_OOR = MVT_MASK_OUT_OF_RANGE };

struct MaskArgs {
  const unsigned char* labels;  // clip (V,T,H,W), one byte per pixel
  const float* depths;          // clip (V,T,1,H,W)
  const float* conf;            // same layout, or NULL
  const float* kinv;            // [V*T][9]
  const float* einv;            // [V*T][12]
  int V, T, H, W;
  float dmin, dmax, thr;
};

// Rule 1 on a labelled pixel: src = its offset in the clip.
__device__ __forceinline__ bool mask_valid(const MaskArgs& a, long long src, float& d) {
  d = a.depths[src];
  const bool ok = isfinite(d) && d > a.dmin && d <= a.dmax;
  return ok && (a.conf == nullptr || a.conf[src] > a.thr);
}

// The world point of pixel (x, y) at depth d: mvt_unproject_point at stride 1 with EVERY rounding stated.  Left to itself the compiler
// fuses some of that function's multiply-adds and not others, differently from kernel to kernel (the count and the scatter kernel
// of mvt_query_pool already differ), so "the same function" does not give the same bits.  This is the sequence mvt_query_pool's
// scatter kernel has -- which products are fused is read from its code -- so a lifted point has the bits of the same pixel's
// frame_pool row, the statistics are sums over exactly the points lift_masks returns, and neither moves when a kernel here is edited.
// tests/test_gpu_mask_queries.py::test_lift_equals_frame_pool_bit_for_bit holds the two together.
__device__ __forceinline__ f32x4 mask_point(const float* __restrict__ K, const float* __restrict__ E, int x, int y, float d) {
#pragma clang fp contract(off)
  const float px = ((float)x + 0.5f) - 0.5f, py = ((float)y + 0.5f) - 0.5f;
  const float cx = (__builtin_fmaf(K[0], px, K[1] * py) + K[2]) * d;
  const float cy = (__builtin_fmaf(K[4], py, K[3] * px) + K[5]) * d;
  const float cz = ((K[6] * px + K[7] * py) + K[8]) * d;
  f32x4 o;
  o[0] = __builtin_fmaf(E[2], cz, __builtin_fmaf(E[1], cy, E[0] * cx)) + E[3];
  o[1] = __builtin_fmaf(E[6], cz, __builtin_fmaf(E[4], cx, E[5] * cy)) + E[7];
  o[2] = (__builtin_fmaf(E[8], cx, E[9] * cy) + E[10] * cz) + E[11];
  o[3] = 0.f;
  return o;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
  u64 u = (u64)v;  // two's complement: the wrap-around sum of the bit patterns is the signed sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) u += shfl_xor_u64(u, o);
  return (long long)u;
}

// ------------------------------------------------------------------------------------------------------------- statistics
__global__ __launch_bounds__(MQ_WG) void mask_clear_kernel(u64* __restrict__ stats, long long words) {  // (words is even: 6 per row)
  const long long i = ((long long)blockIdx.x * MQ_WG + threadIdx.x) * 2;
  if (i < words) *reinterpret_cast<ulonglong2*>(stats + i) = make_ulonglong2(0, 0);
}

// grid (spans, V*T).  A workgroup owns MQ_SPAN consecutive label bytes of one image, counted from the 16-byte boundary at or below
// the image's first byte, so that every lane's 16-byte load is aligned whatever H*W is; bytes of the neighbouring images that the
// first and the last load also bring in are masked out.  The labels are staged in LDS and read back transposed: in step k lane i of
// the workgroup has pixel k * 256 + i of the span, so a wave's 64 lanes hold 64 consecutive pixels (coalesced depth loads, and
// usually one label).
__global__ __launch_bounds__(MQ_WG) void mask_stats_kernel(MaskArgs a, long long HW, long long total, u64* __restrict__ stats) {
  __shared__ u64 s_acc[MQ_L * MQ_WORDS];        // 12 KiB
  __shared__ __attribute__((aligned(16))) unsigned char s_lab[MQ_SPAN];  // 4 KiB
  const int tid = threadIdx.x, lane = tid & 63;
  const long long cam = blockIdx.y;
  const long long img0 = cam * HW, img1 = img0 + HW;
  const long long span0 = (img0 & ~15ll) + (long long)blockIdx.x * MQ_SPAN;
  if (span0 >= img1) return;  // (uniform)
  for (int j = tid; j < MQ_L * MQ_WORDS; j += MQ_WG) s_acc[j] = 0;
  {
    const long long b = span0 + 16ll * tid;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (b + 16 <= total) {
      w = *reinterpret_cast<const uint4*>(a.labels + b);
    } else {
      unsigned char* wb = reinterpret_cast<unsigned char*>(&w);
      for (int e = 0; e < 16; ++e)
        if (b + e < total) wb[e] = a.labels[b + e];
    }
    *reinterpret_cast<uint4*>(s_lab + 16 * tid) = w;
  }
  __syncthreads();
  const float* K = a.kinv + cam * 9;
  const float* E = a.einv + cam * 12;
  // every load of the lane's 16 pixels is issued before the first is used: depth (and confidence) only where a label is set
  int labs[16];
  float dep[16], cnf[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const long long p = span0 + k * MQ_WG + tid;  // offset in the clip
    labs[k] = (p >= img0 && p < img1) ? (int)s_lab[k * MQ_WG + tid] : 0;
    dep[k] = labs[k] != 0 ? a.depths[p] : 0.f;
    cnf[k] = (labs[k] != 0 && a.conf != nullptr) ? a.conf[p] : INFINITY;
  }
  // the lane's pixel walks 256 pixels per step: its (x, y) from one division, then by steps (16 W is added so that the at most
  // 15 bytes before the image do not make the dividend negative; those lanes hold label 0 and their y is never used)
  const int step_x = MQ_WG % a.W, step_y = MQ_WG / a.W;
  const int i0 = (int)(span0 - img0) + tid + 16 * a.W;  // (< 2^24 + 4096 + 16 W: H W <= 2^24)
  int x = i0 % a.W, y = i0 / a.W - 16;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int lab = labs[k];
    const int xk = x, yk = y;
    x += step_x;
    y += step_y;
    if (x >= a.W) {
      x -= a.W;
      ++y;
    }
    const u64 m_lab = __ballot(lab != 0);
    if (m_lab == 0) continue;  // (uniform per wave: background costs its label bytes only)
    bool valid = false, in_range = false;
    long long q[3] = {0, 0, 0};
    if (lab != 0) {
      const float d = dep[k];
      valid = isfinite(d) && d > a.dmin && d <= a.dmax && (a.conf == nullptr || cnf[k] > a.thr);  // rule 1, as mask_valid
      if (valid) {
        const f32x4 pt = mask_point(K, E, xk, yk, d);
        in_range = fabsf(pt[0]) < 262144.f && fabsf(pt[1]) < 262144.f && fabsf(pt[2]) < 262144.f;  // (false for NaN and inf)
        if (in_range)
#pragma unroll
          for (int c = 0; c < 3; ++c) q[c] = (long long)rint((double)pt[c] * 1048576.0);
      }
    }
    const int first = __shfl(lab, __ffsll((long long)m_lab) - 1, 64);
    if (__ballot(lab != 0 && lab != first) == 0) {  // one label in the wave: reduce across it, then one LDS add per word
      const u64 m_in = __ballot(in_range), m_out = __ballot(valid && !in_range);
      long long s[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] = m_in ? wave_sum_i64(q[c]) : 0;
      if (lane == 0) {
        u64* acc = s_acc + first * MQ_WORDS;
        atomicAdd(acc + W_PIXELS, (u64)__popcll(m_lab));
        if (m_in) {
          atomicAdd(acc + W_COUNT, (u64)__popcll(m_in));
#pragma unroll
          for (int c = 0; c < 3; ++c) atomicAdd(acc + W_SUM + c, (u64)s[c]);
        }
        if (m_out) atomicAdd(acc + W_OOR, (u64)__popcll(m_out));
      }
    } else if (lab != 0) {  // several labels: every lane adds its own
      u64* acc = s_acc + lab * MQ_WORDS;
      atomicAdd(acc + W_PIXELS, 1ull);
      if (in_range) {
        atomicAdd(acc + W_COUNT, 1ull);
#pragma unroll
        for (int c = 0; c < 3; ++c) atomicAdd(acc + W_SUM + c, (u64)q[c]);
      } else if (valid) {
        atomicAdd(acc + W_OOR, 1ull);
      }
    }
  }
  __syncthreads();
  // flush the labels this workgroup met: 64-bit integer adds, order-free
  const int l = tid;  // MQ_WG == MQ_L
  if (s_acc[l * MQ_WORDS + W_PIXELS] != 0) {
    u64* dst = stats + (cam * MQ_L + l) * MQ_WORDS;
#pragma unroll
    for (int c = 0; c < MQ_WORDS; ++c) {
      const u64 v = s_acc[l * MQ_WORDS + c];
      if (v != 0) atomicAdd(dst + c, v);
    }
  }
}
static_assert(MQ_WG == MQ_L, "the flush of mask_stats_kernel gives every thread one label");

// One thread per (view, label), its T frames in turn: the centroid where count >= min_pixels, NaN elsewhere.
__global__ __launch_bounds__(MQ_WG) void mask_centroid_kernel(const long long* __restrict__ stats, int V, int T, int min_pixels,
                                                              double* __restrict__ centroid) {
  const int i = blockIdx.x * MQ_WG + threadIdx.x;
  if (i >= V * MQ_L) return;
  const int v = i / MQ_L, l = i % MQ_L;
  for (int t = 0; t < T; ++t) {
    const long long row = ((long long)v * T + t) * MQ_L + l;
    const long long n = stats[row * MQ_WORDS + W_COUNT];
    const bool ok = n >= (long long)min_pixels && n > 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      centroid[row * 3 + c] = ok ? (double)stats[row * MQ_WORDS + W_SUM + c] / (double)n * 0x1p-20 : __builtin_nan("");
  }
}

// ------------------------------------------------------------------------------------------------------------- matching
// Mean centroid distance of (v, l) and (u, m) over their common frames, added in ascending frame order; NaN with fewer than
// min_common of them.
__device__ double pair_distance(const double* __restrict__ centroid, int T, int v, int l, int u, int m, int min_common) {
  double sum = 0.0;
  int n = 0;
  for (int t = 0; t < T; ++t) {
    const double* a = centroid + (((long long)v * T + t) * MQ_L + l) * 3;
    const double* b = centroid + (((long long)u * T + t) * MQ_L + m) * 3;
    if (a[0] == a[0] && b[0] == b[0]) {  // (a centroid is NaN in all three coordinates or in none)
      const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
      sum += sqrt(dx * dx + dy * dy + dz * dz);
      ++n;
    }
  }
  return n >= min_common && n > 0 ? sum / (double)n : __builtin_nan("");
}

// (view, label) i = v * 256 + l is present when it has a centroid in at least one frame.
__device__ bool id_present(const double* __restrict__ centroid, int T, int i) {
  bool p = false;
  for (int t = 0; t < T; ++t) {
    const double c = centroid[(((long long)(i / MQ_L) * T + t) * MQ_L + (i % MQ_L)) * 3];
    p = p || c == c;
  }
  return p;
}

// One workgroup.  ids: the present (view, label) pairs as v * 256 + l, ascending (workspace of V * 256 int32).  The greedy pass takes
// them in that order; the candidates of one id (the present ids of earlier cameras) are dealt over the threads, and the global id it
// joins is the one of the candidate with the smallest (distance, global id) -- the minimum over a global id's members, ties to the
// lowest id, in one reduction that no order of evaluation changes.  state: [0] objects, [1] present ids.
__global__ __launch_bounds__(MQ_WG) void mask_match_kernel(const double* __restrict__ centroid, int V, int T, int min_common, double threshold,
                                                           int match, int* __restrict__ ids, int* __restrict__ global_id,
                                                           double* __restrict__ distance, int* __restrict__ state) {
  __shared__ u64 s_scan[MQ_WG / 64];
  __shared__ double s_d[MQ_WG / 64];
  __shared__ int s_g[MQ_WG / 64];
  __shared__ int s_next;
  const int tid = threadIdx.x, n = V * MQ_L;
  const int chunk = (n + MQ_WG - 1) / MQ_WG;  // (= V)
  // present ids, compacted in ascending order: thread tid owns the ids [tid * chunk, (tid + 1) * chunk); count, scan, write
  u64 mine = 0;
  for (int j = 0; j < chunk; ++j) {
    const int i = tid * chunk + j;
    if (i < n) {
      mine += id_present(centroid, T, i) ? 1 : 0;
      global_id[i] = -1;
      distance[i] = __builtin_nan("");
    }
  }
  u64 total;
  u64 off = wg_excl_scan_u64(mine, s_scan, total);
  for (int j = 0; j < chunk; ++j) {
    const int i = tid * chunk + j;
    if (i < n && id_present(centroid, T, i)) ids[off++] = i;
  }
  const int np = (int)total;
  if (tid == 0) s_next = 0;
  __syncthreads();
  if (!match) {  // the labels are global already: label l is object l - 1
    int top = 0;
    for (int k = tid; k < np; k += MQ_WG) {
      const int i = ids[k];
      global_id[i] = i % MQ_L - 1;
      top = max(top, i % MQ_L);
    }
    atomicMax(&s_next, top);
    __syncthreads();
    if (tid == 0) {
      state[0] = s_next;
      state[1] = np;
    }
    return;
  }
  int v_first = 0;  // index in ids of the first id of the current camera: the candidates are ids[0 .. v_first)
  for (int k = 0; k < np; ++k) {
    const int i = ids[k], v = i / MQ_L, l = i % MQ_L;
    while (ids[v_first] / MQ_L < v) ++v_first;  // (v_first <= k: bounded)
    double best = INFINITY;
    int best_g = 0x7fffffff;
    for (int c = tid; c < v_first; c += MQ_WG) {
      const int j = ids[c];
      const double d = pair_distance(centroid, T, v, l, j / MQ_L, j % MQ_L, min_common);
      const int g = global_id[j];
      if (d == d && (d < best || (d == best && g < best_g))) {
        best = d;
        best_g = g;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double od = __shfl_xor(best, o, 64);
      const int og = __shfl_xor(best_g, o, 64);
      if (od < best || (od == best && og < best_g)) {
        best = od;
        best_g = og;
      }
    }
    if ((tid & 63) == 0) {
      s_d[tid >> 6] = best;
      s_g[tid >> 6] = best_g;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < MQ_WG / 64; ++w)
        if (s_d[w] < best || (s_d[w] == best && s_g[w] < best_g)) {
          best = s_d[w];
          best_g = s_g[w];
        }
      if (best_g != 0x7fffffff && best < threshold) {
        global_id[i] = best_g;
        distance[i] = best;
      } else {
        global_id[i] = s_next++;
      }
    }
    __threadfence_block();
    __syncthreads();  // global_id[i] is read by the next ids' candidates
  }
  if (tid == 0) {
    state[0] = s_next;
    state[1] = np;
  }
}

// ------------------------------------------------------------------------------------------------------------- relabel
// 16 pixels per thread: one 16-byte load, four 16-byte stores.
__global__ __launch_bounds__(MQ_WG) void mask_relabel_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ table,
                                                             long long per_view, long long total, int* __restrict__ out) {
  const long long b = ((long long)blockIdx.x * MQ_WG + threadIdx.x) * 16;
  if (b >= total) return;
  if (b + 16 <= total) {
    const uint4 w = *reinterpret_cast<const uint4*>(labels + b);
    const unsigned char* wb = reinterpret_cast<const unsigned char*>(&w);
    int o[16];
    long long v = b / per_view, next = (v + 1) * per_view;  // one division per thread: the view changes at most 16 times in 16 pixels
    for (int e = 0; e < 16; ++e) {
      while (b + e >= next) {
        ++v;
        next += per_view;
      }
      o[e] = wb[e] ? table[v * MQ_L + wb[e]] : -1;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) *reinterpret_cast<int4*>(out + b + 4 * e) = make_int4(o[4 * e], o[4 * e + 1], o[4 * e + 2], o[4 * e + 3]);
  } else {
    for (long long p = b; p < total; ++p) {
      const int lab = labels[p];
      out[p] = lab ? table[p / per_view * MQ_L + lab] : -1;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- object pool
// Pixel i of the (V,H,W) raster of frame t: kept when it is a valid pixel (rule 1) whose (view, label) belongs to object g.
__device__ __forceinline__ bool object_point(const MaskArgs& a, const int* __restrict__ table, int g, int t, int i, f32x4& p) {
  const int x = i % a.W, r = i / a.W, y = r % a.H, v = r / a.H;
  const long long cam = (long long)v * a.T + t;
  const long long src = (cam * a.H + y) * a.W + x;
  const int lab = a.labels[src];
  if (lab == 0 || table[v * MQ_L + lab] != g) return false;
  float d;
  if (!mask_valid(a, src, d)) return false;
  p = mask_point(a.kinv + cam * 9, a.einv + cam * 12, x, y, d);
  return true;
}

__global__ __launch_bounds__(MQ_WG) void object_count_kernel(MaskArgs a, const int* __restrict__ table, int g, int t, int n,
                                                             int* __restrict__ block_counts) {
  __shared__ int s_cnt[MQ_WG / 64];
  const int i = blockIdx.x * MQ_WG + threadIdx.x;
  f32x4 p;
  const bool keep = i < n && object_point(a, table, g, t, i, p);
  const u64 m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(MQ_WG) void object_scan_kernel(int* __restrict__ block_counts, int nb, int chunk, int* __restrict__ count) {
  block_counts_scan(block_counts, nb, chunk, count);
}

__global__ __launch_bounds__(MQ_WG) void object_scatter_kernel(MaskArgs a, const int* __restrict__ table, int g, int t, int n,
                                                               const int* __restrict__ block_base, int capacity, float* __restrict__ pool,
                                                               int* __restrict__ pixel) {
  __shared__ int s_cnt[MQ_WG / 64];
  const int i = blockIdx.x * MQ_WG + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 p;
  const bool keep = i < n && object_point(a, table, g, t, i, p);
  const u64 m = __ballot(keep);
  if (lane == 0) s_cnt[wave] = __popcll(m);
  __syncthreads();
  int base = block_base[blockIdx.x];
  for (int w = 0; w < wave; ++w) base += s_cnt[w];
  const long long pos = base + __popcll(m & ((1ull << lane) - 1ull));
  if (keep && pos < capacity) {  // (capacity: the rows the caller allocated; a pool that outgrew them is cut, never written past)
    pool[pos * 3] = p[0];
    pool[pos * 3 + 1] = p[1];
    pool[pos * 3 + 2] = p[2];
    pixel[pos] = i;
  }
}

inline bool aligned(const void* p, size_t a) { return p && ((uintptr_t)p % a) == 0; }

inline bool clip_ok(const unsigned char* labels, const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T,
                    int H, int W, float dmin, float dmax, float thr) {
  return aligned(labels, 16) && aligned(depths, 4) && (conf == nullptr || aligned(conf, 4)) && aligned(kinv, 4) && aligned(einv, 4) && V > 0 &&
         T > 0 && H > 0 && W > 0 && (long long)H * W <= (1ll << 24) && (long long)V * T <= 65535 && V <= MVT_MASK_MAX_VIEWS &&
         (long long)V * H * W < (1ll << 31) && dmin == dmin && dmax == dmax && thr == thr;
}

}  // namespace

extern "C" int mvt_mask_stats(const unsigned char* labels, const float* depths, const float* conf, const float* kinv, const float* einv, int V,
                              int T, int H, int W, float min_depth, float max_depth, float conf_thresh, long long* stats, void* stream) {
  MVT_REQUIRE(clip_ok(labels, depths, conf, kinv, einv, V, T, H, W, min_depth, max_depth, conf_thresh) && aligned(stats, 16));
  const long long HW = (long long)H * W, total = HW * V * T;
  MaskArgs a = {labels, depths, conf, kinv, einv, V, T, H, W, min_depth, max_depth, conf_thresh};
  hipStream_t s = mvt_stream(stream);
  const long long words = (long long)V * T * MQ_L * MQ_WORDS;
  hipLaunchKernelGGL(mask_clear_kernel, dim3((unsigned)mvt_cdiv(words, 2 * MQ_WG)), dim3(MQ_WG), 0, s, (u64*)stats, words);
  const int spans = (int)mvt_cdiv(HW + 15, MQ_SPAN);  // an image starts at most 15 bytes after a 16-byte boundary
  hipLaunchKernelGGL(mask_stats_kernel, dim3(spans, V * T), dim3(MQ_WG), 0, s, a, HW, total, (u64*)stats);
  return mvt_launch_status();
}

extern "C" int mvt_mask_centroids(const long long* stats, int V, int T, int min_pixels, double* centroid, void* stream) {
  MVT_REQUIRE(aligned(stats, 8) && aligned(centroid, 8) && V > 0 && V <= MVT_MASK_MAX_VIEWS && T > 0 && (long long)V * T <= 65535 && min_pixels >= 1);
  hipLaunchKernelGGL(mask_centroid_kernel, dim3((int)mvt_cdiv((long long)V * MQ_L, MQ_WG)), dim3(MQ_WG), 0, mvt_stream(stream), stats, V, T,
                     min_pixels, centroid);
  return mvt_launch_status();
}

extern "C" int mvt_mask_match(const double* centroid, int V, int T, int min_common_frames, double distance_threshold, int match, int* ids,
                              int* global_id, double* distance, int* state, void* stream) {
  MVT_REQUIRE(aligned(centroid, 8) && aligned(ids, 4) && aligned(global_id, 4) && aligned(distance, 8) && aligned(state, 4));
  MVT_REQUIRE(V > 0 && V <= MVT_MASK_MAX_VIEWS && T > 0 && (long long)V * T <= 65535 && min_common_frames >= 1);
  MVT_REQUIRE(distance_threshold == distance_threshold && (match == 0 || match == 1));
  hipLaunchKernelGGL(mask_match_kernel, dim3(1), dim3(MQ_WG), 0, mvt_stream(stream), centroid, V, T, min_common_frames, distance_threshold, match,
                     ids, global_id, distance, state);
  return mvt_launch_status();
}

extern "C" int mvt_mask_relabel(const unsigned char* labels, const int* table, int V, int T, int H, int W, int* out, void* stream) {
  MVT_REQUIRE(aligned(labels, 16) && aligned(table, 4) && aligned(out, 16) && V > 0 && V <= MVT_MASK_MAX_VIEWS && T > 0 && H > 0 && W > 0);
  MVT_REQUIRE((long long)H * W <= (1ll << 24) && (long long)V * T <= 65535);
  const long long per_view = (long long)T * H * W, total = per_view * V;
  hipLaunchKernelGGL(mask_relabel_kernel, dim3((unsigned)mvt_cdiv(mvt_cdiv(total, 16), MQ_WG)), dim3(MQ_WG), 0, mvt_stream(stream), labels, table,
                     per_view, total, out);
  return mvt_launch_status();
}

extern "C" int mvt_mask_pool(const unsigned char* labels, const float* depths, const float* conf, const float* kinv, const float* einv, int V,
                             int T, int t, int H, int W, float min_depth, float max_depth, float conf_thresh, const int* table, int object,
                             int capacity, float* pool, int* pixel, int* count, int* block_counts, void* stream) {
  MVT_REQUIRE(clip_ok(labels, depths, conf, kinv, einv, V, T, H, W, min_depth, max_depth, conf_thresh) && t >= 0 && t < T && object >= 0);
  MVT_REQUIRE(aligned(table, 4) && aligned(count, 4) && aligned(block_counts, 4) && capacity >= 0);
  MVT_REQUIRE(capacity == 0 || (aligned(pool, 4) && aligned(pixel, 4)));
  const int n = V * H * W;
  const int nb = (int)mvt_cdiv(n, MQ_WG);
  MaskArgs a = {labels, depths, conf, kinv, einv, V, T, H, W, min_depth, max_depth, conf_thresh};
  hipStream_t s = mvt_stream(stream);
  hipLaunchKernelGGL(object_count_kernel, dim3(nb), dim3(MQ_WG), 0, s, a, table, object, t, n, block_counts);
  hipLaunchKernelGGL(object_scan_kernel, dim3(1), dim3(MQ_WG), 0, s, block_counts, nb, (int)mvt_cdiv(nb, MQ_WG), count);
  hipLaunchKernelGGL(object_scatter_kernel, dim3(nb), dim3(MQ_WG), 0, s, a, table, object, t, n, block_counts, capacity, pool, pixel);
  return mvt_launch_status();
}
