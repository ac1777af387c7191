// Cloud preparation (reference: conversions/droid/utils/optimization.py downsample_pointcloud / estimate_normals, i.e. Open3D's
// voxel_down_sample and estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))).  Two independent parts:
//
// normals      - PCA normals of every point of a cloud over its max_nn nearest points within the radius.  The walk is
//                walk_cloud (cloud_search.h), as in cloud_clean.hip: a wave owns one tile of 64 points, ONE QUERY PER LANE, candidates are
//                broadcast lane by lane; pass 0 visits the ring, pass 1 the rest through the group and tile boxes, and a box is
//                skipped only when its lower bound EXCEEDS the lane's bound (strictly: an equal-d2 point with a lower index in a
//                tile visited later still wins).  What differs is the list: a query keeps the max_nn smallest (d2, index) PAIRS in
//                its own LDS column (d2[k][lane], index[k][lane]: conflict free), with r^2 as the bound until the list is full and
//                the largest key afterwards.  At the end every lane takes its list in ascending key order, gathers the neighbours,
//                sums S1 and S2 of the exact fp64 differences, forms the covariance and solves the 3x3 eigenproblem by cyclic
//                Jacobi with a fixed number of sweeps.  Workgroup = one wave: max_nn * 512 bytes of LDS (32 KiB at 64), no
//                barrier, no atomics, every loop bounded by the tile count, max_nn or the sweep count.
// voxel        - a hash grid.  bounds: the per-axis minimum -> the origin.  insert: one thread per point claims the slot of its
//                cell with a 64-bit compare-and-swap (linear probing bounded by the capacity; a failed swap returns the slot's
//                key, which is either its own or somebody else's: then it moves on -- nothing spins on another thread) and adds
//                its count, its index (atomicMin) and its fixed-point offsets inside the cell with INTEGER atomics, so no result
//                depends on the order of arrival.  emit: the points that are the first of their cell, in input order (count, scan,
//                scatter as mvt_query_pool), each writing its cell's mean, count and first index; then the labels.
// No fused multiply-add is formed from a product and a sum written separately in this file: the fp64 results are those of the
// same operations in numpy.
#include "block_scan.h"
#include "cloud_search.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int NE_SWEEPS = 8;  // cyclic Jacobi sweeps of a 3x3 (fp64 converges in 4 to 5)
constexpr int VX_WG = 256;
static_assert(VX_WG == SCAN_WG, "block_counts_scan is written for this workgroup size");
constexpr u64 VX_EMPTY = ~0ull;  // (a key has 63 bits)

__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000ll); }

// One rotation of the cyclic Jacobi method on the symmetric a, annihilating a[P_][Q_]; the columns of v follow.
template <int P_, int Q_>
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
  constexpr int R_ = 3 - P_ - Q_;
  const double apq = a[P_][Q_];
  if (apq == 0.0) return;
  const double theta = (a[Q_][Q_] - a[P_][P_]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // (theta = +-inf: t = +-0)
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double arp = a[R_][P_], arq = a[R_][Q_];
  a[P_][P_] -= t * apq;
  a[Q_][Q_] += t * apq;
  a[P_][Q_] = a[Q_][P_] = 0.0;
  a[R_][P_] = a[P_][R_] = c * arp - s * arq;
  a[R_][Q_] = a[Q_][R_] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = v[k][P_], vq = v[k][Q_];
    v[k][P_] = c * vp - s * vq;
    v[k][Q_] = s * vp + c * vq;
  }
}

// Unit eigenvector n of the smallest eigenvalue of the covariance c6 = (xx, xy, xz, yy, yz, zz); false when
// lambda_mid <= 1e-12 lambda_max (the neighbours are collinear or coincident).
__device__ __forceinline__ bool smallest_eigenvector(const double (&c6)[6], double (&n)[3]) {
  double a[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < NE_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<1, 2>(a, v);
  }
  const double d0 = a[0][0], d1 = a[1][1], d2 = a[2][2];
  const double lmax = fmax(fmax(d0, d1), d2);
  const double lmid = fmax(fmin(d0, d1), fmin(fmax(d0, d1), d2));
  if (!(lmid > 1e-12 * lmax)) return false;
  const int im = (d0 <= d1 && d0 <= d2) ? 0 : (d1 <= d2 ? 1 : 2);
#pragma unroll
  for (int k = 0; k < 3; ++k) n[k] = im == 0 ? v[k][0] : (im == 1 ? v[k][1] : v[k][2]);
  const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) n[k] /= len;
  return true;
}

// What a query keeps during the walk: the K smallest (d2, index) pairs in its LDS columns, with r2 as the bound until the list is
// full and the largest d2 afterwards.  Candidates arrive in ascending index order within a tile.
struct normals_visitor : walk_defaults {
  float* ld2;  // entry k of this lane's query: ld2[k * 64], lix[k * 64]
  int* lix;
  int K;
  float r2;
  bool valid;
  int cnt, wpos, widx;  // entries kept; the place and the key (wd2, widx) of the largest once cnt == K
  float wd2;
  __device__ __forceinline__ normals_visitor(float* ld2_, int* lix_, int K_, float r2_, bool valid_)
      : ld2(ld2_), lix(lix_), K(K_), r2(r2_), valid(valid_), cnt(0), wpos(0), widx(-1), wd2(-1.f) {}
  // r^2 until the list is full, then its largest d2 (-inf: no query in this lane)
  __device__ __forceinline__ float bound() const { return valid ? (cnt < K ? r2 : wd2) : -inf_f(); }
  __device__ __forceinline__ bool candidate(int, const f32x4& p) const { return finite3(p); }  // NaN points take no part
  __device__ __forceinline__ void visit(int j, int ci, float d2) {
    const int cj = __builtin_amdgcn_readlane(ci, j);
    bool rescan = false;
    if (cnt < K) {
      if (d2 < r2) {
        ld2[cnt * 64] = d2;
        lix[cnt * 64] = cj;
        rescan = ++cnt == K;
      }
    } else if (d2 < wd2 || (d2 == wd2 && cj < widx)) {
      ld2[wpos * 64] = d2;
      lix[wpos * 64] = cj;
      rescan = true;
    }
    if (rescan) {  // the largest key of the full list
      wd2 = -1.f;
      widx = -1;
      for (int k = 0; k < K; ++k) {
        const float v = ld2[k * 64];
        const int ix = lix[k * 64];
        if (v > wd2 || (v == wd2 && ix > widx)) {
          wd2 = v;
          widx = ix;
          wpos = k;
        }
      }
    }
  }
};

// One wave per (cloud, tile); lane = query.  LDS: [K][64] d2, then [K][64] indices.
__global__ __launch_bounds__(64) void normals_kernel(const float* __restrict__ xyz, long long P, int ntiles, int grid_w, int K, float r2,
                                                     const float* __restrict__ box, const float* __restrict__ gbox,
                                                     const float* __restrict__ viewpoint, float* __restrict__ nrm, int* __restrict__ nbr_idx,
                                                     int* __restrict__ nbr_cnt, double* __restrict__ cov) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  const int tile = blockIdx.x;  // (< ntiles: the grid has exactly ntiles workgroups per cloud)
  const long long cloud = blockIdx.y;
  const cloud_view cv = cloud_of(xyz, box, gbox, cloud, P, ntiles, grid_w);
  const float* __restrict__ cand = cv.xyz;
  float* ld2 = lds + lane;                                    // entry k of this lane's query: ld2[k * 64], lix[k * 64]
  int* lix = reinterpret_cast<int*>(lds + (size_t)K * 64) + lane;

  const int qi = cloud_tile_point(tile, lane, grid_w);
  f32x4 q = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};
  if (qi < P) q = *reinterpret_cast<const f32x4*>(cand + (long long)qi * 4);
  const bool valid = finite3(q);
  const f32x4 qlo = *reinterpret_cast<const f32x4*>(cv.box + (long long)tile * 8), qhi = *reinterpret_cast<const f32x4*>(cv.box + (long long)tile * 8 + 4);

  normals_visitor vis(ld2, lix, K, r2, valid);
  const int npass = __ballot(valid) ? 2 : 0;  // (a tile of NaNs has nothing to search for)
  for (int pass = 0; pass < npass; ++pass) walk_cloud(cv, q, qlo, qhi, tile, pass == 0 ? VISIT_RING : VISIT_REST, vis);
  const int cnt = vis.cnt;

  // The list in ascending (d2, index) order: neighbour indices out, S1 and S2 of the exact differences in fp64.
  double s1[3] = {0.0, 0.0, 0.0}, s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double qx = (double)q[0], qy = (double)q[1], qz = (double)q[2];
  const long long row = cloud * P + qi;
  for (int r = 0; r < K; ++r) {
    int mi = -1;
    if (r < cnt) {
      float m = inf_f();
      int mp = 0;
      mi = 0x7fffffff;
      for (int k = 0; k < cnt; ++k) {
        const float v = ld2[k * 64];  // (+inf: taken)
        const int ix = lix[k * 64];
        if (v < m || (v == m && ix < mi)) {
          m = v;
          mi = ix;
          mp = k;
        }
      }
      ld2[mp * 64] = inf_f();
      const f32x4 p = *reinterpret_cast<const f32x4*>(cand + (long long)mi * 4);  // (mi < P: it was read as a candidate)
      const double ex = (double)p[0] - qx, ey = (double)p[1] - qy, ez = (double)p[2] - qz;
      s1[0] += ex, s1[1] += ey, s1[2] += ez;
      s2[0] += ex * ex, s2[1] += ex * ey, s2[2] += ex * ez, s2[3] += ey * ey, s2[4] += ey * ez, s2[5] += ez * ez;
    }
    if (nbr_idx && qi < P) nbr_idx[row * K + r] = mi;
  }
  if (qi >= P) return;
  if (nbr_cnt) nbr_cnt[row] = valid ? cnt : -1;
  double c6[6];
  const double n = (double)cnt;
  const double mx = s1[0] / n, my = s1[1] / n, mz = s1[2] / n;
  c6[0] = s2[0] / n - mx * mx, c6[1] = s2[1] / n - mx * my, c6[2] = s2[2] / n - mx * mz;
  c6[3] = s2[3] / n - my * my, c6[4] = s2[4] / n - my * mz, c6[5] = s2[5] / n - mz * mz;
  if (cov)
    for (int k = 0; k < 6; ++k) cov[row * 6 + k] = valid ? c6[k] : nan_d();
  f32x4 o = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};
  double nv[3];
  if (valid && cnt >= 3 && smallest_eigenvector(c6, nv)) {
    if (viewpoint) {  // towards the viewpoint: n . (vp - p) >= 0
      const float* vp = viewpoint + cloud * 3;
      const double dot = nv[0] * ((double)vp[0] - qx) + nv[1] * ((double)vp[1] - qy) + nv[2] * ((double)vp[2] - qz);
      if (dot < 0.0) nv[0] = -nv[0], nv[1] = -nv[1], nv[2] = -nv[2];
    }
    o[0] = (float)nv[0], o[1] = (float)nv[1], o[2] = (float)nv[2];
  }
  *reinterpret_cast<f32x4*>(nrm + row * 4) = o;
}

// ------------------------------------------------------------------------------------------------------------- voxel grid
// Words of the state (include/mvtracker_hip.h, MVT_VOXEL_*).
enum { VS_ORIGIN = MVT_VOXEL_ORIGIN, VS_SIZE = MVT_VOXEL_SIZE, VS_STATUS = MVT_VOXEL_STATUS, VS_POINTS = MVT_VOXEL_POINTS };

// The table: capacity slots in one buffer of capacity * MVT_VOXEL_SLOT_WORDS 64-bit words.
struct VoxelTable {
  u64* keys;   // [cap] packed cell, VX_EMPTY when free
  u64* sums;   // [cap][3] fixed-point offsets inside the cell
  int* cnt;    // [cap]
  int* first;  // [cap] smallest input index
  int* row;    // [cap] output row (emit)
  u64 mask;
};

__host__ __device__ __forceinline__ VoxelTable voxel_table(long long* table, long long cap) {
  u64* w = reinterpret_cast<u64*>(table);
  int* iw = reinterpret_cast<int*>(w + 4 * cap);
  return {w, w + cap, iw, iw + cap, iw + 2 * cap, (u64)cap - 1};
}

__device__ __forceinline__ u64 voxel_hash(u64 k) {  // splitmix64's finaliser
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

// Cell of p: u = ((double)p - origin) / voxel, cell = floor(u), frac = u - cell.  False when a cell index leaves [0, 2^21).
__device__ __forceinline__ bool voxel_cell(const f32x4& p, const long long* __restrict__ state, u64& key, double (&frac)[3]) {
  const double* st = reinterpret_cast<const double*>(state);
  const double voxel = st[VS_SIZE];
  bool ok = true;
  key = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double u = ((double)p[c] - st[VS_ORIGIN + c]) / voxel;
    const double cell = floor(u);
    ok = ok && cell >= 0.0 && cell < 2097152.0;
    frac[c] = u - cell;
    key |= (ok ? (u64)cell : 0ull) << (21 * c);
  }
  return ok;
}

// The slot that holds key (linear probing from its hash), or -1 when the probe meets a free slot or has gone round.
__device__ __forceinline__ long long voxel_find(const VoxelTable& t, u64 key) {
  u64 slot = voxel_hash(key) & t.mask;
  for (u64 probe = 0; probe <= t.mask; ++probe) {
    const u64 k = t.keys[slot];
    if (k == key) return (long long)slot;
    if (k == VX_EMPTY) return -1;
    slot = (slot + 1) & t.mask;
  }
  return -1;
}

// Point i takes part and lies in a cell: its slot; else -1.
__device__ __forceinline__ long long voxel_slot_of(const float* __restrict__ xyz, long long P, long long i, const long long* __restrict__ state,
                                                   const VoxelTable& t) {
  if (i >= P || state[VS_STATUS] != 0) return -1;
  const f32x4 p = *reinterpret_cast<const f32x4*>(xyz + i * 4);
  u64 key;
  double frac[3];
  if (!finite3(p) || !voxel_cell(p, state, key, frac)) return -1;
  return voxel_find(t, key);
}

// partial [blocks][4]: the minimum of the finite points per axis and their number.
__global__ __launch_bounds__(VX_WG) void voxel_min_kernel(const float* __restrict__ xyz, long long P, double* __restrict__ partial) {
  __shared__ float s_lo[VX_WG / 64][3];
  __shared__ int s_n[VX_WG / 64];
  float lo[3] = {inf_f(), inf_f(), inf_f()};
  int n = 0;
  for (long long i = blockIdx.x * (long long)VX_WG + threadIdx.x; i < P; i += (long long)gridDim.x * VX_WG) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(xyz + i * 4);
    if (finite3(p)) {
      lo[0] = fminf(lo[0], p[0]), lo[1] = fminf(lo[1], p[1]), lo[2] = fminf(lo[2], p[2]);
      ++n;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) lo[c] = -wave_max(-lo[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) {
    for (int c = 0; c < 3; ++c) s_lo[threadIdx.x >> 6][c] = lo[c];
    s_n[threadIdx.x >> 6] = n;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    partial[blockIdx.x * 4 + c] = (double)fminf(fminf(s_lo[0][c], s_lo[1][c]), fminf(s_lo[2][c], s_lo[3][c]));
  }
  if (threadIdx.x == 3) partial[blockIdx.x * 4 + 3] = (double)((long long)s_n[0] + s_n[1] + s_n[2] + s_n[3]);
}

// One wave: origin = lo - voxel / 2 in fp64, the voxel size, a clear status and the number of points taking part.
__global__ __launch_bounds__(64) void voxel_origin_kernel(const double* __restrict__ partial, int nb, double voxel, long long* __restrict__ state) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, n = 0.0;
  for (int b = threadIdx.x; b < nb; b += 64) {
    for (int c = 0; c < 3; ++c) lo[c] = fmin(lo[c], partial[b * 4 + c]);
    n += partial[b * 4 + 3];  // (integers below 2^31: exact in any order)
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int c = 0; c < 3; ++c) lo[c] = fmin(lo[c], __shfl_xor(lo[c], o, 64));
    n += __shfl_xor(n, o, 64);
  }
  if (threadIdx.x == 0) {
    double* st = reinterpret_cast<double*>(state);
    for (int c = 0; c < 3; ++c) st[VS_ORIGIN + c] = lo[c] - voxel * 0.5;
    st[VS_SIZE] = voxel;
    state[VS_STATUS] = 0;
    state[VS_POINTS] = (long long)n;
    state[6] = state[7] = 0;
  }
}

__global__ __launch_bounds__(VX_WG) void voxel_clear_kernel(VoxelTable t) {
  for (u64 s = blockIdx.x * (u64)VX_WG + threadIdx.x; s <= t.mask; s += (u64)gridDim.x * VX_WG) {
    t.keys[s] = VX_EMPTY;
    t.sums[s * 3] = t.sums[s * 3 + 1] = t.sums[s * 3 + 2] = 0;
    t.cnt[s] = 0;
    t.first[s] = 0x7fffffff;
    t.row[s] = -1;
  }
}

__global__ __launch_bounds__(VX_WG) void voxel_insert_kernel(const float* __restrict__ xyz, long long P, long long* __restrict__ state, VoxelTable t) {
  const long long i = blockIdx.x * (long long)VX_WG + threadIdx.x;
  if (i >= P) return;
  const f32x4 p = *reinterpret_cast<const f32x4*>(xyz + i * 4);
  if (!finite3(p)) return;
  u64* status = reinterpret_cast<u64*>(state + VS_STATUS);
  u64 key;
  double frac[3];
  if (!voxel_cell(p, state, key, frac)) {
    atomicOr(status, (u64)MVT_VOXEL_RANGE);
    return;
  }
  u64 slot = voxel_hash(key) & t.mask;
  bool found = false;
  for (u64 probe = 0; probe <= t.mask; ++probe) {
    u64 k = __hip_atomic_load(&t.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == VX_EMPTY) {
      k = atomicCAS(&t.keys[slot], VX_EMPTY, key);  // (the slot's key before the swap: free -> it is ours now)
      if (k == VX_EMPTY) k = key;
    }
    if (k == key) {
      found = true;
      break;
    }
    slot = (slot + 1) & t.mask;  // somebody else's cell: move on
  }
  if (!found) {
    atomicOr(status, (u64)MVT_VOXEL_FULL);
    return;
  }
  atomicAdd(&t.cnt[slot], 1);
  atomicMin(&t.first[slot], (int)i);
#pragma unroll
  for (int c = 0; c < 3; ++c) atomicAdd(&t.sums[slot * 3 + c], (u64)rint(frac[c] * 4294967296.0));  // in [0, 2^32]; P < 2^31 of them stay below 2^63
}

__global__ __launch_bounds__(VX_WG) void voxel_count_kernel(const float* __restrict__ xyz, long long P, const long long* __restrict__ state, VoxelTable t,
                                                            int* __restrict__ block_counts) {
  __shared__ int s_cnt[VX_WG / 64];
  const long long i = blockIdx.x * (long long)VX_WG + threadIdx.x;
  const long long slot = voxel_slot_of(xyz, P, i, state, t);
  const bool keep = slot >= 0 && t.first[slot] == (int)i;
  const u64 m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(VX_WG) void voxel_scan_kernel(int* __restrict__ block_counts, int nb, int chunk, int* __restrict__ n_out) {
  block_counts_scan(block_counts, nb, chunk, n_out);
}

__global__ __launch_bounds__(VX_WG) void voxel_scatter_kernel(const float* __restrict__ xyz, long long P, const long long* __restrict__ state, VoxelTable t,
                                                              const int* __restrict__ block_base, float* __restrict__ points, int* __restrict__ counts,
                                                              int* __restrict__ first) {
  __shared__ int s_cnt[VX_WG / 64];
  const long long i = blockIdx.x * (long long)VX_WG + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long slot = voxel_slot_of(xyz, P, i, state, t);
  const bool keep = slot >= 0 && t.first[slot] == (int)i;
  const u64 m = __ballot(keep);
  if (lane == 0) s_cnt[wave] = __popcll(m);
  __syncthreads();
  int base = block_base[blockIdx.x];  // base + (kept before me in this workgroup) < the total <= the points taking part <= P
  for (int w = 0; w < wave; ++w) base += s_cnt[w];
  if (keep) {
    const long long pos = base + __popcll(m & ((1ull << lane) - 1ull));
    const double* st = reinterpret_cast<const double*>(state);
    const u64 key = t.keys[slot];
    const int n = t.cnt[slot];
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double cell = (double)((key >> (21 * c)) & 0x1fffffull);
      const double mean = (double)t.sums[slot * 3 + c] / ((double)n * 4294967296.0);
      o[c] = (float)(st[VS_ORIGIN + c] + (cell + mean) * st[VS_SIZE]);
    }
    o[3] = 0.f;
    *reinterpret_cast<f32x4*>(points + pos * 4) = o;
    counts[pos] = n;
    first[pos] = (int)i;
    t.row[slot] = (int)pos;
  }
}

__global__ __launch_bounds__(VX_WG) void voxel_label_kernel(const float* __restrict__ xyz, long long P, const long long* __restrict__ state, VoxelTable t,
                                                            int* __restrict__ labels) {
  const long long i = blockIdx.x * (long long)VX_WG + threadIdx.x;
  if (i >= P) return;
  const long long slot = voxel_slot_of(xyz, P, i, state, t);
  labels[i] = slot >= 0 ? t.row[slot] : -1;
}

inline bool voxel_args(const float* xyz, long long P, const long long* state) { return aligned(xyz, 16) && aligned(state, 8) && P > 0 && P < (1ll << 31); }
inline bool voxel_capacity(long long cap, long long P) { return cap >= 2 * P && cap <= (1ll << 32) && (cap & (cap - 1)) == 0; }

}  // namespace

extern "C" int mvt_normals_estimate(const float* xyz, int C, long long P, int grid_w, int grid_h, int max_nn, float radius, const float* tile_box,
                                    const float* group_box, const float* viewpoint, float* nrm, int* nbr_idx, int* nbr_cnt, double* cov,
                                    void* stream) {
  MVT_REQUIRE(aligned(xyz, 16) && aligned(tile_box, 16) && aligned(group_box, 16) && aligned(nrm, 16));
  MVT_REQUIRE((viewpoint == nullptr || aligned(viewpoint, 4)) && (nbr_idx == nullptr || aligned(nbr_idx, 4)) &&
              (nbr_cnt == nullptr || aligned(nbr_cnt, 4)) && (cov == nullptr || aligned(cov, 8)));
  MVT_REQUIRE(cloud_shape_ok(C, P, grid_w, grid_h));
  MVT_REQUIRE(max_nn >= 3 && max_nn <= MVT_NORMALS_MAX_NN && radius > 0.f);  // (radius = +inf: plain kNN; NaN fails the compare)
  const int ntiles = (int)((P + 63) / 64);
  hipLaunchKernelGGL(normals_kernel, dim3((unsigned)ntiles, (unsigned)C), dim3(64), (size_t)max_nn * 512, mvt_stream(stream), xyz, P, ntiles, grid_w,
                     max_nn, radius * radius, tile_box, group_box, viewpoint, nrm, nbr_idx, nbr_cnt, cov);
  return mvt_launch_status();
}

extern "C" int mvt_voxel_bounds(const float* xyz, long long P, double voxel, double* partial, long long* state, void* stream) {
  MVT_REQUIRE(voxel_args(xyz, P, state) && aligned(partial, 8) && voxel > 0.0 && voxel < (double)INFINITY);
  const long long b = mvt_cdiv(P, VX_WG);
  const int nb = (int)(b > MVT_VOXEL_BOUND_BLOCKS ? MVT_VOXEL_BOUND_BLOCKS : b);
  hipLaunchKernelGGL(voxel_min_kernel, dim3(nb), dim3(VX_WG), 0, mvt_stream(stream), xyz, P, partial);
  hipLaunchKernelGGL(voxel_origin_kernel, dim3(1), dim3(64), 0, mvt_stream(stream), partial, nb, voxel, state);
  return mvt_launch_status();
}

extern "C" int mvt_voxel_insert(const float* xyz, long long P, long long* state, long long* table, long long capacity, void* stream) {
  MVT_REQUIRE(voxel_args(xyz, P, state) && aligned(table, 8) && voxel_capacity(capacity, P));
  const VoxelTable t = voxel_table(table, capacity);
  hipLaunchKernelGGL(voxel_clear_kernel, dim3(strided_blocks(capacity)), dim3(VX_WG), 0, mvt_stream(stream), t);
  hipLaunchKernelGGL(voxel_insert_kernel, dim3((unsigned)mvt_cdiv(P, VX_WG)), dim3(VX_WG), 0, mvt_stream(stream), xyz, P, state, t);
  return mvt_launch_status();
}

extern "C" int mvt_voxel_emit(const float* xyz, long long P, const long long* state, long long* table, long long capacity, int* block_counts,
                              float* points, int* counts, int* first, int* labels, int* n_out, void* stream) {
  MVT_REQUIRE(voxel_args(xyz, P, state) && aligned(table, 8) && voxel_capacity(capacity, P));
  MVT_REQUIRE(aligned(block_counts, 4) && aligned(points, 16) && aligned(counts, 4) && aligned(first, 4) && aligned(n_out, 4) &&
              (labels == nullptr || aligned(labels, 4)));
  const VoxelTable t = voxel_table(table, capacity);
  const int nb = (int)mvt_cdiv(P, VX_WG);
  hipStream_t s = mvt_stream(stream);
  hipLaunchKernelGGL(voxel_count_kernel, dim3(nb), dim3(VX_WG), 0, s, xyz, P, state, t, block_counts);
  hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(VX_WG), 0, s, block_counts, nb, (int)mvt_cdiv(nb, VX_WG), n_out);
  hipLaunchKernelGGL(voxel_scatter_kernel, dim3(nb), dim3(VX_WG), 0, s, xyz, P, state, t, block_counts, points, counts, first);
  if (labels) hipLaunchKernelGGL(voxel_label_kernel, dim3(nb), dim3(VX_WG), 0, s, xyz, P, state, t, labels);
  return mvt_launch_status();
}
