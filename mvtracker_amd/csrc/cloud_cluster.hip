// Region clustering: DBSCAN of every cloud of a launch and the largest cluster inside an oriented box (reference:
// conversions/droid/mark_gripper_points.py classify_gripper_points -> sklearn.cluster.DBSCAN, then np.argmax(np.bincount(labels))).
//
// The rule, with adj(i, j) = d2(i, j) <= r2 (a point is its own neighbour; d2 is the scan's gap_d2 in fp32):
//   core(i)  = |{j : adj(i, j)}| >= min_samples;
//   clusters = the connected components of the core points under adj, numbered in ascending order of their lowest core index;
//   a non-core point with a core neighbour takes the lowest cluster number among its core neighbours; every other point is -1.
// The labels are a function of the cloud alone, so no traversal order has to be imitated.
//
// cluster_crop   - a point whose coordinates in the region's frame are not strictly inside the box becomes a NaN row (in place).
// cluster_walk   - the self-search of cloud_clean.hip (one wave per tile, one query per lane, candidates broadcast by v_readlane,
//                  pass 0 the ring, pass 1 the rest through group and tile boxes) with the inclusive test, in three forms:
//                    COUNT : a counter per query that stops at min_samples -> core;
//                    LINK  : core queries unite with every core neighbour of lower index in a min-index union-find;
//                    BORDER: valid non-core queries take the smallest root among their core neighbours.
//                  A tile or group without a finite point (count word 0 of its box) is skipped before any load of its points.
// The union-find - parent[x] <= x always, and a parent only ever decreases (every write is an atomicMin), so there is no cycle and
//                  the root of a tree is its smallest index.  unite(a, b): find both roots, atomicMin(parent[larger], smaller); when
//                  the value returned is not `larger`, another lane hooked it first: the edge larger->old may just have been replaced
//                  by larger->smaller, so the pair (old, smaller) is united next.  Each retry's larger root is below the last, so at
//                  most P retries.  Reads of parent are relaxed agent-scope atomic loads (they bypass the CU's L1, which no other
//                  CU's store refreshes); a stale value is an older parent, which stays connected to x by the edges and pending
//                  unions that replaced it, and whether a hook happened is decided by the atomic's return value alone, never by a
//                  read.  When the launch ends no union is pending, so the trees are exactly the components and every root is the
//                  lowest core index of its component, whatever the order of arrival: the same bits in every run.
//                  Three more writes shorten paths and register no pending union: the candidate's parent is lowered to the new root
//                  after a unite, the query's own parent to the lowest index the lane knows, and flatten sets every core point's
//                  parent to its root.  Each replaces x's out-edge by an edge to a node reached FROM x's former parent, along edges
//                  that are not x's own; and every former parent of a node stays equivalent to it without using that node's own
//                  out-edge (a hook or a lowering only ever moves x to a node that its former parent already reaches, or leaves
//                  the pair (old, smaller) pending), so taking the out-edge away disconnects nothing.
//                  Nothing waits on another wave; a find is bounded by P steps and a unite by P retries, and a lane that exceeds
//                  either sets the status word and stops.  The two bounds are nested, not shared: the combined worst case of one
//                  unite is P^2 loads before the status bit, a bound on termination, not on time.
// cluster_finish - one workgroup per cloud: cluster sizes by integer atomicAdd per root (order-independent), the largest with the
//                  lowest root among equals, dense ids by an order-preserving prefix count of the roots, the two fallbacks.
#include "cloud_search.h"

namespace {

constexpr int CL_WG = 128;  // threads per workgroup of the walks (2 waves, no LDS)
constexpr int CF_WG = 256;  // threads of the per-cloud finish
enum { WALK_COUNT = 0, WALK_LINK = 1, WALK_BORDER = 2 };

__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of x: at most `bound` steps (a parent is below its child, so a walk from x < P has fewer than P steps).
__device__ __forceinline__ int uf_find(const int* parent, int x, int bound, bool& bad) {
  for (int it = 0; it <= bound; ++it) {
    const int p = uf_load(parent + x);
    if (p == x) return x;
    x = p;
  }
  bad = true;
  return x;
}

// Unite the trees of a and b; returns the smaller root.
__device__ __forceinline__ int uf_unite(int* parent, int a, int b, int bound, bool& bad) {
  for (int it = 0; it <= bound; ++it) {
    a = uf_find(parent, a, bound, bad);
    b = uf_find(parent, b, bound, bad);
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    if (bad || lo == hi) return lo;
    const int old = atomicMin(parent + hi, lo);
    if (old == hi) return lo;  // hi was a root and now hangs under lo
    a = old;                   // hi had been hooked under old meanwhile: old and lo are still to be united
    b = lo;
  }
  bad = true;
  return a < b ? a : b;
}

__global__ __launch_bounds__(256) void cluster_crop_kernel(float* __restrict__ xyz, long long P, long long total, const float* __restrict__ rtw,
                                                           float xlo, float xhi, float ylo, float yhi, float zlo, float zhi) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const float* m = rtw + (i / P) * 12;
    const f32x4 p = *reinterpret_cast<const f32x4*>(xyz + i * 4);
    const float cx = __fmaf_rn(m[2], p[2], __fmaf_rn(m[1], p[1], __fmaf_rn(m[0], p[0], m[3])));
    const float cy = __fmaf_rn(m[6], p[2], __fmaf_rn(m[5], p[1], __fmaf_rn(m[4], p[0], m[7])));
    const float cz = __fmaf_rn(m[10], p[2], __fmaf_rn(m[9], p[1], __fmaf_rn(m[8], p[0], m[11])));
    const bool in = finite3(p) && cx > xlo && cx < xhi && cy > ylo && cy < yhi && cz > zlo && cz < zhi;  // (a NaN fails every test)
    if (!in) *reinterpret_cast<f32x4*>(xyz + i * 4) = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};
  }
}

// parent[i] = i, and the clouds' state rows cleared (n = the larger of the two element counts)
__global__ __launch_bounds__(256) void cluster_init_kernel(int* __restrict__ parent, long long P, long long total, long long* __restrict__ state,
                                                           long long words, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (i < total) parent[i] = (int)(i % P);
    if (i < words) state[i] = 0;
  }
}

// What a query does during the walk, with the inclusive test d2 <= r2; r2 is the bound of a lane while it is active.
template <int MODE>
struct cluster_visitor : walk_defaults {
  static constexpr bool skip_empty = true;
  const unsigned char* ccore;
  int* cpar;
  float r2;
  int cap, bound_steps, grid_w;
  int qi, qmax;  // the lane's query; LINK: the largest query index of this tile
  bool act;      // has the lane anything left to find?
  int cnt;       // COUNT: neighbours so far, stopped at cap
  int cur;       // LINK: the lowest index this lane knows in its own tree
  int best;      // BORDER: the lowest root among the core neighbours (bound_steps: none)
  bool bad;
  int pv;  // of the lane's candidate of the tile at hand: LINK: a parent (possibly stale: still in its tree); BORDER: its root
  __device__ __forceinline__ cluster_visitor(const unsigned char* ccore_, int* cpar_, float r2_, int cap_, int bound_, int grid_w_, int qi_, int qmax_,
                                             bool act_)
      : ccore(ccore_), cpar(cpar_), r2(r2_), cap(cap_), bound_steps(bound_), grid_w(grid_w_), qi(qi_), qmax(qmax_), act(act_), cnt(0), cur(qi_),
        best(bound_), bad(false), pv(0) {}
  __device__ __forceinline__ float bound() const { return act ? r2 : -inf_f(); }
  __device__ __forceinline__ bool tile_ok(int t) const {  // (LINK: only candidates below the query unite)
    return MODE == WALK_LINK ? cloud_tile_point(t, 0, grid_w) < qmax : true;
  }
  __device__ __forceinline__ bool candidate(int i, const f32x4& p) {
    bool cok = finite3(p);  // NaN points take no part
    pv = 0;
    if (MODE != WALK_COUNT) {
      cok = cok && ccore[i] != 0;
      if (cok) pv = MODE == WALK_LINK ? uf_load(cpar + i) : cpar[i];
    }
    return cok;
  }
  __device__ __forceinline__ void visit(int j, int ci, float d2) {
    const bool hit = act && d2 <= r2;  // (NaN for a NaN query: the compare fails)
    if (MODE == WALK_COUNT) {
      cnt += hit ? 1 : 0;
    } else {
      const int pj = __builtin_amdgcn_readlane(pv, j);
      if (MODE == WALK_BORDER) {
        best = (hit && pj < best) ? pj : best;
      } else {
        const int cj = __builtin_amdgcn_readlane(ci, j);
        if (hit && cj < qi && pj != cur) {  // (pj == cur: the candidate already hangs under this lane's root)
          const int r = uf_unite(cpar, cur, pj, bound_steps, bad);
          if (bad) {
            act = false;
          } else {
            cur = r;
            if (r < pj) atomicMin(cpar + cj, r);  // shorten the candidate's path: r is in its tree and below its parent
          }
        }
      }
    }
  }
  __device__ __forceinline__ void end_tile() {
    if (MODE == WALK_COUNT) {
      cnt = cnt < cap ? cnt : cap;
      act = act && cnt < cap;  // a query that has reached min_samples has nothing left to find
    }
  }
};

// One wave per (cloud, tile); lane = query.  out: core (COUNT) / nothing (LINK) / root (BORDER).
template <int MODE>
__global__ __launch_bounds__(CL_WG) void cluster_walk_kernel(const float* __restrict__ xyz, long long P, int ntiles, int grid_w, float r2, int cap,
                                                             const float* __restrict__ box, const float* __restrict__ gbox,
                                                             unsigned char* __restrict__ core, int* __restrict__ parent, int* __restrict__ root,
                                                             unsigned long long* __restrict__ state) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * (CL_WG / 64) + wave;
  if (tile >= ntiles) return;  // (wave-uniform; the kernel has no workgroup barrier)
  const long long cloud = blockIdx.y;
  const cloud_view cv = cloud_of(xyz, box, gbox, cloud, P, ntiles, grid_w);
  unsigned char* ccore = core + cloud * P;
  int* cpar = MODE == WALK_COUNT ? nullptr : parent + cloud * P;
  const int bound = (int)P;

  const int qi = cloud_tile_point(tile, lane, grid_w);
  f32x4 q = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};
  if (qi < P) q = *reinterpret_cast<const f32x4*>(cv.xyz + (long long)qi * 4);
  const bool valid = finite3(q);
  const bool qcore = MODE != WALK_COUNT && valid && ccore[qi] != 0;
  const bool act = MODE == WALK_COUNT ? valid : (MODE == WALK_LINK ? qcore : (valid && !qcore));
  cluster_visitor<MODE> vis(ccore, cpar, r2, cap, bound, grid_w, qi, cloud_tile_point(tile, 63, grid_w), act);

  if (__ballot(act)) {
    const f32x4 qlo = *reinterpret_cast<const f32x4*>(cv.box + (long long)tile * 8), qhi = *reinterpret_cast<const f32x4*>(cv.box + (long long)tile * 8 + 4);
    for (int pass = 0; pass < 2; ++pass) walk_cloud(cv, q, qlo, qhi, tile, pass == 0 ? VISIT_RING : VISIT_REST, vis);
  }

  if (MODE == WALK_COUNT) {
    if (qi < P) ccore[qi] = (valid && vis.cnt >= cap) ? 1 : 0;
  } else if (MODE == WALK_LINK) {
    if (qcore && !vis.bad && vis.cur < qi) atomicMin(cpar + qi, vis.cur);  // shorten the query's own path
    if (vis.bad) atomicOr(state + cloud * MVT_CLUSTER_STATE_WORDS + MVT_CLUSTER_STATUS, (unsigned long long)MVT_CLUSTER_BOUND);
  } else {
    if (qi < P) root[cloud * P + qi] = qcore ? cpar[qi] : ((valid && vis.best < bound) ? vis.best : -1);
  }
}

// parent[i] = root(i) for core points.  Other threads may still read an entry that this pass has already replaced by its root:
// a root is an ancestor like any other, so their walks end at the same place.
__global__ __launch_bounds__(256) void cluster_flatten_kernel(const unsigned char* __restrict__ core, int* __restrict__ parent, long long P,
                                                              long long total, unsigned long long* __restrict__ state) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    if (!core[i]) continue;
    const long long cloud = i / P;
    int* cpar = parent + cloud * P;
    const int x = (int)(i - cloud * P);
    bool bad = false;
    const int r = uf_find(cpar, x, (int)P, bad);
    if (bad) atomicOr(state + cloud * MVT_CLUSTER_STATE_WORDS + MVT_CLUSTER_STATUS, (unsigned long long)MVT_CLUSTER_BOUND);
    else if (r < x) atomicMin(cpar + x, r);
  }
}

__device__ __forceinline__ long long block_sum_i64(long long v, long long* s_red) {  // every thread gets the sum (integers: any order)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (long long)shfl_xor_u64((unsigned long long)v, o);
  __syncthreads();  // (s_red may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// One workgroup per cloud.  sizes: zeroed by the launcher; it holds the cluster sizes per root first and the dense ids per root after.
__global__ __launch_bounds__(CF_WG) void cluster_finish_kernel(const float* __restrict__ xyz, long long P, int min_samples,
                                                               const unsigned char* __restrict__ core, const int* __restrict__ root,
                                                               int* __restrict__ sizes, int* __restrict__ labels, unsigned char* __restrict__ select,
                                                               long long* __restrict__ state) {
  __shared__ long long s_red[CF_WG / 64];
  __shared__ int s_wave[CF_WG / 64];
  __shared__ int s_chosen;
  const long long base = (long long)blockIdx.x * P;
  const float* cx = xyz + base * 4;
  const unsigned char* ccore = core + base;
  const int* croot = root + base;
  int* csize = sizes + base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  long long n_cand = 0, n_core = 0, n_root = 0, n_noise = 0;
  for (long long i = threadIdx.x; i < P; i += CF_WG) {
    const bool v = finite3(*reinterpret_cast<const f32x4*>(cx + i * 4));
    const int r = croot[i];
    n_cand += v ? 1 : 0;
    n_core += ccore[i] ? 1 : 0;
    n_root += (ccore[i] && r == (int)i) ? 1 : 0;
    n_noise += (v && r < 0) ? 1 : 0;
    if (r >= 0) atomicAdd(csize + r, 1);  // border points included
  }
  n_cand = block_sum_i64(n_cand, s_red);
  n_core = block_sum_i64(n_core, s_red);
  n_root = block_sum_i64(n_root, s_red);
  n_noise = block_sum_i64(n_noise, s_red);
  __threadfence();
  __syncthreads();  // every size is complete (the atomics were performed at the device's L2; the loads below go there too)

  // the largest cluster, the lowest root (= the lowest id) among equal sizes: max of (size, P - 1 - root)
  unsigned long long key = 0;
  for (long long i = threadIdx.x; i < P; i += CF_WG) {
    if (ccore[i] && croot[i] == (int)i) {
      const unsigned long long k = ((unsigned long long)(unsigned)uf_load(csize + i) << 32) | (unsigned)(P - 1 - i);
      key = k > key ? k : key;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = shfl_xor_u64(key, o);
    key = w > key ? w : key;
  }
  __syncthreads();
  if (lane == 0) s_red[wave] = (long long)key;
  if (threadIdx.x == 0) s_chosen = -1;
  __syncthreads();
  for (int w = 0; w < CF_WG / 64; ++w) key = (unsigned long long)s_red[w] > key ? (unsigned long long)s_red[w] : key;
  const int best_root = n_root > 0 ? (int)(P - 1 - (long long)(unsigned)key) : -1;
  const long long best_size = n_root > 0 ? (long long)(key >> 32) : 0;
  const int fallback = n_cand == 0 ? MVT_CLUSTER_EMPTY : (n_cand < min_samples ? MVT_CLUSTER_FEW : (n_root == 0 ? MVT_CLUSTER_NONE : 0));
  __syncthreads();  // (s_red is reused below)

  // dense ids: the number of roots below i, chunk by chunk in index order
  int before = 0;
  for (long long c0 = 0; c0 < P; c0 += CF_WG) {
    const long long i = c0 + threadIdx.x;
    const bool is_root = i < P && ccore[i] && croot[i] == (int)i;
    const unsigned long long m = __ballot(is_root);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = before;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    if (is_root) {
      const int id = off + __popcll(m & ((1ull << lane) - 1ull));
      __hip_atomic_store(csize + i, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((int)i == best_root) s_chosen = id;
    }
    before += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();  // (s_wave is rewritten by the next chunk)
  }
  __threadfence();
  __syncthreads();

  for (long long i = threadIdx.x; i < P; i += CF_WG) {
    const int r = croot[i];
    labels[base + i] = r >= 0 ? uf_load(csize + r) : -1;
    const bool v = finite3(*reinterpret_cast<const f32x4*>(cx + i * 4));
    select[base + i] = (fallback == MVT_CLUSTER_FEW || fallback == MVT_CLUSTER_NONE) ? (v ? 1 : 0) : ((r >= 0 && r == best_root) ? 1 : 0);
  }
  if (threadIdx.x == 0) {
    long long* st = state + (long long)blockIdx.x * MVT_CLUSTER_STATE_WORDS;
    st[MVT_CLUSTER_CANDIDATES] = n_cand;
    st[MVT_CLUSTER_CORE] = n_core;
    st[MVT_CLUSTER_CLUSTERS] = n_root;
    st[MVT_CLUSTER_CHOSEN] = s_chosen;
    st[MVT_CLUSTER_CHOSEN_SIZE] = best_size;
    st[MVT_CLUSTER_NOISE] = n_noise;
    st[MVT_CLUSTER_FALLBACK] = fallback;  // (word MVT_CLUSTER_STATUS belongs to mvt_cluster_link)
  }
}

}  // namespace

extern "C" int mvt_cluster_crop(float* xyz, int C, long long P, const float* region_T_world, const float* bounds, void* stream) {
  MVT_REQUIRE(aligned(xyz, 16) && aligned(region_T_world, 4) && bounds != nullptr && C > 0 && C <= 65535 && P > 0 && P < (1ll << 31) - 64);
  for (int e = 0; e < 3; ++e)  // 6 floats on the HOST: (lo, hi) per axis, finite, lo < hi
    MVT_REQUIRE(bounds[2 * e] > -INFINITY && bounds[2 * e + 1] < INFINITY && bounds[2 * e] < bounds[2 * e + 1]);
  const long long total = (long long)C * P;
  hipLaunchKernelGGL(cluster_crop_kernel, dim3(strided_blocks(total)), dim3(256), 0, mvt_stream(stream), xyz, P, total, region_T_world, bounds[0],
                     bounds[1], bounds[2], bounds[3], bounds[4], bounds[5]);
  return mvt_launch_status();
}

extern "C" int mvt_cluster_count(const float* xyz, int C, long long P, int grid_w, int grid_h, float r2, int min_samples, const float* tile_box,
                                 const float* group_box, unsigned char* core, void* stream) {
  MVT_REQUIRE(aligned(xyz, 16) && aligned(tile_box, 16) && aligned(group_box, 16) && core != nullptr && cloud_shape_ok(C, P, grid_w, grid_h));
  MVT_REQUIRE(r2 > 0.f && r2 < INFINITY && min_samples >= 1 && min_samples < (1 << 30));
  const int ntiles = (int)((P + 63) / 64);
  hipLaunchKernelGGL(cluster_walk_kernel<WALK_COUNT>, dim3((unsigned)mvt_cdiv(ntiles, CL_WG / 64), (unsigned)C), dim3(CL_WG), 0, mvt_stream(stream),
                     xyz, P, ntiles, grid_w, r2, min_samples, tile_box, group_box, core, (int*)nullptr, (int*)nullptr, (unsigned long long*)nullptr);
  return mvt_launch_status();
}

extern "C" int mvt_cluster_link(const float* xyz, int C, long long P, int grid_w, int grid_h, float r2, const float* tile_box,
                                const float* group_box, const unsigned char* core, int* parent, long long* state, void* stream) {
  MVT_REQUIRE(aligned(xyz, 16) && aligned(tile_box, 16) && aligned(group_box, 16) && core != nullptr && cloud_shape_ok(C, P, grid_w, grid_h));
  MVT_REQUIRE(r2 > 0.f && r2 < INFINITY && aligned(parent, 4) && aligned(state, 8));
  const int ntiles = (int)((P + 63) / 64);
  const long long total = (long long)C * P;
  const long long words = (long long)C * MVT_CLUSTER_STATE_WORDS, n = total > words ? total : words;
  hipLaunchKernelGGL(cluster_init_kernel, dim3(strided_blocks(n)), dim3(256), 0, mvt_stream(stream), parent, P, total, state, words, n);
  hipLaunchKernelGGL(cluster_walk_kernel<WALK_LINK>, dim3((unsigned)mvt_cdiv(ntiles, CL_WG / 64), (unsigned)C), dim3(CL_WG), 0, mvt_stream(stream),
                     xyz, P, ntiles, grid_w, r2, 0, tile_box, group_box, const_cast<unsigned char*>(core), parent, (int*)nullptr,
                     reinterpret_cast<unsigned long long*>(state));
  hipLaunchKernelGGL(cluster_flatten_kernel, dim3(strided_blocks(total)), dim3(256), 0, mvt_stream(stream), core, parent, P, total,
                     reinterpret_cast<unsigned long long*>(state));
  return mvt_launch_status();
}

extern "C" int mvt_cluster_border(const float* xyz, int C, long long P, int grid_w, int grid_h, float r2, const float* tile_box,
                                  const float* group_box, const unsigned char* core, const int* parent, int* root, void* stream) {
  MVT_REQUIRE(aligned(xyz, 16) && aligned(tile_box, 16) && aligned(group_box, 16) && core != nullptr && cloud_shape_ok(C, P, grid_w, grid_h));
  MVT_REQUIRE(r2 > 0.f && r2 < INFINITY && aligned(parent, 4) && aligned(root, 4));
  const int ntiles = (int)((P + 63) / 64);
  hipLaunchKernelGGL(cluster_walk_kernel<WALK_BORDER>, dim3((unsigned)mvt_cdiv(ntiles, CL_WG / 64), (unsigned)C), dim3(CL_WG), 0, mvt_stream(stream),
                     xyz, P, ntiles, grid_w, r2, 0, tile_box, group_box, const_cast<unsigned char*>(core), const_cast<int*>(parent), root,
                     (unsigned long long*)nullptr);
  return mvt_launch_status();
}

extern "C" int mvt_cluster_finish(const float* xyz, int C, long long P, int min_samples, const unsigned char* core, const int* root, int* sizes,
                                  int* labels, unsigned char* select, long long* state, void* stream) {
  MVT_REQUIRE(aligned(xyz, 16) && C > 0 && C <= 65535 && P > 0 && P < (1ll << 31) - 64 && min_samples >= 1 && core != nullptr);
  MVT_REQUIRE(aligned(root, 4) && aligned(sizes, 4) && aligned(labels, 4) && select != nullptr && aligned(state, 8));
  if (hipMemsetAsync(sizes, 0, (size_t)C * P * sizeof(int), mvt_stream(stream)) != hipSuccess) return mvt_launch_status();
  hipLaunchKernelGGL(cluster_finish_kernel, dim3((unsigned)C), dim3(CF_WG), 0, mvt_stream(stream), xyz, P, min_samples, core, root, sizes, labels,
                     select, state);
  return mvt_launch_status();
}
