// Rigid object motion ("Rigid motion"): per (object, frame) the rigid pose that carries the object's tracks from
// its reference frame to that frame, with the tracks that do not move with their object flagged, and the kernels that carry points
// through the clip with those poses (mvt_rigid_move) and put occluded or outlying track points where their object says they are
// (mvt_rigid_fill).
//
// Member lists: count (integer atomics), exclusive scan, stable scatter; one workgroup per object walks the tracks in order, so a
// list is in ascending track order whatever the order of the ids.
//
// Fit: one workgroup per (object, frame).  Every sum is fp64: lane l of the workgroup adds members l, l + 256, l + 512, ... of the
// list, then a fixed tree (xor shuffles in a wave, the four waves in order).  The order of addition is a function of the member
// list alone: two runs give the same bits, and a frame computed alone (its rows and the reference frame's) gives the bits of the
// whole call.  No float atomics.  Every loop is bounded by an argument (the member count, the iteration count, a fixed number of
// Jacobi sweeps).
//
// Rotation: Horn's closed form (J. Opt. Soc. Am. A 4, 1987).  The unit quaternion that maximises q^T N q, N the symmetric 4 x 4
// matrix that is linear in H = sum w (Q - qbar)(P - pbar)^T, is the proper rotation that maximises tr(R^T H): the top eigenvector
// of N by cyclic Jacobi in fp64.  Chosen over an SVD of H built from cloud_prep.hip's 3 x 3 Jacobi because (a) it yields a proper
// rotation directly -- the determinant correction of align_umeyama (the sign on the smallest singular direction) is what the
// maximiser over rotations IS, so there is no branch on a determinant and no third singular vector to complete for a planar cloud;
// (b) it never forms H^T H, which squares the condition number; the eigenvector's error is eps * sigma_1 / (sigma_2 + sigma_3),
// the conditioning of the problem itself.  Where sigma_2 + sigma_3 = 0 the optimum is not unique and one of the optima comes out.
//
// Plain C++, vector stores only.
#include "block_scan.h"

namespace {

typedef unsigned long long u64;

constexpr int RG_WG = 256;
static_assert(RG_WG == SCAN_WG, "wg_excl_scan_u64 is written for this workgroup size");
constexpr int RG_SWEEPS4 = 12;  // cyclic Jacobi sweeps of the 4 x 4 (fp64 converges in 5 to 7)
constexpr int RG_SWEEPS3 = 8;   // and of the 3 x 3 covariance, as cloud_prep.hip
constexpr int RG_LDS_OBJECTS = 128;  // mvt_rigid_move keeps the transforms of one frame in LDS up to this many objects (12 KiB)

__device__ __forceinline__ double rg_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ float rg_nanf() { return __uint_as_float(0x7fc00000u); }

// ------------------------------------------------------------------------------------------------------------- member lists
__global__ __launch_bounds__(RG_WG) void rigid_init_kernel(int G, int* __restrict__ counts, int* __restrict__ ref) {
  const int g = blockIdx.x * RG_WG + threadIdx.x;
  if (g < G) {
    counts[g] = 0;
    ref[g] = -1;
  }
}

__global__ __launch_bounds__(RG_WG) void rigid_count_kernel(const int* __restrict__ ids, const int* __restrict__ qf, int N, int G, int T,
                                                            int* __restrict__ counts, int* __restrict__ ref) {
  const int i = blockIdx.x * RG_WG + threadIdx.x;
  if (i >= N) return;
  const int g = ids[i];
  if (g < 0 || g >= G) return;
  atomicAdd(counts + g, 1);
  atomicMax(ref + g, min(max(qf[i], 0), T - 1));
}

// One workgroup: offsets[0 .. G] <- the exclusive prefix of counts; thread t owns the chunk [t * chunk, (t + 1) * chunk).
__global__ __launch_bounds__(RG_WG) void rigid_scan_kernel(const int* __restrict__ counts, int G, int chunk, int* __restrict__ offsets) {
  __shared__ u64 s_scan[RG_WG / 64];
  const int g0 = threadIdx.x * chunk;
  u64 sum = 0;
  for (int j = 0; j < chunk; ++j)
    if (g0 + j < G) sum += (u64)counts[g0 + j];
  u64 total;
  u64 off = wg_excl_scan_u64(sum, s_scan, total);
  for (int j = 0; j < chunk; ++j)
    if (g0 + j < G) {
      offsets[g0 + j] = (int)off;
      off += (u64)counts[g0 + j];
    }
  if (threadIdx.x == 0) offsets[G] = (int)total;
}

// Workgroup g walks the N tracks in steps of 256 and appends those of object g: ballot, popcount below the lane, the waves in order.
__global__ __launch_bounds__(RG_WG) void rigid_scatter_kernel(const int* __restrict__ ids, int N, const int* __restrict__ offsets,
                                                              int* __restrict__ members) {
  __shared__ int s_cnt[2][RG_WG / 64];
  const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = offsets[g];
  const int end = offsets[g + 1];
  if (base == end) return;  // (uniform)
  const int steps = (N + RG_WG - 1) / RG_WG;
  for (int s = 0; s < steps; ++s) {
    const int i = s * RG_WG + threadIdx.x;
    const bool keep = i < N && ids[i] == g;
    const u64 m = __ballot(keep);
    if (lane == 0) s_cnt[s & 1][wave] = __popcll(m);
    __syncthreads();  // (two buffers: the next step's writes cannot overtake this step's reads)
    int pos = base;
    for (int w = 0; w < wave; ++w) pos += s_cnt[s & 1][w];
    pos += __popcll(m & ((1ull << lane) - 1ull));
    if (keep && pos < end) members[pos] = i;
    base += s_cnt[s & 1][0] + s_cnt[s & 1][1] + s_cnt[s & 1][2] + s_cnt[s & 1][3];
  }
}

// ------------------------------------------------------------------------------------------------------------- fit
// Sums of K doubles over the workgroup: the fixed tree per wave, then the four waves in order; every thread gets the sums.
template <int K>
__device__ __forceinline__ void block_sums(double (&v)[K], double (*s_red)[RG_WG / 64]) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum_f64(v[k]);
  __syncthreads();  // (s_red may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_red[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (s_red[k][0] + s_red[k][1]) + (s_red[k][2] + s_red[k][3]);
}

// One rotation of the cyclic Jacobi method on the symmetric n x n a, annihilating a[P_][Q_]; the columns of v follow (the
// convention of cloud_prep.hip's jacobi_rotate).
template <int NN, int P_, int Q_>
__device__ __forceinline__ void rg_rotate(double (&a)[NN][NN], double (&v)[NN][NN]) {
  const double apq = a[P_][Q_];
  if (apq == 0.0) return;
  const double theta = (a[Q_][Q_] - a[P_][P_]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // (theta = +-inf: t = +-0)
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P_][P_] -= t * apq;
  a[Q_][Q_] += t * apq;
  a[P_][Q_] = a[Q_][P_] = 0.0;
#pragma unroll
  for (int k = 0; k < NN; ++k) {
    if (k != P_ && k != Q_) {
      const double akp = a[k][P_], akq = a[k][Q_];
      a[k][P_] = a[P_][k] = c * akp - s * akq;
      a[k][Q_] = a[Q_][k] = s * akp + c * akq;
    }
    const double vp = v[k][P_], vq = v[k][Q_];
    v[k][P_] = c * vp - s * vq;
    v[k][Q_] = s * vp + c * vq;
  }
}

// The second-largest eigenvalue of the symmetric 3 x 3 (xx, xy, xz, yy, yz, zz).
__device__ __noinline__ double rg_mid_eigenvalue(const double (&c6)[6]) {
  double a[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < RG_SWEEPS3; ++sweep) {
    rg_rotate<3, 0, 1>(a, v);
    rg_rotate<3, 0, 2>(a, v);
    rg_rotate<3, 1, 2>(a, v);
  }
  const double d0 = a[0][0], d1 = a[1][1], d2 = a[2][2];
  return fmax(fmin(d0, d1), fmin(fmax(d0, d1), d2));
}

// R (row-major) <- the proper rotation that maximises tr(R^T H), H = sum w q' p'^T (row-major, h[3 * a + b] = sum w q'_a p'_b).
__device__ __noinline__ void rg_horn(const double (&h)[9], double (&R)[9]) {
  // Horn's S_ab = sum p'_a q'_b = h[3 * b + a]
  const double Sxx = h[0], Sxy = h[3], Sxz = h[6], Syx = h[1], Syy = h[4], Syz = h[7], Szx = h[2], Szy = h[5], Szz = h[8];
  double a[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double v[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < RG_SWEEPS4; ++sweep) {
    rg_rotate<4, 0, 1>(a, v);
    rg_rotate<4, 0, 2>(a, v);
    rg_rotate<4, 0, 3>(a, v);
    rg_rotate<4, 1, 2>(a, v);
    rg_rotate<4, 1, 3>(a, v);
    rg_rotate<4, 2, 3>(a, v);
  }
  int im = 0;
  double dm = a[0][0];
  if (a[1][1] > dm) { dm = a[1][1]; im = 1; }
  if (a[2][2] > dm) { dm = a[2][2]; im = 2; }
  if (a[3][3] > dm) { dm = a[3][3]; im = 3; }
  double q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = im == 0 ? v[k][0] : (im == 1 ? v[k][1] : (im == 2 ? v[k][2] : v[k][3]));
  const double len = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
  const double w = q[0] / len, x = q[1] / len, y = q[2] / len, z = q[3] / len;
  R[0] = 1.0 - 2.0 * (y * y + z * z);
  R[1] = 2.0 * (x * y - w * z);
  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);
  R[4] = 1.0 - 2.0 * (x * x + z * z);
  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);
  R[7] = 2.0 * (y * z + w * x);
  R[8] = 1.0 - 2.0 * (x * x + y * y);
}

struct FitArgs {
  const float* tracks;
  const unsigned char* vis;
  const int* qf;
  const int* offsets;
  const int* members;
  const int* ref;
  int T, N, G;
  double thr;
  int iterations, min_points, use_vis;
  double spread2;  // min_spread^2
  int live_before;
};

// Member i of (frame t, reference frame r): its points in fp64 and its base weight.
__device__ __forceinline__ bool rg_member(const FitArgs& a, int i, int t, int r, double (&P)[3], double (&Q)[3]) {
  const float* p = a.tracks + ((long long)r * a.N + i) * 3;
  const float* q = a.tracks + ((long long)t * a.N + i) * 3;
  const float p0 = p[0], p1 = p[1], p2 = p[2], q0 = q[0], q1 = q[1], q2 = q[2];
  P[0] = p0, P[1] = p1, P[2] = p2, Q[0] = q0, Q[1] = q1, Q[2] = q2;
  bool base = (a.live_before || t >= a.qf[i]) && isfinite(p0) && isfinite(p1) && isfinite(p2) && isfinite(q0) && isfinite(q1) && isfinite(q2);
  if (a.use_vis) base = base && a.vis[(long long)t * a.N + i] != 0 && a.vis[(long long)r * a.N + i] != 0;
  return base;
}

__device__ __forceinline__ double rg_residual(const double (&R)[9], const double (&tr)[3], const double (&P)[3], const double (&Q)[3]) {
  const double dx = ((R[0] * P[0] + R[1] * P[1]) + R[2] * P[2]) + tr[0] - Q[0];
  const double dy = ((R[3] * P[0] + R[4] * P[1]) + R[5] * P[2]) + tr[1] - Q[1];
  const double dz = ((R[6] * P[0] + R[7] * P[1]) + R[8] * P[2]) + tr[2] - Q[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// grid (T, G).  Every quantity that steers the control flow is a workgroup-wide sum every thread holds: the branches are uniform.
__global__ __launch_bounds__(RG_WG) void rigid_fit_kernel(FitArgs a, float* __restrict__ poses, float* __restrict__ residual,
                                                          unsigned char* __restrict__ inliers, int* __restrict__ used,
                                                          int* __restrict__ inlier_count, float* __restrict__ rmse, int* __restrict__ status) {
  __shared__ double s_red[13][RG_WG / 64];
  const int t = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
  const int m0 = a.offsets[g], n = a.offsets[g + 1] - m0;
  const int r = a.ref[g];
  const int* mem = a.members + m0;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tr[3] = {0.0, 0.0, 0.0};
  int st = MVT_RIGID_OK, n_used = 0;
  if (n == 0 || r < 0) st = MVT_RIGID_TOO_FEW;
  bool fitted = false;
  for (int it = 0; it < a.iterations && st == MVT_RIGID_OK; ++it) {
    // pass A: the weight sum and the weighted centroids
    double sa[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < n; j += RG_WG) {
      double P[3], Q[3];
      bool w = rg_member(a, mem[j], t, r, P, Q);
      if (w && fitted) w = rg_residual(R, tr, P, Q) <= a.thr;
      if (w) {
        sa[0] += 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) sa[1 + c] += P[c], sa[4 + c] += Q[c];
      }
    }
    block_sums<7>(sa, s_red);
    const int cnt = (int)sa[0];
    if (!fitted) n_used = cnt;
    if (cnt < a.min_points) {
      if (!fitted) st = MVT_RIGID_TOO_FEW;
      break;  // (a refit that keeps too few: the previous fit stands, and every later refit would find the same weights)
    }
    double pb[3], qb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) pb[c] = sa[1 + c] / sa[0], qb[c] = sa[4 + c] / sa[0];
    // pass B: H = sum w q' p'^T (9) and the upper triangle of sum w p' p'^T (6), in two reductions
    double sh[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < n; j += RG_WG) {
      double P[3], Q[3];
      bool w = rg_member(a, mem[j], t, r, P, Q);
      if (w && fitted) w = rg_residual(R, tr, P, Q) <= a.thr;
      if (w) {
        const double px = P[0] - pb[0], py = P[1] - pb[1], pz = P[2] - pb[2];
        const double qx = Q[0] - qb[0], qy = Q[1] - qb[1], qz = Q[2] - qb[2];
        sh[0] += qx * px, sh[1] += qx * py, sh[2] += qx * pz;
        sh[3] += qy * px, sh[4] += qy * py, sh[5] += qy * pz;
        sh[6] += qz * px, sh[7] += qz * py, sh[8] += qz * pz;
        sc[0] += px * px, sc[1] += px * py, sc[2] += px * pz, sc[3] += py * py, sc[4] += py * pz, sc[5] += pz * pz;
      }
    }
    block_sums<9>(sh, s_red);
    block_sums<6>(sc, s_red);
    if (!(rg_mid_eigenvalue(sc) / sa[0] >= a.spread2)) {
      if (!fitted) st = MVT_RIGID_DEGENERATE;
      break;
    }
    rg_horn(sh, R);
#pragma unroll
    for (int c = 0; c < 3; ++c) tr[c] = qb[c] - ((R[3 * c] * pb[0] + R[3 * c + 1] * pb[1]) + R[3 * c + 2] * pb[2]);
    fitted = true;
  }
  // outputs of the fit that stood
  double so[2] = {0.0, 0.0};
  for (int j = tid; j < n; j += RG_WG) {
    const int i = mem[j];
    double P[3], Q[3];
    const bool base = rg_member(a, i, t, r, P, Q);
    float res = rg_nanf();
    bool in = false;
    if (st == MVT_RIGID_OK) {
      const double d = rg_residual(R, tr, P, Q);
      res = (float)d;
      in = base && d <= a.thr;
      if (in) so[0] += 1.0, so[1] += d * d;
    }
    residual[(long long)t * a.N + i] = res;
    inliers[(long long)t * a.N + i] = in ? 1 : 0;
  }
  block_sums<2>(so, s_red);
  if (tid < 16) {
    const int row = tid >> 2, col = tid & 3;
    float v = st == MVT_RIGID_OK && row == 3 ? (col == 3 ? 1.f : 0.f) : rg_nanf();  // (all 16 are NaN where status != 0)
    if (st == MVT_RIGID_OK && row < 3) {
      // (selected without indexing the arrays by a runtime value)
      double d = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k)
        if (k == row * 3 + col) d = R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (col == 3 && k == row) d = tr[k];
      v = (float)d;
    }
    poses[((long long)g * a.T + t) * 16 + tid] = v;
  }
  if (tid == 0) {
    const long long o = (long long)g * a.T + t;
    used[o] = n_used;
    inlier_count[o] = (int)so[0];
    rmse[o] = st == MVT_RIGID_OK ? (float)sqrt(so[1] / so[0]) : rg_nanf();
    status[o] = st;
  }
}

// residual <- NaN and inliers <- 0 for the tracks of no object (the fit kernel writes every member's).
__global__ __launch_bounds__(RG_WG) void rigid_clear_kernel(const int* __restrict__ ids, int T, int N, int G, float* __restrict__ residual,
                                                            unsigned char* __restrict__ inliers) {
  const int i = blockIdx.x * RG_WG + threadIdx.x, t = blockIdx.y;
  if (i >= N) return;
  const int g = ids[i];
  if (g >= 0 && g < G) return;
  residual[(long long)t * N + i] = rg_nanf();
  inliers[(long long)t * N + i] = 0;
}

// ------------------------------------------------------------------------------------------------------------- compose
__global__ __launch_bounds__(RG_WG) void rigid_compose_kernel(const float* __restrict__ poses, const int* __restrict__ status, int G, int T,
                                                              int frame, double* __restrict__ xf) {
  const long long o = (long long)blockIdx.x * RG_WG + threadIdx.x;  // (g, t)
  if (o >= (long long)G * T) return;
  const float* A = poses + o * 16;
  double M[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) M[k] = (double)A[k];
  bool ok = status[o] == MVT_RIGID_OK;
  if (frame >= 0) {
    const long long of = o / T * T + frame;
    const float* B = poses + of * 16;
    ok = ok && status[of] == MVT_RIGID_OK;
    double Bm[12], C[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Bm[k] = (double)B[k];
    // C = A B^-1: rotation A_R B_R^T, translation A_t - C_R B_t
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) C[4 * i + j] = (M[4 * i] * Bm[4 * j] + M[4 * i + 1] * Bm[4 * j + 1]) + M[4 * i + 2] * Bm[4 * j + 2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) C[4 * i + 3] = M[4 * i + 3] - ((C[4 * i] * Bm[3] + C[4 * i + 1] * Bm[7]) + C[4 * i + 2] * Bm[11]);
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = C[k];
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) xf[o * 12 + k] = ok ? M[k] : rg_nan();
}

// ------------------------------------------------------------------------------------------------------------- move and fill
// Four consecutive points of a (rows, 3) fp32 array from row i0: three 16-byte accesses when all four exist and the address is
// 16-byte aligned (vec), else element by element up to row `rows`.
__device__ __forceinline__ void rg_load4(const float* __restrict__ base, long long i0, long long rows, bool vec, float (&p)[12]) {
  if (vec && i0 + 4 <= rows) {
    const f32x4* s = reinterpret_cast<const f32x4*>(base + i0 * 3);
    const f32x4 a = s[0], b = s[1], c = s[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = a[k], p[4 + k] = b[k], p[8 + k] = c[k];
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) p[k] = (i0 * 3 + k < rows * 3) ? base[i0 * 3 + k] : 0.f;
  }
}

__device__ __forceinline__ void rg_store4(float* __restrict__ base, long long i0, long long rows, bool vec, const float (&p)[12]) {
  if (vec && i0 + 4 <= rows) {
    f32x4* d = reinterpret_cast<f32x4*>(base + i0 * 3);
    d[0] = (f32x4){p[0], p[1], p[2], p[3]};
    d[1] = (f32x4){p[4], p[5], p[6], p[7]};
    d[2] = (f32x4){p[8], p[9], p[10], p[11]};
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (i0 * 3 + k < rows * 3) base[i0 * 3 + k] = p[k];
  }
}

// out <- M p in fp64 from fp32 operands, rounded once; M: rows 0..2 of a transform, 12 doubles.
__device__ __forceinline__ void rg_apply(const double* __restrict__ M, const float* p, float* out) {
  const double x = p[0], y = p[1], z = p[2];
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (float)(((M[4 * c] * x + M[4 * c + 1] * y) + M[4 * c + 2] * z) + M[4 * c + 3]);
}

// grid (ceil(M / 1024), T): a thread moves four consecutive points through frame t.  vec: M % 4 == 0 and aligned pointers, so that
// every row of out starts on a 16-byte boundary.
__global__ __launch_bounds__(RG_WG) void rigid_move_kernel(const float* __restrict__ points, const int* __restrict__ objects,
                                                           const double* __restrict__ xf, int Mn, int T, int G, int vec,
                                                           float* __restrict__ out) {
  __shared__ double s_xf[RG_LDS_OBJECTS * 12];
  const int t = blockIdx.y;
  const bool lds = G <= RG_LDS_OBJECTS;  // (uniform)
  if (lds) {
    for (int k = threadIdx.x; k < G * 12; k += RG_WG) s_xf[k] = xf[((long long)(k / 12) * T + t) * 12 + k % 12];
    __syncthreads();
  }
  const long long i0 = ((long long)blockIdx.x * RG_WG + threadIdx.x) * 4;
  if (i0 >= Mn) return;
  float p[12], o[12];
  rg_load4(points, i0, Mn, vec, p);
  int ids[4];
  if (vec && i0 + 4 <= Mn) {
    const int4 w = *reinterpret_cast<const int4*>(objects + i0);
    ids[0] = w.x, ids[1] = w.y, ids[2] = w.z, ids[3] = w.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) ids[e] = i0 + e < Mn ? objects[i0 + e] : -1;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int g = ids[e];
    if (g < 0 || g >= G) {
      o[3 * e] = o[3 * e + 1] = o[3 * e + 2] = rg_nanf();
    } else if (lds) {
      rg_apply(s_xf + g * 12, p + 3 * e, o + 3 * e);
    } else {
      rg_apply(xf + ((long long)g * T + t) * 12, p + 3 * e, o + 3 * e);
    }
  }
  rg_store4(out + (long long)t * Mn * 3, i0, Mn, vec, o);
}

struct FillArgs {
  const float* tracks;
  const unsigned char* vis;
  const unsigned char* inl;
  const int* qf;
  const int* ids;
  const int* ref;
  const float* poses;
  const int* status;
  int T, N, G, replace, live_before;
};

// grid (ceil(N / 1024), T): a thread has four consecutive tracks of frame t.  The reference point of a track that is filled is
// read where it is needed: few tracks are.
__global__ __launch_bounds__(RG_WG) void rigid_fill_kernel(FillArgs a, int vec, float* __restrict__ out, unsigned char* __restrict__ filled) {
  const int t = blockIdx.y;
  const long long i0 = ((long long)blockIdx.x * RG_WG + threadIdx.x) * 4;
  if (i0 >= a.N) return;
  const long long row = (long long)t * a.N;
  float p[12];
  rg_load4(a.tracks + row * 3, i0, a.N, vec, p);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long i = i0 + e;
    if (i >= a.N) break;
    const int g = a.ids[i];
    bool fill = false;
    if (g >= 0 && g < a.G && a.status[(long long)g * a.T + t] == MVT_RIGID_OK && (a.live_before || t >= a.qf[i])) {
      fill = ((a.replace & MVT_RIGID_FILL_OCCLUDED) && a.vis[row + i] == 0) || ((a.replace & MVT_RIGID_FILL_OUTLIERS) && a.inl[row + i] == 0);
    }
    if (fill) {
      const float* A = a.poses + ((long long)g * a.T + t) * 16;
      double M[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) M[k] = (double)A[k];
      const float* P = a.tracks + ((long long)a.ref[g] * a.N + i) * 3;
      const float pr[3] = {P[0], P[1], P[2]};
      rg_apply(M, pr, p + 3 * e);
    }
    filled[row + i] = fill ? 1 : 0;
  }
  rg_store4(out + row * 3, i0, a.N, vec, p);
}

inline bool aligned(const void* p, size_t a) { return p && ((uintptr_t)p % a) == 0; }

// (N <= 2^30: a thread's track index, block * 256 + lane, stays an int)
inline bool dims_ok(int T, int N, int G) { return T > 0 && N > 0 && N <= (1 << 30) && G > 0 && G <= MVT_RIGID_MAX_OBJECTS && T <= 65535; }

}  // namespace

extern "C" int mvt_rigid_members(const int* object_ids, const int* query_frames, int N, int G, int T, int* counts, int* offsets, int* members,
                                 int* reference_frames, void* stream) {
  MVT_REQUIRE(dims_ok(T, N, G) && aligned(object_ids, 4) && aligned(query_frames, 4) && aligned(counts, 4) && aligned(offsets, 4) &&
              aligned(members, 4) && aligned(reference_frames, 4));
  hipStream_t s = mvt_stream(stream);
  hipLaunchKernelGGL(rigid_init_kernel, dim3((unsigned)mvt_cdiv(G, RG_WG)), dim3(RG_WG), 0, s, G, counts, reference_frames);
  hipLaunchKernelGGL(rigid_count_kernel, dim3((unsigned)mvt_cdiv(N, RG_WG)), dim3(RG_WG), 0, s, object_ids, query_frames, N, G, T, counts,
                     reference_frames);
  hipLaunchKernelGGL(rigid_scan_kernel, dim3(1), dim3(RG_WG), 0, s, counts, G, (int)mvt_cdiv(G, RG_WG), offsets);
  hipLaunchKernelGGL(rigid_scatter_kernel, dim3(G), dim3(RG_WG), 0, s, object_ids, N, offsets, members);
  return mvt_launch_status();
}

extern "C" int mvt_rigid_fit(const float* tracks, const unsigned char* visibility, const int* query_frames, const int* object_ids,
                             const int* offsets, const int* members, const int* reference_frames, int T, int N, int G, double inlier_threshold,
                             int iterations, int min_points, int use_visibility, double min_spread, int live_before_query, float* poses,
                             float* residual, unsigned char* inliers, int* used, int* inlier_count, float* rmse, int* status, void* stream) {
  MVT_REQUIRE(dims_ok(T, N, G) && aligned(tracks, 4) && visibility != nullptr && aligned(query_frames, 4) && aligned(object_ids, 4) &&
              aligned(offsets, 4) && aligned(members, 4) && aligned(reference_frames, 4));
  MVT_REQUIRE(aligned(poses, 4) && aligned(residual, 4) && inliers != nullptr && aligned(used, 4) && aligned(inlier_count, 4) &&
              aligned(rmse, 4) && aligned(status, 4));
  MVT_REQUIRE(inlier_threshold >= 0.0 && iterations >= 1 && iterations <= MVT_RIGID_MAX_ITERATIONS && min_points >= 3 && min_spread >= 0.0);
  MVT_REQUIRE((use_visibility == 0 || use_visibility == 1) && (live_before_query == 0 || live_before_query == 1));
  FitArgs a = {tracks,     visibility, query_frames,   offsets,          members, reference_frames,        T,
               N,          G,          inlier_threshold, iterations,     min_points, use_visibility, min_spread * min_spread,
               live_before_query};
  hipStream_t s = mvt_stream(stream);
  hipLaunchKernelGGL(rigid_clear_kernel, dim3((unsigned)mvt_cdiv(N, RG_WG), T), dim3(RG_WG), 0, s, object_ids, T, N, G, residual, inliers);
  hipLaunchKernelGGL(rigid_fit_kernel, dim3(T, G), dim3(RG_WG), 0, s, a, poses, residual, inliers, used, inlier_count, rmse, status);
  return mvt_launch_status();
}

extern "C" int mvt_rigid_compose(const float* poses, const int* status, int G, int T, int frame, double* xf, void* stream) {
  MVT_REQUIRE(dims_ok(T, 1, G) && aligned(poses, 4) && aligned(status, 4) && aligned(xf, 8) && frame >= -1 && frame < T);
  hipLaunchKernelGGL(rigid_compose_kernel, dim3((unsigned)mvt_cdiv((long long)G * T, RG_WG)), dim3(RG_WG), 0, mvt_stream(stream), poses, status,
                     G, T, frame, xf);
  return mvt_launch_status();
}

extern "C" int mvt_rigid_move(const float* points, const int* point_objects, const double* xf, int M, int T, int G, float* out, void* stream) {
  MVT_REQUIRE(dims_ok(T, M, G) && aligned(points, 4) && aligned(point_objects, 4) && aligned(xf, 8) && aligned(out, 4));
  const int vec = M % 4 == 0 && aligned(points, 16) && aligned(point_objects, 16) && aligned(out, 16);
  hipLaunchKernelGGL(rigid_move_kernel, dim3((unsigned)mvt_cdiv(mvt_cdiv(M, 4), RG_WG), T), dim3(RG_WG), 0, mvt_stream(stream), points,
                     point_objects, xf, M, T, G, vec, out);
  return mvt_launch_status();
}

extern "C" int mvt_rigid_fill(const float* tracks, const unsigned char* visibility, const unsigned char* inliers, const int* query_frames,
                              const int* object_ids, const int* reference_frames, const float* poses, const int* status, int T, int N, int G,
                              int replace, int live_before_query, float* out, unsigned char* filled, void* stream) {
  MVT_REQUIRE(dims_ok(T, N, G) && aligned(tracks, 4) && visibility != nullptr && inliers != nullptr && aligned(query_frames, 4) &&
              aligned(object_ids, 4) && aligned(reference_frames, 4) && aligned(poses, 4) && aligned(status, 4) && aligned(out, 4) &&
              filled != nullptr);
  MVT_REQUIRE(replace >= 0 && replace <= (MVT_RIGID_FILL_OCCLUDED | MVT_RIGID_FILL_OUTLIERS) && (live_before_query == 0 || live_before_query == 1));
  MVT_REQUIRE(tracks != out);
  FillArgs a = {tracks, visibility, inliers, query_frames, object_ids, reference_frames, poses, status, T, N, G, replace, live_before_query};
  const int vec = N % 4 == 0 && aligned(tracks, 16) && aligned(out, 16);
  hipLaunchKernelGGL(rigid_fill_kernel, dim3((unsigned)mvt_cdiv(mvt_cdiv(N, 4), RG_WG), T), dim3(RG_WG), 0, mvt_stream(stream), a, vec, out,
                     filled);
  return mvt_launch_status();
}
