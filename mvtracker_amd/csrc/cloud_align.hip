// Camera alignment: point-to-plane ICP of one view's clouds onto the clouds of the other views (reference:
// conversions/droid/utils/optimization.py run_icp_point_to_plane -> Open3D registration_icp with
// TransformationEstimationPointToPlane, whose loop, residual, Jacobian and convergence rule the entries restate).
//
// align_normals    - normals of organised clouds from the four grid neighbours (central differences), NaN rows where there is none.
// align_transform  - xyz = D xyz0, every coordinate in fp64, rounded to fp32 once.
// align_correspond - the search: a wave owns a tile of 64 queries of the source cloud, ONE QUERY PER LANE; the query is D p0 with the
//                    rounding of align_transform.  Candidate tiles of every target cloud are loaded one point per lane and broadcast
//                    lane by lane (v_readlane): 3 subtracts, 3 multiply-adds and one 64-bit compare per candidate for 64 queries.
//                    A query keeps ONE key (d2 bits << 32 | global target index), started at (cap2 bits << 32): a candidate replaces
//                    it only when its key is smaller, which is "d2 < cap2, nearest, ties to the lower (cloud, index)" in one compare
//                    (d2 >= 0, so its bits order as the value; a NaN d2 has bits above those of any finite cap2).
//                    Boxes only prune: a group or tile is skipped when its box distance, taken with the scan's monotone arithmetic,
//                    EXCEEDS the bound (the query's current d2, cap2 at the start).  The test is strict, as in mvt_knn_scan: tiles
//                    of an organised cloud are 8x8 patches, so a tile visited later can hold a LOWER index at exactly the bound,
//                    and that point must still be seen to win the tie.
//                    The tile's normal equations leave in one row of 30 doubles, summed over the lanes by a fixed shuffle tree.
// align_solve      - one workgroup: the rows summed in a fixed order, LDL^T, T(x) D, the iteration's figures and the done flag.
// No atomics, no host read: align_correspond and align_solve return at once when the done flag is set, so the host enqueues
// max_iterations + 1 pairs of them whatever the data.
#include "cloud_search.h"

namespace {

constexpr int AC_WG = 128;  // threads per workgroup of the search (2 waves)
constexpr int AS_WG = 256;  // the solve's one workgroup
constexpr int ROW = MVT_ALIGN_ROW;

__device__ __forceinline__ float wave_min_f(float v) {  // (fminf drops a NaN operand)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// D p in fp64 (row r: ((D[4r] x + D[4r+1] y) + D[4r+2] z) + D[4r+3], multiply-adds fused), rounded to fp32 once; .w = 0.
// A row whose result is not finite in all three coordinates (a NaN or infinite input, an overflow) becomes all NaN.
__device__ __forceinline__ f32x4 xform_point(const double* __restrict__ D, const f32x4& p) {
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  f32x4 o;
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = (float)(fma(D[4 * r + 2], z, fma(D[4 * r + 1], y, D[4 * r] * x)) + D[4 * r + 3]);
  o[3] = 0.f;
  if (!finite3(o)) o = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};  // (a NaN or an overflow anywhere: the point takes no part)
  return o;
}

__global__ __launch_bounds__(256) void align_normals_kernel(const float* __restrict__ xyz, long long total, int gw, int gh, float me2,
                                                            float* __restrict__ nrm) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % gw), y = (int)((i / gw) % gh);
    f32x4 o = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};
    if (x > 0 && x < gw - 1 && y > 0 && y < gh - 1) {
      const f32x4 c = *reinterpret_cast<const f32x4*>(xyz + i * 4);
      const f32x4 l = *reinterpret_cast<const f32x4*>(xyz + (i - 1) * 4), r = *reinterpret_cast<const f32x4*>(xyz + (i + 1) * 4);
      const f32x4 u = *reinterpret_cast<const f32x4*>(xyz + (i - gw) * 4), d = *reinterpret_cast<const f32x4*>(xyz + (i + gw) * 4);
      bool ok = finite3(c) && finite3(l) && finite3(r) && finite3(u) && finite3(d);
      ok = ok && gap_d2(l[0] - c[0], l[1] - c[1], l[2] - c[2]) <= me2 && gap_d2(r[0] - c[0], r[1] - c[1], r[2] - c[2]) <= me2 &&
           gap_d2(u[0] - c[0], u[1] - c[1], u[2] - c[2]) <= me2 && gap_d2(d[0] - c[0], d[1] - c[1], d[2] - c[2]) <= me2;
      if (ok) {
        const float ax = r[0] - l[0], ay = r[1] - l[1], az = r[2] - l[2];
        const float bx = d[0] - u[0], by = d[1] - u[1], bz = d[2] - u[2];
        // a x b, every product and difference rounded on its own (no contraction)
        const float cx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
        const float cy = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
        const float cz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
        const float len = __fsqrt_rn(gap_d2(cx, cy, cz));
        if (len > 0.f && len < inf_f()) o = (f32x4){__fdiv_rn(cx, len), __fdiv_rn(cy, len), __fdiv_rn(cz, len), 0.f};
      }
    }
    *reinterpret_cast<f32x4*>(nrm + i * 4) = o;
  }
}

__global__ __launch_bounds__(256) void align_transform_kernel(const float* __restrict__ xyz0, const double* __restrict__ D, long long n,
                                                              float* __restrict__ xyz) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    *reinterpret_cast<f32x4*>(xyz + i * 4) = xform_point(D, *reinterpret_cast<const f32x4*>(xyz0 + i * 4));
}

// The target clouds of one launch, BY VALUE as a kernel argument (indexed by wave-uniform values only).
struct align_targets {
  const float* xyz[MVT_ALIGN_MAX_TARGETS];
  const float* nrm[MVT_ALIGN_MAX_TARGETS];
  const float* box[MVT_ALIGN_MAX_TARGETS];
  const float* gbox[MVT_ALIGN_MAX_TARGETS];
  long long P[MVT_ALIGN_MAX_TARGETS];
  long long off[MVT_ALIGN_MAX_TARGETS];  // global index of the cloud's point 0
  int grid_w[MVT_ALIGN_MAX_TARGETS];
  int n;
};

// Query slot (tile, lane) -> source point index, or -1.  Point lists: slot = index.  Organised clouds: the pixels (y, x) with
// y % s == 0 and x % s == 0 form a grid of hs x ws samples, cut into 8x8 patches of samples (qtx patches per row).
__device__ __forceinline__ long long query_point(int tile, int lane, long long P, int gw, int gh, int s, int qtx) {
  if (gw == 0) {
    const long long i = (long long)tile * 64 + lane;
    return i < P ? i : -1;
  }
  const int ws = (gw + s - 1) / s, hs = (gh + s - 1) / s;
  const int ty = tile / qtx, tx = tile - ty * qtx;
  const int sy = ty * 8 + (lane >> 3), sx = tx * 8 + (lane & 7);
  return (sy < hs && sx < ws) ? (long long)sy * s * gw + (long long)sx * s : -1;
}

// The search keeps its own copy of the walk that walk_cloud (cloud_search.h) states for the self-searches: taken through walk_cloud with
// a visitor the kernel measured 1.6 to 2.8 % slower on organised 512x512 clouds, with every output bit equal.
__global__ __launch_bounds__(AC_WG) void align_correspond_kernel(const float* __restrict__ src0, long long Ps, int src_gw, int src_gh, int stride,
                                                                 int ntq, int qtx, const double* __restrict__ D, float cap2, align_targets tg,
                                                                 const int* __restrict__ ist, double* __restrict__ partial,
                                                                 int* __restrict__ q_idx, float* __restrict__ q_d2) {
  if (ist[MVT_ALIGN_I_DONE]) return;  // (uniform over the grid)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * (AC_WG / 64) + wave;
  if (tile >= ntq) return;  // (wave-uniform; the kernel has no workgroup barrier)
  const long long f = blockIdx.y;

  const long long qi = query_point(tile, lane, Ps, src_gw, src_gh, stride, qtx);
  f32x4 q = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};
  if (qi >= 0) q = xform_point(D, *reinterpret_cast<const f32x4*>(src0 + (f * Ps + qi) * 4));
  const bool valid = finite3(q);
  const unsigned long long key0 = (unsigned long long)__float_as_uint(cap2) << 32;
  unsigned long long best = key0;

  if (__ballot(valid)) {
    // the query tile's own box (NaN lanes dropped by fminf / fmaxf)
    f32x4 qlo, qhi;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      qlo[e] = wave_min_f(valid ? q[e] : inf_f());
      qhi[e] = wave_max(valid ? q[e] : -inf_f());
    }
    float mine = valid ? cap2 : -inf_f();  // this lane's bound: no candidate ABOVE it can replace the key
    for (int k = 0; k < tg.n; ++k) {
      const long long Pk = tg.P[k];
      const int gwk = tg.grid_w[k];
      const int ntiles = (int)((Pk + 63) >> 6), ng = (ntiles + 63) >> 6;
      const float* __restrict__ cand = tg.xyz[k] + f * Pk * 4;
      const float* __restrict__ cnrm = tg.nrm[k] + f * Pk * 4;
      const float* __restrict__ fbox = tg.box[k] + f * ntiles * 8;
      const float* __restrict__ fgbox = tg.gbox[k] + f * ng * 8;
      const int off = (int)tg.off[k];
      for (int gb = 0; gb < ng; gb += 64) {
        float tmax = wave_max(mine);
        bool gnear = gb + lane < ng;
        if (gnear) {
          const float* gp = fgbox + (long long)(gb + lane) * 8;
          const float lb = box_box_d2(qlo, qhi, *reinterpret_cast<const f32x4*>(gp), *reinterpret_cast<const f32x4*>(gp + 4));
          gnear = !(lb > tmax);  // (strict: a point AT the bound can still win a tie by its index; a NaN bound never culls)
        }
        unsigned long long gmask = __ballot(gnear);
        while (gmask) {
          const int tb = (gb + __builtin_ctzll(gmask)) * 64;
          gmask &= gmask - 1;
          const int t = tb + lane;
          bool tnear = t < ntiles;
          if (tnear) {
            const float* bp = fbox + (long long)t * 8;
            const float lb = box_box_d2(qlo, qhi, *reinterpret_cast<const f32x4*>(bp), *reinterpret_cast<const f32x4*>(bp + 4));
            tnear = !(lb > tmax);
          }
          unsigned long long tmask = __ballot(tnear);
          while (tmask) {
            const int tt = tb + __builtin_ctzll(tmask);
            tmask &= tmask - 1;
            const float* bp = fbox + (long long)tt * 8;
            const float lbq = point_box_d2(q, *reinterpret_cast<const f32x4*>(bp), *reinterpret_cast<const f32x4*>(bp + 4));
            if (!__ballot(valid && !(lbq > mine))) continue;
            const int ci = cloud_tile_point(tt, lane, gwk);
            f32x4 p = (f32x4){nan_f(), nan_f(), nan_f(), 0.f};
            float nx = nan_f();
            if (ci < Pk) {
              p = *reinterpret_cast<const f32x4*>(cand + (long long)ci * 4);
              nx = cnrm[(long long)ci * 4];
            }
            const int gi = off + ci;
            unsigned long long cm = __ballot(finite3(p) && nx == nx);  // only points with a valid normal take part
            while (cm) {
              const int j = __builtin_ctzll(cm);
              cm &= cm - 1;
              const float cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p[0]), j));
              const float cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p[1]), j));
              const float cz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p[2]), j));
              const unsigned gj = (unsigned)__builtin_amdgcn_readlane(gi, j);
              const float d2 = gap_d2(cx - q[0], cy - q[1], cz - q[2]);
              const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | gj;
              best = key < best ? key : best;
            }
            mine = valid ? __uint_as_float((unsigned)(best >> 32)) : -inf_f();
          }
          tmax = wave_max(mine);  // (bounds only shrink: the group mask taken with the older value stays valid)
        }
      }
    }
  }

  const bool found = best < key0;
  const int gidx = found ? (int)(unsigned)(best & 0xffffffffull) : -1;
  const float d2 = found ? __uint_as_float((unsigned)(best >> 32)) : nan_f();
  if (q_idx) {
    const long long slot = (f * ntq + tile) * 64 + lane;
    q_idx[slot] = gidx;
    q_d2[slot] = d2;
  }
  // the matched target point and its normal
  f32x4 tp = (f32x4){0.f, 0.f, 0.f, 0.f}, tn = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < tg.n; ++k) {
    const long long o = tg.off[k];
    if (found && gidx >= o && gidx < o + tg.P[k]) {
      tp = *reinterpret_cast<const f32x4*>(tg.xyz[k] + (f * tg.P[k] + (gidx - o)) * 4);
      tn = *reinterpret_cast<const f32x4*>(tg.nrm[k] + (f * tg.P[k] + (gidx - o)) * 4);
    }
  }
  // r = (p - q) . n and J = [p x n | n] in fp64 from the fp32 values (p: the query, q: the target point)
  const double w = found ? 1.0 : 0.0;
  const double px = found ? (double)q[0] : 0.0, py = found ? (double)q[1] : 0.0, pz = found ? (double)q[2] : 0.0;
  const double nx = (double)tn[0], ny = (double)tn[1], nz = (double)tn[2];
  const double r = fma(pz - (double)tp[2], nz, fma(py - (double)tp[1], ny, (px - (double)tp[0]) * nx));
  double J[6];
  J[0] = py * nz - pz * ny;
  J[1] = pz * nx - px * nz;
  J[2] = px * ny - py * nx;
  J[3] = nx;
  J[4] = ny;
  J[5] = nz;
  double* row = partial + (f * ntq + tile) * ROW;
  int c = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) {
      const double s = wave_sum_f64(J[i] * J[j]);
      if (lane == 0) row[c] = s;
      ++c;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double s = wave_sum_f64(J[i] * r);
    if (lane == 0) row[21 + i] = s;
  }
  const double s_n = wave_sum_f64(w), s_r2 = wave_sum_f64(r * r), s_d2 = wave_sum_f64(found ? (double)d2 : 0.0);
  if (lane == 0) {
    row[27] = s_n;
    row[28] = s_r2;
    row[29] = s_d2;
  }
}

// One workgroup.  Column c of the rows is summed by 8 threads (thread g takes rows g, g + 8, ... in ascending order) and the 8 partial
// sums are added in the order g = 0..7: an order fixed by n_rows alone.
__global__ __launch_bounds__(AS_WG) void align_solve_kernel(const double* __restrict__ partial, long long n_rows, const double* __restrict__ n_queries,
                                                            int final_call, int max_hist, double* __restrict__ D, int* __restrict__ ist,
                                                            double* __restrict__ hist, double* __restrict__ sums_out, double* __restrict__ result) {
  __shared__ double s_part[8][32];
  __shared__ double S[32];
  __shared__ double A[6][6], L[6][6], dd[6], y[6], x[6];
  if (ist[MVT_ALIGN_I_DONE]) return;
  const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
  double acc = 0.0;
  if (c < ROW)
    for (long long r = g; r < n_rows; r += 8) acc += partial[r * ROW + c];
  s_part[g][c] = acc;
  __syncthreads();
  if (threadIdx.x < ROW) {
    double s = s_part[0][threadIdx.x];
    for (int k = 1; k < 8; ++k) s += s_part[k][threadIdx.x];
    S[threadIdx.x] = s;
    if (sums_out) sums_out[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;

  const int eval = ist[MVT_ALIGN_I_EVALS];
  int iters = ist[MVT_ALIGN_I_ITERATIONS], status = ist[MVT_ALIGN_I_STATUS], done = 0;
  const double count = S[27], nq = n_queries[0];
  const double fitness = nq > 0.0 ? count / nq : 0.0;
  const double rmse = count > 0.0 ? sqrt(S[29] / count) : 0.0;
  double* h = eval < max_hist ? hist + (long long)eval * MVT_ALIGN_HIST : nullptr;
  if (h) {
    h[0] = count, h[1] = fitness, h[2] = rmse, h[3] = S[28];
    for (int i = 0; i < 6; ++i) h[4 + i] = 0.0;
  }
  const double pf = result[0], pr = result[1];  // the previous evaluation's figures
  if (eval > 0 && fabs(fitness - pf) < 1e-6 && fabs(rmse - pr) < 1e-6) {
    done = 1;
  } else if (!final_call) {
    if (count < 6.0) {
      status |= MVT_ALIGN_FEW, done = 1;
    } else {
      int cidx = 0;
      double maxd = 0.0;
      for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = S[cidx++];
      for (int i = 0; i < 6; ++i) maxd = fmax(maxd, A[i][i]);
      bool ok = maxd > 0.0;
      for (int j = 0; j < 6 && ok; ++j) {  // A = L diag(dd) L^T
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * dd[k];
        if (!(d > 1e-12 * maxd)) {
          ok = false;
          break;
        }
        dd[j] = d;
        for (int i = j + 1; i < 6; ++i) {
          double v = A[i][j];
          for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * dd[k];
          L[i][j] = v / d;
        }
      }
      if (!ok) {
        status |= MVT_ALIGN_SINGULAR, done = 1;
      } else {
        for (int i = 0; i < 6; ++i) {  // L y = -J^T r
          double v = -S[21 + i];
          for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
          y[i] = v;
        }
        for (int i = 5; i >= 0; --i) {  // L^T x = y / dd
          double v = y[i] / dd[i];
          for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
          x[i] = v;
        }
        // T(x) = [Rz(x2) Ry(x1) Rx(x0) | x3..5], D <- T D
        const double sa = sin(x[0]), ca = cos(x[0]), sb = sin(x[1]), cb = cos(x[1]), sg = sin(x[2]), cg = cos(x[2]);
        const double R00 = cg * cb, R01 = cg * sb * sa - sg * ca, R02 = cg * sb * ca + sg * sa;
        const double R10 = sg * cb, R11 = sg * sb * sa + cg * ca, R12 = sg * sb * ca - cg * sa;
        const double R20 = -sb, R21 = cb * sa, R22 = cb * ca;
        double n0[4], n1[4], n2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double d0 = D[j], d1 = D[4 + j], d2 = D[8 + j];
          n0[j] = R00 * d0 + R01 * d1 + R02 * d2;
          n1[j] = R10 * d0 + R11 * d1 + R12 * d2;
          n2[j] = R20 * d0 + R21 * d1 + R22 * d2;
        }
        n0[3] += x[3], n1[3] += x[4], n2[3] += x[5];
#pragma unroll
        for (int j = 0; j < 4; ++j) D[j] = n0[j], D[4 + j] = n1[j], D[8 + j] = n2[j];
        if (h)
          for (int i = 0; i < 6; ++i) h[4 + i] = x[i];
        ++iters;
      }
    }
  }
  result[0] = fitness, result[1] = rmse, result[2] = (double)iters, result[3] = (double)status;
  ist[MVT_ALIGN_I_DONE] = done;
  ist[MVT_ALIGN_I_ITERATIONS] = iters;
  ist[MVT_ALIGN_I_STATUS] = status;
  ist[MVT_ALIGN_I_EVALS] = eval + 1;
}

}  // namespace

extern "C" int mvt_align_normals(const float* xyz, int C, int grid_w, int grid_h, float max_edge, float* nrm, void* stream) {
  MVT_REQUIRE(aligned(xyz, 16) && aligned(nrm, 16) && C > 0 && C <= 65535 && grid_w > 0 && grid_h > 0 && grid_w % 8 == 0 && grid_h % 8 == 0);
  MVT_REQUIRE((long long)grid_w * grid_h < (1ll << 31) - 64 && max_edge > 0.f && max_edge < INFINITY);
  const long long total = (long long)C * grid_w * grid_h;
  hipLaunchKernelGGL(align_normals_kernel, dim3(strided_blocks(total)), dim3(256), 0, mvt_stream(stream), xyz, total, grid_w, grid_h,
                     max_edge * max_edge, nrm);
  return mvt_launch_status();
}

extern "C" int mvt_align_transform(const float* xyz0, const double* D, long long n, float* xyz, void* stream) {
  MVT_REQUIRE(aligned(xyz0, 16) && aligned(xyz, 16) && aligned(D, 8) && n > 0 && n < (1ll << 40));
  hipLaunchKernelGGL(align_transform_kernel, dim3(strided_blocks(n)), dim3(256), 0, mvt_stream(stream), xyz0, D, n, xyz);
  return mvt_launch_status();
}

extern "C" int mvt_align_queries(long long P, int grid_w, int grid_h, int sample_stride, int* tiles_per_row) {
  if (!cloud_shape_ok(1, P, grid_w, grid_h) || sample_stride < 1 || (grid_w == 0 && sample_stride != 1)) return -1;
  if (grid_w == 0) {
    if (tiles_per_row) *tiles_per_row = 0;
    return (int)((P + 63) / 64);
  }
  const int ws = (grid_w + sample_stride - 1) / sample_stride, hs = (grid_h + sample_stride - 1) / sample_stride;
  if (tiles_per_row) *tiles_per_row = (ws + 7) / 8;
  return ((ws + 7) / 8) * ((hs + 7) / 8);
}

extern "C" int mvt_align_correspond(const float* src_xyz0, long long src_P, int src_grid_w, int src_grid_h, int sample_stride, int frames,
                                    const double* D, float cap2, const mvt_align_cloud* targets, int n_targets, const int* istate,
                                    double* partial, int* q_idx, float* q_d2, void* stream) {
  MVT_REQUIRE(aligned(src_xyz0, 16) && aligned(D, 8) && aligned(istate, 4) && aligned(partial, 8) && targets != nullptr);
  MVT_REQUIRE((q_idx == nullptr) == (q_d2 == nullptr) && (q_idx == nullptr || (aligned(q_idx, 4) && aligned(q_d2, 4))));
  MVT_REQUIRE(frames > 0 && frames <= 65535 && n_targets >= 1 && n_targets <= MVT_ALIGN_MAX_TARGETS && cap2 > 0.f && cap2 < INFINITY);
  int qtx = 0;
  const int ntq = mvt_align_queries(src_P, src_grid_w, src_grid_h, sample_stride, &qtx);
  MVT_REQUIRE(ntq > 0);
  align_targets tg = {};
  long long off = 0;
  for (int k = 0; k < n_targets; ++k) {
    const mvt_align_cloud& t = targets[k];
    MVT_REQUIRE(aligned(t.xyz, 16) && aligned(t.nrm, 16) && aligned(t.tile_box, 16) && aligned(t.group_box, 16));
    MVT_REQUIRE(cloud_shape_ok(1, t.P, t.grid_w, t.grid_h));
    tg.xyz[k] = t.xyz, tg.nrm[k] = t.nrm, tg.box[k] = t.tile_box, tg.gbox[k] = t.group_box;
    tg.P[k] = t.P, tg.off[k] = off, tg.grid_w[k] = t.grid_w;
    off += t.P;
  }
  MVT_REQUIRE(off < (1ll << 31) - 64);  // the global target index is an int32
  tg.n = n_targets;
  hipLaunchKernelGGL(align_correspond_kernel, dim3((unsigned)mvt_cdiv(ntq, AC_WG / 64), (unsigned)frames), dim3(AC_WG), 0, mvt_stream(stream),
                     src_xyz0, src_P, src_grid_w, src_grid_h, sample_stride, ntq, qtx, D, cap2, tg, istate, partial, q_idx, q_d2);
  return mvt_launch_status();
}

extern "C" int mvt_align_solve(const double* partial, long long n_rows, const double* n_queries, int final_call, int max_hist, double* D,
                               int* istate, double* hist, double* sums, double* result, void* stream) {
  MVT_REQUIRE(aligned(partial, 8) && aligned(n_queries, 8) && aligned(D, 8) && aligned(istate, 4) && aligned(hist, 8) && aligned(result, 8));
  MVT_REQUIRE(n_rows > 0 && n_rows < (1ll << 31) && max_hist >= 0 && (sums == nullptr || aligned(sums, 8)));
  hipLaunchKernelGGL(align_solve_kernel, dim3(1), dim3(AS_WG), 0, mvt_stream(stream), partial, n_rows, n_queries, final_call ? 1 : 0, max_hist, D,
                     istate, hist, sums, result);
  return mvt_launch_status();
}
