// Track overlays: the tracker's 3-D tracks drawn into every view's frames (reference: mvtracker/utils/visualizer_mp4.py
// Visualizer.visualize / draw_tracks_on_video / _draw_pred_tracks, which draws on the CPU with one cv2.line per (frame, older frame,
// track)).  The drawing rule is stated in include/mvtracker_hip.h and DESIGN section 8 "Track overlays".
//
// project - one thread per (view, frame, track): world_space_to_pixel_xy_and_camera_z in fp32 with every product, sum and quotient
//           rounded on its own, so numpy float32 gives the same bits; optionally the integer point (clip, + pad, truncate) with its
//           validity, and the track's rainbow colour from the launch that projects its query frame.
// draw    - the scatter of ONE frame: the V * M markers of frame t and the V * M segments (t-1 -> t).  A primitive belongs to a group
//           of 8 lanes, which walks the rows of its clipped bounding box with the lanes across the columns; for a long segment the
//           columns of a row are narrowed to the part of the segment that can reach the row, so the walk is O(length), not O(box).
//           A covered pixel keeps the maximum of the 64-bit key order << 24 | rgb through ONE unsigned 64-bit atomicMax: the painter's
//           last writer, whatever the order of arrival.  Segment order is (s+1) << 20 | track in a key plane that persists over the
//           frames (a newer segment always outranks an older one, so only the new segments are scattered per frame); marker order is
//           track + 1 in a plane of its own.  Every address is checked against the padded image before the atomic.
// compose - per pixel of the padded image: marker key, else the line key if its segment is inside the trail window, else the frame's
//           byte (or 255 on the border); the frame is read once, the output written once, the marker plane reset as it is read.
// Integer max does not depend on the order of arrival: the same bits in every run.  No float atomics, no locks, every loop bounded.
#include "common.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int OV_WG = 256;
constexpr int OV_GROUP = 8;  // lanes per primitive

// The integer point of the drawing rule.  false: the point is invalid (x, y are then 0).
__device__ __forceinline__ bool ov_pixel(float px, float py, float z, float pad, int use_min_depth, float min_depth, int& x, int& y) {
#pragma clang fp contract(off)
  x = y = 0;
  if (px != px || py != py) return false;
  if (use_min_depth && !(z > min_depth)) return false;
  // a comparison chain, not fminf / fmaxf: those drop a NaN (none is left here) and the rule is easier to read this way
  const float cx = px < -1e4f ? -1e4f : (px > 1e4f ? 1e4f : px);
  const float cy = py < -1e4f ? -1e4f : (py > 1e4f ? 1e4f : py);
  x = (int)(cx + pad);  // truncation toward zero, as the reference's .long()
  y = (int)(cy + pad);
  return true;
}

__global__ __launch_bounds__(OV_WG) void project_kernel(const float* __restrict__ tracks, const float* __restrict__ intrs,
                                                        const float* __restrict__ extrs, int V, int T, int N, float* __restrict__ xyz,
                                                        int* __restrict__ points, float pad, int use_min_depth, float min_depth,
                                                        const int* __restrict__ query_frames, int frame0,
                                                        const unsigned char* __restrict__ lut, int color_view, int Hp,
                                                        unsigned char* __restrict__ colors) {
#pragma clang fp contract(off)
  const i64 idx = blockIdx.x * (i64)OV_WG + threadIdx.x;
  if (idx >= (i64)V * T * N) return;
  const int n = (int)(idx % N);
  const int t = (int)((idx / N) % T);
  const int v = (int)(idx / ((i64)N * T));
  const float* p = tracks + ((i64)t * N + n) * 3;
  const float* K = intrs + ((i64)v * T + t) * 9;
  const float* E = extrs + ((i64)v * T + t) * 12;
  const float x = p[0], y = p[1], z = p[2];
  float c[3], h[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) c[r] = ((E[4 * r] * x + E[4 * r + 1] * y) + E[4 * r + 2] * z) + E[4 * r + 3];
#pragma unroll
  for (int r = 0; r < 3; ++r) h[r] = (K[3 * r] * c[0] + K[3 * r + 1] * c[1]) + K[3 * r + 2] * c[2];
  const float px = h[0] / h[2], py = h[1] / h[2];  // correctly rounded: the build keeps hipcc's default IEEE fp32 division
  if (xyz) {
    float* o = xyz + idx * 3;  // (V, T, N, 3)
    o[0] = px, o[1] = py, o[2] = c[2];
  }
  if (points == nullptr && lut == nullptr) return;
  int xi, yi;
  const bool valid = ov_pixel(px, py, c[2], pad, use_min_depth, min_depth, xi, yi);
  if (points) {
    int* o = points + (((i64)t * V + v) * N + n) * 4;  // (T, V, N, 4)
    o[0] = xi, o[1] = yi, o[2] = valid ? 1 : 0, o[3] = 0;
  }
  if (lut && v == color_view && frame0 + t == max(query_frames[n], 0)) {
    const int yc = valid ? yi : (int)pad;
    const int k = yc <= 0 ? 0 : min(255, (int)(((i64)yc * 256) / Hp));
    colors[n * 3] = lut[k * 3], colors[n * 3 + 1] = lut[k * 3 + 1], colors[n * 3 + 2] = lut[k * 3 + 2];
  }
}

// pixel p against the stroke of width w from a to b (the rule of the header), all in 64-bit integers
__device__ __forceinline__ bool ov_stroke_covers(i64 px, i64 py, i64 ax, i64 ay, i64 bx, i64 by, i64 dx, i64 dy, i64 L2, i64 w2) {
  const i64 ex = px - ax, ey = py - ay;
  const i64 q = ex * dx + ey * dy;
  if (q <= 0) return 4 * (ex * ex + ey * ey) <= w2;
  if (q >= L2) {
    const i64 fx = px - bx, fy = py - by;
    return 4 * (fx * fx + fy * fy) <= w2;
  }
  const i64 cr = ex * dy - ey * dx;
  return 4 * (cr * cr) <= w2 * L2;
}

__global__ __launch_bounds__(OV_WG) void draw_kernel(const int* __restrict__ prev, const int* __restrict__ cur,
                                                     const unsigned char* __restrict__ visibility, const int* __restrict__ query_frames,
                                                     const unsigned char* __restrict__ colors, int V, int N, int M, int t, int w, int Hp,
                                                     int Wp, u64* __restrict__ line_keys, u64* __restrict__ marker_keys) {
  const i64 gid = blockIdx.x * (i64)OV_WG + threadIdx.x;
  const i64 prim = gid / OV_GROUP;
  const int lane = (int)(gid % OV_GROUP);
  const i64 VM = (i64)V * M;
  if (prim >= (prev ? 2 * VM : VM)) return;
  const bool segment = prim >= VM;  // markers first, then the segments
  const i64 r = segment ? prim - VM : prim;
  const int v = (int)(r / M), i = (int)(r % M);
  const int q = query_frames[i];
  const int* b = cur + ((i64)v * N + i) * 4;
  if (!b[2]) return;
  const int bx = b[0], by = b[1];
  const u64 rgb = ((u64)colors[i * 3] << 16) | ((u64)colors[i * 3 + 1] << 8) | (u64)colors[i * 3 + 2];
  const i64 plane = (i64)v * Hp * Wp;
  if (!segment) {
    if (q > t || bx == 0 || by == 0) return;
    const bool disc = visibility ? visibility[i] != 0 : true;
    const int R = 2 * w;
    const u64 key = ((u64)(i + 1) << 24) | rgb;
    const i64 R2 = (i64)R * R, lo = (i64)(2 * R - 1) * (2 * R - 1), hi = (i64)(2 * R + 1) * (2 * R + 1);
    const int y0 = max(by - R - 1, 0), y1 = min(by + R + 1, Hp - 1);
    const int x0 = max(bx - R - 1, 0), x1 = min(bx + R + 1, Wp - 1);
    for (int y = y0; y <= y1; ++y)
      for (int x = x0 + lane; x <= x1; x += OV_GROUP) {
        const i64 ex = x - bx, ey = y - by, d2 = ex * ex + ey * ey;
        if (disc ? d2 <= R2 : (lo <= 4 * d2 && 4 * d2 <= hi)) atomicMax(marker_keys + plane + (i64)y * Wp + x, key);
      }
    return;
  }
  const int* a = prev + ((i64)v * N + i) * 4;
  if (t - 1 < q || !a[2]) return;
  const int ax = a[0], ay = a[1];
  if ((ax == 0 && ay == 0) || (bx == 0 && by == 0)) return;
  const u64 key = ((((u64)t << 20) | (u64)i) << 24) | rgb;  // order (s + 1) << 20 | i with s + 1 = t
  const int h = (w + 1) / 2;
  const i64 dx = (i64)bx - ax, dy = (i64)by - ay, L2 = dx * dx + dy * dy, w2 = (i64)w * w;
  const int y0 = max(min(ay, by) - h, 0), y1 = min(max(ay, by) + h, Hp - 1);
  for (int y = y0; y <= y1; ++y) {
    // A covered pixel lies within h of its nearest point of the segment, so that point's row is within h of y: only the part of
    // the segment with |row - y| <= h can reach this row.  Its columns, widened by h and by one more for the float arithmetic.
    int xlo = min(ax, bx) - h, xhi = max(ax, bx) + h;
    if (dy != 0) {
      const float inv = 1.0f / (float)dy;
      float t0 = (float)(y - h - ay) * inv, t1 = (float)(y + h - ay) * inv;
      if (t0 > t1) {
        const float s = t0;
        t0 = t1, t1 = s;
      }
      t0 = fminf(fmaxf(t0, 0.f), 1.f), t1 = fminf(fmaxf(t1, 0.f), 1.f);
      const float xa = (float)ax + t0 * (float)dx, xb = (float)ax + t1 * (float)dx;
      xlo = max(xlo, (int)floorf(fminf(xa, xb)) - h - 1);
      xhi = min(xhi, (int)ceilf(fmaxf(xa, xb)) + h + 1);
    }
    xlo = max(xlo, 0), xhi = min(xhi, Wp - 1);
    for (int x = xlo + lane; x <= xhi; x += OV_GROUP)
      if (ov_stroke_covers(x, y, ax, ay, bx, by, dx, dy, L2, w2)) atomicMax(line_keys + plane + (i64)y * Wp + x, key);
  }
}

__global__ __launch_bounds__(OV_WG) void compose_kernel(const void* __restrict__ frames, int is_u8, int V, int T, int tl, int H, int W,
                                                        int pad, const u64* __restrict__ line_keys, u64 min_line_key,
                                                        u64* __restrict__ marker_keys, unsigned char* __restrict__ out) {
  const int Hp = H + 2 * pad, Wp = W + 2 * pad;
  const i64 HWp = (i64)Hp * Wp, HW = (i64)H * W;
  const i64 idx = blockIdx.x * (i64)OV_WG + threadIdx.x;
  if (idx >= V * HWp) return;
  const int v = (int)(idx / HWp);
  const i64 pix = idx - v * HWp;
  const int y = (int)(pix / Wp), x = (int)(pix - (i64)y * Wp);
  const u64 mk = marker_keys[idx];
  if (mk) marker_keys[idx] = 0;
  const u64 lk = line_keys ? line_keys[idx] : 0;
  unsigned char* o = out + ((i64)v * T + tl) * 3 * HWp + pix;
  if (mk || (lk && lk >= min_line_key)) {
    const unsigned rgb = (unsigned)(mk ? mk : lk) & 0xFFFFFFu;
    o[0] = (unsigned char)(rgb >> 16), o[HWp] = (unsigned char)(rgb >> 8), o[2 * HWp] = (unsigned char)rgb;
    return;
  }
  const int fy = y - pad, fx = x - pad;
  if (fy < 0 || fy >= H || fx < 0 || fx >= W) {
    o[0] = o[HWp] = o[2 * HWp] = 255;
    return;
  }
  const i64 src = ((i64)v * T + tl) * 3 * HW + (i64)fy * W + fx;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int val;
    if (is_u8) {
      val = reinterpret_cast<const unsigned char*>(frames)[src + c * HW];
    } else {  // clamp to [0, 255] and truncate; NaN -> 0
      const float f = reinterpret_cast<const float*>(frames)[src + c * HW];
      val = f >= 255.f ? 255 : (f > 0.f ? (int)f : 0);
    }
    o[c * HWp] = (unsigned char)val;
  }
}

inline bool aligned(const void* p, size_t a) { return p && ((uintptr_t)p % a) == 0; }
inline bool ov_counts_ok(int V, int T, int N) {
  return V > 0 && T > 0 && N > 0 && N < MVT_OVERLAY_MAX_INDEX && T < MVT_OVERLAY_MAX_INDEX && (long long)V * T * N < (1ll << 31);
}
inline bool ov_image_ok(int V, int Hp, int Wp) {
  return Hp > 0 && Wp > 0 && Hp <= MVT_OVERLAY_MAX_SIDE && Wp <= MVT_OVERLAY_MAX_SIDE && (long long)V * Hp * Wp < (1ll << 31);
}

}  // namespace

extern "C" int mvt_overlay_project(const float* tracks, const float* intrs, const float* extrs, int V, int T, int N, float* xyz, int* points,
                                   int pad, int use_min_depth, float min_depth, const int* query_frames, int frame0, const unsigned char* lut,
                                   int color_view, int Hp, unsigned char* colors, void* stream) {
  MVT_REQUIRE(aligned(tracks, 4) && aligned(intrs, 4) && aligned(extrs, 4) && ov_counts_ok(V, T, N));
  MVT_REQUIRE((xyz == nullptr || aligned(xyz, 4)) && (points == nullptr || aligned(points, 16)) && (xyz != nullptr || points != nullptr || lut != nullptr));
  MVT_REQUIRE(pad >= 0 && pad <= MVT_OVERLAY_MAX_PAD && (!use_min_depth || (min_depth == min_depth && fabsf(min_depth) < INFINITY)));
  if (lut) {
    MVT_REQUIRE(aligned(query_frames, 4) && colors != nullptr && color_view >= 0 && color_view < V && Hp > 2 * pad && Hp <= MVT_OVERLAY_MAX_SIDE &&
                frame0 >= 0 && frame0 < MVT_OVERLAY_MAX_INDEX - T);
  }
  hipLaunchKernelGGL(project_kernel, dim3((unsigned)mvt_cdiv((long long)V * T * N, OV_WG)), dim3(OV_WG), 0, mvt_stream(stream), tracks, intrs, extrs, V,
                     T, N, xyz, points, (float)pad, use_min_depth ? 1 : 0, min_depth, query_frames, frame0, lut, color_view, Hp, colors);
  return mvt_launch_status();
}

extern "C" int mvt_overlay_draw(const int* prev, const int* cur, const unsigned char* visibility, const int* query_frames,
                                const unsigned char* colors, int V, int N, int M, int t, int linewidth, int Hp, int Wp,
                                unsigned long long* line_keys, unsigned long long* marker_keys, void* stream) {
  MVT_REQUIRE(aligned(cur, 16) && aligned(query_frames, 4) && colors != nullptr && aligned(marker_keys, 8));
  MVT_REQUIRE((prev == nullptr) == (line_keys == nullptr) && (prev == nullptr || (aligned(prev, 16) && aligned(line_keys, 8) && t >= 1)));
  MVT_REQUIRE(V > 0 && N > 0 && N < MVT_OVERLAY_MAX_INDEX && M >= 1 && M <= N && t >= 0 && t < MVT_OVERLAY_MAX_INDEX && (long long)V * N < (1ll << 27));
  MVT_REQUIRE(linewidth >= 1 && linewidth <= MVT_OVERLAY_MAX_LINEWIDTH && ov_image_ok(V, Hp, Wp));
  const long long prims = (long long)V * M * (prev ? 2 : 1);
  hipLaunchKernelGGL(draw_kernel, dim3((unsigned)mvt_cdiv(prims * OV_GROUP, OV_WG)), dim3(OV_WG), 0, mvt_stream(stream), prev, cur, visibility,
                     query_frames, colors, V, N, M, t, linewidth, Hp, Wp, line_keys, marker_keys);
  return mvt_launch_status();
}

extern "C" int mvt_overlay_compose(const void* frames, int is_u8, int V, int T, int t_local, int H, int W, int pad,
                                   const unsigned long long* line_keys, int first_segment, unsigned long long* marker_keys, unsigned char* out,
                                   void* stream) {
  MVT_REQUIRE(frames != nullptr && (is_u8 || aligned(frames, 4)) && (line_keys == nullptr || aligned(line_keys, 8)) && aligned(marker_keys, 8) &&
              out != nullptr);
  MVT_REQUIRE(V > 0 && T > 0 && t_local >= 0 && t_local < T && H > 0 && W > 0 && pad >= 0 && pad <= MVT_OVERLAY_MAX_PAD);
  MVT_REQUIRE(ov_image_ok(V, H + 2 * pad, W + 2 * pad) && first_segment >= 0 && first_segment < MVT_OVERLAY_MAX_INDEX);
  const long long total = (long long)V * (H + 2 * pad) * (W + 2 * pad);
  hipLaunchKernelGGL(compose_kernel, dim3((unsigned)mvt_cdiv(total, OV_WG)), dim3(OV_WG), 0, mvt_stream(stream), frames, is_u8 ? 1 : 0, V, T, t_local, H,
                     W, pad, line_keys, (u64)(first_segment + 1) << 44, marker_keys, out);
  return mvt_launch_status();
}
