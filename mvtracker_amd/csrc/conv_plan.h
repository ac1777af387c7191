// Launch plans of the GEMM and convolution kernels (gemm.hip, conv_rows.hip) and of the composite encoder that sequences them
// (encoder_forward.hip): which kernel family runs, with which template tuple, on what grid, with how many statistics slots, and
// what a call is refused for.  Every threshold of that dispatch and every tile constant that both a kernel and the dispatch use is
// stated here and nowhere else: the entries launch what these functions return, mvt_conv2d_stat_slots is conv_stat_slots, and the
// CPU test tests/test_conv_plan_host.py compiles this header with the host compiler alone and compares it with the dispatch
// restatements of the exact GPU suites, with a written-out launch table and with recorded slot counts.  Host-only and HIP-free like
// launch_plan.h: plain functions of sizes, flags and switch values, no environment reads.
#pragma once
#include "launch_plan.h"

namespace mvt_plan {

// ---- tile constants shared by the kernels and the dispatch

constexpr int BK = 32;    // k-tile of the fp32 GEMM kernel
constexpr int BKB = 64;   // k-tile of the bf16 GEMM kernels; weight rows are [Cout][round_up(K, BKB)], zero padded
constexpr int HT = 8, HW_ = 16;  // output tile of the 3x3 halo kernel (gemm.hip): four 32-pixel statistics slots
constexpr int TR = 8;     // output rows per workgroup (stem, big tile and the default stride-1 3x3 row tile)
constexpr int TC = 32;    // output columns per workgroup of every row-tile kernel
constexpr int CK = 32;    // channels per chunk
constexpr int LDP = CK + 8;   // bf16 per pixel / weight-row slot of the row tiles' LDS (80 B)
constexpr int MAXC = 512;     // input channels the in-kernel normalisation of the row tiles supports
constexpr int SKW = 7 * 32;   // K of the 7x7 stem (Cin padded to 4: one 32-wide k-tile per filter row)
constexpr int BG_BN = 256;    // output channels per workgroup of conv3x3_big_bf16

// Elements of the per-wave LDS staging tile of the bf16 epilogue: 32 pixels x (TN * 32 + 8) channels.
constexpr int stage_elems(int tn) { return 32 * (tn * 32 + 8); }
// Pixel slots of the input patch of one row-tile workgroup (Geo<TM, KS, S, NW>::NSLOT in conv_rows.hip): NW * TM output rows of TC
// pixels; a stride-2 3x3 row is stored as its even and its odd columns.
constexpr int patch_slots(int tm, int ks, int s, int nw) {
  const int rows = nw * tm, pr = ks == 1 ? rows : s * (rows - 1) + 3, pc = ks == 1 ? TC : s * (TC - 1) + 3;
  return pr * (ks == 3 && s == 2 ? 2 * ((pc + 1) / 2) : pc);
}
// The staged bf16 epilogue exists where the per-wave staging tiles fit the patch LDS they reuse.
constexpr bool rows_staged_fits(int tm, int tn, int ks, int s, int nw) { return nw * stage_elems(tn) <= patch_slots(tm, ks, s, nw) * LDP; }

// The tuning switches of the convolution dispatch, as conv_switches() (conv_rows.hip) reads them from the environment:
// MVT_ROWS_NW8 (its atoi; once per process), MVT_CONV_BIG not 0 (every call), MVT_FOLD_DOWNSAMPLE not 0 (once per process).
struct ConvSwitches {
  int rows_nw8;
  bool conv_big;
  bool fold_downsample;
};

// ---- GEMM tiles: gemm_mfma_f32 / gemm_mfma_bf16 <TM, TN, WM, WN> (workgroup tile WM * TM * 32 rows x WN * TN * 32 columns)

struct GemmTile {
  int tm, tn, wm, wn;
  long long blocks;
};
// The tuple as the decimal digits TM TN WM WN (every value is a single digit): <2, 2, 4, 1> is 2241.  The launchers switch over it;
// a tuple that a launcher does not name is MVT_ERR_ARG, and tests/test_conv_plan_host.py holds the rules to the tuples that exist.
inline int tile_key(const GemmTile& t) { return ((t.tm * 10 + t.tn) * 10 + t.wm) * 10 + t.wn; }
namespace detail {
inline GemmTile tile(int tm, int tn, int wm, int wn, long long row_tiles, int N) { return {tm, tn, wm, wn, row_tiles * cdiv(N, wn * tn * 32)}; }
inline GemmTile gemm(int tm, int tn, int wm, int wn, long long M, int N) { return tile(tm, tn, wm, wn, cdiv(M, wm * tm * 32), N); }
}  // namespace detail
// The largest tile that still gives every CU at least two workgroups (latency hiding comes from co-resident blocks); narrow N picks
// the matching BN so no MFMA columns are wasted.
inline GemmTile gemm_tile(long long M, int N) {
  if (N % 128 != 0 && N % 96 == 0) return detail::gemm(1, 3, 4, 1, M, N);  // 128 x 96
  if (N <= 64) {
    const GemmTile t = detail::gemm(2, 2, 4, 1, M, N);                     // 256 x 64, else 64 x 64
    return t.blocks >= 512 ? t : detail::gemm(1, 1, 2, 2, M, N);
  }
  GemmTile t = detail::gemm(2, 2, 2, 2, M, N);                             // 128 x 128
  if (t.blocks >= 512) return t;
  t = detail::gemm(1, 2, 2, 2, M, N);                                      // 64 x 128
  return t.blocks >= 512 ? t : detail::gemm(1, 1, 2, 2, M, N);             // 64 x 64
}
// conv3x3_halo_bf16 <TM, TN, WM, WN>: `tiles` HT x HW_ pixel tiles, each times the channel blocks of 96, 64 or 128.
inline GemmTile halo_tile(long long tiles, int N) {
  if (N % 128 != 0 && N % 96 == 0) return detail::tile(1, 3, 4, 1, tiles, N);
  if (N <= 64) return detail::tile(1, 2, 4, 1, tiles, N);
  return detail::tile(2, 2, 2, 2, tiles, N);
}

// ---- convolutions

inline int conv_out(int size, int k, int stride, int pad) { return (size + 2 * pad - k) / stride + 1; }
// Weight row stride: [Cout][round_up(K, 64)], K = KH * KW * Cin, or KH * 32 for the stem's Cin = 4.
inline int conv_ldw(int Cin, int KH, int KW) { return (int)cdiv(Cin == 4 ? KH * 32 : KH * KW * Cin, BKB) * BKB; }

// The shapes the kernel families take (bf16 mode): row tiles, the halo kernel, the stem.
inline bool rows_shape(int Cin, int KH, int KW, int pad) { return Cin % 32 == 0 && KH == KW && ((KH == 3 && pad == 1) || (KH == 1 && pad == 0)); }
inline bool halo_shape(int Cin, int KH, int KW, int stride, int pad) { return KH == 3 && KW == 3 && stride == 1 && pad == 1 && Cin % CK == 0; }
inline bool stem_shape(int Cin, int KH, int KW, int stride, int pad) { return Cin == 4 && KH == 7 && KW == 7 && stride == 2 && pad == 3; }

// Output rows of one row-tile workgroup (NW * TM) = of one statistics slot, for (kernel size, stride): the stride-2 patch is four
// times larger per output pixel, hence 4 x 32 pixel tiles; rows_nw8 = 1: sixteen rows of eight waves where they tile Ho, 2: four rows.
inline int tile_rows(int ksize, int stride, int Ho, const ConvSwitches& sw) {
  if (ksize == 3 && stride == 1) return (sw.rows_nw8 == 1 && Ho % 16 == 0) ? 16 : (sw.rows_nw8 == 2 ? 4 : 8);
  return ksize == 3 ? 4 : 8;  // (1x1, and the stem's TR)
}
// Statistics slots of a kernel family: one per row-tile workgroup, four per halo tile, one per 32 output pixels of the im2col GEMM
// (whose tiles are <= 256 rows and must not straddle images).
inline int rows_slots(int Ho, int Wo, int rows) { return (int)(cdiv(Ho, rows) * cdiv(Wo, TC)); }
inline long long halo_tiles(int Ho, int Wo) { return cdiv(Ho, HT) * cdiv(Wo, HW_); }
inline int im2col_slots(int Ho, int Wo) { return ((long long)Ho * Wo) % 256 == 0 ? Ho * Wo / 32 : 0; }

// mvt_conv2d_stat_slots: the slots by which the caller sizes out_partial, [n][slots][Cout][2].  split: bf16x3 (a lo weight part).
inline int conv_stat_slots(int H, int W, int Cin, int KH, int KW, int stride, int pad, bool split, const ConvSwitches& sw) {
  const int Ho = conv_out(H, KH, stride, pad), Wo = conv_out(W, KW, stride, pad);
  if (Ho <= 0 || Wo <= 0) return 0;
  if (!split && rows_shape(Cin, KH, KW, pad) && stride <= 2) return rows_slots(Ho, Wo, tile_rows(KH, stride, Ho, sw));
  if (halo_shape(Cin, KH, KW, stride, pad)) return (int)(halo_tiles(Ho, Wo) * 4);
  if (!split && stem_shape(Cin, KH, KW, stride, pad)) return rows_slots(Ho, Wo, TR);
  return im2col_slots(Ho, Wo);
}

enum ConvFamily { CONV_REFUSED = 0, CONV_GEMM_F32, CONV_IM2COL, CONV_HALO, CONV_STEM_ROWS, CONV_ROWS, CONV_BIG };

// One launch.  The template tuple by family:
//   CONV_GEMM_F32  gemm_mfma_f32<tile>            CONV_IM2COL  gemm_mfma_bf16<tile, split>         CONV_HALO  conv3x3_halo_bf16<tile, split>
//   CONV_STEM_ROWS stem7x7_rows_bf16<tn, staged>  CONV_ROWS    conv_rows_bf16<tm, tn, ks, s, inb, nw, staged>  CONV_BIG  conv3x3_big_bf16
// rows: output rows of one workgroup tile (0: the GEMM families); slots: conv_stat_slots of the call; ldw: weight row stride.
struct ConvPlan {
  ConvFamily family;
  GemmTile tile;
  int tm, tn, ks, s, nw;
  bool inb, out_bf16, staged, split;  // bf16 input / output tensor, staged epilogue, bf16x3
  int threads;
  long long grid;
  int rows, slots, ldw;
};

struct ConvCall {
  int n, H, W, Cin, Cout, KH, KW, stride, pad, ldo, act;
  int io_flags;     // MVT_IO_*
  bool fp32;        // mvt_conv2d: the fp32 kernels (no io flags, lo part, statistics)
  bool has_lo, has_in_stats, has_out_partial;
  bool in_al16, out_al16, w_al8, w_al16, lo_al8, stats_al16;  // alignment of in, out, the (hi) weights, the lo part, in_stats
};

namespace detail {
inline ConvPlan no_conv() { return ConvPlan{}; }
// bf16 output goes through the LDS-staged epilogue when the tensor allows 16-byte pieces
inline bool staged_ok(int Cout, int ldo, int io_flags, bool out_al16) { return (io_flags & MVT_IO_OUT_BF16) && Cout % 8 == 0 && ldo % 8 == 0 && out_al16; }
inline bool grid_ok(long long tiles) { return tiles < (1LL << 31); }
}  // namespace detail

// The 7x7 / stride-2 / pad-3 stem on row tiles (Cin padded to 4, Cout <= 64, fp32 input: the [n][H][W][4] tensor or the planar clip).
inline ConvPlan plan_stem(int n, int H, int W, int Cout, int ldo, int io_flags, bool out_al16) {
  const int Ho = conv_out(H, 7, 2, 3), Wo = conv_out(W, 7, 2, 3);
  ConvPlan p{};
  p.ldw = conv_ldw(4, 7, 7);  // (>= SKW)
  p.grid = (long long)n * cdiv(Ho, TR) * cdiv(Wo, TC);
  if (Cout <= 0 || Cout > 64 || (long long)H * W * 4 >= (1LL << 31) || (io_flags & MVT_IO_IN_BF16)) return detail::no_conv();
  if (!detail::grid_ok(p.grid) || (long long)(TC + 8) * ldo * 4 >= (1LL << 31)) return detail::no_conv();
  p.family = CONV_STEM_ROWS;
  p.tm = 2, p.tn = Cout <= 32 ? 1 : 2, p.ks = 7, p.s = 2, p.nw = 4;
  p.out_bf16 = (io_flags & MVT_IO_OUT_BF16) != 0;
  p.staged = detail::staged_ok(Cout, ldo, io_flags, out_al16);
  p.threads = 256;
  p.rows = TR;
  p.slots = rows_slots(Ho, Wo, TR);
  return p;
}

// mvt_conv3x3s2_down_bf16: the stride-2 3x3 convolution of a ResidualBlock and the block's 1x1 / stride-2 downsample of the same
// input in one launch of conv_rows_bf16<1, tn, 3, 2, true, 4, true, DS = true>; bf16 tensors, staged epilogue.  ldw: the 3x3
// weights' row stride, ldwd: the downsample weights'.
struct DownPlan {
  bool ok;
  int tn, threads, rows, slots, ldw, ldwd;
  long long grid;
};
inline DownPlan plan_down(int n, int H, int W, int Cin, int Cout, int ldo, bool same_partials, bool all_al16) {
  static_assert(rows_staged_fits(1, 2, 3, 2, 4) && rows_staged_fits(1, 3, 3, 2, 4), "the fused downsample always takes the staged epilogue");
  const int Ho = conv_out(H, 3, 2, 1), Wo = conv_out(W, 3, 2, 1);
  DownPlan p{};
  p.tn = (Cout % 64 != 0 && Cout % 96 == 0) ? 3 : 2;
  p.threads = 256;
  p.rows = 4;
  p.slots = rows_slots(Ho, Wo, 4);
  p.ldw = conv_ldw(Cin, 3, 3), p.ldwd = conv_ldw(Cin, 1, 1);
  p.grid = (long long)n * cdiv(Ho, 4) * cdiv(Wo, TC) * cdiv(Cout, p.tn * 32);
  p.ok = n > 0 && Cin > 0 && Cin % CK == 0 && Cout > 0 && Cout % 32 == 0 && ldo % 8 == 0 && ldo >= Cout && (long long)H * W * Cin < (1LL << 31) &&
         (long long)Cout * p.ldw < (1LL << 31) && (long long)n * Ho * Wo < (1LL << 31) && all_al16 && same_partials && detail::grid_ok(p.grid);
  return p;
}

// mvt_conv2d (c.fp32) and mvt_conv2d_bf16, after the entries' range checks (sizes positive, kernel <= 7, stride 1 or 2, pad <= 3,
// H, W < 16384, ldo >= Cout, act in 0..3).  In bf16 mode without a lo part:
//   the stem shape with Cout <= 64 and no activation                -> stem rows
//   every 3x3 (pad 1) and 1x1 (pad 0), Cin % 32 == 0, no activation -> row tiles, or the big tile
// else 3x3 / stride 1 / pad 1 with Cin % 32 == 0 -> the halo kernel, everything else -> the im2col / stem loaders of the GEMM kernels.
// A grid of 2^31 workgroups or more is refused.
// The big tile (one 512-thread workgroup per 8 x 32 pixels and 256 channels, LDS-DMA staging; conv_big = false keeps the row tiles)
// takes wide 3x3 / stride-1 layers of aligned bf16 tensors without normalise-on-load, outside short-workgroup calls.  Its
// statistics slots are its own TR-row tiles while the caller sized out_partial by conv_stat_slots, which follows the row tile that
// rows_nw8 selects: where the two differ (16 rows: slots written past the image's part of the buffer; 4 rows: slots never written) a
// launch that takes statistics stays on the row tiles.
// Statistics are refused wherever the family that runs does not write the slots of conv_stat_slots (the stem shape with Cout > 64
// runs the GEMM kernel, whose 32-pixel slots are not the stem's tiles).
inline ConvPlan plan_conv(const ConvCall& c, const ConvSwitches& sw) {
  using namespace detail;
  if (!(c.Cin % 32 == 0 || c.Cin == 4) || !c.in_al16) return no_conv();
  if (c.fp32 ? !c.w_al16 : !(c.w_al8 && (!c.has_lo || c.lo_al8))) return no_conv();
  const int Ho = conv_out(c.H, c.KH, c.stride, c.pad), Wo = conv_out(c.W, c.KW, c.stride, c.pad);
  if (Ho <= 0 || Wo <= 0) return no_conv();
  const long long M = (long long)c.n * Ho * Wo;
  if (M >= (1LL << 31)) return no_conv();
  ConvPlan p{};
  p.ldw = conv_ldw(c.Cin, c.KH, c.KW);
  p.split = c.has_lo;
  p.threads = 256;
  if (c.fp32) {
    p.family = CONV_GEMM_F32;
    p.tile = gemm_tile(M, c.Cout);
    p.grid = p.tile.blocks;
    return p;
  }
  const bool inb = (c.io_flags & MVT_IO_IN_BF16) != 0;
  const bool halo = halo_shape(c.Cin, c.KH, c.KW, c.stride, c.pad);
  const bool rows = !c.has_lo && c.act == MVT_ACT_NONE && rows_shape(c.Cin, c.KH, c.KW, c.pad);
  if (c.has_in_stats && !((halo || rows) && c.stats_al16)) return no_conv();  // normalise-on-load: halo / row-tile kernels only
  if (c.io_flags & ~(MVT_IO_IN_BF16 | MVT_IO_OUT_BF16 | MVT_IO_SHORT_WG)) return no_conv();
  if ((c.io_flags & (MVT_IO_IN_BF16 | MVT_IO_OUT_BF16)) && c.has_lo) return no_conv();  // bf16 tensors: bf16 mode only
  if (inb && c.Cin % 32 != 0) return no_conv();                                         // (the stem reads fp32 RGB)
  p.slots = conv_stat_slots(c.H, c.W, c.Cin, c.KH, c.KW, c.stride, c.pad, c.has_lo, sw);
  if (c.has_out_partial && !(p.slots > 0 && (c.has_lo || c.act == MVT_ACT_NONE))) return no_conv();
  int own_slots;  // the slots the family that runs writes
  if (!c.has_lo && stem_shape(c.Cin, c.KH, c.KW, c.stride, c.pad) && c.Cout <= 64 && c.act == MVT_ACT_NONE) {
    const int slots = p.slots;
    p = plan_stem(c.n, c.H, c.W, c.Cout, c.ldo, c.io_flags, c.out_al16);
    own_slots = p.slots;
    p.slots = slots;
  } else if (rows) {
    if ((c.has_in_stats && c.Cin > MAXC) || (long long)c.H * c.W * c.Cin >= (1LL << 31) || (long long)c.Cout * p.ldw >= (1LL << 31) ||
        (long long)(TC + 8) * c.ldo * 4 >= (1LL << 31))
      return no_conv();
    const bool st_ok = staged_ok(c.Cout, c.ldo, c.io_flags, c.out_al16);
    p.ks = c.KH, p.s = c.stride, p.inb = inb, p.out_bf16 = (c.io_flags & MVT_IO_OUT_BF16) != 0;
    p.rows = tile_rows(c.KH, c.stride, Ho, sw);
    if (c.KH == 3 && c.stride == 1 && !c.has_in_stats && (!c.has_out_partial || p.rows == TR) && !(c.io_flags & MVT_IO_SHORT_WG) && inb && st_ok &&
        c.Cout % BG_BN == 0 && c.Cin % 8 == 0 && p.ldw % 8 == 0 && c.w_al16 && (long long)c.Cout * p.ldw * 2 < (1LL << 31) &&
        (long long)c.H * c.W * c.Cin * 2 < (1LL << 31) && sw.conv_big) {
      p.family = CONV_BIG;
      p.rows = TR;
      p.tm = 4, p.tn = 2, p.nw = 8, p.staged = true;
      p.threads = 512;
      p.grid = (long long)c.n * cdiv(Ho, TR) * cdiv(Wo, TC) * (c.Cout / BG_BN);
    } else {
      // (64-channel tiles keep three workgroups per CU with bf16 tensors: measured 1.4x faster than 128-channel tiles at one per CU)
      p.family = CONV_ROWS;
      p.tn = (c.Cout % 64 != 0 && c.Cout % 96 == 0) ? 3 : 2;
      p.nw = p.rows == 16 ? 8 : 4;
      p.tm = p.rows / p.nw;
      p.staged = st_ok && rows_staged_fits(p.tm, p.tn, p.ks, p.s, p.nw);
      p.threads = 64 * p.nw;
      p.grid = (long long)c.n * cdiv(Ho, p.rows) * cdiv(Wo, TC) * cdiv(c.Cout, p.tn * 32);
    }
    own_slots = rows_slots(Ho, Wo, p.rows);
  } else if (halo && (long long)c.n * halo_tiles(Ho, Wo) * 4 < (1LL << 31)) {
    p.family = CONV_HALO;
    p.tile = halo_tile((long long)c.n * halo_tiles(Ho, Wo), c.Cout);
    p.grid = p.tile.blocks;
    own_slots = (int)(halo_tiles(Ho, Wo) * 4);
  } else {
    p.family = CONV_IM2COL;
    p.tile = gemm_tile(M, c.Cout);
    p.grid = p.tile.blocks;
    own_slots = im2col_slots(Ho, Wo);
  }
  if (p.family == CONV_REFUSED || !grid_ok(p.grid) || (c.has_out_partial && own_slots != p.slots)) return no_conv();
  return p;
}

// ---- the composite encoder (encoder_forward.hip): BasicEncoder's 23 convolutions on H x W images, latent_dim C

// Convolution ci of mvt_encoder_weights on its H x W x Cin input; stats: its InstanceNorm statistics are taken.  with_down: conv1 of
// a strided block launched together with the block's downsample convolution ci + 2 (plan_down), whose own entry is then `folded`:
// the two halves of one launch's partials.
struct EncConv {
  int H, W, Cin, Cout, k, stride;
  bool stats, with_down, folded;
};
// conv indices: 0 stem; layer l (1..4): 1 + 5 (l - 1) + {0: .0.conv1, 1: .0.conv2, 2: .0.downsample, 3: .1.conv1, 4: .1.conv2};
// 21: conv2 (3x3, 416 -> 2C); 22: conv3 (1x1, 2C -> C)
inline void encoder_convs(int H, int W, int C, const ConvSwitches& sw, EncConv t[MVT_ENCODER_CONVS]) {
  const int couts[4] = {64, 96, 128, 128};
  int hh = H / 2, ww = W / 2, cin = 64;
  t[0] = EncConv{H, W, 4, 64, 7, 2, true, false, false};
  for (int l = 0; l < 4; ++l) {
    const int b0 = 1 + 5 * l, cout = couts[l], stride = l ? 2 : 1;
    const bool fold = l && cout % 32 == 0 && sw.fold_downsample;  // conv1 + downsample[0] read the same x: one launch
    t[b0] = EncConv{hh, ww, cin, cout, 3, stride, true, fold, false};
    t[b0 + 2] = EncConv{hh, ww, cin, cout, 1, stride, l != 0, false, fold};  // (layer 1 has no downsample branch: never launched)
    hh = conv_out(hh, 3, stride, 1), ww = conv_out(ww, 3, stride, 1);
    t[b0 + 1] = t[b0 + 3] = t[b0 + 4] = EncConv{hh, ww, cout, cout, 3, 1, true, false, false};
    cin = cout;
  }
  t[21] = EncConv{H / 4, W / 4, 416, 2 * C, 3, 1, true, false, false};
  t[22] = EncConv{H / 4, W / 4, 2 * C, C, 1, 1, false, false, false};
}
// Statistics slots of convolution t of the encoder (each half of a folded launch has as many).
inline int encoder_slots(const EncConv& t, const ConvSwitches& sw) { return conv_stat_slots(t.H, t.W, t.Cin, t.k, t.k, t.stride, t.k / 2, false, sw); }
// Floats of the encoder's partials buffer, and the channels a statistics table / a partials slot is sized for: the 8 x 32 tiles of
// the H/2 map times the widest launch -- conv2 with 2C channels, or the 2 x 128 of a folded launch.  Every launch fits that
// product, not each factor: with rows_nw8 = 2 the 64-channel layer 1 has twice the slots (four-row tiles), 2 x 64 <= 256 -- and
// every later map has at most half the rows, so its four-row tiles are no more than the H/2 map's eight-row ones.
inline long long encoder_stat_channels(int C) { return 2 * C > 256 ? 2 * C : 256; }
inline long long encoder_part_floats(long long n, int H, int W, int C) { return n * rows_slots(H / 2, W / 2, TR) * encoder_stat_channels(C) * 2; }
// The partial sums of every launch fit the partials buffer: n * slots * Cout * 2 floats, twice that where a strided block's conv1
// and downsample[0] share one launch.
inline bool encoder_partials_fit(const EncConv t[MVT_ENCODER_CONVS], long long n, long long part_floats, const ConvSwitches& sw) {
  for (int ci = 0; ci < MVT_ENCODER_CONVS; ++ci) {
    if (!t[ci].stats || t[ci].folded) continue;
    const int slots = encoder_slots(t[ci], sw);
    if (slots <= 0 || (t[ci].with_down ? 2 : 1) * n * slots * t[ci].Cout * 2 > part_floats) return false;
  }
  return true;
}

}  // namespace mvt_plan
