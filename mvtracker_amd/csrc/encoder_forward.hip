// Composite entry point of the CNN encoder: BasicEncoder.forward (spatracker/blocks.py:214-284) on n images as ONE C call
// (SURVEY.md section 8b).  No kernels of its own: it sequences the library's bf16 kernels -- row-tile convolutions with the
// InstanceNorm statistics taken in their epilogues and InstanceNorm + ReLU of the producer applied while a consumer loads its
// patch, the per-tile statistics reduction, the residual InstanceNorm pass, the one-launch concat -- on the caller's stream over a
// caller-provided workspace.  bf16 mode, bf16 activations (the configuration bench.py measures).  56 launches per call; beside
// the tracking windows the half-resolution layers run a few images at a time (group_size below): 12 launches per further group.
#include "common.h"
#include "conv_detail.h"
#include <stdlib.h>

namespace {

inline long long align256(long long b) { return (b + 255) & ~255LL; }

struct Plan {
  long long stem, z0, y, s[4], d, cat, c2, part, st, total;  // byte offsets
  long long st_ch;                                           // channels a statistics table / a partials slot is sized for
  long long part_floats;                                     // floats of the partials buffer
};

// workspace: bf16 activations + statistics scratch.  stem / z0 / y: one 64-channel map at H/2 each (the largest activation);
// s[l]: the output of stage l, alive until the concat; d: the 1x1 downsample branch of a stage's first block.
inline Plan plan(long long n, int H, int W, int C) {
  const long long h2 = H / 2, w2 = W / 2, hs = H / 4, ws = W / 4;
  Plan P{};
  long long o = 0;
  auto take = [&](long long bytes) { const long long at = o; o += align256(bytes); return at; };
  const long long big = n * h2 * w2 * 64 * 2;
  P.stem = take(big);
  P.z0 = take(big);
  P.y = take(big);
  const int couts[4] = {64, 96, 128, 128};
  long long hh = h2, ww = w2;
  for (int l = 0; l < 4; ++l) {
    if (l) {
      hh = (hh - 1) / 2 + 1;
      ww = (ww - 1) / 2 + 1;
    }
    P.s[l] = take(n * hh * ww * couts[l] * 2);
  }
  P.d = take(n * hs * ws * 96 * 2);
  P.cat = take(n * hs * ws * 416 * 2);
  P.c2 = take(n * hs * ws * 2 * C * 2);
  // statistics: per conv n * slots * Cout * 2 floats (conv_plan.h has the sizing rule).  encoder_run checks every launch against
  // part_floats before the first one (encoder_partials_fit).
  P.st_ch = mvt_plan::encoder_stat_channels(C);
  P.part_floats = mvt_plan::encoder_part_floats(n, H, W, C);
  P.part = take(P.part_floats * 4);
  P.st = take(8 * n * P.st_ch * 2 * 4);            // up to 8 live (mean, rstd) tables
  P.total = o;
  return P;
}

// Images per group of the half-resolution section (encoder_run): g = budget / live bytes per image, the live set being three
// H/2 maps (skip, y, z).  Measured ("cache-sized image groups"): a call that has the chip to itself gains
// nothing from groups -- its kernels take the same time with their maps resident, and every group adds launches -- so it makes
// one pass; the calls marked short_workgroups run beside the tracking windows, and there groups of about 72 MiB shorten the
// step.  A budget below one image's live set means one pass too.  MVT_ENC_GROUP=N forces groups of N images for every call
// (unset or 0: the rule); read on every call (A/B runs, tests).  -> g in [1, n]; g == n is the single pass.
constexpr long long GROUP_BUDGET_SHARED = 80LL << 20;
inline int group_size(int n, int h2, int w2, int shared, int* g_out) {
  long long g = shared ? GROUP_BUDGET_SHARED / (3LL * h2 * w2 * 64 * 2) : n;
  if (g < 1) g = n;
  if (const char* e = getenv("MVT_ENC_GROUP")) {
    const long v = strtol(e, nullptr, 10);
    if (v < 0) return MVT_ERR_ARG;
    if (v > 0) g = v;
  }
  *g_out = (int)(g > n ? n : g);
  return MVT_OK;
}

}  // namespace

extern "C" long long mvt_encoder_workspace_bytes(int n, int H, int W, int C) {
  if (n <= 0 || H < 16 || W < 16 || C <= 0) return -1;
  return plan(n, H, W, C).total;
}

#define ENC_TRY(call)              \
  do {                             \
    const int rc_ = (call);        \
    if (rc_ != MVT_OK) return rc_; \
  } while (0)

// x4 != null: normalised [n][H][W][4] input; else the planar clip rgb (V,T,3,H,W), images img0 .. img0 + n - 1 frame-major
static int encoder_run(const mvt_encoder_weights* w, const float* x4, const void* rgb, int rgb_u8, int rgb_V, int rgb_T, long long img0,
                       int n, int H, int W, void* out_rows, int ldo, int out_bf16, void* workspace, long long workspace_bytes, void* stream) {
  MVT_REQUIRE(w && (x4 || rgb) && out_rows && workspace && n > 0 && H >= 16 && W >= 16 && H % 4 == 0 && W % 4 == 0);
  const int C = w->latent_dim;
  MVT_REQUIRE(C > 0 && C % 32 == 0 && ldo >= C && (out_bf16 == 0 || out_bf16 == 1));
  const Plan P = plan(n, H, W, C);
  MVT_REQUIRE(workspace_bytes >= P.total && ((uintptr_t)workspace % 256) == 0);
  for (int i = 0; i < MVT_ENCODER_CONVS; ++i) MVT_REQUIRE(w->conv[i].w && w->conv[i].b);
  char* base = (char*)workspace;
  float* part = (float*)(base + P.part);
  float* stb = (float*)(base + P.st);
  const long long st_stride = (long long)n * P.st_ch * 2;
  int st_next = 0;
  auto new_st = [&]() { float* s = stb + (st_next % 8) * st_stride; ++st_next; return s; };
  const int BF = MVT_IO_IN_BF16 | MVT_IO_OUT_BF16;
  const int h2 = H / 2, w2 = W / 2;
  int g = n;
  ENC_TRY(group_size(n, h2, w2, w->short_workgroups, &g));

  // The network's convolutions, the one table that the launches below take their geometry from.  The partial sums of every launch
  // fit the partials buffer (plan()): checked here over the same table, for the whole sequence, so that a refusal leaves nothing queued.
  const mvt_plan::ConvSwitches sw = mvt_detail_conv_switches();
  mvt_plan::EncConv net[MVT_ENCODER_CONVS];
  mvt_plan::encoder_convs(H, W, C, sw, net);
  MVT_REQUIRE(mvt_plan::encoder_partials_fit(net, n, P.part_floats, sw));

  // The launches below act on images [ga, ga + gn) of the call.  Every buffer keeps the whole call's layout -- image i owns slice
  // i of each activation buffer, of the partial sums of a launch and of a (mean, rstd) table -- so a group is the same launch
  // with its pointers advanced by ga images and gn in place of n; (0, n) is the plain single pass.
  int ga = 0, gn = n;
  auto img = [&](const void* p, long long bytes_per_image) { return (char*)p + ga * bytes_per_image; };
  auto rows_of = [&](const float* table, int ch) { return table ? table + (long long)ga * ch * 2 : nullptr; };

  // convolution ci of the table (+ the (mean, rstd) of its output where st_out is given; *st_out is the whole call's table)
  auto conv = [&](int ci, const void* in, int io_in, void* out, int ld_out, const float* in_stats, float** st_out, int io_out) -> int {
    const mvt_conv_weights& cw = w->conv[ci];
    const mvt_plan::EncConv& t = net[ci];
    const int pad = t.k / 2, ho = mvt_plan::conv_out(t.H, t.k, t.stride, pad), wo = mvt_plan::conv_out(t.W, t.k, t.stride, pad);
    const long long in_img = (long long)t.H * t.W * t.Cin * (io_in & MVT_IO_IN_BF16 ? 2 : 4);
    const long long out_img = (long long)ho * wo * ld_out * (io_out & MVT_IO_OUT_BF16 ? 2 : 4);
    const int slots = st_out ? mvt_plan::encoder_slots(t, sw) : 0;
    float* pp = st_out ? part + (long long)ga * slots * t.Cout * 2 : nullptr;
    if (ci == 0 && !x4) {
      // the stem reads the clip's planar frames itself (normalisation on load): no [n][H][W][4] staging tensor, one launch less
      const mvt_plan::ConvPlan p = mvt_plan::plan_stem(gn, t.H, t.W, t.Cout, ld_out, io_out, ((uintptr_t)img(out, out_img) & 15) == 0);
      ENC_TRY(mvt_detail_stem7x7_rows_src(p, nullptr, rgb, rgb_u8, rgb_V, rgb_T, img0 + ga, cw.w, cw.b, img(out, out_img), gn, t.H, t.W, t.Cout,
                                          ld_out, pp, mvt_stream(stream)));
    } else {
      ENC_TRY(mvt_conv2d_bf16(img(in, in_img), cw.w, nullptr, cw.b, img(out, out_img), gn, t.H, t.W, t.Cin, t.Cout, t.k, t.k, t.stride, pad, ld_out,
                              MVT_ACT_NONE, io_in | io_out | (w->short_workgroups ? MVT_IO_SHORT_WG : 0), rows_of(in_stats, t.Cin), pp, stream));
    }
    if (st_out) {
      *st_out = new_st();
      ENC_TRY(mvt_instnorm_finish_slots(pp, slots, (float*)rows_of(*st_out, t.Cout), gn, (long long)ho * wo, t.Cout, stream));
    }
    return MVT_OK;
  };

  // ResidualBlock (blocks.py:84-128): conv1 -> IN -> ReLU -> conv2 -> IN -> ReLU, + (downsampled, normalised) input, ReLU
  auto res_block = [&](int c1, int c2, int cd, const void* xin, const float* x_stats, void* zout) -> int {
    const int hh = net[c1].H, ww = net[c1].W, cin = net[c1].Cin, cout = net[c1].Cout, ho = net[c2].H, wo = net[c2].W;
    const long long in_img = (long long)hh * ww * cin * 2, out_img = (long long)ho * wo * cout * 2;
    float *s1 = nullptr, *s2 = nullptr, *sd = nullptr;
    const bool fold = net[c1].with_down;  // conv1 + downsample[0] read the same x: one launch
    if (fold) {
      const int slots = mvt_plan::encoder_slots(net[c1], sw);
      float* part_3 = part + (long long)ga * slots * cout * 2;
      float* part_d = part_3 + (long long)n * slots * cout * 2;  // (both halves fit: partials_fit)
      ENC_TRY(mvt_conv3x3s2_down_bf16(img(xin, in_img), w->conv[c1].w, w->conv[c1].b, w->conv[cd].w, w->conv[cd].b, img(base + P.y, out_img),
                                      img(base + P.d, out_img), gn, hh, ww, cin, cout, cout, part_3, part_d, stream));
      s1 = new_st();
      ENC_TRY(mvt_instnorm_finish_slots(part_3, slots, (float*)rows_of(s1, cout), gn, (long long)ho * wo, cout, stream));
      sd = new_st();
      ENC_TRY(mvt_instnorm_finish_slots(part_d, slots, (float*)rows_of(sd, cout), gn, (long long)ho * wo, cout, stream));
    } else {
      ENC_TRY(conv(c1, xin, MVT_IO_IN_BF16, base + P.y, cout, x_stats, &s1, MVT_IO_OUT_BF16));
    }
    ENC_TRY(conv(c2, base + P.y, MVT_IO_IN_BF16, zout, cout, s1, &s2, MVT_IO_OUT_BF16));
    const void* skip = xin;
    long long skip_img = in_img;
    const float* skip_stats = x_stats;
    int flags = BF | (x_stats ? MVT_APPLY_SKIP_RELU : 0);
    if (cd >= 0) {
      if (!fold) ENC_TRY(conv(cd, xin, MVT_IO_IN_BF16, base + P.d, cout, nullptr, &sd, MVT_IO_OUT_BF16));
      skip = base + P.d;
      skip_img = out_img;
      skip_stats = sd;
      flags = BF;
    }
    return mvt_instnorm_apply(img(zout, out_img), rows_of(s2, cout), img(skip, skip_img), rows_of(skip_stats, cout), img(zout, out_img), gn,
                              (long long)ho * wo, cout, flags, stream);
  };

  // layer l (0..3) = two blocks, convolutions b0 = 1 + 5 l .. b0 + 4 of the table (mvt_plan::encoder_convs has the indices);
  // only a strided layer's first block has a downsample branch
  auto layer = [&](int l, const void* xin, const float* xst) -> int {
    const int b0 = 1 + 5 * l;
    ENC_TRY(res_block(b0, b0 + 1, l == 0 ? -1 : b0 + 2, xin, xst, base + P.z0));
    return res_block(b0 + 3, b0 + 4, -1, base + P.z0, nullptr, base + P.s[l]);
  };

  // The half-resolution section (stem and layer 1, the largest maps of the network) in groups of g images, up to where s[0] is
  // complete.  A group reads and writes its own images' slices only.  The ring position is rewound for every group: each fills
  // its images' rows of the same five tables an ungrouped call uses, so no group overwrites a row another group's consumer still
  // has to read, and the tables of the later stages land where they always did.
  for (ga = 0; ga < n; ga += g) {
    gn = n - ga < g ? n - ga : g;
    st_next = 0;
    // stem: 7x7 / 2, its InstanceNorm + ReLU is applied by its two consumers (conv1 of layer1.0 and that block's skip)
    float* st_stem = nullptr;
    ENC_TRY(conv(0, x4, 0, base + P.stem, 64, nullptr, &st_stem, MVT_IO_OUT_BF16));
    ENC_TRY(layer(0, base + P.stem, st_stem));
  }
  ga = 0, gn = n;
  const void* stage[4];
  int sh[4], swd[4], sc[4];
  for (int l = 0; l < 4; ++l) {
    if (l) ENC_TRY(layer(l, base + P.s[l - 1], nullptr));
    const mvt_plan::EncConv& last = net[1 + 5 * l + 4];  // (3x3 / stride 1: its output has its input's size)
    stage[l] = base + P.s[l]; sh[l] = last.H; swd[l] = last.W; sc[l] = last.Cout;
  }
  ENC_TRY(mvt_concat_resize_bilinear_ac(4, stage, sh, swd, sc, base + P.cat, n, net[21].H, net[21].W, net[21].Cin, BF, stream));
  float* st_c2 = nullptr;
  ENC_TRY(conv(21, base + P.cat, MVT_IO_IN_BF16, base + P.c2, 2 * C, nullptr, &st_c2, MVT_IO_OUT_BF16));
  return conv(22, base + P.c2, MVT_IO_IN_BF16, out_rows, ldo, st_c2, nullptr, out_bf16 ? MVT_IO_OUT_BF16 : 0);
}

extern "C" int mvt_encoder_forward(const mvt_encoder_weights* w, const float* x4, int n, int H, int W, void* out_rows, int ldo,
                                   int out_bf16, void* workspace, long long workspace_bytes, void* stream) {
  MVT_REQUIRE(x4);
  return encoder_run(w, x4, nullptr, 0, 0, 0, 0, n, H, W, out_rows, ldo, out_bf16, workspace, workspace_bytes, stream);
}

extern "C" int mvt_encoder_forward_rgb(const mvt_encoder_weights* w, const void* rgbs, int is_u8, int V, int T, long long img0, int n, int H,
                                       int W, void* out_rows, int ldo, int out_bf16, void* workspace, long long workspace_bytes,
                                       void* stream) {
  MVT_REQUIRE(rgbs && (is_u8 == 0 || is_u8 == 1) && V > 0 && T > 0 && img0 >= 0 && n > 0 && img0 + n <= (long long)V * T);
  return encoder_run(w, nullptr, rgbs, is_u8, V, T, img0, n, H, W, out_rows, ldo, out_bf16, workspace, workspace_bytes, stream);
}
