/*
 * mvtracker_hip.h -- C ABI of libmvtracker_hip.so, the MI355X (gfx950) implementation of the
 * multi-view point-tracking forward path.
 *
 * The reference (samiazirar/mvtracker) is pure Python on torch ATen; it has no FFI of its own
 * for this path.  The entry points below are the set of operations its hot path performs
 * (SURVEY.md section 8a/8b); each one names the reference code it replaces (paths relative to
 * the reference root).  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 / int32 / uint64 data unless marked "host";
 *     tensors are dense row-major with the layouts stated per function;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued
 *     asynchronously on it; no entry point allocates, frees or synchronises;
 *   - return value: 0 = ok, MVT_ERR_ARG = rejected arguments (nothing launched),
 *     1000 + hipError_t = launch failure; no exceptions, no global state, re-entrant per stream;
 *   - inputs are borrowed and never written; outputs are fully overwritten unless stated.
 *
 * Internal clip layout ("frame store"): features of pyramid level l are kept frame-major as
 *   fvec_l [T][V][h_l][w_l][C]  (fp32, channels last), xyz_l [T][V][h_l][w_l][4] (x,y,z,0),
 * so the fused point cloud of frame t (reference: init_pointcloud_from_rgbd,
 * mvtracker/models/core/model_utils.py:420-482, layout (B*S, V*H*W, C)) is the contiguous slice
 * [t] with P_l = V*h_l*w_l points.  Track state is track-major: coords [N][S][3],
 * ffeats [N][S][C], tokens [N][S][D].
 */
#ifndef MVTRACKER_HIP_H
#define MVTRACKER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVT_OK 0
#define MVT_ERR_ARG 1
#define MVT_ERR_HIP_BASE 1000

/* activation codes of mvt_gemm / mvt_conv2d epilogues */
#define MVT_ACT_NONE 0
#define MVT_ACT_RELU 1
#define MVT_ACT_GELU_TANH 2 /* nn.GELU(approximate="tanh"), cotracker2/blocks.py:289 */
#define MVT_ACT_GELU_ERF 3  /* nn.GELU(), mvtracker.py:179 */

/* library / device introspection (host) */
int mvt_abi_version(void);
const char* mvt_build_arch(void); /* "gfx950" */

/* ---------------------------------------------------------------------------------------------
 * Dense GEMM on the matrix cores (fp32 MFMA 32x32x2, exact fp32 FMA chains).
 *   C[M][ldc] = R[M][ldr] (optional) + act(A[M][lda] . Wt[N][ldw]^T + bias[N] (optional))
 * A rows must be readable for round_up(K,4) floats; Wt is the torch nn.Linear weight layout
 * [out][in] repacked so that ldw = round_up(K,32) with zero padding.  Replaces every
 * nn.Linear of the updater (cotracker2/blocks.py:55-67, 254-271, 364-382, 456, 489) and
 * ffeats_updater (mvtracker.py:179, 396).  R may alias C.
 * --------------------------------------------------------------------------------------------- */
int mvt_gemm(const float* A, int lda, const float* Wt, int ldw, const float* bias, const float* R, int ldr,
             float* C, int ldc, int M, int N, int K, int act, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 2-D convolution as implicit GEMM on the matrix cores, channels-last.
 *   in  [n][H][W][Cin]   (Cin % 32 == 0, or Cin == 4 for the 7x7 stem with kw*4+c packing)
 *   wt  [Cout][round_up(K,64)], row = [KH][KW][Cin] (K = KH*KW*Cin) repacked from torch's
 *       [Cout][Cin][KH][KW] and zero padded; for the stem row = [KH][32] (K = KH*32) with element
 *       kw*4+c (c<3, kw<7) and zeros elsewhere
 *   out [n][Ho][Wo][ldo] (ldo >= Cout; lets a conv write into a channel slice / the frame store)
 * Zero padding `pad`, stride `stride`.  Replaces nn.Conv2d in BasicEncoder / ResidualBlock
 * (mvtracker/models/core/spatracker/blocks.py:74-82, 116, 157-193).
 * --------------------------------------------------------------------------------------------- */
int mvt_conv2d(const float* in, const float* wt, const float* bias, float* out, int n, int H, int W, int Cin,
               int Cout, int KH, int KW, int stride, int pad, int ldo, int act, void* stream);

/* ---------------------------------------------------------------------------------------------
 * bf16 matrix-core variants of the two entry points above (v_mfma_f32_32x32x16_bf16, fp32 accumulate).
 * Activations stay fp32 in memory and are converted while staged into LDS; weights are pre-split with
 * mvt_split_bf16 into row-major bf16 [N][ldw], ldw = round_up(K,64), zero padded (conv: K = KH*KW*Cin in
 * [kh][kw][cin] order, stem K = KH*32).
 *   w_lo == NULL : plain bf16 operands (the arithmetic torch autocast gives the reference's convs/linears).
 *   w_lo != NULL : split precision "bf16x3": x = hi + lo, products hi*hi + hi*lo + lo*hi -> fp32-grade
 *                  results (dropped term 2^-16 relative) at 3/16 of the fp32-MFMA cost.
 * --------------------------------------------------------------------------------------------- */
/* hi[i] = bf16(src[i]) (round to nearest even), lo[i] = bf16(src[i] - hi[i]) (lo optional); n % 4 == 0. */
int mvt_split_bf16(const float* src, unsigned short* hi, unsigned short* lo, long long n, void* stream);
int mvt_gemm_bf16(const float* A, int lda, const unsigned short* w_hi, const unsigned short* w_lo, int ldw,
                  const float* bias, const float* R, int ldr, void* C, int ldc, int M, int N, int K, int act,
                  int io_flags /* MVT_IO_OUT_BF16: C is a bf16 tensor */, void* stream);
/* InstanceNorm fusion of the bf16 convolutions (saves the separate statistics pass and the normalise pass between
 * the two convs of a ResidualBlock, blocks.py:119-122):
 *   in_stats    [n][Cin][2] (mean, rstd) or NULL: the input is read as relu((x - mean) * rstd) (3x3 stride-1 pad-1 only);
 *   out_partial [n][slots][Cout][2] or NULL: per-channel (sum, sum of squares) of the outputs of every 32-pixel block,
 *               slots = mvt_conv2d_stat_slots(...) (0 = not available for this shape; the 3x3 kernels of the two
 *               precisions cut the image differently); one writer per slot, reduced in a
 *               fixed order by mvt_instnorm_finish_slots -> deterministic.
 *
 * io_flags: element type of the activation tensors.  In bf16 mode (wt_lo == NULL) the encoder keeps its intermediate
 * activations in bf16 -- its big layers are HBM-bound, and the MFMA operands are bf16 anyway:
 *   MVT_IO_IN_BF16  `in` is bf16 [n][H][W][Cin]   (Cin % 32 == 0; the stem always reads fp32)
 *   MVT_IO_OUT_BF16 `out` is bf16 [n][Ho][Wo][ldo] (rounded to nearest even from the fp32 accumulator; the statistics
 *                   in out_partial are taken before the rounding)
 *   MVT_IO_SHORT_WG keep every workgroup short-lived: the wide 3x3 layers (Cout % 256 == 0, no normalise-on-load) otherwise run as
 *                   one 512-thread, 144-KiB-LDS workgroup per CU and pixel tile (conv3x3_big_bf16, ~100 us each), which starves
 *                   kernels of OTHER streams of CU slots while it runs -- set it for launches that share the GPU with latency-bound
 *                   work (the encoder blocks that run beside the refinement windows).  Results are bit-identical either way. */
#define MVT_IO_IN_BF16 1
#define MVT_IO_OUT_BF16 2
#define MVT_IO_SHORT_WG 4
int mvt_conv2d_stat_slots(int H, int W, int Cin, int KH, int KW, int stride, int pad, int split /* wt_lo != NULL */);
/* The first two convolutions of a strided ResidualBlock that read the block input (spatracker/blocks.py:84-128: conv1 = 3x3 / stride 2
 * / pad 1 and downsample[0] = 1x1 / stride 2 of the SAME x) in ONE launch, bf16 mode, bf16 tensors: the downsample samples input
 * pixel (2y, 2x) = the centre tap of the 3x3 window around output (y, x), so it is computed from the patch conv1 has staged, with its
 * own weights wd [Cout][ldwd] (rows = cin), bias, output tensor and statistics -- one launch, one staging of the input and one
 * InstanceNorm-finish fewer per block.  out3 / outd [n][Ho][Wo][ldo] bf16; part3 / partd [n][slots][Cout][2] with
 * slots = mvt_conv2d_stat_slots(H, W, Cin, 3, 3, 2, 1, 0) for BOTH (both NULL: no statistics).  Cin % 32 == 0, Cout % 32 == 0.
 * Values identical to the two separate mvt_conv2d_bf16 launches (same accumulation order); the downsample's statistics are cut
 * into this kernel's 4-row tiles instead of the 1x1 kernel's 8-row tiles (another fixed summation order). */
int mvt_conv3x3s2_down_bf16(const void* in, const unsigned short* w3, const float* b3, const unsigned short* wd, const float* bd,
                            void* out3, void* outd, int n, int H, int W, int Cin, int Cout, int ldo, float* part3, float* partd,
                            void* stream);
int mvt_conv2d_bf16(const void* in, const unsigned short* wt_hi, const unsigned short* wt_lo, const float* bias,
                    void* out, int n, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int ldo,
                    int act, int io_flags, const float* in_stats, float* out_partial, void* stream);
int mvt_instnorm_finish_slots(const float* partial, int slots, float* mean_rstd, int n, long long HW, int C, void* stream);

/* mvt_gemm_bf16 with LayerNorm (biased variance, eps, optional affine ln_w / ln_b of length K) applied to every A
 * row on the fly: C = R + act(LayerNorm(A) . W^T + bias).  K % 4 == 0, K <= 1024.  Replaces the norm1 / norm_context
 * + to_q / to_kv pairs of AttnBlock / CrossAttnBlock (cotracker2/blocks.py:298, 335) without materialising the
 * normalised tokens. */
int mvt_ln_gemm_bf16(const float* A, int lda, const float* ln_w, const float* ln_b, float ln_eps,
                     const unsigned short* w_hi, const unsigned short* w_lo, int ldw, const float* bias, const float* R,
                     int ldr, float* C, int ldc, int M, int N, int K, int act, void* stream);

/* Fused transformer MLP on the bf16 matrix cores, in place:
 *   x[m][0:C] += W2 . gelu_tanh(W1 . LayerNorm(x[m][0:C]) + b1) + b2      (LayerNorm without affine, given eps)
 * (AttnBlock / CrossAttnBlock second half, cotracker2/blocks.py:299-300, 336-337).  w1 [H][ldw1] and
 * w2 [C][ldw2] are bf16 (mvt_split_bf16 hi parts); C == 256, H % 64 == 0.  The hidden activations stay in
 * registers (the first GEMM's accumulator is the second GEMM's operand). */
int mvt_mlp_fused_bf16(float* x, int ldx, const unsigned short* w1, int ldw1, const float* b1,
                       const unsigned short* w2, int ldw2, const float* b2, long long M, int C, int H, float eps,
                       void* stream);

/* Fused remainder of an AttnBlock / CrossAttnBlock on the bf16 matrix cores (cotracker2/blocks.py:297-300, 334-337),
 * in place on the token rows x [M][ldx] (C == 256):
 *     x += att . Wo^T + bo                                  (att [M][ldatt], Ko == 288 columns; att == NULL skips it)
 *     x += W2 . gelu_tanh(W1 . LayerNorm(x) + b1) + b2      (LayerNorm eps 1e-6, no affine; H % 128 == 0, H <= 1024)
 *     y_i = LayerNorm_i(x) . Wn_i^T + bn_i                  (n_next <= 2 follow-up projections: the q / kv / qkv
 *                                                            of the blocks that consume x next)
 * All weights bf16 in the fragment-major layout of mvt_pack_frag_bf16 (ldwo / ldw1 / ldw2 / next.ldw are ignored).
 * One launch replaces GEMM, LayerNorm, GEMM, GEMM, LayerNorm, GEMM [, LayerNorm, GEMM]. */
/* Row-major bf16 w [N][ld] -> fragment-major out [ceil(N/32)][K/16][64][8]: lane (r = l&31, h = l>>5) of fragment
 * (nb, ks) holds w[nb*32 + r][ks*16 + 8h .. +7] (zero rows past N) -- the MFMA 32x32x16 A operand, one coalesced 1-KiB
 * load per wave and k-step.  K % 16 == 0. */
int mvt_pack_frag_bf16(const unsigned short* w, int ld, int N, int K, unsigned short* out, void* stream);
typedef struct mvt_block_next {
  const unsigned short* w; /* fragment-major bf16 of [N][256] */
  const float* b;          /* [N] */
  const float* lnw;        /* LayerNorm affine [256] or NULL (both) */
  const float* lnb;
  float* y;                /* [M][ldy] fp32, or bf16 when y_bf16 */
  int ldw, N, ldy;
  float eps;
  long long row_lo, row_hi; /* the projection is evaluated for rows [row_lo, row_hi) only (y is indexed by the global row);
                               row_hi == 0: every row */
  int y_bf16;               /* 1: y is a bf16 tensor (the q / k / v operands of mvt_attention_bf16) */
} mvt_block_next;
#define MVT_BLOCK_MAX_NEXT 3
int mvt_block_fused_bf16(float* x, int ldx, const void* att /* fp32, or bf16 when att_bf16 */, int att_bf16, int ldatt, int Ko,
                         const unsigned short* wo, int ldwo,
                         const float* bo, const unsigned short* w1, int ldw1, const float* b1, const unsigned short* w2,
                         int ldw2, const float* b2, int H, const mvt_block_next* next, int n_next, long long M, int C,
                         float* workspace /* NULL, or (H/256 + 1) * M * C floats: lets small M (<= 2048 rows, M % 32 == 0) run
                                             as two launches cut over 4x more workgroups (deterministic partial sums); scratch
                                             in the kernels' own tile order, no state between calls */,
                         void* stream);

/* mvt_block_fused_bf16 with the attention that precedes the block computed INSIDE the kernel (no attention launch, no
 * attention tensor in HBM); heads = 6, dim_head = 48.  x rows are track-major, row = token * S + frame.
 *   MVT_ATTN_TIME  (AttnBlock over time, cotracker2/blocks.py:464-467): every token attends over its own S <= 32 frames;
 *                  q, k, v [M][ld] bf16 indexed by the block's rows.
 *   MVT_ATTN_FRAME (CrossAttnBlock / AttnBlock over space, blocks.py:477-483): the tokens of frame t attend over the
 *                  n_keys <= 64 context tokens of frame t; q [M][ldq] indexed by the block's rows, k / v [n_keys * S][ldkv]
 *                  with context token j of frame t at row j * S + t.  M < 4096: two-launch split path, workspace required,
 *                  (M / S) % 32 == 0. */
#define MVT_ATTN_TIME 1
#define MVT_ATTN_FRAME 2
/*   MVT_ATTN_PARTIALS: the attention was computed key-split by mvt_attention_bf16(MVT_ATTN_PARTIALS_ONLY) (64 queries per
 *                  frame, the virtual tokens: M = 64 * S); the kernel combines the n_splits partial states itself -- same
 *                  arithmetic and order as the merge launch it replaces -- instead of reading a merged attention tensor. */
#define MVT_ATTN_PARTIALS 3
/*   MVT_ATTN_FRAME_CTX: MVT_ATTN_FRAME (M >= 4096, n_keys == 64) whose context tokens are the rows of a split-path block called
 *                  with defer_pass2: that block's second launch is skipped and every workgroup here finishes the context rows of
 *                  its frame itself (x = x_mid + b2 + partial sums in pass 2's order, LayerNorm, k|v projection -- bit-identical
 *                  to the pass-2 launch), keeps k|v in LDS, and the context's x / one further projection are written once per
 *                  frame.  k, v are unused.  One launch and one write-then-read of k|v less per updater layer. */
#define MVT_ATTN_FRAME_CTX 4
typedef struct mvt_block_ctx {
  const float* ws;     /* the `workspace` of the deferred block: (chunks + 1) * 64 * S * C floats */
  int chunks;          /* its H / 256 */
  const float* b2;     /* its fc2 bias */
  float* x;            /* its x rows [64 * S][ldx] (row = token * S + frame): final values are written here */
  int ldx;
  mvt_block_next kv;   /* LayerNorm + k|v projection of the context rows: N = 576 (k | v, 6 heads x 48); y is not written */
  mvt_block_next next; /* optional (w == NULL: none): one more projection of the context rows, written to y [64 * S][ldy] */
} mvt_block_ctx;
typedef struct mvt_block_attn {
  int kind, S, n_keys, heads, dim_head, ldq, ldkv;
  const unsigned short* q;
  const unsigned short* k;
  const unsigned short* v;
  const float* partials; /* MVT_ATTN_PARTIALS: the workspace of mvt_attention_bf16 */
  int n_splits;
  int defer_pass2;       /* split-path forms (workspace given, M < 4096): launch pass 1 only; x and the follow-up projections are
                            finished by the consumer (MVT_ATTN_FRAME_CTX) */
  const mvt_block_ctx* ctx; /* MVT_ATTN_FRAME_CTX */
} mvt_block_attn;
int mvt_attn_block_fused_bf16(float* x, int ldx, const mvt_block_attn* attn, const unsigned short* wo, const float* bo,
                              const unsigned short* w1, const float* b1, const unsigned short* w2, const float* b2, int H,
                              const mvt_block_next* next, int n_next, long long M, int C, float* workspace, void* stream);

/* The updater's input in one launch (cotracker2/blocks.py:456-459 + the first projection): rows < Mp of x [M][ldx] =
 * tokens [Mp][ldtok] (token_dim <= 592 columns used) . Win^T + bin, rows >= Mp = virtual_tokens[(row - Mp) / S]; x is written,
 * then y_i = LayerNorm_i(x) . Wn_i^T + bn_i as in mvt_ln_proj_bf16.  win: fragment-major bf16 of [256][592] (zero padded). */
int mvt_input_proj_bf16(const float* tokens, int ldtok, int token_dim, long long Mp, const unsigned short* win, const float* bin,
                        const float* virtual_tokens, int S, float* x, int ldx, const mvt_block_next* next, int n_next, long long M, int C,
                        void* stream);

/* LayerNorm + projections only (x is read, never written): y_i = LayerNorm_i(x) . Wn_i^T + bn_i with the mvt_block_next
 * descriptors of mvt_block_fused_bf16 -- the first q|k|v projection of an updater call. */
int mvt_ln_proj_bf16(const float* x, int ldx, const mvt_block_next* next, int n_next, long long M, int C, void* stream);

/* rgbs [V][T][3][H][W] (values 0..255) -> x [T_sel][V][H][W][4] = (2*(rgb/255)-1, 0) for frames
 * t0..t0+nt-1 (mvtracker.py:565-567 normalisation + channels-last repack). */
int mvt_rgb_to_nhwc4(const float* rgbs, float* out, int V, int T, int H, int W, int t0, int nt, void* stream);
/* same from uint8 frames, the storage type of the sample files (demo.py:650, 922-929): the clip stays 1 byte per value in HBM
 * and over PCIe; (float)u8 is exact, so the result is bit-identical to converting first. */
int mvt_rgb_u8_to_nhwc4(const unsigned char* rgbs, float* out, int V, int T, int H, int W, int t0, int nt, void* stream);
/* same for an arbitrary run of images numbered frame-major (image t * V + v = view v of frame t, the order of the frame store):
 * images img0 .. img0+nimg-1 -> out [nimg][H][W][4].  The multi-GPU encoder split cuts the V*T images -- not frames -- evenly
 * across ranks.  is_u8: rgbs holds bytes. */
int mvt_rgb_images_to_nhwc4(const void* rgbs, int is_u8, float* out, int V, int T, int H, int W, long long img0, int nimg, void* stream);

/* nearest-neighbour resize of [n][C][Hi][Wi] planes to [n][C][Ho][Wo] with torch's index rule
 * (evaluation_predictor_3dpt.py:76-81, F.interpolate(mode="nearest")). */
int mvt_resize_nearest(const float* in, float* out, long long planes, int Hi, int Wi, int Ho, int Wo, void* stream);

/* InstanceNorm2d (eps 1e-5, biased variance, no affine; blocks.py:99-103,150-152) on
 * channels-last x [n][HW][C]:  stats -> mean_rstd [n][C][2]; `partial` is scratch of
 * n*MVT_IN_SLABS*C*2 doubles. */
#define MVT_IN_SLABS 64
int mvt_instnorm_stats(const void* x, int ldx, double* partial, float* mean_rstd, int n, long long HW, int C,
                       int io_flags /* MVT_IO_IN_BF16: x is bf16 */, void* stream);
/* y = relu((x-mean)*rstd)                                  (skip == NULL)
 * y = relu(skip' + relu((x-mean)*rstd)), skip' = skip or (skip-mean_s)*rstd_s when skip_stats
 * is given (ResidualBlock.forward, blocks.py:119-128); with MVT_APPLY_SKIP_RELU in io_flags skip' = relu((skip-mean_s)*rstd_s),
 * i.e. the skip tensor is itself a raw conv output whose norm + ReLU was never materialised (the stem).  y may alias x. */
#define MVT_APPLY_SKIP_RELU 4
int mvt_instnorm_apply(const void* x, const float* mean_rstd, const void* skip, const float* skip_stats, void* y,
                       int n, long long HW, int C, int io_flags /* 0, or IN|OUT: x, skip and y are all bf16 */, void* stream);

/* bilinear resize, align_corners=True, of channels-last src [n][Hs][Ws][C] into the channel
 * slice [c_off, c_off+C) of dst [n][Hd][Wd][ldd] (blocks.py:254-280, the 416-channel concat). */
int mvt_resize_bilinear_ac(const void* src, void* dst, int n, int Hs, int Ws, int C, int Hd, int Wd, int ldd,
                           int c_off, int io_flags /* 0, or IN|OUT: src and dst are bf16 */, void* stream);
/* The encoder's concat in ONE launch (spatracker/blocks.py:266-276): nsrc <= 4 stage outputs [n][Hs_k][Ws_k][C_k], each resized
 * like mvt_resize_bilinear_ac, written side by side (channel offsets 0, C_0, C_0 + C_1, ...) into dst [n][Hd][Wd][ldd]; a wave
 * writes whole contiguous pixel rows.  srcs / Hs / Ws / Cs: HOST arrays.  io_flags: 0 (fp32) or IN_BF16 | OUT_BF16. */
int mvt_concat_resize_bilinear_ac(int nsrc, const void* const* srcs, const int* Hs, const int* Ws, const int* Cs, void* dst, int n,
                                  int Hd, int Wd, int ldd, int io_flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frame store construction (reference: init_pointcloud_from_rgbd, model_utils.py:420-482, and
 * the depth resampling of mvtracker.py:558-562).
 * --------------------------------------------------------------------------------------------- */
/* intrs [n][3][3], extrs [n][3][4] (world->camera) -> kinv [n][9], einv [n][12] (rows 0..2 of the
 * inverse 4x4), closed form in fp64 rounded to fp32 (model_utils.py:453-457). */
int mvt_invert_cameras(const float* intrs, const float* extrs, float* kinv, float* einv, int n, void* stream);
/* depths [V][T][H][W] -> level-0 strided depth [T][V][H/s][W/s], nearest: source pixel (s*i, s*j)
 * (mvtracker.py:558-562). */
int mvt_depth_subsample(const float* depths, float* out, int V, int T, int H, int W, int s, void* stream);
/* View assignment of MonocularToMultiViewAdapter (monocular_baselines.py:630-680): for every query
 * (t, x, y, z) the view whose depth map, sampled bilinearly at the query's projection at frame t, exceeds the query's camera
 * depth the most (-1e4 for projections outside the image or behind the camera); the first maximum wins.
 * depths [V][T][H][W], intrs [V][T][3][3], extrs [V][T][3][4], query_points [N][4]; view_out [N] int32;
 * xyz_out NULL or [V][N][3] = (pixel x, pixel y, camera z) of every query in every view. */
int mvt_adapter_best_view(const float* depths, const float* intrs, const float* extrs, const float* query_points, int V, int T,
                          int H, int W, int N, int* view_out, float* xyz_out, void* stream);
/* 2x2 average pool of channels-last [n][h][w][C] -> [n][h/2][w/2][C] (model_utils.py:440).  io_flags: 0 (fp32 rows) or
 * MVT_IO_IN_BF16 | MVT_IO_OUT_BF16 (the bf16 frame store of bf16 mode -- under autocast the reference's fmaps are bf16 and
 * every pooled level is rounded to bf16 again, model_utils.py:436-440; the 2x2 mean itself is taken in fp32). */
int mvt_avgpool2(const void* in, void* out, long long n, int h, int w, int C, int io_flags, void* stream);
/* xyz_l [T][V][h_l][w_l][4] from level-0 strided depth [T][V][hs][ws] (nearest-subsampled by
 * 2^level, model_utils.py:443-444), pixel grid (i+0.5)*stride*2^level-0.5 (:462-466), kinv/einv
 * indexed [v*T+t] (:467-473). */
int mvt_unproject(const float* depth_s, const float* kinv, const float* einv, float* xyz, int V, int T, int hs,
                  int ws, int stride, int level, void* stream);

/* ---------------------------------------------------------------------------------------------
 * kNN + correlation (reference: knn / PointcloudCorrBlock.corr_sample, mvtracker.py:26-90,
 * 800-846; feature init 1-NN, mvtracker.py:627-643).
 * --------------------------------------------------------------------------------------------- */
/* THE FRAME RULE of every entry below that takes `int base, int R, int lo, int hi` (the entries that map a window slot to a frame of
 * the frame store).  The store tensors -- xyz [R][P][4], fvec [R][P][C], tile_box / group_box [R][..][8] -- hold R frame slots; frame
 * f lives in slot (f - base) mod R and frames [lo, hi] are resident (0 <= base <= lo <= hi, hi - lo < R).  Slot s of a window reads
 *   frame_of_slot = clamp(frame0 + s*frame_step, lo, hi)
 * (frame_step may be negative: the time-reversed pass of backward tracking runs its slots downwards and repeats frame lo; hi = the
 * last frame received is the repeat-last-frame padding at the clip's end).  frame0 itself must be resident; anything else is refused
 * (MVT_ERR_ARG).  A linear store of T frames, the whole clip on the device, is (base, R, lo, hi) = (0, T, 0, T-1): slot = frame.
 * A ring (streaming: device memory independent of the clip length) and a linear store that hold the same frames give the same bits.
 *
 * Exact brute-force kNN.  For every (query n, slot s): candidates are the P points of frame_of_slot; query = coords[(n*S+s)*3..].
 * d2 = fma(dz,dz,fma(dy,dy,dx*dx)), neighbours ascending by (d2, index).  The candidate range
 * is cut into nseg segments scanned by different waves; keys [N][S][nseg][K] receive
 * (d2 bits << 32 | index) per segment, ascending (KEY_MAX = ~0 pads a segment that holds fewer than K
 * survivors of a seeded scan).  1 <= K <= 16, P >= K.
 * Optional pruning seed (exactness preserved): seed_idx [N][S][seed_k] int32, seed_k >= K distinct point
 * indices per (query, slot) -- e.g. the previous iteration's neighbours (seed_cw == 0), or the neighbours found
 * on the next coarser pyramid level (seed_cw, seed_ch = coarse per-view grid; seed_fw, seed_fh = this level's
 * per-view grid; coarse (v,y,x) maps to (v,2y,2x)).  The scan then starts from the bound
 * max_j d2(query, seed_j) >= (K-th nearest distance) instead of +inf.
 * Optional tile culling (exactness preserved): the scan walks the cloud in tiles of 64 points and skips a tile
 * whose bounding box (tile_box, from mvt_tile_aabb with the same grid_w/grid_h) lies farther than the current bound
 * from all queries of the wave; the box distance is evaluated with the scan's own arithmetic, every rounding step
 * of which is monotonic, so it never exceeds the d2 of a point inside the box.  grid_w = grid_h = 0: tile t = points
 * [64t, 64t+64); grid_w, grid_h > 0 (multiples of 8, P = views*grid_h*grid_w in raster order): 8x8 pixel patches.
 * The segments are runs of tiles; only the merged result (mvt_knn_merge) is layout independent. */
int mvt_tile_aabb(const float* xyz, long long P, int T, int grid_w, int grid_h,
                  float* box /* [T][ceil(P/64)][8] = lo.xyz, finite-point count, hi.xyz, 0 */,
                  void* stream);
/* Coarse level of the culling hierarchy: group_box [T][ceil(ntiles/64)][8] = the union of the boxes of 64 consecutive tiles
 * (same record layout).  Used by the single-segment searches below (clouds of 65..4096 tiles), which test the group boxes first
 * and skip whole runs of tiles; exactness is unaffected (a group box contains its tiles' boxes). */
int mvt_tile_group_aabb(const float* box, long long P, int T, float* group_box, void* stream);
int mvt_knn_scan(const float* xyz, long long P, const float* coords, int N, int S, int frame0, int frame_step, int base, int R,
                 int lo, int hi, int K, int nseg, unsigned long long* keys, const int* seed_idx, int seed_k, int seed_cw,
                 int seed_ch, int seed_fw, int seed_fh, const float* tile_box, int grid_w, int grid_h, void* stream);
/* Merge the nseg per-segment key lists of mvt_knn_scan: idx_out [N][S][K] int32 = the K nearest neighbour
 * indices, ascending by (d2, index); indices are clamped to [0, P) (only NaN queries can be out of range). */
int mvt_knn_merge(const unsigned long long* keys, int N, int S, int K, int nseg, long long P, int* idx_out,
                  void* stream);
/* mvt_knn_scan (one segment) + mvt_knn_merge in ONE launch: every (track, slot) is searched by a single wave over the whole cloud
 * and its K neighbour indices go straight to idx_out [N][S][K] -- bit for bit the merged result of the two-launch form.  tile_box
 * required, group_box optional; seeds as in mvt_knn_scan (NULL: unseeded).  idx_out must not alias seed_idx when the seed comes
 * from another level (seed_cw > 0 reads other entries' indices only of the coarser tensor, never of idx_out). */
int mvt_knn_search(const float* xyz, long long P, const float* coords, int N, int S, int frame0, int frame_step, int base, int R,
                   int lo, int hi, int K, const int* seed_idx, int seed_k, int seed_cw, int seed_ch, int seed_fw, int seed_fh,
                   const float* tile_box, const float* group_box, int grid_w, int grid_h, int* idx_out, void* stream);
/* Scan / merge of several pyramid levels in ONE launch each (grid.y = level).  After the first refinement iteration every
 * level is seeded by its own previous neighbours (seed_idx [N][S][seed_k], same-level indices), so the scans are
 * independent; one launch removes three launch / tail latencies per iteration.  Semantics per level = mvt_knn_scan /
 * mvt_knn_merge.  seed_k == 0: unseeded (every seed_idx NULL). */
typedef struct mvt_knn_level {
  const float* xyz;         /* [R][P][4] */
  long long P;
  unsigned long long* keys; /* [N][S][nseg][K] */
  const int* seed_idx;      /* [N][S][seed_k] or NULL */
  const float* tile_box;    /* from mvt_tile_aabb(grid_w, grid_h) or NULL */
  int nseg, grid_w, grid_h;
  int* idx_out;             /* [N][S][K] (merge) */
  const float* group_box;   /* from mvt_tile_group_aabb or NULL: coarse culling level of mvt_knn_search_levels */
} mvt_knn_level;
int mvt_knn_scan_levels(int levels, const mvt_knn_level* lv, const float* coords, int N, int S, int frame0, int frame_step,
                        int base, int R, int lo, int hi, int K, int seed_k, void* stream);
int mvt_knn_merge_levels(int levels, const mvt_knn_level* lv, int N, int S, int K, void* stream);
/* Seeded scan + merge of all levels in ONE launch: every (track, slot) is searched by a single wave over the whole cloud
 * (tile boxes required; nseg and keys are ignored) and its K neighbour indices go straight to idx_out -- the result of
 * mvt_knn_scan_levels + mvt_knn_merge_levels, bit for bit (exact kNN, ties by index).  idx_out may alias seed_idx: a wave reads
 * the seeds of its own entries before it writes them.  seed_k >= K, or seed_k == 0 with every seed_idx NULL: unseeded searches
 * (the initial threshold is the farthest-corner bound of the nearest tile with >= K finite points). */
int mvt_knn_search_levels(int levels, const mvt_knn_level* lv, const float* coords, int N, int S, int frame0, int frame_step,
                          int base, int R, int lo, int hi, int K, int seed_k, void* stream);
/* Gather-dot correlation for `levels` pyramid levels in ONE launch (grid.y = level).  Host arrays of per-level
 * DEVICE pointers: xyz[l] [R][P_l][4], fvec[l] [R][P_l][C] (C in {32,64,128,256}, groups == 1), idx[l]
 * [N][S][K] int32 from mvt_knn_merge, P[l].  For k < K:
 *   out[(n*S+s)*ldo + o_off + l*4K + 4k + {0,1,2,3}] = { <target, f_k>/sqrt(C), xyz_k - coord }
 * (mvtracker.py:827-842 with corr_add_neighbor_offset=True; the level-major concat of :374).  targets [N][S][C] fp32.
 * fvec_bf16: the feature rows are bf16 (256-B rows at C = 128; the dot accumulates in fp32). */
int mvt_corr_gather_dot(int levels, const float* const* xyz, const void* const* fvec, int fvec_bf16, const long long* P,
                        const int* const* idx, int C, const float* targets, const float* coords, int N, int S, int frame0,
                        int frame_step, int base, int R, int lo, int hi, int K, float* out, int ldo, int o_off, void* stream);
/* The same operator with the reference's non-default correlation options (mvtracker.py:130-149, 832-846): `groups` grouped dots per
 * neighbour (each over C / groups channels, / sqrt(C / groups); a power of two dividing the lanes of a feature row), the neighbour
 * offset (add_offset) and / or the neighbour's coordinates (add_xyz) appended: OW = groups + 3 add_offset + 3 add_xyz values per
 * neighbour at out[(n*S+s)*ldo + o_off + (l*K + k)*OW ...]. */
int mvt_corr_gather_dot_opts(int levels, const float* const* xyz, const void* const* fvec, int fvec_bf16, const long long* P,
                             const int* const* idx, int C, const float* targets, const float* coords, int N, int S, int frame0,
                             int frame_step, int base, int R, int lo, int hi, int K, int groups, int add_offset, int add_xyz,
                             float* out, int ldo, int o_off, void* stream);
/* 1-NN feature init: feat_out[n][C] (fp32) = fvec[slot of frame][idx] with idx from keys [n][1][nseg][1]
 * (mvtracker.py:640-643); idx_out optional.  fvec_bf16: bf16 feature rows.  `frame` must be resident (the frame rule). */
int mvt_knn1_gather(const void* fvec, int fvec_bf16, long long P, int C, const unsigned long long* keys, int n, int nseg,
                    int frame, int base, int R, int lo, int hi, float* feat_out, int* idx_out, void* stream);

/* Secondary operator: bilinear-window correlation (CorrBlock.corr_sample,
 * spatracker/blocks.py:492-533 + bilinear_sampler :604-619).  fmap_l channels-last
 * [BS][h][w][C] for ONE level; targets [BS][N][C]; coords [BS][N][2] level-0 pixels;
 * out[(bs*N+n)*ldo + o_off + i*(2r+1)+j] for the (2r+1)^2 window around coords/2^level. */
int mvt_window_corr(const float* fmap, const float* targets, const float* coords, float* out, int BS, int N,
                    int C, int h, int w, int level, int radius, int ldo, int o_off, void* stream);
/* ... all pyramid levels of CorrBlock.corr_sample in ONE launch (the form the primary operator mvt_corr_gather_dot has), fp32 or
 * bf16 maps (fmap_bf16: under autocast the reference's CorrBlock holds bf16 fmaps and bf16 avg-pooled levels, blocks.py:423-449;
 * fp32 accumulation here).  fmaps[l] channels-last [BS][hs[l]][ws[l]][C]; out[(bs*N+n)*ldo + o_off + l*(2r+1)^2 + i*(2r+1)+j]. */
int mvt_window_corr_levels(int levels, const void* const* fmaps, int fmap_bf16, const int* hs, const int* ws, const float* targets,
                           const float* coords, float* out, int BS, int N, int C, int radius, int ldo, int o_off, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Token assembly and track update (mvtracker.py:324-349, 374-408; embeddings.py:35-50,
 * 88-106, 134-161).
 * --------------------------------------------------------------------------------------------- */
/* pos [N][D] = first D entries of the 3x(dim3/3) sin|cos embedding (dim_padded wide) of coords0 (row n at
 * coords[(n*S)*3], fp64 math, omega_j = 10000^(-j/(dim3/6))) (embeddings.py:35-50).  omega: NULL (computed in the kernel) or a
 * DEVICE table of dim_padded/6 doubles -- the reference's own numpy values (embeddings.py:95-97). */
int mvt_pos_embed(const float* coords, int N, int S, int D, int dim_padded, const double* omega, float* pos, void* stream);
/* x[(n*S+s)*ldx + ..] = cat[flow_embed(coords[n,s]-coords[n,0]) (3*E+3) | fcorr (Fc) |
 * ffeats (C) | mask | vis] + pos[n] + time[s]  (mvtracker.py:379-386). */
int mvt_token_assemble(const float* coords, const float* fcorr, int Fc, const float* ffeats, int C,
                       const float* mask_vis, const float* pos, const float* time_embed, int N, int S, int E,
                       float* x, int ldx, void* stream);
/* delta [N*S][ldd] -> coords += delta[:, 0:3]; dn [N*S][C] = GroupNorm(1,C)(delta[:, 3:3+C])
 * (eps 1e-5, affine gw/gb) (mvtracker.py:392-395, 398).  nan_flag (optional int*) is set to 1
 * if any updated coordinate is NaN (deferred form of the guard at :401-404). */
int mvt_delta_split(const float* delta, int ldd, const float* gw, const float* gb, float* coords, float* dn,
                    long long rows, int C, int* nan_flag, void* stream);
/* out[r] = <x[r][0:C], w> + b  (vis_predictor, mvtracker.py:180, 408). */
int mvt_rowdot(const float* x, int ldx, const float* w, const float* b, float* out, long long rows, int C,
               void* stream);

/* ---------------------------------------------------------------------------------------------
 * Updater transformer pieces (cotracker2/blocks.py:246-337, 455-494).
 * --------------------------------------------------------------------------------------------- */
/* y[r] = LayerNorm(x[r][0:C]) * w + b (w,b optional), biased variance, given eps (:284-287, 314-315). */
int mvt_layernorm(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, long long rows,
                  int C, float eps, void* stream);
/* softmax(q k^T / sqrt(dh)) v for `groups` independent groups, `heads` heads of width dh <= 64.
 * Row r of query item i in group g is  q + (g*q_gs + i*q_is) * ldq  (+ head*dh); likewise k, v, o.
 * One wave per (group, head, query); keys on lanes, online softmax in fp32
 * (FlashAttention.forward, blocks.py:258-271, attn_mask None). */
int mvt_attention(const float* q, int ldq, long long q_gs, long long q_is, const float* k, const float* v,
                  int ldkv, long long k_gs, long long k_is, float* o, int ldo, int groups, int nq, int nk,
                  int heads, int dh, void* stream);
/* Same contract on the bf16 matrix cores (flash-style, scores never leave registers; dh == 48): q/k/v are rounded to
 * bf16, accumulation and softmax in fp32. */
int mvt_attention_bf16(const void* q, int ldq, long long q_gs, long long q_is, const void* k, const void* v,
                       int ldkv, long long k_gs, long long k_is, void* o, int ldo, int groups, int nq, int nk,
                       int heads, int dh, int io_flags /* MVT_IO_IN_BF16: q, k, v are bf16 tensors; MVT_IO_OUT_BF16: o is */,
                       float* workspace /* NULL, or 4 * groups*heads*ceil(nq/64) * 4352 floats: lets a long-key attention
                                           with few (group, head) chunks cut its keys over 4 workgroups per chunk */,
                       void* stream);
/* io_flags bit: stop after the key-split partials (no merge launch, `o` is not written); the consumer combines them
 * (mvt_attn_block_fused_bf16, MVT_ATTN_PARTIALS).  Only valid when the key-split path is taken (nk >= 512, < 256 chunks). */
#define MVT_ATTN_PARTIALS_ONLY 8
#define MVT_ATTN_NSPLIT 4 /* key splits of that path */
/* x[(n*S+s)*ld + 0:C] = v[n][0:C] for all s  (virtual-token broadcast, blocks.py:458-459). */
int mvt_broadcast_rows(const float* v, float* x, int ld, int n, int S, int C, void* stream);
/* Segmented forms of mvt_attention / mvt_attention_bf16: nseg independent attentions through one launch per kernel form.
 * Segment s reads its queries from rows q_row0[s] + (group stride, item stride) of q (writes o at the same rows) and its keys
 * from rows k_row0[s] + ... of k / v, with nq[s] queries and nk[s] keys per group; q_row0 / nq / k_row0 / nk are HOST arrays
 * of nseg entries.  Every segment's output is bit-identical to the ungrouped call on that segment alone: each one takes the
 * kernel form, key partition and key-split decision of that call.  The bf16 workspace (NULL: no key split) holds
 * 4 * groups*heads*ceil(nq[s]/64) * 4352 floats for every segment that takes the key-split path; ws_floats is its size. */
int mvt_attention_segmented(const float* q, int ldq, long long q_gs, long long q_is, const float* k, const float* v, int ldkv,
                            long long k_gs, long long k_is, float* o, int ldo, int groups, int heads, int dh, int nseg,
                            const long long* q_row0, const int* nq, const long long* k_row0, const int* nk, void* stream);
int mvt_attention_bf16_segmented(const void* q, int ldq, long long q_gs, long long q_is, const void* k, const void* v, int ldkv,
                                 long long k_gs, long long k_is, void* o, int ldo, int groups, int heads, int dh, int io_flags, int nseg,
                                 const long long* q_row0, const int* nq, const long long* k_row0, const int* nk, float* workspace,
                                 long long ws_floats, void* stream);
/* x[(r*S+s)*ld + 0:C] = v[r % n][0:C] for r < reps*n, all s: the virtual tokens of `reps` independent query sets. */
int mvt_broadcast_rows_repeat(const float* v, float* x, int ld, int n, int S, int C, int reps, void* stream);

/* Track state of one sliding window (mvtracker.py:505-511, 645-655, 695).  Slot s of the window is clip frame
 * frame0 + frame_step * s, clamped to the clip [0, T): frame_step = +1 is the forward pass (n tracks sorted by query frame),
 * frame_step = -1 the time-reversed pass of backward tracking (tracks sorted by DESCENDING query frame; qt holds the query frames
 * themselves in both).  qxyz [n][3], qt [n] int32 query frames, feat_init [n][C].  Writes coords [n][S][3], mask_vis [n][S][2] =
 * (track mask, initial visibility), ffeats [n][S][C].  A carried track continues from the second half of its row of the previous
 * window (prev_coords [.][S][3], prev_vis [.][S] logits; window stride S/2), a new one starts at its query point with logit 10.
 * Without a map (carry_src NULL) the first p0 tracks are carried, each from its own row.  With one (several independent query sets
 * in one window, each with its own carried prefix) p0 must be 0, and carry_src[tr] >= 0 is the row of prev_* track tr continues
 * from, -1 a track that enters here; prev_* may then be NULL only if no entry is >= 0.  The track mask of slot s, at frame f, is
 * frame_step * (f - qt) >= 0 (the query frame reached), except in the half window the previous window covered
 * (frame_step * (f - frame0) < S/2) for a carried track. */
int mvt_window_prepare(const float* qxyz, const int* qt, const float* feat_init, const float* prev_coords, const float* prev_vis,
                       const int* carry_src, int n, int p0, int S, int C, int frame0, int frame_step, int T, float* coords,
                       float* mask_vis, float* ffeats, void* stream);
/* Results of the window into the clip outputs in the caller's query order (mvtracker.py:692-693, 710-711).  traj [f1-f0][N][3],
 * vis_* [f1-f0][N] hold frames [f0, f1) of a clip of T frames (T: as far as it is known, f1 <= T); the whole clip is f0 = 0,
 * f1 = T, a chunk of it is what streaming emits.  Slot s whose frame f = frame0 + frame_step * s lies in the clip is written to row
 * f - f0 iff f0 <= f < f1 and (before == NULL or f < before[i]):  traj[f - f0][order[i]] = coords[i][s], vis_logit = vis[i][s],
 * vis_prob = sigmoid(vis[i][s]).  order [n] int64, before [n] int32.  The reversed pass gives its query frames as `before`: frames
 * from the query frame on are the forward pass's and are never touched.  No slot inside [f0, f1): nothing is written.  Rows no
 * window writes keep what the caller put there (zeros, in the tracker's results). */
int mvt_window_store(const float* coords, const float* vis, const long long* order, const int* before, int n, int S, int frame0,
                     int frame_step, int T, int f0, int f1, int N, float* traj, float* vis_logit, float* vis_prob, void* stream);

/* Per-track evaluation metrics (mvtracker/evaluation/metrics.py:10-58, 61-171, 327-330; query_mode "first"): one row of
 * 11 + 2K floats per track -- movement, visible frames, occlusion accuracy (all / gt-occluded / gt-visible), average Jaccard,
 * average pts-within, MTE (lower median), ATE, FDE, survival, then pts-within[K] and Jaccard[K] (fractions, NaN where the
 * reference divides by zero).  gt_tracks / pred_tracks [T][N][D] (D = 2 or 3), gt_visible / pred_occluded [T][N] bytes,
 * query_frame [N] int32, thresholds: HOST array of K <= 8 distances.  T <= 1024. */
int mvt_track_metrics(const float* gt_tracks, const float* pred_tracks, const unsigned char* gt_visible,
                      const unsigned char* pred_occluded, const int* query_frame, int T, int N, int D, const float* thresholds, int K,
                      float survival_threshold, float* out, int ldo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Composite entry points: one C call per stage of the hot path instead of one per kernel, so that a
 * non-Python caller can run the updater as ONE operation and the launch order lives in the library, not in host glue.
 *
 * mvt_updateformer_forward = EfficientUpdateFormer.forward (cotracker2/blocks.py:455-494) on the bf16 matrix cores for the
 * shipped geometry (hidden 256, 6 heads x 48, MLP 1024, 64 virtual tracks; configs/model/mvtracker.yaml): input transform,
 * virtual-token broadcast, depth x (time block, virtual<-point, virtual self, point<-virtual), flow head.
 *   x     [n*S][ldx] fp32 tokens (K = token_dim columns used), track-major (row = track * S + frame)
 *   delta [n*S][ldd] fp32, out_dim columns written
 * Weights: device pointers prepared once by the caller -- `frag` = fragment-major bf16 of mvt_pack_frag_bf16, `rows` = row-major
 * bf16 [N][ldw] (ldw = round_up(K, 64), zero padded) as mvt_gemm_bf16 takes them; biases / LayerNorm affines fp32.
 * flow0 / flow2 must be packed with N rounded up to a multiple of 4 (zero rows, zero bias) so that the pad columns of the hidden
 * activations -- read as K padding by the next layer -- are written as exact zeros by the GEMM itself.
 * `workspace`: mvt_updateformer_workspace_bytes(n, S) bytes, 256-B aligned, no state carried between calls.
 * --------------------------------------------------------------------------------------------- */
typedef struct mvt_lin_frag {
  const unsigned short* w; /* fragment-major bf16 of [N][K] */
  const float* b;          /* [N] */
  int N, K;
} mvt_lin_frag;
typedef struct mvt_lin_rows {
  const unsigned short* w; /* row-major bf16 [N][ldw] */
  const float* b;
  int N, K, ldw;
} mvt_lin_rows;
typedef struct mvt_updater_block {
  mvt_lin_frag qkv;   /* self-attention blocks (time, virtual self): fused [q|k|v] projection, N = 3 * heads * dim_head */
  mvt_lin_frag q, kv; /* cross-attention blocks: to_q on the block's own tokens, to_kv on the context tokens */
  const float* ctx_ln_w; /* cross blocks: norm_context affine (eps 1e-5, cotracker2/blocks.py:314-315) */
  const float* ctx_ln_b;
  mvt_lin_frag out, fc1, fc2;
} mvt_updater_block;
#define MVT_UPDATER_MAX_DEPTH 8
typedef struct mvt_updater_weights {
  int depth, hidden, heads, dim_head, n_virtual, S, token_dim, out_dim;
  int fuse_attention; /* bit 0: time attention, bit 1: point<-virtual, bit 2: virtual self attention run inside the block kernels
                         (mvt_attn_block_fused_bf16) instead of as separate launches; bit 3: unused (ignored); bit 4: the virtual<-point block
                         combines the key-split partials (MVT_ATTN_PARTIALS, no merge launch); bit 5 (with bits 1 and 2, >= 4096 point rows): the
                         virtual-self block's second launch runs inside the point<-virtual block (MVT_ATTN_FRAME_CTX).  Bits 4 and 5 only move
                         WHERE partial sums are combined: bit-identical with and without.  Bits 0-2 change the attention arithmetic (one
                         softmax pass over all key blocks, the time attention of a tile as one block-diagonal unit per head): results agree
                         with the separate launches to bf16 rounding (max ~7e-3 of the output scale), not bit for bit */
  const float* virtual_tokens; /* [n_virtual][hidden] */
  mvt_lin_rows input_transform, flow0, flow2, flow4;
  mvt_updater_block time_blk[MVT_UPDATER_MAX_DEPTH], v2p[MVT_UPDATER_MAX_DEPTH], vself[MVT_UPDATER_MAX_DEPTH], p2v[MVT_UPDATER_MAX_DEPTH];
  /* optional, for the fused track update of mvt_updateformer_forward (NULL w = not available): the flow head once more as
   * fragment-major bf16 (K of flow2 / flow4 padded to 144) and the feature updater of mvtracker.py:178-179, 393-399 */
  mvt_lin_frag flow0_frag, flow2_frag, flow4_frag, ffeats_updater;
  mvt_lin_frag input_frag; /* optional: input_transform once more as fragment-major bf16 with K padded to 592 (mvt_input_proj_bf16) */
  const float* ffeats_norm_w; /* GroupNorm(1, 128) affine */
  const float* ffeats_norm_b;
} mvt_updater_weights;
long long mvt_updateformer_workspace_bytes(int n, int S); /* host; -1 on bad arguments */
/* delta may be NULL when the track update is fused: with coords != NULL ([n*S][3]) and ffeats ([n*S][128]) the call also applies
 * coords += delta[:, 0:3], ffeats += gelu(Linear(GroupNorm(delta[:, 3:]))) (mvtracker.py:392-399) in the flow-head kernel
 * (mvt_update_head_bf16) and ORs 1 into *nan_flag (optional) when a coordinate became NaN (:401-404). */
int mvt_updateformer_forward(const mvt_updater_weights* w /* host struct of device pointers */, const float* x, int ldx, int n,
                             float* delta, int ldd, float* coords, float* ffeats, int* nan_flag, void* workspace,
                             long long workspace_bytes, void* stream);
/* mvt_encoder_forward = BasicEncoder.forward (spatracker/blocks.py:214-284) on n images as one call: x4 [n][H][W][4] normalised
 * RGB (mvt_rgb_*_to_nhwc4) -> out_rows [n][H/4][W/4][ldo] (latent_dim columns; bf16 when out_bf16 -- the frame store of bf16 mode).
 * bf16 mode with bf16 activations.  conv[i]: row-major bf16 weights [Cout][ldw] with rows (kh, kw, cin) as mvt_conv2d_bf16 takes them
 * (the 7x7 stem as [64][7][8][4]) + fp32 bias, in the order: 0 conv1; for layer l = 1..4: 1 + 5(l-1) + {0 .0.conv1, 1 .0.conv2,
 * 2 .0.downsample.0 (unused for l = 1), 3 .1.conv1, 4 .1.conv2}; 21 conv2; 22 conv3.  workspace: mvt_encoder_workspace_bytes bytes,
 * 256-B aligned, no state between calls. */
#define MVT_ENCODER_CONVS 23
typedef struct mvt_conv_weights {
  const unsigned short* w;
  const float* b;
} mvt_conv_weights;
typedef struct mvt_encoder_weights {
  int latent_dim;
  int short_workgroups; /* != 0: every convolution with MVT_IO_SHORT_WG (the call shares the GPU with other streams) */
  mvt_conv_weights conv[MVT_ENCODER_CONVS];
} mvt_encoder_weights;
long long mvt_encoder_workspace_bytes(int n, int H, int W, int latent_dim); /* host; -1 on bad arguments */
int mvt_encoder_forward(const mvt_encoder_weights* w, const float* x4, int n, int H, int W, void* out_rows, int ldo, int out_bf16,
                        void* workspace, long long workspace_bytes, void* stream);
/* ... the same with the stem reading the clip's planar frames itself: rgbs (V,T,3,H,W) in [0, 255], fp32 or (is_u8) uint8; the n images
 * img0 .. img0 + n - 1 in frame-major numbering (image t * V + v = view v of frame t); normalised on load exactly as mvt_rgb_*_to_nhwc4
 * does (2 (x / 255) - 1, mvtracker.py:455) -- bit-identical results without the [n][H][W][4] staging tensor and its launch. */
int mvt_encoder_forward_rgb(const mvt_encoder_weights* w, const void* rgbs, int is_u8, int V, int T, long long img0, int n, int H, int W,
                            void* out_rows, int ldo, int out_bf16, void* workspace, long long workspace_bytes, void* stream);

/* mvt_updateformer_forward with the 581-wide token rows ASSEMBLED inside its first kernel (mvt_token_input_proj_bf16: the
 * arithmetic of mvt_token_assemble) instead of read from a token matrix: one refinement iteration after the correlation is then
 * this single call.  coords [n][S][3], fcorr [n][S][Fc], ffeats [n][S][Cf], mask_vis [n][S][2], pos [n][D], time_embed [S][D],
 * D = 3E + 3 + Fc + Cf + 2 = token_dim.  Needs w->input_frag. */
typedef struct mvt_token_inputs {
  const float* coords;
  const float* fcorr;
  const float* ffeats;
  const float* mask_vis;
  const float* pos;
  const float* time_embed;
  int Fc, Cf, E;
} mvt_token_inputs;
int mvt_updateformer_forward_tokens(const mvt_updater_weights* w, const mvt_token_inputs* tokens, int n, float* delta, int ldd,
                                    float* coords, float* ffeats, int* nan_flag, void* workspace, long long workspace_bytes, void* stream);
/* The same two entries for G independent query sets (MVTracker.forward_grouped): the point tracks of set g are group_n[g] (HOST
 * array, sum = n) consecutive tracks, each set has its own n_virtual virtual tracks (rows n*S + (g*n_virtual + j)*S + t) and
 * attends only within itself (segmented space attentions).  fuse_attention bits 2, 4, 16 and 32 (in-kernel attentions without a
 * set dimension) fall back to their separate launches when G > 1; with G = 1 the launch sequence is the ungrouped one.
 * Workspace: mvt_updateformer_grouped_workspace_bytes(n, S, G) bytes. */
long long mvt_updateformer_grouped_workspace_bytes(int n, int S, int G);
int mvt_updateformer_forward_grouped(const mvt_updater_weights* w, const float* x, int ldx, int n, int G, const int* group_n, float* delta,
                                     int ldd, float* coords, float* ffeats, int* nan_flag, void* workspace, long long workspace_bytes,
                                     void* stream);
int mvt_updateformer_forward_tokens_grouped(const mvt_updater_weights* w, const mvt_token_inputs* tokens, int n, int G, const int* group_n,
                                            float* delta, int ldd, float* coords, float* ffeats, int* nan_flag, void* workspace,
                                            long long workspace_bytes, void* stream);
int mvt_token_input_proj_bf16(const float* coords, const float* fcorr, int Fc, const float* ffeats, int Cf, const float* mask_vis,
                              const float* pos, const float* time_embed, int n_tracks, int S, int E, const unsigned short* win,
                              const float* bin, const float* virtual_tokens, float* x, int ldx, const mvt_block_next* next, int n_next,
                              long long M, int C, void* stream);

/* The head alone: flow head (256 -> 131 -> 131 -> 131, ReLU) on tok [rows][ldt] + track / feature update, see above.  w0 / w2 /
 * w4 / wu fragment-major bf16 of [131][256], [131][144], [131][144], [128][128] (mvt_pack_frag_bf16, zero padded). */
int mvt_update_head_bf16(const float* tok, int ldt, const unsigned short* w0, const float* b0, const unsigned short* w2,
                         const float* b2, const unsigned short* w4, const float* b4, const float* gn_w, const float* gn_b,
                         const unsigned short* wu, const float* bu, float* coords, float* ffeats, float* delta /* NULL or [rows][ldd] */,
                         int ldd, long long rows, int hidden, int out_dim, int* nan_flag, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Query sampling from depth for unlabelled clips (reference: evaluation/evaluator_3dpt.py:286-388,
 * kmeans_sample :42-59).  Every sum taken across lanes or workgroups is an integer (fixed point):
 * the results do not depend on the order of addition.  No kernel waits on another workgroup.
 * --------------------------------------------------------------------------------------------- */
#define MVT_POOL_RADIUS_INCLUSIVE 1 /* x^2 + y^2 <= radius^2 (demo.py:980) instead of the evaluator's < */
/* Candidate pool of frame t: every pixel of depths (V,T,1,H,W) at frame t (read in place), unprojected with mvt_unproject's
 * arithmetic at stride 1 (kinv / einv [V*T] from mvt_invert_cameras), kept when it is valid -- conf > conf_threshold with a
 * confidence map (same layout), depth > 0 without one (conf = NULL) -- and inside the cylinder (x-x0)^2 + (y-y0)^2 < radius_sq
 * (squares and sum rounded separately, as torch does), z_min <= z <= z_max; radius_sq / z_min / z_max may be infinite.
 * pool [V*H*W][3] receives the kept points in raster order (view, row, column = init_pointcloud_from_rgbd's order), *count their
 * number M; rows from M on are not written.  block_counts: workspace of ceil(V*H*W / 256) int32.  V*H*W < 2^31.
 * Three launches: per-workgroup counts, a one-workgroup scan, a scatter at wave-ballot prefix positions. */
int mvt_query_pool(const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T, int t, int H, int W,
                   float conf_threshold, float x0, float y0, float radius_sq, float z_min, float z_max, int flags, float* pool,
                   int* count, int* block_counts, void* stream);

/* k-means over pts [M][3], 1 <= k <= MVT_KMEANS_MAX_K, k <= M < 2^31 (anything else: MVT_ERR_ARG before any launch).
 * state: MVT_KM_WORDS 64-bit words on the device, doubles and integers as named below. */
#define MVT_KMEANS_MAX_K 4096
#define MVT_KMEANS_MAX_CAND 10       /* 2 + floor(ln 4096) candidates per seeding step */
#define MVT_KMEANS_SEED_BLOCKS 4096  /* workgroups of a seeding pass (their prefix lives in LDS) */
#define MVT_KMEANS_STAT_BLOCKS 1024
#define MVT_KM_LO 0           /* 3 doubles: bounding-box minimum */
#define MVT_KM_HI 3           /* 3 doubles: bounding-box maximum */
#define MVT_KM_SCALE 6        /* double, a power of two: fixed-point units per coordinate unit */
#define MVT_KM_SCALE2 7       /* double, a power of two: fixed-point units per squared-distance unit */
#define MVT_KM_TOL 8          /* double: tol * mean per-coordinate variance (sklearn's stopping threshold) */
#define MVT_KM_ITER 9         /* int64: Lloyd iterations done */
#define MVT_KM_CONVERGED 10   /* int64 flag */
#define MVT_KM_EMPTY 11       /* int64: empty clusters of the last assignment */
#define MVT_KM_INERTIA 12     /* double: inertia of the last assignment */
#define MVT_KM_INERTIA_ACC 13 /* uint64: running fixed-point inertia */
#define MVT_KM_SHIFT 14       /* double: sum of squared centre shifts of the last update */
#define MVT_KM_POT 15         /* uint64: fixed-point potential after the last seeding step */
#define MVT_KM_CAND 16        /* MVT_KMEANS_MAX_CAND int64: candidate point indices of the running seeding step */
#define MVT_KM_WORDS 32
/* Bounding box, fixed-point scales (a value gets min(2^40, 2^62 / M) levels: M of them sum below 2^63), the stopping threshold,
 * and the counters of a fresh run.  partial: workspace of MVT_KMEANS_STAT_BLOCKS * 6 doubles. */
int mvt_kmeans_stats(const float* pts, long long M, float tol, double* partial, long long* state, void* stream);
/* Greedy k-means++ (sklearn _kmeans_plusplus): the first centre uniform, then per centre 2 + floor(ln k) candidates drawn with
 * probability proportional to the squared distance to the nearest centre so far, the one that lowers the potential most kept.
 * Draws are a hash of (seed, step, candidate).  Two launches per centre, no host read-back.  centres [k][3] out;
 * min_d2: workspace [M] floats; partials: workspace of MVT_KMEANS_MAX_CAND * MVT_KMEANS_SEED_BLOCKS uint64.  Needs mvt_kmeans_stats. */
int mvt_kmeans_seed(const float* pts, long long M, int k, long long seed, float* min_d2, void* partials, float* centres,
                    long long* state, void* stream);
/* Nearest centre of every point (direct dx^2 + dy^2 + dz^2 in fp32 against centres in LDS, ties to the lowest index) -> labels [M],
 * and acc [k][4] uint64 += (fixed-point coordinate sums, count); the inertia in fp64 per point, summed in fixed point.  acc must
 * be zero on entry (mvt_kmeans_update leaves it so).  Returns at once when the state says converged or max_iter iterations are
 * done, unless final_pass. */
int mvt_kmeans_assign(const float* pts, long long M, const float* centres, int k, int* labels, void* acc, long long* state,
                      int max_iter, int final_pass, void* stream);
/* centre = lo + sum / (count * scale) in fp64, stored as fp32 (an empty cluster keeps its centre), acc cleared, iteration
 * counted, converged when the sum of squared shifts <= the threshold.  final_pass: only report inertia and empty clusters of the
 * assignment in acc (centres, acc and the counters stay). */
int mvt_kmeans_update(float* centres, int k, void* acc, long long* state, int max_iter, int final_pass, void* stream);
/* n_iters <= 64 times (assign, update) in one call; iterations after convergence or max_iter are empty launches. */
int mvt_kmeans_iterate(const float* pts, long long M, float* centres, int k, int* labels, void* acc, long long* state, int n_iters,
                       int max_iter, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scene normalisation (reference: datasets/generic_scene_dataset.py:288-358 compute_auto_scene_normalization,
 * datasets/utils.py:210-301 transform_scene).  Sums across workgroups are integers, or fp64 sums in an
 * order fixed by the problem size: two runs give the same bits.  No kernel waits on another workgroup.
 * --------------------------------------------------------------------------------------------- */
#define MVT_SELECT_WS_WORDS 264 /* uint32 words of a select's workspace: 256 histogram bins, prefix, rank, two words of the successor */
/* out[0] = the k-th smallest (0-based) of n fp32 values, the bits of np.sort(values)[k].  Radix select on the monotone uint32
 * image of the float (sign bit set: all bits flipped; clear: the sign bit set), four passes of 8 bits: a digit histogram in LDS,
 * integer adds into 256 global bins, then one workgroup picks the digit and the remaining rank -- no host read between passes.
 * Order rule: the image's, so -0.0 < +0.0 (numpy calls them equal and may place them either way) and NaNs sort by their bits;
 * callers refuse NaN.  1 <= n < 2^31, 0 <= k < n, else MVT_ERR_ARG before any launch.  workspace: MVT_SELECT_WS_WORDS uint32. */
int mvt_select_kth(const float* values, long long n, long long k, float* out, void* workspace, void* stream);

#define MVT_SCENE_BLOCKS 1024 /* workgroups of the passes that leave per-workgroup fp64 partial sums */
/* state of mvt_scene_stats: MVT_SN_WORDS 64-bit words on the device */
#define MVT_SN_M 0           /* int64: points kept */
#define MVT_SN_CENTROID 1    /* 3 doubles */
#define MVT_SN_Z_QUANTILE 4  /* double: the q_floor quantile of z */
#define MVT_SN_FLOOR 5       /* double: that quantile - centroid z (the reference's quantile of the centred z, up to rounding) */
#define MVT_SN_Z_LO 6        /* double: order statistic Z_RANK of z */
#define MVT_SN_Z_HI 7        /* double: order statistic Z_RANK + 1 (Z_LO again when there is none) */
#define MVT_SN_Z_RANK 8      /* int64: floor(q_floor * (M - 1)), the product rounded to fp32 as torch.quantile does for a float32 tensor */
#define MVT_SN_R_QUANTILE 9  /* double: the q_radius quantile of |p - centroid - (0, 0, floor)| */
#define MVT_SN_R_LO 10
#define MVT_SN_R_HI 11
#define MVT_SN_R_RANK 12
#define MVT_SN_NONFINITE 13  /* int64: valid pixels whose depth is not finite */
#define MVT_SN_Z_WEIGHT 14   /* double: the rank's fraction, the interpolation weight between LO and HI */
#define MVT_SN_R_WEIGHT 15
#define MVT_SN_WORDS 16
/* Pool statistics of frame t of depths (V,T,1,H,W) [conf: the same layout or NULL], both read in place.  A pixel is valid when
 * conf > conf_thresh && depth > 0 (conf = NULL: depth > 0); a view with fewer than min_points valid pixels is left out whole; the
 * rest is unprojected with mvt_unproject's arithmetic at stride 1 (kinv / einv [V*T] from mvt_invert_cameras).  state receives the
 * kept count M, the centroid (fp64 sums in a fixed order), the q_floor quantile of z and, when q_radius >= 0, the q_radius
 * quantile of the centred-and-lifted points' norms (each norm in fp64, rounded to fp32 once); quantiles are torch.quantile's
 * default: linear interpolation between two exact order statistics (radix select, as mvt_select_kth).  M = 0 leaves the
 * quantiles meaningless.  Workspaces: keys V*H*W uint32, partial MVT_SCENE_BLOCKS * 3 doubles, iws MVT_SELECT_WS_WORDS + V int32.
 * V*H*W < 2^31.  14 launches, 25 with the radius quantile; no host read. */
int mvt_scene_stats(const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T, int t, int H, int W,
                    float conf_thresh, int min_points, float q_floor, float q_radius, unsigned int* keys, double* partial, int* iws,
                    long long* state, void* stream);

/* The similarity transform X' = t + R (s X) of transform_scene.  xf: 13 doubles on the HOST (s, R row-major, t), s finite and
 * positive.  Any of the three parts may be absent (count 0).  depths_out [n_depth] = depths * s; extrs_out [n_extr][3][4] =
 * [Re | s te] [R^T | -R^T t; 0 1] (the rigid inverse in closed form); queries_out [n_query][4] = (t, t + R (s xyz)).  All
 * arithmetic in fp64, rounded to fp32 once; out of place (in == out is allowed). */
int mvt_scene_apply(const float* depths, float* depths_out, long long n_depth, const float* extrs, float* extrs_out, int n_extr,
                    const float* queries, float* queries_out, long long n_query, const double* xf, void* stream);
/* The same map on rows of three floats (track points); with the inverse's parameters (1/s, R^T, -R^T t / s) it undoes it. */
int mvt_scene_tracks(const float* tracks, float* out, long long n_rows, const double* xf, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depth cleaning: statistical and radius outlier removal of every (view, frame) cloud (reference: the demo's
 * --clean_pointcloud, utils/visualizer_rerun.py _clean_point_cloud_with_open3d, i.e. Open3D's remove_statistical_outlier /
 * remove_radius_outlier, whose rules the entries restate: the neighbour searches include the query point itself, the sample
 * deviation divides by valid - 1, the radius test is strict).  Every (view, frame) depth map is its own cloud.
 * Three stages, five launches with the two box launches between the first two, no host read between them:
 *   mvt_clean_points -> mvt_tile_aabb -> mvt_tile_group_aabb -> mvt_clean_search -> mvt_clean_mask
 * Workspace per cloud of P points: xyz 16 P, a / c 4 P, keep P, boxes 32 ceil(P / 64) (1 + 1/64) bytes: under 22 bytes a
 * point.  The Python layer (mvtracker_amd/clean.py) cuts a clip into runs of frames of at most 2^23 padded points, which bounds
 * the workspace at 176 MiB whatever the clip's length.
 * --------------------------------------------------------------------------------------------- */
#define MVT_CLEAN_STATISTICAL 0
#define MVT_CLEAN_RADIUS 1
#define MVT_CLEAN_MAX_K 64
/* Cloud points of frames [t0, t0 + nt) of depths (V,T,1,H,W) [conf: the same layout or NULL], both read in place:
 * xyz [V*nt][Hp*Wp][4], cloud v * nt + (t - t0), raster order on the grid padded to whole 8x8 patches (Hp, Wp = H, W rounded
 * up to multiples of 8), which is the patch-tile layout of mvt_tile_aabb with grid_w = Wp, grid_h = Hp.  A pixel is valid when
 * its depth is finite and > 0, conf > conf_thresh (conf given), its point is finite and (sphere given: 4 floats on the HOST,
 * centre and radius > 0) fma(dz,dz,fma(dy,dy,dx*dx)) < fl(radius radius), the d2 of the searches.  A valid pixel
 * gets the bits mvt_unproject gives at stride 1, level 0 (kinv / einv [V*T] from mvt_invert_cameras) and .w = 0; every other
 * pixel, and the padding, gets (NaN, NaN, NaN, 0): mvt_tile_aabb ignores it and the search skips it.
 * H, W <= 32768, Hp * Wp < 2^31, V * nt <= 65535.  1 launch. */
int mvt_clean_points(const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T, int t0, int nt, int H,
                     int W, float conf_thresh, const float* sphere, float* xyz, void* stream);
/* The self-search: every point of each of the C clouds xyz [C][P][4] is a query against its own cloud.  A point takes part
 * when its three coordinates are finite.  d2(i,j) = fma(dz,dz,fma(dy,dy,dx*dx)) in fp32, the arithmetic of mvt_knn_scan.
 *   MVT_CLEAN_STATISTICAL (1 <= K <= MVT_CLEAN_MAX_K): a_out [C][P] = the mean Euclidean distance from the point to its
 *     k' = min(K, M) nearest points of the cloud, ITSELF INCLUDED at distance 0 (M = points taking part): each distance is the
 *     fp64 sqrt of the fp32 d2, summed in fp64 in ascending order of d2, divided by k', rounded to fp32 once.  NaN for a point
 *     that takes no part.
 *   MVT_CLEAN_RADIUS (radius > 0, min_points >= 0): c_out [C][P] = min(#{j : d2(i,j) < fl(radius radius)}, min_points + 1),
 *     self included; -1 for a point that takes no part.
 * Exact at any point order: tile_box [C][ceil(P/64)][8] from mvt_tile_aabb(xyz, P, C, grid_w, grid_h) and group_box
 * [C][ceil(ntiles/64)][8] from mvt_tile_group_aabb(tile_box, P, C) only prune, and a box is skipped only when its distance,
 * taken with the scan's own monotone arithmetic on the per-axis gaps, exceeds the current bound.  grid_w = grid_h = 0: linear
 * tiles of 64 points (an unorganised list); grid_w, grid_h > 0 (multiples of 8, P = grid_w * grid_h): 8x8 patches of ONE image
 * per cloud.  The result is the same, only the speed differs.  One wave per tile, one query per lane; LDS K * 512 bytes per
 * workgroup of 128 threads; every loop is bounded by the tile count (a cloud of NaNs, an empty cloud and M < K end normally).
 * C <= 65535, P < 2^31 - 64.  1 launch. */
int mvt_clean_search(const float* xyz, int C, long long P, int grid_w, int grid_h, int mode, int K, float radius, int min_points,
                     const float* tile_box, const float* group_box, float* a_out, int* c_out, void* stream);
/* Cloud statistics and the keep mask.  state [C][4] doubles = {M, mu, sigma, thr}, keep [C][P] uint8.
 *   MVT_CLEAN_STATISTICAL (a [C][P] from the search, c ignored): M = points taking part (a not NaN);
 *     mu = (sum of the a > 0) / M; sigma = sqrt(sum over a > 0 of (a - mu)^2 / (M - 1)); thr = mu + std_ratio sigma;
 *     keep = a > 0 && a < thr; M <= 1 keeps nothing (sigma = 0).  The divisor is M, every point taking part, not the number
 *     of a > 0.  fp64 sums in an order fixed by P alone (thread-strided, a shuffle tree, the four waves in order): no atomics,
 *     the same bits in every run.
 *   MVT_CLEAN_RADIUS (c [C][P], a ignored): M = points taking part (c >= 0), mu = sigma = thr = 0; keep = c > min_points.
 * One workgroup per cloud.  1 launch. */
int mvt_clean_mask(const float* a, const int* c, int C, long long P, int mode, float std_ratio, int min_points, double* state,
                   unsigned char* keep, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Camera alignment: point-to-plane ICP of one view's clouds onto the clouds of the other views (reference:
 * conversions/droid/utils/optimization.py run_icp_point_to_plane, i.e. Open3D registration_icp with
 * TransformationEstimationPointToPlane, whose rules the entries restate: the correspondence is the nearest target point strictly
 * inside max_correspondence_distance, r = (p - q) . n, J = [p x n | n], J^T J x = -J^T r, T(x) = TransformVector6dToMatrix4d(x),
 * fitness = correspondences / source points, inlier_rmse = sqrt(sum d2 / correspondences), stop when both change by less than
 * 1e-6).  Clouds are [frames][P][4] float rows (x, y, z, 0) with NaN rows for points that take no part: organised (grid_w x grid_h,
 * multiples of 8, P = grid_w grid_h, raster order: what mvt_clean_points writes with nt = frames) or point lists (grid 0, 0).
 * A frame's source cloud only meets the same frame's target clouds; the normal equations are summed over the frames.
 * One ICP run of max_iterations is max_iterations + 1 times (mvt_align_correspond, mvt_align_solve), the last solve with
 * final_call = 1, then mvt_align_transform -> mvt_align_normals -> mvt_tile_aabb -> mvt_tile_group_aabb of the moved clouds.
 * No atomics and no host read: both entries return at once when istate[MVT_ALIGN_I_DONE] is set.
 * --------------------------------------------------------------------------------------------- */
#define MVT_ALIGN_MAX_TARGETS 8
#define MVT_ALIGN_ROW 30  /* doubles per partial row: 21 upper entries of J^T J (row-major), 6 of J^T r, count, sum r^2, sum d2 */
#define MVT_ALIGN_HIST 10 /* doubles per evaluation: count, fitness, rmse, sum r^2, x[6] (0 when no update followed) */
#define MVT_ALIGN_I_DONE 0 /* words of istate (4 int32, zeroed by the caller before a run) */
#define MVT_ALIGN_I_ITERATIONS 1
#define MVT_ALIGN_I_STATUS 2
#define MVT_ALIGN_I_EVALS 3
#define MVT_ALIGN_FEW 1      /* status bit: fewer than 6 correspondences, D left as it was */
#define MVT_ALIGN_SINGULAR 2 /* status bit: a pivot <= 1e-12 x the largest diagonal entry, D left as it was */
typedef struct mvt_align_cloud {
  const float* xyz;       /* [frames][P][4] the target's points as they stand now */
  const float* nrm;       /* [frames][P][4] their normals; a point with a NaN normal.x takes no part */
  const float* tile_box;  /* [frames][ceil(P/64)][8] from mvt_tile_aabb(xyz, P, frames, grid_w, grid_h) */
  const float* group_box; /* [frames][ceil(ntiles/64)][8] from mvt_tile_group_aabb */
  long long P;
  int grid_w, grid_h;
} mvt_align_cloud;
/* Normals of C organised clouds xyz [C][grid_h grid_w][4]: with a = p[x+1] - p[x-1], b = p[y+1] - p[y-1] (fp32),
 * c = a x b with every product and difference rounded on its own, n = c / sqrt(fma(cz,cz,fma(cy,cy,cx cx))) (correctly rounded
 * sqrt and divisions).  Valid when the pixel is not on the border, the centre and the four neighbours are finite, each neighbour
 * has d2(neighbour, centre) <= fl(max_edge max_edge) (the d2 of the searches) and the length is > 0 and finite; every other pixel
 * gets (NaN, NaN, NaN, 0).  The orientation is left as it falls: point-to-plane only uses (n . d)^2.  1 launch. */
int mvt_align_normals(const float* xyz, int C, int grid_w, int grid_h, float max_edge, float* nrm, void* stream);
/* xyz[i] = D xyz0[i] for n rows of 4 floats; D: 12 doubles ON THE DEVICE (rows of [R|t]).  Coordinate r is
 * fma(D[4r+2], z, fma(D[4r+1], y, D[4r] x)) + D[4r+3] in fp64, rounded to fp32 once; a NaN row stays NaN, and so does every row whose
 * result is not finite in all three coordinates (an infinite input, an overflow): the marker of a point that takes no part; .w = 0. */
int mvt_align_transform(const float* xyz0, const double* D, long long n, float* xyz, void* stream);
/* Query tiles of a source cloud (host arithmetic, no launch): the number of 64-query tiles per frame, or -1 for arguments the
 * search refuses.  Point list (grid 0, 0; sample_stride 1): query slot q = point q.  Organised: the pixels with y % s == 0 and
 * x % s == 0 form hs x ws samples (hs = ceil(grid_h / s), ws = ceil(grid_w / s)), cut into 8x8 patches of samples,
 * *tiles_per_row = ceil(ws / 8) patches per row; slot (tile, lane) is sample (8 (tile / tpr) + lane / 8, 8 (tile % tpr) + lane % 8),
 * pixel (s sy, s sx), and takes no part when it lies outside the samples. */
int mvt_align_queries(long long P, int grid_w, int grid_h, int sample_stride, int* tiles_per_row);
/* The search and the tile sums.  Queries: the slots above of src_xyz0 [frames][src_P][4], each taken as D p0 with
 * mvt_align_transform's rounding.  Candidates: the points with a valid normal of targets[0..n_targets) (host array), same frame.
 * d2 = fma(dz,dz,fma(dy,dy,dx dx)) in fp32, the arithmetic of mvt_knn_scan.  Result per query: the candidate with the smallest
 * (d2, cloud, index) among those with d2 < cap2 (strict; cap2 = fl(fl(cap) fl(cap)) comes in rounded).  Tile and group boxes only
 * prune: a box is skipped when its distance, with the same monotone arithmetic, EXCEEDS the query's current bound (its best d2,
 * cap2 at the start) -- strictly, so that a point at exactly the bound in a tile visited later still wins a tie by its index.
 * q_idx / q_d2 [frames][tiles 64] (both or neither): the global target index (point j of target k is sum of P of the targets
 * before k, + j; -1 for none) and d2 (NaN for none).  partial [frames][tiles][MVT_ALIGN_ROW]: the sums over the tile's matched
 * queries, each by the shuffle tree lane ^ 32, ^ 16, .. ^ 1 in fp64, with r and J in fp64 from the fp32 p (query), q (target
 * point) and n.  One wave per tile, one query per lane, 128 threads, no LDS.  Returns at once when istate[0] != 0.
 * The targets' points together < 2^31 - 64.  1 launch. */
int mvt_align_correspond(const float* src_xyz0, long long src_P, int src_grid_w, int src_grid_h, int sample_stride, int frames,
                         const double* D, float cap2, const mvt_align_cloud* targets, int n_targets, const int* istate,
                         double* partial, int* q_idx, float* q_d2, void* stream);
/* One evaluation of the ICP loop, in one workgroup.  Column c of partial [n_rows][MVT_ALIGN_ROW] is summed by 8 threads (thread g
 * takes rows g, g + 8, .. ascending; the 8 sums are added for g = 0..7: an order fixed by n_rows) -> sums [30] (optional).
 * count = sums[27], fitness = count / *n_queries (device double: the source points taking part), rmse = sqrt(sums[29] / count),
 * written to hist[evals] (MVT_ALIGN_HIST doubles, while evals < max_hist) and to result [4] = {fitness, rmse, iterations, status}.
 * If this is not the first evaluation and |fitness - previous| < 1e-6 and |rmse - previous| < 1e-6 (the previous ones read from
 * result): done.  Otherwise, unless final_call: count < 6 -> MVT_ALIGN_FEW and done; else LDL^T of J^T J (a pivot
 * <= 1e-12 max diagonal -> MVT_ALIGN_SINGULAR and done), x = solution of J^T J x = -J^T r, T(x) = [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5],
 * D <- T(x) D, iterations += 1, x to the hist row.  Returns at once when istate[0] != 0.  1 launch. */
int mvt_align_solve(const double* partial, long long n_rows, const double* n_queries, int final_call, int max_hist, double* D,
                    int* istate, double* hist, double* sums, double* result, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cloud preparation: PCA normals and voxel downsampling (reference: conversions/droid/utils/optimization.py estimate_normals /
 * downsample_pointcloud, i.e. Open3D's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) and voxel_down_sample, whose rules
 * the entries restate).  The two parts share no kernel.
 * --------------------------------------------------------------------------------------------- */
#define MVT_NORMALS_MAX_NN 64
/* Normals of every point of each of the C clouds xyz [C][P][4] from a PCA over its neighbours in the same cloud.  A point takes
 * part when its three coordinates are finite.  d2(i,j) = fma(dz,dz,fma(dy,dy,dx*dx)) in fp32, the arithmetic of mvt_knn_scan.
 * Neighbours of point i: of the points taking part with d2 < fl(fl(radius) fl(radius)) (strict; i itself is one, at d2 = 0), the
 * max_nn smallest by the key (d2, index) -- Open3D's knnSearch(max_nn) cut at r^2, so r^2 bounds the search from the first
 * candidate on.  radius = +inf gives plain kNN.  3 <= max_nn <= MVT_NORMALS_MAX_NN.
 * With n neighbours: e_j = (double)p_j - (double)p_i (exact), S1 = sum e_j and S2 = sum e_j e_j^T in fp64 in ascending key order,
 * C = S2 / n - (S1 / n)(S1 / n)^T, and the normal is a unit eigenvector of the smallest eigenvalue of C (cyclic Jacobi in fp64, a
 * fixed number of sweeps), rounded to fp32 once; .w = 0.
 * DEVIATION from Open3D: with n < 3, or lambda_mid <= 1e-12 lambda_max (collinear or coincident neighbours), and for a point that
 * takes no part, the row is (NaN, NaN, NaN, 0), which mvt_align_correspond skips; Open3D leaves (0, 0, 1) there, which ICP would
 * take for a real plane.
 * viewpoint: NULL, or [C][3] floats on the device: the normal is flipped so that n . (vp - p_i) >= 0 in fp64 (Open3D's
 * orient_normals_towards_camera_location).  Without it the sign is left as it falls: point-to-plane only uses (n . d)^2.
 * Optional outputs (NULL: not written): nbr_idx [C][P][max_nn] the neighbours in ascending key order, padded with -1;
 * nbr_cnt [C][P] = n, -1 for a point that takes no part; cov [C][P][6] = C as (xx, xy, xz, yy, yz, zz), NaN for such a point.
 * grid_w, grid_h, tile_box, group_box: as mvt_clean_search takes them (they only prune: a box is skipped only when its lower
 * bound EXCEEDS the query's bound, so an equal-d2 point with a lower index in a later tile still wins).  One wave per tile, one
 * query per lane, workgroups of 64 threads with max_nn * 512 bytes of LDS; no barrier, no atomics; every loop is bounded by the
 * tile count, max_nn or the sweep count.  C <= 65535, P < 2^31 - 64.  1 launch. */
int mvt_normals_estimate(const float* xyz, int C, long long P, int grid_w, int grid_h, int max_nn, float radius, const float* tile_box,
                         const float* group_box, const float* viewpoint, float* nrm, int* nbr_idx, int* nbr_cnt, double* cov,
                         void* stream);

/* Voxel downsampling of ONE cloud xyz [P][4], 0 < P < 2^31 (Open3D voxel_down_sample), three entries with no host read between:
 *   mvt_voxel_bounds -> mvt_voxel_insert -> mvt_voxel_emit
 * state: MVT_VOXEL_STATE_WORDS 64-bit words on the device, doubles and integers as named below. */
#define MVT_VOXEL_RANGE 1        /* status bit: a cell index >= 2^21 on some axis; nothing is emitted */
#define MVT_VOXEL_FULL 2         /* status bit: the table had no slot left for a cell; nothing is emitted */
#define MVT_VOXEL_ORIGIN 0       /* 3 doubles */
#define MVT_VOXEL_SIZE 3         /* double: the voxel size */
#define MVT_VOXEL_STATUS 4       /* int64: MVT_VOXEL_* bits */
#define MVT_VOXEL_POINTS 5       /* int64: points taking part */
#define MVT_VOXEL_STATE_WORDS 8
#define MVT_VOXEL_BOUND_BLOCKS 1024
#define MVT_VOXEL_SLOT_WORDS 6   /* 64-bit words per slot of the table: key, three sums, count / first, row / spare */
/* lo = the per-axis minimum of the points taking part (finite coordinates), origin = lo - voxel / 2 in fp64; the status is
 * cleared.  voxel finite and > 0.  partial: workspace of MVT_VOXEL_BOUND_BLOCKS * 4 doubles.  2 launches. */
int mvt_voxel_bounds(const float* xyz, long long P, double voxel, double* partial, long long* state, void* stream);
/* The hash grid.  u = ((double)p - origin) / voxel (a division, as in Open3D), cell = floor(u); the key is the three 21-bit cells
 * packed into 64 bits.  table: capacity * MVT_VOXEL_SLOT_WORDS 64-bit words, capacity a power of two >= 2 P (cleared here).  A
 * point claims its cell's slot with a 64-bit atomicCAS and linear probing bounded by the capacity: a failed swap returns the slot's
 * key, which is its own or another cell's, and then it moves on -- nothing spins on another thread; no slot left sets
 * MVT_VOXEL_FULL, a cell index >= 2^21 MVT_VOXEL_RANGE.  Per slot, integer atomics only: the count, first = the smallest input
 * index, and three uint64 sums of rint((u - cell) 2^32) (P < 2^31 keeps them below 2^63), so no result depends on the order of
 * arrival; which slot a cell gets does, but no output depends on that.  2 launches. */
int mvt_voxel_insert(const float* xyz, long long P, long long* state, long long* table, long long capacity, void* stream);
/* One row per occupied cell, in ascending order of `first` (a voxel appears where its first point appeared):
 * points [Mv][4] = origin + (cell + sum / (count 2^32)) voxel per axis in fp64, rounded to fp32 once, .w = 0; counts [Mv];
 * first [Mv]; *n_out = Mv; labels (optional) [P] = the output row of every input point, -1 for a point that takes no part.
 * The outputs need room for as many rows as points take part (at most P).  With a status bit set *n_out = 0, no row is written and
 * every label is -1.  block_counts: workspace of ceil(P / 256) int32.  Count, scan, scatter as mvt_query_pool, then the labels:
 * 3 or 4 launches. */
int mvt_voxel_emit(const float* xyz, long long P, const long long* state, long long* table, long long capacity, int* block_counts,
                   float* points, int* counts, int* first, int* labels, int* n_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reprojection check: a z-buffered render of points into cameras, and scores of the render against the camera's own frame and
 * depth map (reference: conversions/droid/reproject_depth_into_videos.py render_dense_pointcloud, and
 * conversions/droid/debug/compare_photometric_error.py compute_mse / compute_psnr / compute_mae / compute_ssim).
 *
 * THE RENDERING RULE.  A source point is three fp32 world coordinates X = (x, y, z); a camera is fp32 intr K (3,3) and extr E (3,4),
 * world -> camera.  All arithmetic is fp64 with every product, sum and quotient rounded on its own (no fused multiply-add):
 *   c_r = ((E[r][0] x + E[r][1] y) + E[r][2] z) + E[r][3]                      r = 0, 1, 2
 *   uf  = (c_0 fx) / c_2 + cx,   vf = (c_1 fy) / c_2 + cy                       fx, fy, cx, cy = K00, K11, K02, K12 (skew ignored)
 * The point is drawn when X is finite, c_2 > (double)min_depth (strict), uf and vf are finite with |uf|, |vf| < 2^31, and with
 * u = (int)uf, v = (int)vf (truncation TOWARD ZERO, the reference's astype(int32): uf in (-1, 0) lands in column 0) 0 <= u < W and
 * 0 <= v < H.  A pixel's value is the minimum over its points of the 64-bit key (bits of (float)c_2) << 32 | source index: the
 * nearest point, and among points of equal fp32 depth the lowest index; one unsigned 64-bit atomicMin per point and pixel, so the
 * result does not depend on the order of arrival.  An empty pixel keeps the key ~0.  (A c_2 beyond the fp32 range is drawn with
 * depth +inf, behind every finite one.)  splat = s in {1, 3, 5}: the same key goes to the s x s pixels centred on (u, v), clipped to
 * the image -- a depth-tested point sprite (the centre must lie in the image).
 * keys: [n_targets][H W] 64-bit words, set to ~0 by mvt_reproject_clear before the splats that share them.
 * One render is  mvt_reproject_clear (a memset, no launch) -> mvt_reproject_splat_* (1 launch) -> mvt_reproject_resolve (1 launch).
 * --------------------------------------------------------------------------------------------- */
#define MVT_REPROJECT_MAX_TARGETS 16
/* keys[0..n) = ~0 (hipMemsetAsync of 0xFF on the stream). */
int mvt_reproject_clear(unsigned long long* keys, long long n, void* stream);
/* The clip form: the source points are the pixels of frame t of depths [V][T][1][H][W], read in place (conf: the same layout or
 * NULL), each valid as in mvt_clean_points (depth finite and > 0, conf > conf_thresh, point finite) with exactly its point bits
 * (mvt_unproject at stride 1 through kinv / einv [V T][9] / [V T][12] of mvt_invert_cameras); no cloud is materialised.  Rendered
 * into n_targets cameras at once: target k is view target_views[k] (HOST array) with the camera intrs [k][9], extrs [k][12] (device,
 * fp32).  exclude_self: target k takes no point of source view target_views[k] ("others", the leave-one-out of the alignment);
 * otherwise every view's ("all").  Source index = view H W + y W + x.  V H W < 2^31, 1 <= n_targets <= MVT_REPROJECT_MAX_TARGETS,
 * min_depth finite and >= 0.  1 launch: one thread per source pixel, a loop over the targets. */
int mvt_reproject_splat_depths(const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T, int t, int H,
                               int W, float conf_thresh, const int* target_views, int n_targets, const float* intrs, const float* extrs,
                               int exclude_self, float min_depth, int splat, unsigned long long* keys, void* stream);
/* The list form: points [M][3] fp32 into n_targets cameras; source index = row.  0 < M < 2^31.  1 launch. */
int mvt_reproject_splat_points(const float* points, long long M, int n_targets, const float* intrs, const float* extrs, int H, int W,
                               float min_depth, int splat, unsigned long long* keys, void* stream);
/* Per pixel of target k: index (int32; -1: empty), depth (fp32: the key's high word; 0: empty, the project's "no depth") and color
 * (uint8, planar [3][H W]; (0,0,0): empty), target k at image k * target_stride of each output (index / depth [.][H W], color
 * [.][3][H W]).  The colour is gathered from frame t of rgbs [V][T][3][H][W] in place (clip form; uint8 when rgb_u8, else fp32, a
 * value becoming min(max(rintf(x), 0), 255)) or from colors [M][3] uint8 (list form; rgbs NULL).  1 launch. */
int mvt_reproject_resolve(const unsigned long long* keys, int n_targets, int H, int W, const void* rgbs, int rgb_u8, int V, int T, int t,
                          const unsigned char* colors, long long M, long long target_stride, int* index, float* depth, unsigned char* color,
                          void* stream);
/* Scores of n image pairs: a [n][3][H W] the renders, b [n][3][H W] the real frames (each uint8 or fp32 by its flag, an fp32 value
 * converted by the rule above), with the renders' index / depth [n][H W] and the targets' own depth maps target_depth [n][H W].
 * scores [n][MVT_SCORE_WORDS] 64-bit words:
 *   N = H W; COVERED = pixels with index >= 0 (int64); SSE, SAE = sums over pixels and the 3 channels of (a - b)^2 and |a - b|
 *   (uint64, exact); SSE_COV, SAE_COV the same over the covered pixels; SSIM, SSIM_COV = the sum of the SSIM map over all / the
 *   covered pixels (double); N_DEPTH = covered pixels whose target depth is finite and > 0; N_CLOSE = of those,
 *   fabs((double)zr - (double)zt) <= (double)depth_tol; DEPTH_SAE, DEPTH_SAE_CLOSE = the sum of |zr - zt| over the N_DEPTH / the
 *   N_CLOSE pixels (double).  Words 12..15 are 0.
 * SSIM is the reference's compute_ssim with OpenCV's parameters: grey Y = (4899 R + 9617 G + 1868 B + 8192) >> 14 on the 8-bit
 * values; the maps x, y, x^2, y^2, xy blurred in fp64 with the separable 11-tap Gaussian exp(-(i - 5)^2 / 4.5) normalised to sum 1,
 * border reflect-101; C1 = 6.5025, C2 = 58.5225; ssim = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)).
 * One workgroup per 16 x 16 tile (a 5-pixel halo in LDS) writes one record to partial [n][mvt_photometric_blocks(H, W)]
 * [MVT_SCORE_WORDS]; a second launch adds an image's records in an order fixed by their number (no float atomics: the same bits in
 * every run).  H, W >= 6 (one reflection reaches the halo), n <= 65535.  2 launches. */
#define MVT_SCORE_WORDS 16
#define MVT_SCORE_N 0
#define MVT_SCORE_COVERED 1
#define MVT_SCORE_SSE 2
#define MVT_SCORE_SAE 3
#define MVT_SCORE_SSE_COV 4
#define MVT_SCORE_SAE_COV 5
#define MVT_SCORE_SSIM 6
#define MVT_SCORE_SSIM_COV 7
#define MVT_SCORE_N_DEPTH 8
#define MVT_SCORE_N_CLOSE 9
#define MVT_SCORE_DEPTH_SAE 10
#define MVT_SCORE_DEPTH_SAE_CLOSE 11
/* Records per image of mvt_photometric_score's workspace (host arithmetic, no launch); -1 for a size it refuses. */
int mvt_photometric_blocks(int H, int W);
int mvt_photometric_score(const void* a, int a_u8, const void* b, int b_u8, const int* index, const float* depth,
                          const float* target_depth, int n, int H, int W, float depth_tol, unsigned long long* partial,
                          unsigned long long* scores, void* stream);

/* ---- region clustering (csrc/cloud_cluster.hip; mvtracker_amd/cluster.py drives these) ----
 * DBSCAN of C clouds xyz (C, P, 4) fp32 per launch, NaN rows taking no part; grid = (w, h) of organised clouds padded to whole 8x8
 * patches (w * h = P) or (0, 0) for point lists; tile_box / group_box from mvt_tile_aabb / mvt_tile_group_aabb of the same
 * clouds (after the crop).  Two points are neighbours when the scan's fp32 d2 <= r2 (a point is its own neighbour); r2 is given
 * as such, rounded once by the caller.  A point is core with >= min_samples neighbours; clusters are the connected components of
 * the core points, numbered in ascending order of their lowest core index; a non-core point with core neighbours takes the lowest
 * cluster number among them; every other point is -1.  The results depend on the clouds alone: the same bits in every run.
 * state: MVT_CLUSTER_STATE_WORDS int64 per cloud on the device. */
#define MVT_CLUSTER_CANDIDATES 0   /* points taking part */
#define MVT_CLUSTER_CORE 1         /* core points */
#define MVT_CLUSTER_CLUSTERS 2     /* clusters */
#define MVT_CLUSTER_CHOSEN 3       /* id of the largest cluster (the lowest id among equal sizes), -1 without one */
#define MVT_CLUSTER_CHOSEN_SIZE 4  /* its points, border points included */
#define MVT_CLUSTER_NOISE 5        /* points taking part with label -1 */
#define MVT_CLUSTER_FALLBACK 6     /* 0, or why `select` is not the largest cluster: */
#define MVT_CLUSTER_STATUS 7       /* MVT_CLUSTER_BOUND: a union-find loop exceeded its bound (written by mvt_cluster_link) */
#define MVT_CLUSTER_STATE_WORDS 8
#define MVT_CLUSTER_FEW 1    /* fewer than min_samples points: all of them are selected */
#define MVT_CLUSTER_NONE 2   /* no cluster: every point taking part is selected */
#define MVT_CLUSTER_EMPTY 3  /* no point takes part: nothing is selected */
#define MVT_CLUSTER_BOUND 1
/* In place: a point of cloud c whose coordinates region_T_world[c] (3x4 fp32 rows on the device, fused multiply-adds x, y, z in
 * turn onto the translation) are not strictly inside bounds (6 floats on the HOST: lo, hi per axis) becomes a NaN row. */
int mvt_cluster_crop(float* xyz, int C, long long P, const float* region_T_world, const float* bounds, void* stream);
/* core (C, P) uint8: 1 where the point has >= min_samples neighbours (the count stops there), 0 elsewhere and on NaN rows. */
int mvt_cluster_count(const float* xyz, int C, long long P, int grid_w, int grid_h, float r2, int min_samples, const float* tile_box,
                      const float* group_box, unsigned char* core, void* stream);
/* parent (C, P) int32: for core points the lowest core index of their component (a lock-free min-index union-find over the core
 * neighbours, then flattened); state rows are cleared and word MVT_CLUSTER_STATUS written.  3 launches. */
int mvt_cluster_link(const float* xyz, int C, long long P, int grid_w, int grid_h, float r2, const float* tile_box, const float* group_box,
                     const unsigned char* core, int* parent, long long* state, void* stream);
/* root (C, P) int32: parent for core points, the lowest parent among the core neighbours for the others, -1 without one. */
int mvt_cluster_border(const float* xyz, int C, long long P, int grid_w, int grid_h, float r2, const float* tile_box, const float* group_box,
                       const unsigned char* core, const int* parent, int* root, void* stream);
/* labels (C, P) int32, select (C, P) uint8 (the largest cluster, or the fallback's points) and words 0..6 of the state rows.
 * sizes: workspace (C, P) int32, cleared here. */
int mvt_cluster_finish(const float* xyz, int C, long long P, int min_samples, const unsigned char* core, const int* root, int* sizes,
                       int* labels, unsigned char* select, long long* state, void* stream);

/* ---- motion masks (csrc/motion.hip; mvtracker_amd/motion.py drives these) ----
 * Static-background detection on a clip rgbs (V, T, 3, H, W), planar, uint8 or fp32 (reference:
 * mvtracker/datasets/generic_scene_dataset.py _static_bg_mask_from_window, demo.py _detect_static_prefix_frames).  The diff of
 * boundary b (frames b, b + 1) at a pixel is d_b = ((|dc0| + |dc1|) + |dc2|) / 3.0f in fp32 with an IEEE division, uint8 values
 * converted first; change[v, t, y, x] is the maximum of d_b over b in [t - win, t + win - 1] n [0, T - 2] and over the patch
 * |dy|, |dx| <= r clipped to the image; a pixel is static when change < thresh.  A NaN diff wins every maximum.
 * T >= 2, V * T <= 65535, H * W < 2^31 - 1024.  No atomics: the same bits in every run. */
#define MVT_MOTION_BLOCK_PIXELS 1024 /* pixels of one plane per workgroup of mvt_motion_temporal */
#define MVT_MOTION_TILE_W 64         /* mask pixels per workgroup of mvt_motion_mask */
#define MVT_MOTION_TILE_H 32
#define MVT_MOTION_MAX_RADIUS 15
/* Workgroups per view of mvt_motion_temporal / tiles per image of mvt_motion_mask (host arithmetic, no launch); -1 for a size
 * they refuse. */
int mvt_motion_blocks(int H, int W);
int mvt_motion_tiles(int H, int W);
/* One pass over the frames, each read once.  all_mode: out (V, H, W) = the maximum of d_b over every boundary; otherwise out
 * (V, T-1, H, W) = every d_b.  partial (V * mvt_motion_blocks, T-1) fp64: per workgroup and boundary the sum of
 * |dc0| + |dc1| + |dc2| over its pixels (exact on integer-valued frames). */
int mvt_motion_temporal(const void* rgbs, int is_u8, int V, int T, int H, int W, int all_mode, float* out, double* partial, void* stream);
/* mask (V, T, H, W) one byte per pixel, 1 = static.  win >= 1: src = the (V, T-1, H, W) diffs, the window's maximum is taken
 * while a tile is staged; win == 0: src = the (V, H, W) maximum of all_mode, pooled once and written to all T frames.
 * 0 <= r <= MVT_MOTION_MAX_RADIUS.  counts (V * T or, win == 0, V; mvt_motion_tiles) int32: static pixels per tile. */
int mvt_motion_mask(const float* src, int V, int T, int H, int W, int win, int r, float thresh, unsigned char* mask, int* counts,
                    void* stream);
/* report (T-1 + V * T) fp64: the T-1 sums of partial's columns, then the static pixels of every (view, frame) from counts (laid
 * out as mvt_motion_mask wrote them: all_mode = its win == 0), each added in an order fixed by the number of terms. */
int mvt_motion_report(const double* partial, const int* counts, int V, int T, int H, int W, int all_mode, double* report, void* stream);

/* ---- track overlays (csrc/overlay.hip; mvtracker_amd/overlay.py drives these) ----
 * The tracker's world-space tracks drawn into every view's frames (reference: mvtracker/utils/visualizer_mp4.py Visualizer.visualize,
 * draw_tracks_on_video, _draw_pred_tracks; DESIGN section 8 "Track overlays" states the rule and its deviations).
 * Projection of track point (x, y, z) by K (3x3) and E (3x4) of its (view, frame), fp32, every operation rounded on its own:
 *   c_r = ((E[r,0] x + E[r,1] y) + E[r,2] z) + E[r,3];  h_r = (K[r,0] c_0 + K[r,1] c_1) + K[r,2] c_2;  px = h_0 / h_2, py = h_1 / h_2.
 * Integer point: px, py clipped to [-1e4, 1e4], + pad in fp32, truncated toward zero.  It is invalid when px or py is NaN, or when
 * use_min_depth and not c_2 > min_depth.
 * Frame t of a view, later overwrites earlier: the frame (a float frame clamped to [0, 255] and truncated, NaN -> 0; 255 on the
 * border of `pad` pixels); for s in the trail window, ascending, for track i ascending, the stroke from point (s, i) to point
 * (s+1, i) unless s < query_frames[i], an endpoint is invalid or an endpoint is (0, 0); for i ascending the marker of point (t, i)
 * unless query_frames[i] > t, it is invalid, or x == 0 or y == 0: a disc of radius R = 2 linewidth when visible, else a ring.
 * Primitives, integer, not anti-aliased, clipped to the padded image: stroke of width w from a to b with d = b - a, L2 = |d|^2,
 * q = (p - a).d covers p iff (q <= 0: 4 |p-a|^2 <= w^2; q >= L2: 4 |p-b|^2 <= w^2; else 4 ((p-a) x d)^2 <= w^2 L2); disc
 * |p-c|^2 <= R^2; ring (2R-1)^2 <= 4 |p-c|^2 <= (2R+1)^2.
 * Key planes (V, Hp, Wp) uint64, Hp = H + 2 pad, zero = empty, key = order << 24 | r << 16 | g << 8 | b kept by atomic maximum:
 * the line plane persists over the frames of a clip (order (s+1) << 20 | i), the marker plane (order i + 1) is reset by
 * mvt_overlay_compose.  Limits: N and every frame number < MVT_OVERLAY_MAX_INDEX, Hp and Wp <= MVT_OVERLAY_MAX_SIDE (all integer
 * terms then fit 64 bits), V * Hp * Wp < 2^31.  The same bits in every run. */
#define MVT_OVERLAY_MAX_LINEWIDTH 8
#define MVT_OVERLAY_MAX_PAD 64
#define MVT_OVERLAY_MAX_SIDE 8192
#define MVT_OVERLAY_MAX_INDEX (1 << 20)
/* tracks (T, N, 3), intrs (V, T, 3, 3), extrs (V, T, 3, 4).  Any of: xyz (V, T, N, 3) fp32 <- (px, py, c_2), the reference's
 * world_space_to_pixel_xy_and_camera_z per view; points (T, V, N, 4) int32 <- (x, y, valid, 0); and, with lut (256, 3) uint8,
 * colors[n] <- lut[min(255, max(0, y * 256 / Hp))] for every track n whose query frame max(query_frames[n], 0) is frame0 + t for
 * a t of this launch, y the integer y in view color_view (pad when that point is invalid).  frame0: the clip's number of t = 0. */
int mvt_overlay_project(const float* tracks, const float* intrs, const float* extrs, int V, int T, int N, float* xyz, int* points, int pad,
                        int use_min_depth, float min_depth, const int* query_frames, int frame0, const unsigned char* lut, int color_view, int Hp,
                        unsigned char* colors, void* stream);
/* The scatter of frame t: the markers of cur (V, N, 4) into marker_keys and, with prev (the points of frame t-1; t >= 1) and
 * line_keys, the segments t-1 -> t into line_keys (both or neither).  Tracks 0..M-1 of N are drawn; visibility (N) bytes of
 * frame t or NULL (all visible); colors (N, 3) uint8; query_frames (N) int32. */
int mvt_overlay_draw(const int* prev, const int* cur, const unsigned char* visibility, const int* query_frames, const unsigned char* colors, int V,
                     int N, int M, int t, int linewidth, int Hp, int Wp, unsigned long long* line_keys, unsigned long long* marker_keys,
                     void* stream);
/* out[:, t_local] of (V, T, 3, Hp, Wp) uint8 <- marker key, else the line key when its segment s >= first_segment (line_keys NULL:
 * no lines), else frames[:, t_local] of (V, T, 3, H, W) uint8 or fp32, else 255; marker_keys is zero again afterwards. */
int mvt_overlay_compose(const void* frames, int is_u8, int V, int T, int t_local, int H, int W, int pad, const unsigned long long* line_keys,
                        int first_segment, unsigned long long* marker_keys, unsigned char* out, void* stream);

/* ---- mask queries (csrc/mask_queries.hip; mvtracker_amd/masks.py drives these; DESIGN section 8 "Mask queries") ----
 * labels (V, T, H, W), one byte per pixel: 0 = background, 1..255 a camera's local instance ids; the pointer is 16-byte aligned.
 * depths / conf (V, T, 1, H, W) fp32 (conf may be NULL), kinv [V*T][9], einv [V*T][12] as mvt_query_pool takes them.
 * A labelled pixel is VALID when its depth is finite, min_depth < depth <= max_depth (fp32 comparisons) and, with conf,
 * conf > conf_thresh.  Its world point is mvt_query_pool's (the same unprojection at stride 1).
 * Limits: V <= MVT_MASK_MAX_VIEWS, V * T <= 65535, H * W <= 2^24, V * H * W < 2^31; anything else: MVT_ERR_ARG before any launch.
 * Everything summed is an integer: the same bits in every run. */
#define MVT_MASK_LABELS 256
#define MVT_MASK_MAX_LABEL 255
#define MVT_MASK_MAX_VIEWS 64
#define MVT_MASK_FRAC_BITS 20   /* fixed point of the coordinate sums: q = (int64) rint((double) x * 2^20) */
#define MVT_MASK_RANGE_BITS 18  /* a valid point with a non-finite coordinate or |coordinate| >= 2^18 is left out and counted */
#define MVT_MASK_STAT_WORDS 6   /* int64 words per (view, frame, label): */
#define MVT_MASK_PIXELS 0       /*   labelled pixels */
#define MVT_MASK_COUNT 1        /*   valid pixels whose point is in range: the terms of the sums */
#define MVT_MASK_SUM 2          /*   .. 4: fixed-point sums of x, y, z */
#define MVT_MASK_OUT_OF_RANGE 5 /*   valid pixels left out of the sums */
/* stats (V, T, 256, MVT_MASK_STAT_WORDS) int64, 16-byte aligned, cleared here, then one pass over the clip.  Row 0 of every image
 * stays zero. */
int mvt_mask_stats(const unsigned char* labels, const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T,
                   int H, int W, float min_depth, float max_depth, float conf_thresh, long long* stats, void* stream);
/* centroid (V, T, 256, 3) fp64 <- (double) sum / (double) count * 2^-20 where count >= min_pixels (>= 1), NaN elsewhere. */
int mvt_mask_centroids(const long long* stats, int V, int T, int min_pixels, double* centroid, void* stream);
/* The greedy "average distance" matching on the centroids.  global_id (V, 256) int32 <- the object of every (view, label), -1 where
 * it has no centroid in any frame; distance (V, 256) fp64 <- the distance it joined its object at, NaN where it opened a new one;
 * state int32[2] <- (objects, present ids); ids: workspace of V * 256 int32.  match == 0: label l is object l - 1 in every view,
 * objects = the largest present label. */
int mvt_mask_match(const double* centroid, int V, int T, int min_common_frames, double distance_threshold, int match, int* ids,
                   int* global_id, double* distance, int* state, void* stream);
/* out (V, T, H, W) int32 <- table[v][label], -1 for background; table (V, 256) int32; out is 16-byte aligned. */
int mvt_mask_relabel(const unsigned char* labels, const int* table, int V, int T, int H, int W, int* out, void* stream);
/* The pool of (object, frame t): the valid pixels of frame t whose table[v][label] == object, in raster order (view, row, column):
 * pool (capacity, 3) fp32 <- their world points, pixel (capacity) int32 <- their raster index (v * H + y) * W + x, count <- how many
 * there are (rows beyond capacity are counted, not written).  block_counts: workspace of ceil(V * H * W / 256) int32.  Count, scan,
 * scatter as mvt_query_pool; the clip is read in place. */
int mvt_mask_pool(const unsigned char* labels, const float* depths, const float* conf, const float* kinv, const float* einv, int V, int T,
                  int t, int H, int W, float min_depth, float max_depth, float conf_thresh, const int* table, int object, int capacity,
                  float* pool, int* pixel, int* count, int* block_counts, void* stream);

/* ---- rigid object motion (csrc/rigid_motion.hip; mvtracker_amd/rigid.py drives these; DESIGN section 8 "Rigid motion") ----
 * tracks (T, N, 3) fp32, visibility (T, N) bytes (0 / 1), query_frames (N) int32, object_ids (N) int32: track i belongs to object
 * object_ids[i] when 0 <= object_ids[i] < G and to none otherwise.  A pose is a row-major 4 x 4 fp32 matrix [R t; 0 0 0 1] that maps
 * an object's reference configuration (its members' points at its reference frame) to a frame.  All sums are fp64 over a fixed
 * order (a lane's stride of the member list, then a fixed tree): the same bits in every run, no float atomics; the results of one
 * (object, frame) depend on that frame's rows and the reference frame's rows only.
 * Limits: 1 <= T <= 65535, 1 <= N (and M) <= 2^30, 1 <= G <= MVT_RIGID_MAX_OBJECTS; anything else: MVT_ERR_ARG before any launch. */
#define MVT_RIGID_MAX_OBJECTS 65535
#define MVT_RIGID_MAX_ITERATIONS 64
#define MVT_RIGID_OK 0          /* status of an (object, frame): fitted */
#define MVT_RIGID_TOO_FEW 1     /*   fewer than min_points members with base weight 1 (an object without members: everywhere) */
#define MVT_RIGID_DEGENERATE 2  /*   the members' reference points are collinear or coincident (see mvt_rigid_fit) */
#define MVT_RIGID_FILL_OCCLUDED 1 /* mvt_rigid_fill's replace bits */
#define MVT_RIGID_FILL_OUTLIERS 2
/* The member lists: counts (G) <- members per object, offsets (G + 1) <- their exclusive prefix, members (N) <- the tracks of object g
 * at members[offsets[g] .. offsets[g + 1]) in ascending track order, reference_frames (G) <- the largest query frame of the object's
 * members, clamped to [0, T - 1]; -1 for an object without members.  Count (integer atomics), scan, stable scatter. */
int mvt_rigid_members(const int* object_ids, const int* query_frames, int N, int G, int T, int* counts, int* offsets, int* members,
                      int* reference_frames, void* stream);
/* One workgroup per (object g, frame t), r = reference_frames[g], P_i = tracks[r, i], Q_i = tracks[t, i].  Base weight of member i: 1
 * when (t >= query_frames[i] or live_before_query) and (not use_visibility or visibility[t, i] and visibility[r, i]) and P_i, Q_i are
 * finite.  Weighted Kabsch in fp64 (centroids, then the centred moments; the proper rotation that maximises tr(R^T H) as the top
 * eigenvector of Horn's 4 x 4 matrix), iterations - 1 refits on base and (residual of the previous fit <= inlier_threshold); a refit
 * that keeps fewer than min_points members, or a degenerate set, is dropped and the previous fit stands.  Degenerate: the
 * second-largest eigenvalue of the weighted covariance of P, over the weight sum, is below min_spread^2.
 * poses (G, T, 16), used / inlier_count / status (G, T) int32, rmse (G, T) fp32 (over the inliers), residual (T, N) fp32 and
 * inliers (T, N) bytes: residual = ||R P + t - Q|| of the fit that stood for every member (NaN where status != 0, and for tracks
 * of no object), inliers = base and residual <= inlier_threshold. */
int mvt_rigid_fit(const float* tracks, const unsigned char* visibility, const int* query_frames, const int* object_ids, const int* offsets,
                  const int* members, const int* reference_frames, int T, int N, int G, double inlier_threshold, int iterations,
                  int min_points, int use_visibility, double min_spread, int live_before_query, float* poses, float* residual,
                  unsigned char* inliers, int* used, int* inlier_count, float* rmse, int* status, void* stream);
/* xf (G, T, 12) fp64 <- rows 0..2 of pose[g, t] (frame < 0) or of pose[g, t] * pose[g, frame]^-1 (0 <= frame < T; the inverse of a
 * rigid pose is [R^T, -R^T t]), composed in fp64; NaN where status[g, t] != 0 or, with a frame, status[g, frame] != 0. */
int mvt_rigid_compose(const float* poses, const int* status, int G, int T, int frame, double* xf, void* stream);
/* out (T, M, 3) fp32 <- xf[point_objects[m], t] applied to points[m] (M, 3) in fp64, rounded once; NaN for a point of no object
 * (an id outside [0, G)). */
int mvt_rigid_move(const float* points, const int* point_objects, const double* xf, int M, int T, int G, float* out, void* stream);
/* out (T, N, 3) <- pose[g, t] * tracks[r_g, i] (fp64, rounded once) and filled (T, N) bytes <- 1 where track i of object g has
 * status[g, t] == 0, is live (t >= query_frames[i] or live_before_query) and is not visible (MVT_RIGID_FILL_OCCLUDED) or not an
 * inlier (MVT_RIGID_FILL_OUTLIERS); everywhere else the bits of tracks and 0. */
int mvt_rigid_fill(const float* tracks, const unsigned char* visibility, const unsigned char* inliers, const int* query_frames,
                   const int* object_ids, const int* reference_frames, const float* poses, const int* status, int T, int N, int G,
                   int replace, int live_before_query, float* out, unsigned char* filled, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVTRACKER_HIP_H */
