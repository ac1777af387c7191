// Internal interface between gemm.hip, conv_rows.hip and encoder_forward.hip: the plans (conv_plan.h), the one reading place of
// the convolution switches and the launchers of the row-tile kernels.  A launcher takes the plan its caller asked for and launches
// what it says; it does not choose.  Not part of the ABI: hidden symbols.
#pragma once
#include "common.h"
#include "conv_plan.h"

#define MVT_HIDDEN __attribute__((visibility("hidden")))

// MVT_ROWS_NW8 and MVT_FOLD_DOWNSAMPLE as the process first saw them, MVT_CONV_BIG as it is now (conv_rows.hip).
MVT_HIDDEN mvt_plan::ConvSwitches mvt_detail_conv_switches();

// CONV_ROWS / CONV_BIG of plan_conv: 3x3 (pad 1) or 1x1 (pad 0) convolution, stride 1 or 2, Cin % 32 == 0, bf16 mode.
MVT_HIDDEN int mvt_detail_conv_rows(const mvt_plan::ConvPlan& p, const void* in, const unsigned short* w, const float* bias, void* out, int n,
                                    int H, int W, int Cin, int Cout, int ldo, const float* in_stats, float* out_partial, hipStream_t stream);

// plan_down: the stride-2 3x3 convolution of a ResidualBlock together with the block's 1x1 / stride-2 downsample of the same input.
MVT_HIDDEN int mvt_detail_conv3x3s2_down(const mvt_plan::DownPlan& p, const void* in, const unsigned short* w3, const float* b3,
                                         const unsigned short* wd, const float* bd, void* out3, void* outd, int n, int H, int W, int Cin,
                                         int Cout, int ldo, float* part3, float* partd, hipStream_t stream);

// plan_stem / CONV_STEM_ROWS: the input is either the normalised [n][H][W][4] fp32 tensor `in`, or (in == null) the planar clip
// `rgb` (V,T,3,H,W), fp32 or uint8, images rgb_img0 .. rgb_img0 + n - 1 frame-major.
MVT_HIDDEN int mvt_detail_stem7x7_rows_src(const mvt_plan::ConvPlan& p, const float* in, const void* rgb, int rgb_u8, int rgb_V, int rgb_T,
                                           long long rgb_img0, const unsigned short* w, const float* bias, void* out, int n, int H, int W,
                                           int Cout, int ldo, float* out_partial, hipStream_t stream);
