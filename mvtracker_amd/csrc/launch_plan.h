// Launch plans of the updater's block and attention kernels: which kernel form runs, on what grid, and what a form refuses.
// Every threshold of that dispatch is stated here and nowhere else: the entries of block_fused.hip and attention_mfma.hip launch
// what these functions return, updater.hip asks them which forms its launch sequence will take, and the CPU test
// tests/test_launch_plan_host.py compiles this header with the host compiler alone and compares it with the dispatch restatements
// of the exact GPU suites.  Host-only and HIP-free: plain functions of sizes and switch values, no environment reads.
#pragma once
#include <stdint.h>

#include "../../include/mvtracker_hip.h"

// Key-split attention partials in global memory (attention_mfma.hip writes, its merge variants and block_fused.hip's ATT 3 read):
// one record per (split, chunk) = 17 quads x 64 lanes x 4 floats, QUAD-major, so that every access of a wave is one contiguous
// 1-KiB piece (lane-major 68-float records made every load and store of a wave touch 64 different cache lines).  Quad 0 =
// (m[0], m[1], l[0], l[1]); quad 1 + (mb*2 + db)*4 + g = accumulator registers 4g..4g+3 of O^T block (mb, db).
#define MVT_PART_FLOATS (17 * 64 * 4)

namespace mvt_plan {

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// The once-per-process tuning switches of the block kernels, as block_fused.hip reads them from the environment:
// MVT_BLOCK_NMB (nmb_forced, nmb_force = its atoi), MVT_BLOCK_NOSPLIT set, MVT_TIME_NMB1 / MVT_FRAME_NMB1 not 0.
struct BlockSwitches {
  int nmb_force;
  bool nmb_forced, no_split, time_small, frame_small;
};

// One launch of block_fused_bf16<NMB, MODE, ATT> on grid (gx, gy, gz).
struct BlockLaunch {
  int nmb, mode, att;
  unsigned gx, gy, gz;
};
// The launches of one entry call, in order.  ok = false: the form that the sizes select refuses the call (MVT_ERR_ARG, nothing
// launched).  uses_ws: the form keeps x and the MLP partials in the workspace, which must then be 16-byte aligned.
// bmv: rows per tile of the time forms (whole tracks), 0 elsewhere.
struct BlockPlan {
  bool ok, uses_ws;
  int n, bmv;
  BlockLaunch l[2];
};

namespace detail {
inline BlockPlan refused() { return BlockPlan{}; }
inline BlockPlan one(int nmb, int mode, int att, long long gx, long long gy = 1, long long gz = 1, int bmv = 0) {
  BlockPlan p{};
  p.ok = true;
  p.n = 1;
  p.bmv = bmv;
  p.l[0] = BlockLaunch{nmb, mode, att, (unsigned)gx, (unsigned)gy, (unsigned)gz};
  return p;
}
// the two-launch split path: pass 1 <1, 1, att1> over the H / 256 hidden chunks, pass 2 <1, 2, att2> over the column slices of
// the follow-up projections on the SAME tiles (the workspace is tile-native); a deferred pass 2 is left to the consumer
inline BlockPlan split(int att1, int att2, long long gx, int H, int slices, long long gz, bool defer_pass2) {
  BlockPlan p = one(1, 1, att1, gx, H / 256, gz);
  p.uses_ws = true;
  if (!defer_pass2) p.l[p.n++] = BlockLaunch{1, 2, att2, (unsigned)gx, (unsigned)slices, (unsigned)gz};
  return p;
}
}  // namespace detail

// Column slices of pass 2 of the split path (and of the small ln-proj form): 8 column blocks of 32 per workgroup.
inline int pass2_slices(const mvt_block_next* next, int n_next) {
  int maxblk = 1;
  for (int q = 0; q < n_next; ++q) maxblk = (next[q].N + 31) / 32 > maxblk ? (next[q].N + 31) / 32 : maxblk;
  return n_next ? (int)cdiv(maxblk, 8) : 1;
}

// mvt_block_fused_bf16 (attention tensor from memory, or none).
inline BlockPlan plan_block(long long M, int H, bool has_ws, int slices, const BlockSwitches& sw) {
  const int nmb = sw.nmb_forced ? sw.nmb_force : (M >= 4096 ? 2 : 1);  // 64-row workgroups measured 1.6x faster than 128-row ones at M = 12288
  if (nmb == 2) return detail::one(2, 0, 0, cdiv(M, 64));
  if (has_ws && !sw.no_split && M <= 2048 && M % 32 == 0)  // (whole 32-row tiles: the workspace is tile-native)
    return detail::split(0, 0, cdiv(M, 32), H, slices, 1, false);
  return detail::one(1, 0, 0, cdiv(M, 32));
}

// mvt_attn_block_fused_bf16, MVT_ATTN_TIME: tiles of whole tracks, S <= 32 keys per track (one MFMA key block).
// The small-M form: 32-row tiles (S = 12: two whole tracks, 24 rows) while they fit ONE round of workgroups at one per CU -- twice
// the weight bytes in total, half the work per workgroup: a whole updater call 903 -> 819 us at 342 tracks, 932 -> 861 at 448; at
// 512 tracks (288 workgroups) 929 -> 977: not there.  time_small = false: the 64-row tiles everywhere.
inline BlockPlan plan_time(long long M, int S, bool has_ws, const BlockSwitches& sw) {
  if (S < 1 || S > 32 || has_ws) return detail::refused();
  const int b32 = (32 / S) * S, b64 = (64 / S) * S;
  if (sw.time_small && cdiv(M, b32) <= 256) return detail::one(1, 0, 1, cdiv(M, b32), 1, 1, b32);
  return detail::one(2, 0, 1, cdiv(M, b64), 1, 1, b64);
}

// MVT_ATTN_PARTIALS: the attention tile from the key-split partials (64 queries = the virtual tokens, frame = group): split path only.
inline BlockPlan plan_partials(long long M, int S, int H, int n_keys, int n_splits, bool has_ws, bool defer_pass2, int slices) {
  if (n_splits < 1 || n_splits > MVT_ATTN_NSPLIT || n_keys != 64 || M != 64LL * S || !has_ws || M > 2048) return detail::refused();
  return detail::split(3, 5, 2, H, slices, S, defer_pass2);
}

// MVT_ATTN_FRAME over M = ntok * S rows.
// The small-M form (512 tracks per GPU = 6 144 point rows): 32-token tiles.  At 64 tokens per tile the launch is 96 workgroups on 256
// CUs; 192 workgroups of 32 tokens stream twice the weight bytes in total but finish the launch sooner -- a whole updater call
// 929 -> 882 us (tools/time_updater.py 512) -- only while the block has at least 4 096 rows and the 32-token tiles still fit ONE round
// of workgroups at one per CU (680 tracks: 264 workgroups, 927 -> 1 026 us).  frame_small = false: the 64-token tiles.
// Few rows (the 64 virtual tracks): the split path; pass 1 (frame-major tiles, attention recomputed by each of the H / 256 chunk
// workgroups: it is tiny) leaves x and the MLP partials in the workspace by GLOBAL row.
inline BlockPlan plan_frame(long long M, int S, int H, bool has_ws, bool defer_pass2, int slices, const BlockSwitches& sw) {
  const long long ntok = M / S;
  if (ntok * S >= 4096) {
    if (has_ws) return detail::refused();
    if (sw.frame_small && cdiv(ntok, 32) * S <= 256) return detail::one(1, 0, 2, cdiv(ntok, 32), 1, S);
    return detail::one(2, 0, 2, cdiv(ntok, 64), 1, S);
  }
  if (!has_ws || M > 2048 || ntok % 32 != 0) return detail::refused();  // (whole tiles: tile-native workspace)
  return detail::split(2, 5, ntok / 32, H, slices, S, defer_pass2);
}

// MVT_ATTN_FRAME_CTX: per-frame attention whose 64 context tokens are the rows of a split-path block with a deferred pass 2 of
// ctx_chunks hidden chunks; its first workgroups of a frame also evaluate the context block's follow-up projection of ctx_next_N
// columns (0: none), 8 column blocks each.
inline BlockPlan plan_frame_ctx(long long M, int S, int n_keys, bool has_ws, bool defer_pass2, int ctx_chunks, int ctx_next_N) {
  const long long ntok = M / S, tiles = cdiv(ntok, 64);
  if (n_keys != 64 || ntok * S < 4096 || has_ws || defer_pass2 || ctx_chunks < 1 || ctx_chunks > 4) return detail::refused();
  if (ctx_next_N > 0 && (ctx_next_N + 31) / 32 > 8 * tiles) return detail::refused();
  return detail::one(2, 0, 6, tiles, 1, S);
}

// mvt_input_proj_bf16 / mvt_token_input_proj_bf16.
inline BlockPlan plan_input_proj(long long M) { return detail::one(2, 3, 4, cdiv(M, 64)); }

// mvt_ln_proj_bf16.  M >= 4096: whole 64-row tiles, every column block in the workgroup -- x and its LayerNorm are read / computed
// once per tile; else pass 2 of the split path without a workspace.
inline BlockPlan plan_ln_proj(long long M, int slices) {
  return M >= 4096 ? detail::one(2, 3, 0, cdiv(M, 64)) : detail::one(1, 2, 0, cdiv(M, 32), slices);
}

// ---- mvt_attention_bf16 and each segment of mvt_attention_bf16_segmented

enum AttnKernel { ATTN_KEYSPLIT = 0, ATTN_KS4 = 1, ATTN_KS1 = 2 };
// blocks: workgroups along x.  ATTN_KEYSPLIT: one per (group, head, 64-query) chunk, times MVT_ATTN_NSPLIT along y, then the merge.
struct AttnForm {
  AttnKernel kernel;
  long long blocks;
};
// The key-split rule: too few chunks to fill the chip, and at least 512 keys in MVT_ATTN_NSPLIT x whole 32-key blocks, cuts the keys
// over MVT_ATTN_NSPLIT workgroups per chunk as well (needs the partials workspace).
inline AttnForm attn_form(long long groups, int heads, int nq, int nk, bool has_ws) {
  const long long nchunk = groups * heads * cdiv(nq, 64);
  if (nk >= 512 && nchunk < 256 && has_ws && cdiv(nk, 32) % MVT_ATTN_NSPLIT == 0) return {ATTN_KEYSPLIT, nchunk};
  if (nk >= 512 && nchunk < 1024) return {ATTN_KS4, nchunk};
  return {ATTN_KS1, cdiv(nchunk, 4)};
}
// Floats of the key-split workspace of a chunk count, and of the updater's 64-query virtual<-point attention over G query sets.
inline long long attn_partials_floats(long long nchunk) { return (long long)MVT_ATTN_NSPLIT * nchunk * MVT_PART_FLOATS; }
inline long long attn_partials_floats(long long G, long long S, int heads) { return G * attn_partials_floats(S * heads); }

// ---- the per-layer forms of the composite updater call (updater.hip)

constexpr int UPD_HEADS = 6, UPD_DIM_HEAD = 48, UPD_INNER = UPD_HEADS * UPD_DIM_HEAD, UPD_NV = 64, UPD_MLP = 1024;

enum UpdTime { TIME_SEPARATE, TIME_FUSED };
enum UpdV2p { V2P_PLAIN, V2P_PARTIALS, V2P_SEGMENTED };
enum UpdVself { VSELF_SEPARATE, VSELF_FRAME, VSELF_DEFERRED, VSELF_SEGMENTED };
enum UpdP2v { P2V_SEPARATE, P2V_FRAME, P2V_CTX, P2V_SEGMENTED };
struct UpdaterForms {
  UpdTime time;
  UpdV2p v2p;
  UpdVself vself;
  UpdP2v p2v;
};
// n point tracks in G query sets, S frames; fuse_attention: the bits of mvt_updater_weights.  The sets meet only in the three space
// attentions, which run segmented for G > 1; the block kernels whose in-kernel attention has no set dimension then run in their
// separate-launch forms.  Each choice asks the plan of the entry that would run it:
//   time fused:    the time plan takes the call (S <= 32);
//   v2p partials:  the 64-query attention over n keys takes the key-split kernel;
//   p2v frame:     the frame plan of the n * S point rows runs without a workspace (>= 4096 rows);
//   ctx/deferred:  bit 5, both space attentions in their block kernels, the context plan takes the call (>= 4096 point rows, enough
//                  tiles for the next layer's time q|k|v of the virtual rows) and the frame plan would NOT take its 32-token tiles:
//                  there the point<-virtual block runs on twice the workgroups and the virtual-self block keeps its own second
//                  launch (measured faster at 400 / 512 tracks, 958 -> 906 / 929 -> 882 us per call).
inline UpdaterForms updater_forms(int n, int S, int G, int fuse_attention, const BlockSwitches& sw) {
  const bool grouped = G > 1;
  const long long Mp = (long long)n * S, M = Mp + (long long)G * UPD_NV * S;
  const BlockPlan frame = plan_frame(Mp, S, UPD_MLP, false, false, 1, sw);
  const bool fuse_p2v = (fuse_attention & 2) && !grouped, fuse_vs = (fuse_attention & 4) && !grouped;
  const bool fold = (fuse_attention & 32) && fuse_p2v && fuse_vs && frame.ok && frame.l[0].nmb == 2 &&
                    plan_frame_ctx(Mp, S, UPD_NV, false, false, UPD_MLP / 256, 3 * UPD_INNER).ok;
  UpdaterForms f;
  f.time = (fuse_attention & 1) && plan_time(M, S, false, sw).ok ? TIME_FUSED : TIME_SEPARATE;
  f.v2p = grouped ? V2P_SEGMENTED
                  : ((fuse_attention & 16) && attn_form(S, UPD_HEADS, UPD_NV, n, true).kernel == ATTN_KEYSPLIT ? V2P_PARTIALS : V2P_PLAIN);
  f.vself = fold ? VSELF_DEFERRED : (fuse_vs ? VSELF_FRAME : (grouped ? VSELF_SEGMENTED : VSELF_SEPARATE));
  f.p2v = fold ? P2V_CTX : (fuse_p2v && frame.ok ? P2V_FRAME : (grouped ? P2V_SEGMENTED : P2V_SEPARATE));
  return f;
}

}  // namespace mvt_plan
