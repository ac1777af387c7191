"""MVTracker on MI355X: host-side mirror of the reference model's interface.

Same constructor kwargs, ``forward`` signature, result dict and ``state_dict`` keys as
``mvtracker.models.core.mvtracker.mvtracker.MVTracker`` (reference mvtracker.py:93-181, 412-732),
so a Hydra ``_target_`` or a checkpoint can be pointed at this class unchanged.  All arithmetic
runs in libmvtracker_hip.so (see include/mvtracker_hip.h); this file only sequences kernel
launches, owns device buffers and does the per-window bookkeeping on tiny tensors.

Differences from the reference, all result-preserving:
  * every frame is encoded exactly once up front into a frame-major, channels-last "frame store"
    (features + world-space points for the 4 pyramid levels); windows are slices of it, the
    reference's repeat-last-frame padding is a clamped frame index inside the kernels;
  * track state is track-major ([N][S][.]) so the token / delta layouts need no permutes;
  * one host sync per call (the query frame indices), none inside the refinement loop; the NaN
    guard (reference mvtracker.py:401-404) is a device flag read once at the end.
"""
from __future__ import annotations

import logging
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import hip
from .backward import reversed_layout, window_prefixes
from .encoder import EncoderMixin, _ClipImages  # noqa: F401  (_ClipImages: imported from here by tests and tools)
from .frame_store import FrameStoreMixin, nseg
from .grouped import grouped_layout
from .updater import UpdaterMixin
from .weights import WeightsMixin, _insert, _param_epoch, _round_up

log = logging.getLogger(__name__)


def _f32(t, dev):
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _call_outputs(dev, T, N, C):
    """Device-side results of one tracking call: trajectories and visibilities (un-sorted by the window store kernels, zero
    where no window writes), the initial feature rows in sorted order, the deferred NaN flag."""
    return dict(traj=torch.zeros(T, N, 3, device=dev), vis_prob=torch.zeros(T, N, device=dev), vis_logit=torch.zeros(T, N, device=dev),
                feat_init=torch.zeros(N, C, device=dev), nan_flag=torch.zeros(1, device=dev, dtype=torch.int32))


class MVTracker(nn.Module, WeightsMixin, EncoderMixin, UpdaterMixin, FrameStoreMixin):
    """Constructor, state-dict contract, one window's refinement loop, the window loop and the public calls; the packed weights,
    the encoder, the update transformer and the frame store (weights / encoder / updater / frame_store.py) are mixed in."""

    def __init__(
            self,
            sliding_window_len=12,
            stride=4,
            normalize_scene_in_fwd_pass=False,
            fmaps_dim=128,
            add_space_attn=True,
            num_heads=6,
            hidden_size=384,
            space_depth=6,
            time_depth=6,
            num_virtual_tracks=64,
            use_flash_attention=True,
            corr_n_groups=1,
            corr_n_levels=4,
            corr_neighbors=16,
            corr_add_neighbor_offset=True,
            corr_add_neighbor_xyz=False,
            corr_filter_invalid_depth=False,
    ):
        super().__init__()
        if normalize_scene_in_fwd_pass:
            raise NotImplementedError("normalize_scene_in_fwd_pass is broken upstream (mvtracker.py:463-477)")
        if corr_filter_invalid_depth:
            raise NotImplementedError("corr_filter_invalid_depth=True gathers with mismatched indices upstream "
                                      "(mvtracker.py:820-829); only the default False is implemented")
        lanes = fmaps_dim // 8  # lanes of a bf16 feature row: the grouped dots stop their reduction at whole lanes
        if corr_n_groups < 1 or corr_n_groups & (corr_n_groups - 1) or corr_n_groups > lanes:
            raise NotImplementedError(f"corr_n_groups must be a power of two <= fmaps_dim / 8 = {lanes}")
        if not add_space_attn or time_depth != space_depth:
            raise NotImplementedError("only add_space_attn=True with time_depth == space_depth is implemented")
        if fmaps_dim not in (32, 64, 128, 256) or not (1 <= corr_neighbors <= 16) or stride != 4:
            raise NotImplementedError("fmaps_dim in {32,64,128,256}, corr_neighbors <= 16, stride 4")
        self.S = sliding_window_len
        self.stride = stride
        self.latent_dim = fmaps_dim
        self.flow_embed_dim = 64
        self.corr_n_levels = corr_n_levels
        self.corr_neighbors = corr_neighbors
        # correlation features per neighbour (mvtracker.py:136-141): grouped dots, neighbour offset, neighbour coordinates
        self.corr_n_groups = corr_n_groups
        self.corr_add_neighbor_offset = bool(corr_add_neighbor_offset)
        self.corr_add_neighbor_xyz = bool(corr_add_neighbor_xyz)
        self.corr_width = corr_n_groups + 3 * int(self.corr_add_neighbor_offset) + 3 * int(self.corr_add_neighbor_xyz)
        self.num_heads = num_heads
        self.dim_head = 48
        self.hidden = hidden_size
        self.depth = time_depth
        self.nv = num_virtual_tracks
        self.use_flash_attention = use_flash_attention  # accepted for config compatibility; same math
        self.updateformer_input_dim = (self.flow_embed_dim + 1) * 3 + corr_neighbors * corr_n_levels * self.corr_width + fmaps_dim + 2
        self.out_dim = 3 + fmaps_dim
        for key, shape in self._shapes().items():
            _insert(self, key, self._init_tensor(key, shape))
        self._packed: Optional[dict] = None
        self._packed_sig = None
        self._plist = None
        self._plist_epoch = -1
        self._slot_cache = {}
        # arithmetic of the matrix-core kernels (convs + linears); everything else is always fp32:
        #   "fp32"   v_mfma_f32_32x32x2_f32, exact fp32 FMA chains
        #   "bf16x3" split-precision bf16 MFMA (hi*hi + hi*lo + lo*hi), fp32-grade results, ~5x the fp32 MFMA rate
        #   "bf16"   operands rounded to bf16, fp32 accumulate (the arithmetic of torch autocast in the reference demo)
        self.precision = os.environ.get("MVT_PRECISION", "fp32")
        self.fuse_mlp = True
        self.fuse_blocks = True
        self.mfma_attention = True
        self.overlap_encoder = os.environ.get("MVT_OVERLAP", "1") != "0"  # encode later frames on a second stream
        self._side = {}
        self._scratch = {}
        self.bf16_tokens = os.environ.get("MVT_BF16_TOK", "1") != "0"  # bf16 mode: q/k/v and attention outputs stored as bf16
        self.bf16_activations = os.environ.get("MVT_BF16_ACT", "1") != "0"  # bf16 mode: encoder activations stored as bf16
        self.bf16_store = os.environ.get("MVT_BF16_STORE", "1") != "0"  # bf16 mode: bf16 feature rows in the frame store
        # attention inside the block kernels: bit 0 time, bit 1 point<-virtual, bit 2 virtual self; bit 4: the virtual<-point block
        # combines the key-split partials in its prologue, no merge launch; bit 5: the virtual-self block's pass 2 inside the
        # point<-virtual block.  Bits 4 / 5 are bit-identical to the launches they replace; bits 0-2 agree with the separate attention
        # launches to bf16 rounding only (single-pass softmax, block-diagonal time attention: round 3)
        self.fuse_attention = int(os.environ.get("MVT_FUSE_ATTN", "55"))
        self.seed_across_windows = os.environ.get("MVT_SEED_WINDOWS", "1") != "0"  # previous window's neighbours seed the first scan
        self.encoder_chunk_images = int(os.environ.get("MVT_ENC_CHUNK", "0"))  # images per encoder call (0: max(16, V * S/2))
        self.encoder_streams = int(os.environ.get("MVT_ENC_STREAMS", "2"))  # 2: the chunks of an encoder call alternate between two streams
        self.presearch = os.environ.get("MVT_PRESEARCH", "1") != "0"  # first searches of new tracks beside the first encoder block
        self.stem_reads_clip = os.environ.get("MVT_STEM_RGB", "1") != "0"  # composite encoder: the stem reads the planar clip itself
        # the wide conv2 as one 512-thread workgroup per CU (conv3x3_big_bf16) also for the encoder blocks that run on the second
        # stream BESIDE the refinement windows: "0" never (its ~100-us workgroups starve the windows' kernels -- above all the
        # latency-bound correlation gather -- of CU slots), "1" always, "auto": when the encoder, not the windows, bounds the call
        # (the second stream has more than twice the images of the first block; BASELINE config C5: -6 % per step)
        self.wide_conv_shared = os.environ.get("MVT_CONV_BIG_SHARED", "auto")
        self._shared_gpu = False  # set around the encoder calls issued beside the windows (``_beside_windows``)
        # MVT_SYNC_DEBUG=1: synchronise the whole device at every cross-stream hand-over of a call ("hand-over
        # table"): if results change with it, an event / wait_stream is missing somewhere (tests: bit-identical with and without)
        self.sync_debug = os.environ.get("MVT_SYNC_DEBUG", "0") != "0"
        self.composite_encoder = os.environ.get("MVT_COMPOSITE_ENCODER", "1") != "0"  # the CNN as one library call (bf16 mode)
        self.fuse_tokens = os.environ.get("MVT_FUSE_TOKENS", "1") != "0"  # ... with the token rows assembled inside that launch
        self.fuse_input = os.environ.get("MVT_FUSE_INPUT", "1") != "0"  # input transform + virtual tokens + first q|k|v in one launch
        self.fuse_head = os.environ.get("MVT_FUSE_HEAD", "1") != "0"  # flow head + track / feature update in one kernel
        self.fuse_norm = True  # InstanceNorm statistics from the conv epilogue + normalise-on-load (bf16 / bf16x3 convs)
        self.fold_downsample = os.environ.get("MVT_FOLD_DOWNSAMPLE", "1") != "0"  # strided blocks: conv1 + downsample[0] in one launch
        d = self.updateformer_input_dim
        self._time_embed_host = self._make_time_embed(self.S, d)

    # ------------------------------------------------------------------ parameters
    def _shapes(self) -> Dict[str, Tuple[int, ...]]:
        """state_dict contract."""
        s: Dict[str, Tuple[int, ...]] = {}

        def wb(name, *shape):
            s[name + ".weight"] = tuple(shape)
            s[name + ".bias"] = (shape[0],)

        wb("fnet.conv1", 64, 3, 7, 7)
        cin = 64
        for li, cout in ((1, 64), (2, 96), (3, 128), (4, 128)):
            wb(f"fnet.layer{li}.0.conv1", cout, cin, 3, 3)
            wb(f"fnet.layer{li}.0.conv2", cout, cout, 3, 3)
            if li != 1:
                wb(f"fnet.layer{li}.0.downsample.0", cout, cin, 1, 1)
            wb(f"fnet.layer{li}.1.conv1", cout, cout, 3, 3)
            wb(f"fnet.layer{li}.1.conv2", cout, cout, 3, 3)
            cin = cout
        wb("fnet.conv2", self.latent_dim * 2, 416, 3, 3)
        wb("fnet.conv3", self.latent_dim, self.latent_dim * 2, 1, 1)
        h, inner, mlp = self.hidden, self.num_heads * self.dim_head, int(self.hidden * 4.0)
        u = "updateformer."
        s[u + "virual_tracks"] = (1, self.nv, 1, h)
        wb(u + "input_transform", h, self.updateformer_input_dim)
        wb(u + "flow_head.0", self.out_dim, h)
        wb(u + "flow_head.2", self.out_dim, self.out_dim)
        wb(u + "flow_head.4", self.out_dim, self.out_dim)
        for i in range(self.depth):
            for blk, attn in (("time_blocks", "attn"), ("space_virtual_blocks", "attn"),
                              ("space_point2virtual_blocks", "cross_attn"), ("space_virtual2point_blocks", "cross_attn")):
                p = f"{u}{blk}.{i}"
                if attn == "cross_attn":
                    s[p + ".norm_context.weight"] = (h,)
                    s[p + ".norm_context.bias"] = (h,)
                wb(f"{p}.{attn}.to_q", inner, h)
                wb(f"{p}.{attn}.to_kv", 2 * inner, h)
                wb(f"{p}.{attn}.to_out", h, inner)
                wb(p + ".mlp.fc1", mlp, h)
                wb(p + ".mlp.fc2", h, mlp)
        s["ffeats_norm.weight"] = (self.latent_dim,)
        s["ffeats_norm.bias"] = (self.latent_dim,)
        wb("ffeats_updater.0", self.latent_dim, self.latent_dim)
        wb("vis_predictor.0", 1, self.latent_dim)
        return s

    @staticmethod
    def _init_tensor(key: str, shape) -> torch.Tensor:
        t = torch.zeros(shape)
        if key.endswith("virual_tracks"):
            return torch.randn(shape)
        if key.endswith(".bias"):
            return t
        if "norm" in key.split(".")[-2]:
            return torch.ones(shape)
        if key.startswith("fnet."):
            nn.init.kaiming_normal_(t, mode="fan_out", nonlinearity="relu")
        elif "flow_head" in key:
            nn.init.trunc_normal_(t, std=0.001)
        else:
            nn.init.xavier_uniform_(t)
        return t

    @staticmethod
    def _make_time_embed(S: int, D: int) -> torch.Tensor:
        """1-D sin|cos embedding of s/S, fp64 on the host, first D of D+D%2 columns (mvtracker.py:333-344)."""
        dim = D + (D % 2)
        omega = np.arange(dim // 2, dtype=np.float64)
        omega /= dim / 2.0
        omega = 1.0 / 10000 ** omega
        pos = (torch.linspace(0, S - 1, S).reshape(S, 1) / S).numpy().reshape(-1)
        out = np.einsum("m,d->md", pos, omega)
        return torch.from_numpy(np.concatenate([np.sin(out), np.cos(out)], axis=1)).float()[:, :D].contiguous()

    def register_parameter(self, name, param):
        _param_epoch[0] += 1
        super().register_parameter(name, param)

    def init_stats(self):  # reference API (mvtracker.py:190-242); statistics are not collected here
        pass

    def consume_stats(self):
        pass

    # ------------------------------------------------------------------ one window (mvtracker.py:244-410)
    @hip.guarded
    def refine_window(self, store, frame0, coords, vis_init, track_mask, feat_init, iters=4, nan_flag=None, trace=None):
        """Iterative refinement of one window (test / parity entry; ``forward`` prepares the same state with one kernel).

        coords (n,S,3) world xyz, vis_init (n,S) logits, track_mask (n,S) {0,1}, feat_init (n,S,C).  Window slot s reads
        frame min(frame0+s, T-1).  Returns (list of coords per iteration, vis logits (n,S))."""
        coords = coords.contiguous().clone()
        ffeats = feat_init.contiguous().clone()
        mask_vis = torch.stack([track_mask.float(), vis_init.float()], dim=2).contiguous()
        return self._refine(store, frame0, coords, ffeats, mask_vis, iters, nan_flag, trace)[:2]

    def _refine(self, store, frame0, coords, ffeats, mask_vis, iters=4, nan_flag=None, trace=None, carry=None, pre_idx=None, seg=None,
                frame_step=1, after_first_corr=None):
        """The refinement loop (mvtracker.py:350-408) on prepared state: coords (n,S,3) and ffeats (n,S,C) are updated IN PLACE,
        mask_vis (n,S,2) = (track mask, initial visibility logit).  Returns ([coords per traced iteration ..., final], vis,
        neighbour indices (L,n,S,K) of the last iteration).
        ``carry`` = (those indices of the previous window, p0): the first p0 tracks continue from that window, so its neighbours
        seed (bound) this window's first exact scan.
        ``frame_step``: slot s reads store frame clamp(frame0 + s * frame_step, 0, T-1); -1 is the time-reversed pass of backward
        tracking (the seeding above works in slot space and is the same in both directions).
        ``after_first_corr``: host callback, called once right behind the first correlation launch (``_plan_frame_store``)."""
        S, C, K, L, E = self.S, self.latent_dim, self.corr_neighbors, self.corr_n_levels, self.flow_embed_dim
        n = coords.shape[0]
        dev = coords.device
        pk = self._pack(dev)
        D = self.updateformer_input_dim
        # a ring store (streaming) is read through the ring forms of the same entries: ``T`` is then its (base, R, lo, hi)
        ring = store.get("ring")
        T = store["T"] if ring is None else ring
        knn_search_levels, corr_gather_dot, corr_gather_dot_opts = (
            (hip.knn_search_levels, hip.corr_gather_dot, hip.corr_gather_dot_opts) if ring is None else
            (hip.knn_search_levels_ring, hip.corr_gather_dot_ring, hip.corr_gather_dot_opts_ring))
        Fc = L * K * self.corr_width
        default_corr = self.corr_n_groups == 1 and self.corr_add_neighbor_offset and not self.corr_add_neighbor_xyz
        pos = torch.empty(n, D, device=dev)
        hip.pos_embed(coords, n, S, D, _round_up(D, 6), pos, pk["pos_omega"])
        fcorr = torch.empty(n, S, Fc, device=dev)
        ldx = _round_up(D, 4)
        x = torch.empty(n * S, ldx, device=dev)      # (token_assemble writes the pad columns as zeros)
        ldd = _round_up(self.out_dim, 4)
        delta = torch.empty(n * S, ldd, device=dev)  # (out_dim columns are written and read; the pad column is never read)
        dn = torch.empty(n * S, C, device=dev)
        # neighbour indices of every level: returned for tracing AND used to seed (prune) the next exact scan
        # (``pre_idx``: the same buffer with the NEW tracks' rows of the first iteration already searched -- forward runs those
        #  unseeded searches, which depend on the query points and the geometry only, on the second stream beside the encoder)
        idx = pre_idx if pre_idx is not None else torch.empty(L, n, S, K, device=dev, dtype=torch.int32)
        assert tuple(idx.shape) == (L, n, S, K)
        preds = []
        if trace is not None:  # the state every iteration's search / correlation starts from (teacher-forced parity checks)
            trace["coords_in"], trace["ffeats_in"] = coords.clone(), ffeats.clone()
        levels =[dict(xyz=store["xyz"][lvl], P=store["P"][lvl], seed_idx=idx[lvl], box=store["box"][lvl],
                       grid=store["tile_grid"][lvl], idx_out=idx[lvl], gbox=store["gbox"][lvl]) for lvl in range(L)]
        for it in range(iters):
            if it > 0:
                # every level is seeded by its own previous neighbours: the four scans are independent -> one launch
                knn_search_levels(levels, coords, n, S, frame0, frame_step, T, K, seed_k=K)
            else:
                n0 = 0
                if carry is not None and carry[1] > 0 and self.seed_across_windows:
                    # Tracks carried over from the previous window (mvtracker.py:648-651 start them at its last estimates): that
                    # window's final neighbours -- slot s continues slot s + S/2, the last slot held -- are K distinct points of
                    # every frame's cloud (same pixel grid), i.e. an exact upper bound of the K-th distance, and a tight one; all
                    # four levels in one seeded launch instead of four coarse-to-fine scans.  Exactness is unaffected.
                    prev_idx, n0 = carry
                    # (cached on the device: building it from a Python list is a synchronous host-to-device copy -- the host,
                    #  several milliseconds ahead of the GPU, would stall here until the stream drains)
                    slot = self._slot_cache.get((S, dev))
                    if slot is None:
                        slot = self._slot_cache[(S, dev)] = torch.tensor([min(s_ + S // 2, S - 1) for s_ in range(S)], device=dev)
                    seed_t = prev_idx[:, :n0].index_select(2, slot).contiguous()
                    lv0 = [dict(lv, seed_idx=seed_t[l_], idx_out=idx[l_][:n0]) for l_, lv in enumerate(levels)]
                    knn_search_levels(lv0, coords, n0, S, frame0, frame_step, T, K, seed_k=K)
                # rows [n1, n) were searched ahead of time (``pre_idx``: the tracks that enter at this window, i.e. everything behind the
                # carried ones); rows [n0, n1) still need their first, unseeded search -- empty unless the carried tracks were not seeded
                # from the previous window (``seed_across_windows`` off)
                n1 = n if pre_idx is None else (carry[1] if carry is not None else 0)
                if n0 < n1:
                    # new tracks: all four levels in ONE unseeded launch (every search starts from the farthest-corner bound of the
                    # nearest full tile) -- 262 us against four dependent coarse-to-fine launches of ~100 us each
                    lv1 = [dict(lv, seed_idx=None, idx_out=idx[l_][n0:n1]) for l_, lv in enumerate(levels)]
                    knn_search_levels(lv1, coords[n0:n1], n1 - n0, S, frame0, frame_step, T, K, seed_k=0)
            if default_corr:
                corr_gather_dot(store["xyz"], store["fvec"], store["P"], [idx[lvl] for lvl in range(L)], C, ffeats, coords, n, S, frame0,
                                frame_step, T, K, fcorr, Fc, 0)
            else:  # the reference's non-default correlation layouts (grouped dots, no offsets, neighbour coordinates)
                corr_gather_dot_opts(store["xyz"], store["fvec"], store["P"], [idx[lvl] for lvl in range(L)], C, ffeats, coords, n, S,
                                     frame0, frame_step, T, K, self.corr_n_groups, self.corr_add_neighbor_offset, self.corr_add_neighbor_xyz,
                                     fcorr, Fc, 0)
            if it == 0 and after_first_corr is not None:  # (forward: the later frame blocks' encoder starts on the second stream now)
                after_first_corr()
            if (trace is None and "updater_struct" in pk and self.fuse_head and self.fuse_input and self.fuse_tokens
                    and pk["updater_struct"].input_frag.w):
                # everything after the correlation in ONE library call: token rows assembled inside the updater's first kernel,
                # the transformer, flow head and track / feature update (no token matrix, no delta tensor in HBM)
                self._composite_call("updateformer_forward_tokens", "updateformer_forward_tokens_grouped", n, seg, pk,
                                     (coords, fcorr, Fc, ffeats, C, mask_vis, pos, pk["time_embed"], E), None, ldd, (coords, ffeats, nan_flag))
                continue
            hip.token_assemble(coords, fcorr, Fc, ffeats, C, mask_vis, pos, pk["time_embed"], n, S, E, x, ldx)
            # (the delta tensor itself only leaves the fused head for tracing)
            updated = self._update_former(pk, x, ldx, n, delta if trace is not None else None, ldd, coords, ffeats, nan_flag, seg=seg) \
                if "updater_struct" in pk and self.fuse_head else self._update_former(pk, x, ldx, n, delta, ldd, seg=seg)
            if trace is not None:
                trace.setdefault("knn_idx", []).append(idx.clone())
                trace.setdefault("fcorrs", []).append(fcorr.clone())
                trace.setdefault("tokens", []).append(x[:, :D].reshape(n, S, D).clone())
                trace.setdefault("delta", []).append(delta[:, :self.out_dim].reshape(n, S, -1).clone())
            if not updated:
                hip.delta_split(delta, ldd, pk["ffeats_norm"].w, pk["ffeats_norm"].b, coords, dn, n * S, C, nan_flag)
                self._lin(pk, "ffeats_updater.0", dn, C, n * S, ffeats, C, hip.ACT_GELU_ERF, R=ffeats, ldr=C)
            if trace is not None:  # (the intermediate estimates only feed the training loss upstream)
                preds.append(coords.clone())
                trace.setdefault("coords_iters", []).append(preds[-1])
                trace.setdefault("ffeats_iters", []).append(ffeats.clone())
        if trace is None:
            preds.append(coords)
        vis = torch.empty(n, S, device=dev)
        hip.rowdot(ffeats, C, pk["vis"].w, pk["vis"].b, vis, n * S, C)
        if trace is not None:
            trace["ffeats"] = ffeats
        return preds, vis, idx

    # ------------------------------------------------------------------ forward (mvtracker.py:412-732)
    def _normalise_inputs(self, rgbs, depths, intrs, extrs, is_train, logging_hooks):
        """What ``forward`` and ``forward_grouped`` check and convert alike: inference only, the reference's logging hooks ignored,
        batch size 1.  Returns the clip without its batch dimension on the device: depths / intrs / extrs fp32 and contiguous, rgbs
        fp32 or uint8."""
        if is_train:
            raise NotImplementedError("inference only: the MI355X path has no backward")
        if logging_hooks:
            log.warning("save_debug_logs / save_rerun_logs are host-side visualisation hooks of the reference; ignored")
        batch_size, num_views, num_frames, _, height, width = rgbs.shape
        assert rgbs.shape == (batch_size, num_views, num_frames, 3, height, width)
        assert depths.shape == (batch_size, num_views, num_frames, 1, height, width)
        assert intrs.shape == (batch_size, num_views, num_frames, 3, 3)
        assert extrs.shape == (batch_size, num_views, num_frames, 3, 4)
        assert batch_size == 1, "Batch size > 1 is not supported yet"
        hip.require_device(rgbs)
        dev = rgbs.device
        # (uint8 frames -- the sample files' storage type -- stay uint8: the encoder's first kernel converts them)
        rgbs = rgbs[0].to(dev).contiguous() if rgbs.dtype == torch.uint8 else _f32(rgbs[0], dev)
        return rgbs, _f32(depths[0], dev), _f32(intrs[0], dev), _f32(extrs[0], dev)

    def _feat_init_scan(self, store, frames, qxyz, a0, a1, keys_for=None):
        """Scan half of the feature init (mvtracker.py:607-645: 1-NN in the level-0 cloud of each row's query frame) for rows
        [a0, a1) of ``qxyz`` (device).  ``frames`` (host) holds the rows' query frames, equal frames in runs: one ``knn_scan`` with
        K = 1 per run.  Yields (a, b, frame, keys) run by run, so that a consumer can gather right behind each scan.  ``keys_for``:
        the stream that will consume the keys, when they are allocated under another one."""
        P0 = store["P"][0]
        ns = nseg(P0, 1)
        cuts = [a0, *(a0 + 1 + np.flatnonzero(np.diff(frames[a0:a1]))).tolist(), a1] if a1 > a0 else [a0]
        for a, b in zip(cuts[:-1], cuts[1:]):
            t = int(frames[a])
            keys = torch.empty((b - a) * ns, device=qxyz.device, dtype=torch.int64)
            if store.get("ring") is None:
                hip.knn_scan(store["xyz"][0], P0, qxyz[a:b], b - a, 1, t, 0, store["T"], 1, ns, keys, box=store["box"][0],
                             grid=store["tile_grid"][0])
            else:
                hip.knn_scan_ring(store["xyz"][0], P0, qxyz[a:b], b - a, 1, t, 0, store["ring"], 1, ns, keys, box=store["box"][0],
                                  grid=store["tile_grid"][0])
            if keys_for is not None:
                keys.record_stream(keys_for)
            yield a, b, t, keys

    def _feat_init_gather(self, store, groups, feat):
        """Gather half of the feature init: the feature row of each scanned key into rows [a, b) of ``feat``."""
        P0 = store["P"][0]
        ns = nseg(P0, 1)
        for a, b, t, keys in groups:
            if store.get("ring") is None:
                hip.knn1_gather(store["fvec"][0], P0, self.latent_dim, keys, b - a, ns, t, feat[a:b])
            else:
                hip.knn1_gather_ring(store["fvec"][0], P0, self.latent_dim, keys, b - a, ns, t, store["ring"], feat[a:b])

    def _feat_init(self, store, frames, qxyz, a0, a1, feat):
        self._feat_init_gather(store, self._feat_init_scan(store, frames, qxyz, a0, a1), feat)

    def _presearch(self, st, windows, frames, qxyz, pre):
        """Everything of the call that needs the point clouds but no features: the first, UNSEEDED neighbour search of the tracks
        that enter at each window (their coordinates are the query points, mvtracker.py:505-511) and the 1-NN scans of the
        feature init (:607-645).  Issued on the second stream between the geometry and the encoder of the first window's frames,
        so these searches (~0.4 ms at C3, latency-bound gathers) run beside the convolutions instead of after them.
        Fills ``pre``: window start -> (neighbour buffer with the new tracks' first search done, 1-NN keys per query-frame run,
        the searched coordinates), and "event" -> what the main stream waits for before it uses any of them."""
        dev = qxyz.device
        if dev.type != "cuda" or not self.presearch:
            return
        S, K, L, T = self.S, self.corr_neighbors, self.corr_n_levels, st["T"]
        side = self._side_stream(dev)
        main_s = torch.cuda.current_stream(dev)
        # hand-over H4: point clouds / tile boxes / sorted query rows (all enqueued on the caller's stream BEFORE the geometry event)
        side.wait_stream(main_s) if "geo_event" not in st else side.wait_event(st["geo_event"])
        self._handover(dev)
        with torch.cuda.stream(side):
            q0 = 0
            for ww, q1 in windows:
                if q1 > q0:
                    m = q1 - q0
                    idxb = torch.empty(L, q1, S, K, device=dev, dtype=torch.int32)
                    c0 = qxyz[q0:q1, None, :].expand(m, S, 3).contiguous()
                    lv = [dict(xyz=st["xyz"][l], P=st["P"][l], seed_idx=None, box=st["box"][l], grid=st["tile_grid"][l],
                               idx_out=idxb[l][q0:], gbox=st["gbox"][l]) for l in range(L)]
                    hip.knn_search_levels(lv, c0, m, S, ww, 1, T, K, seed_k=0)
                    # (keys allocated under the second stream, consumed on the caller's)
                    groups = list(self._feat_init_scan(st, frames, qxyz, q0, q1, keys_for=main_s))
                    idxb.record_stream(main_s)
                    pre[ww] = (idxb, groups, c0)
                q0 = q1
            ev = torch.cuda.Event()
            ev.record(side)
        pre["event"] = ev

    def _plan_frame_store(self, rgbs, depths, intrs, extrs, geometry, frame_store, windows, backward, after_first_chunk):
        """Where the call's frame features come from: a supplied store, the whole clip encoded up front, or the first window's
        frames now and the rest on the second stream.  Returns (store, pending, pending_back, start_side_encoder): (first frame,
        event) of the feature blocks in flight that the forward windows / only the reversed pass read, and the host callback that
        starts the second stream's encoder (None when there is none to start).  ``after_first_chunk(store)`` is called as soon as
        the first encoder chunk of a store built here has been enqueued."""
        S, T = self.S, rgbs.shape[1]
        if frame_store is not None:
            # (first frame, event) of feature blocks still in flight
            return frame_store, list(frame_store.get("pending", ())) if windows else [], [], None
        if not windows:  # every query within the clip's last S/2 frames: only a reversed pass needs a store
            return (self.build_frame_store(rgbs, depths, intrs, extrs, t0=0, geometry=geometry) if backward else None), [], [], None
        w = max(windows[0][0], 0)
        if not self.overlap_encoder or w + S >= T or rgbs.device.type != "cuda":
            store = self.build_frame_store(rgbs, depths, intrs, extrs, t0=0 if backward else w, after_geometry=after_first_chunk,
                                           geometry=geometry)
            return store, [], [], None
        # The first window needs frames [w, w+S).  The remaining frames are encoded on a second HIP stream while
        # the updater of the earlier windows runs: its kernels over the 64 virtual tracks fill a fraction of the
        # CUs, the encoder's convolutions take the rest.
        ready = w + S
        store = self.build_frame_store(rgbs, depths, intrs, extrs, t0=w, t1=ready, after_geometry=after_first_chunk, geometry=geometry)
        later = list(range(ready, T, S // 2))  # first frames of the S/2-frame blocks still to encode
        # backward tracking reads the frames before the first forward window too: first frames of the S/2-frame blocks of [0, w)
        early = list(range(0, w, S // 2)) if backward else []
        pending, pending_back = [], []

        def start_side_encoder():
            # started by the first window BEHIND its first correlation launch (``_refine`` calls it): the first kernels
            # of that window -- feature init, window state, the first correlation gather -- are latency-bound and otherwise
            # start in the same instant as the second stream's first convolutions
            self._encode_on_side_stream(store, rgbs, later, pending)
            if early:  # the frames only the reversed pass reads, BEHIND the forward pass's blocks (hand-over H3)
                self._encode_on_side_stream(store, rgbs, early, pending_back, end=w)

        return store, pending, pending_back, start_side_encoder

    def _run_windows(self, store, windows, frame0s, frame_step, rows, order, out, iters, trace, before=None, store_slots=True,
                     enter_frames=None, pre=None, pending=(), after_first_corr=None, carry=None, T=None):
        """One pass of the reference's window loop (mvtracker.py:537-695) over ``windows`` = [(start, active prefix), ...], slot s
        of window i reading store frame clamp(frame0s[i] + s * frame_step, 0, T-1).  The pass supplies data only: ``rows`` = (query
        xyz, query frames, initial feature rows) in the pass's sorted order on the device, ``order`` = the position of each sorted
        row in the caller's query list (the un-sort of the result store), ``before`` = an optional per-row frame bound of the result
        store (the reversed pass's query frames: it writes only the frames before them).  ``out``: the call's result tensors.
        Forward pass only: ``enter_frames`` (host query frames: the feature rows of the tracks that enter a window are initialised
        there), ``pre`` (``_presearch``), ``pending`` ((first frame, event) of the feature blocks in flight on the second stream, in
        frame order), ``after_first_corr`` (``_refine``, first window).  Returns the windows run.
        Streaming (``mvtracker_amd.streaming``) runs the loop a few windows at a time: ``carry`` is a dict that holds what one window
        hands to the next (p0, coords, vis, prev_idx, w) between calls, ``T`` the clip length as far as it is known (``out`` then only
        needs the NaN flag), and with ``store_slots`` False the session stores the carried window's slots itself."""
        S, C = self.S, self.latent_dim
        qxyz, qt_d, feat = rows
        dev = qxyz.device
        if T is None:
            T = out["traj"].shape[0]
        pre = {} if pre is None else pre
        done = []
        p0 = 0
        coords = vis = prev_idx = None
        if carry:
            p0, coords, vis, prev_idx = carry["p0"], carry["coords"], carry["vis"], carry["prev_idx"]
        for (w, p1), f0 in zip(windows, frame0s):  # mvtracker.py:537; p1 = number of queries with t < w+S (:538-540)
            assert p1 > 0
            while pending and pending[0][0] < w + S:  # the frames this window reads must have left the encoder
                torch.cuda.current_stream(dev).wait_event(pending.pop(0)[1])  # hand-over H5: feature rows encoded on the second stream
                self._handover(dev)
            if "event" in pre:  # the searches issued ahead of time on the second stream
                torch.cuda.current_stream(dev).wait_event(pre.pop("event"))  # hand-over H6: neighbour buffers / 1-NN keys (record_stream'd)
                self._handover(dev)
            pre_w = pre.get(w)
            if p1 > p0 and enter_frames is not None:
                if pre_w is not None:  # feature init from the 1-NN keys scanned ahead of time
                    self._feat_init_gather(store, pre_w[1], feat)
                else:
                    self._feat_init(store, enter_frames, qxyz, p0, p1, feat)
            # window state in one launch: carry-over of coords / visibility LOGITS from the previous window (:648-655), track mask
            # (:505-507, :695; the repeat-last-frame padding of :598-604 is a clamped frame index), features repeated over S (:645)
            wc = torch.empty(p1, S, 3, device=dev)
            wf = torch.empty(p1, S, C, device=dev)
            wm = torch.empty(p1, S, 2, device=dev)
            hip.window_prepare(qxyz, qt_d, feat, coords, vis, p1, p0, S, C, f0, T, wc, wm, wf, frame_step=frame_step)
            wtrace = None
            if trace is not None:
                wtrace = {} if frame_step > 0 else dict(reversed_window=w)
                trace.append(wtrace)
            preds, vis, prev_idx = self._refine(store, f0, wc, wf, wm, iters=iters, nan_flag=out["nan_flag"], trace=wtrace,
                                                carry=(prev_idx, p0) if p0 > 0 else None, pre_idx=pre_w[0] if pre_w is not None else None,
                                                frame_step=frame_step, after_first_corr=after_first_corr)
            after_first_corr = None
            coords = preds[-1]
            # :692-693, un-sorted (:710-711); the reversed pass writes only frames before each row's query frame
            if store_slots:
                hip.window_store(coords, vis, order, p1, S, f0, T, out["traj"].shape[1], out["traj"], out["vis_logit"], out["vis_prob"],
                                 frame_step=frame_step, before=before)
            done.append((w, p1))
            p0 = p1
            if carry is not None:
                carry.update(p0=p0, coords=coords, vis=vis, prev_idx=prev_idx, w=w)
        return done

    @torch.no_grad()
    @hip.guarded
    def forward(
            self,
            rgbs,
            depths,
            query_points,
            intrs,
            extrs,
            iters=4,
            image_features=None,
            is_train=False,
            save_debug_logs=False,
            debug_logs_path="",
            save_rerun_logs: bool = False,
            save_rerun_logs_output_rrd_path: Optional[str] = None,
            frame_store: Optional[dict] = None,
            trace: Optional[list] = None,
            backward_tracking: bool = False,
            **kwargs,
    ):
        """``backward_tracking``: also fill the frames BEFORE each query's frame, from a time-reversed pass over the same frame store
        (``mvtracker_amd.backward``).  Frames from the query frame on are the same bits with the option on or off.
        The reversed pass's windows are left in ``last_windows_backward`` as (start in reversed time, active tracks)."""
        rgbs, depths, intrs, extrs = self._normalise_inputs(rgbs, depths, intrs, extrs, is_train, save_debug_logs or save_rerun_logs)
        N = query_points.shape[1]
        assert query_points.shape == (1, N, 4)
        dev = rgbs.device
        T, S, C = rgbs.shape[1], self.S, self.latent_dim
        query_points = _f32(query_points[0], dev)

        # ---- the one host sync of the call: integer query frames (mvtracker.py:489, truncation toward zero).  The read-back is
        # asynchronous (pinned buffer + event) and the query-independent geometry kernels are enqueued BEHIND it before the host
        # waits: in back-to-back calls the host wakes up when the previous call's last kernel ends, and the GPU then has the
        # geometry to run while the host enqueues the first encoder block (the kernel trace showed ~0.3 ms of idle GPU there)
        qt_dev = query_points[:, 0].long()
        geometry = None
        if dev.type == "cuda":
            qt_pin = self._pinned_i64(dev, N)
            qt_pin.copy_(qt_dev, non_blocking=True)
            ev_q = torch.cuda.Event()
            ev_q.record(torch.cuda.current_stream(dev))
            if frame_store is None:
                geometry = self.store_geometry(depths, intrs, extrs)
            ev_q.synchronize()
            qt = qt_pin.numpy().copy()
        else:
            qt = qt_dev.cpu().numpy()

        # ---- host layout: sort order, the windows of both passes, one small upload
        order = np.argsort(qt, kind="stable")  # mvtracker.py:514 (order among equal t is unobservable)
        qt_s = qt[order]
        fwd = window_prefixes(qt_s, S, T)  # the reference's loop (:537-540) as [(window start, active prefix), ...]
        # backward tracking: the reversed pass's rows and windows, known on the host from here on (their index arrays ride in the same
        # upload); ``back`` stays None when no reversed window runs, and the call is then the plain forward
        back = reversed_layout(qt, S, T) if backward_tracking else None
        if back is not None and not back["windows"]:
            back = None
        small = [order.astype(np.int64), qt_s.astype(np.int32)]
        fix_rows = np.zeros(0, dtype=np.int64)
        if back is not None:
            # rows of feat_init (sorted by query frame) that only the reversed pass reaches take that pass's feature row
            inv_b = np.empty(N, dtype=np.int64)
            inv_b[back["order"]] = np.arange(N)
            tail = np.arange(fwd[-1][1] if fwd else 0, N)
            fix_rows = tail[inv_b[order[tail]] < back["active"]]
            small += [back["order"].astype(np.int64), back["sorted_qt"].astype(np.int32)]
            if len(fix_rows):
                small += [fix_rows, inv_b[order[fix_rows]]]
        # (the tiny host-to-device copies go first, while the GPU is idle anyway, through a cached PINNED staging buffer,
        #  asynchronously: from pageable memory each copy is a host-blocking staged transfer that waits until the stream has drained
        #  -- ~60 us of idle GPU apiece in the kernel trace, milliseconds after the first encoder chunk.  The buffer may be rewritten
        #  by the next call: its host sync above comes after these copies in stream order)
        small_d = self._upload_small(dev, *small)
        order_d, qt_sd = small_d[:2]
        # (N,3) query points sorted by start frame -- enqueued HERE, ahead of the geometry event: the searches issued on the second
        # stream order themselves after that event only, and they read these rows
        qxyz = query_points[order_d, 1:].contiguous()
        if geometry is not None:
            # hand-over H4: the searches issued on the second stream order themselves after this event -- it has to come AFTER the
            # gather above (the geometry itself was enqueued, and its own event recorded, before the host sync)
            geometry["geo_event"] = torch.cuda.Event()
            geometry["geo_event"].record(torch.cuda.current_stream(dev))

        # ---- frame-store plan
        if back is not None and frame_store is not None and frame_store.get("feat_t0", 0) > 0:
            raise ValueError(f"backward_tracking needs a frame store with features from frame 0 on (queries up to frame {int(qt.max())} are "
                             f"tracked back to the clip's start), but the supplied frame_store was built from frame "
                             f"{frame_store['feat_t0']}: build it with t0=0")
        out, pre = {}, {}

        def after_first_chunk(st):
            # Device-side bookkeeping of the call, created AFTER the first encoder chunk has been enqueued: the GPU idles from the
            # host sync above until the first kernels arrive, so nothing that can wait goes before them
            out.update(_call_outputs(dev, T, N, C))
            self._presearch(st, fwd, qt_s, qxyz, pre)

        store, pending, pending_back, start_side_encoder = self._plan_frame_store(rgbs, depths, intrs, extrs, geometry, frame_store, fwd,
                                                                                  back is not None, after_first_chunk)
        if not out:  # (no store was built behind an encoder chunk)
            out.update(_call_outputs(dev, T, N, C))
        if start_side_encoder is not None and iters < 1:  # (no correlation launch to start it behind)
            start_side_encoder()
            start_side_encoder = None

        # ---- forward pass
        windows = self._run_windows(store, fwd, [w for w, _ in fwd], 1, (qxyz, qt_sd, out["feat_init"]), order_d, out, iters, trace,
                                    enter_frames=qt_s, pre=pre, pending=pending, after_first_corr=start_side_encoder)
        for _, ev in pending:  # frames no window consumed: still join the side stream before the inputs are released
            torch.cuda.current_stream(dev).wait_event(ev)  # hand-over H7: the caller's inputs (read by the second stream) are released

        # ---- the time-reversed pass (one stream): the same window loop on the same store, slots running downwards from frame
        # T-1-wr.  Its store kernel writes only frames before each row's query frame, which IS the merge of the two passes.
        windows_b = []
        if back is not None:
            for _, ev in pending_back + list(store.get("pending", ()) if frame_store is not None else ()):
                torch.cuda.current_stream(dev).wait_event(ev)  # hand-over H5 for the early frames
            if pending_back:
                self._handover(dev)
            order_bd, qt_bd = small_d[2:4]
            qxyz_b = query_points[order_bd, 1:].contiguous()
            feat_b = torch.zeros(N, C, device=dev)
            # feature init of the reversed pass's rows (:607-645): the same query frame, the same 1-NN
            self._feat_init(store, back["sorted_qt"], qxyz_b, 0, back["active"], feat_b)
            if len(fix_rows):
                out["feat_init"].index_copy_(0, small_d[4], feat_b.index_select(0, small_d[5]))
            windows_b = self._run_windows(store, back["windows"], back["frame0"], -1, (qxyz_b, qt_bd, feat_b), order_bd, out, iters, trace,
                                          before=qt_bd)

        self.last_windows = windows
        self.last_windows_backward = windows_b
        self.last_vis_logits = out["vis_logit"][None]
        self.last_nan_flag = out["nan_flag"]
        return {
            "traj_e": out["traj"][None],
            "feat_init": out["feat_init"][None, None].expand(1, S, -1, -1),
            "vis_e": out["vis_prob"][None],
        }

    @torch.no_grad()
    @hip.guarded
    def forward_grouped(self, rgbs, depths, query_points_list, intrs, extrs, iters=4, frame_store=None, trace=None, is_train=False,
                        save_debug_logs=False, save_rerun_logs=False, backward_tracking=False, **kwargs):
        """G independent ``forward`` calls through one launch sequence: query_points_list[g] (1,N_g,4) is a query set of its own
        (its own windows, its own 64 virtual tracks, its own softmax in the space attentions).  Returns one result dict per group,
        with the keys, shapes and dtypes of ``forward``'s.  Groups whose first windows coincide run in the same windows; the rows
        of a window are the concatenation of every member group's active tracks (``grouped.grouped_layout``).  ``trace``: a list
        that receives ``forward``'s per-window dicts in that layout, plus the window start, member groups and row offsets.  The
        other options are ``forward``'s and are handled as there (no training; the reference's logging hooks are ignored)."""
        if backward_tracking:
            raise NotImplementedError("forward_grouped has no backward_tracking (per-set directions inside one launch sequence are not "
                                      "built): call forward(..., backward_tracking=True) per query set")
        if not isinstance(query_points_list, (list, tuple)) or not query_points_list:
            raise ValueError("query_points_list must be a non-empty list of (1, N_g, 4) tensors")
        for g, qp in enumerate(query_points_list):
            if qp.dim() != 3 or qp.shape[0] != 1 or qp.shape[2] != 4:
                raise ValueError(f"group {g}: query points must be (1, N_g, 4), got {tuple(qp.shape)}")
            if qp.shape[1] == 0:
                raise ValueError(f"group {g} has no queries")
        rgbs, depths, intrs, extrs = self._normalise_inputs(rgbs, depths, intrs, extrs, is_train, save_debug_logs or save_rerun_logs)
        dev = rgbs.device
        T, S, C = rgbs.shape[1], self.S, self.latent_dim
        qcat = torch.cat([_f32(qp[0], dev) for qp in query_points_list], 0)  # caller rows
        sizes = [int(qp.shape[1]) for qp in query_points_list]
        qt_all = qcat[:, 0].long().cpu().numpy()  # the one host sync of the call (mvtracker.py:489, truncation toward zero)
        lay = grouped_layout(np.split(qt_all, np.cumsum(sizes)[:-1]), S, T)
        N = len(qt_all)
        wins = lay["windows"]
        # every index map of the call in ONE upload: sorted -> caller rows, then per window rows / carry map / un-sort map
        parts = [lay["sorted_src"]] + [a for wd in wins for a in (wd["rows"], wd["carry"], wd["out"])]
        idx_d = torch.from_numpy(np.concatenate(parts).astype(np.int64)).to(dev)
        sorted_src_d = idx_d[:N]
        qxyz = qcat[sorted_src_d, 1:].contiguous()  # sorted rows
        qt_sd = torch.from_numpy(lay["sorted_qt"].astype(np.int32)).to(dev)
        out = _call_outputs(dev, T, N, C)  # (feat_init in sorted rows, as forward's)
        traj, vis_prob, vis_logit, feat_init, nan_flag = (out[k] for k in ("traj", "vis_prob", "vis_logit", "feat_init", "nan_flag"))
        if wins:
            store = frame_store if frame_store is not None else self.build_frame_store(
                rgbs, depths, intrs, extrs, t0=max(min(wd["w"] for wd in wins), 0))
            for _, ev in store.get("pending", ()):  # feature blocks of a shared store still in flight
                torch.cuda.current_stream(dev).wait_event(ev)
            # feature init of every track that ever enters a window (:607-645): 1-NN in the level-0 cloud of its query frame,
            # all groups at once, sorted by query frame (the searches are per query: batching them changes no result)
            ent = np.concatenate([lay["base"][g] + np.arange(lay["active"][g]) for g in range(len(sizes))])
            ent = ent[np.argsort(lay["sorted_qt"][ent], kind="stable")]
            ent_d = torch.from_numpy(ent.astype(np.int64)).to(dev)
            qx_e = qxyz[ent_d].contiguous()
            fe = torch.empty(len(ent), C, device=dev)
            self._feat_init(store, lay["sorted_qt"][ent], qx_e, 0, len(ent), fe)
            feat_init.index_copy_(0, ent_d, fe)
        o = N
        coords = vis = None
        windows = []
        for wd in wins:
            n = int(wd["off"][-1])
            rows_d, carry_d, out_d = idx_d[o:o + n], idx_d[o + n:o + 2 * n], idx_d[o + 2 * n:o + 3 * n]
            o += 3 * n
            if wd["new_tracks"]:
                coords = vis = None
            wc = torch.empty(n, S, 3, device=dev)
            wf = torch.empty(n, S, C, device=dev)
            wm = torch.empty(n, S, 2, device=dev)
            hip.window_prepare(qxyz[rows_d].contiguous(), qt_sd[rows_d].contiguous(), feat_init[rows_d].contiguous(), coords, vis, n, 0, S, C,
                               wd["w"], T, wc, wm, wf, carry_src=carry_d.to(torch.int32))
            wtrace = None
            if trace is not None:
                wtrace = dict(w=wd["w"], groups=list(wd["groups"]), group_offsets=wd["off"].tolist(), carried=wd["p0"].tolist())
                trace.append(wtrace)
            preds, vis, _ = self._refine(store, wd["w"], wc, wf, wm, iters=iters, nan_flag=nan_flag, trace=wtrace,
                                         seg=[int(c) for c in np.diff(wd["off"])])
            coords = preds[-1]
            hip.window_store(coords, vis, out_d, n, S, wd["w"], T, N, traj, vis_logit, vis_prob)  # caller rows
            windows.append((wd["w"], n))
        self.last_windows = windows
        self.last_vis_logits = vis_logit[None]
        self.last_nan_flag = nan_flag
        results = []
        for g in range(len(sizes)):
            b0, b1 = int(lay["base"][g]), int(lay["base"][g + 1])
            results.append({
                "traj_e": traj[None, :, b0:b1],
                "feat_init": feat_init[None, None, b0:b1].expand(1, S, -1, -1),
                "vis_e": vis_prob[None, :, b0:b1],
            })
        return results

    def open_stream(self, query_points, iters=4, ring_blocks=3, backward_tracking=False):
        """Streaming session (``mvtracker_amd.streaming.StreamSession``): push frame blocks as they arrive, get
        the tracks of the frames that became final, from a ring frame store whose size does not depend on the clip length.  The
        concatenated emissions are the bits of ``forward`` on the whole clip.  ``query_points`` (1,N,4), N >= 1."""
        from .streaming import StreamSession
        if backward_tracking:
            raise NotImplementedError("there is no streaming form of backward_tracking: the time-reversed pass starts at the clip's last "
                                      "frame and is inherently offline (call forward(..., backward_tracking=True) on the whole clip)")
        if isinstance(query_points, (list, tuple)):
            raise NotImplementedError("there is no streaming form of forward_grouped: open one session per query set")
        return StreamSession(self, query_points, iters=iters, ring_blocks=ring_blocks)

    def check_finite(self):
        """Deferred NaN guard (reference mvtracker.py:401-404): raises if the last forward produced NaN tracks."""
        if int(self.last_nan_flag.item()) != 0:
            raise FloatingPointError("Got NaN values in coords, perhaps the training exploded")
