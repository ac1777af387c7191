"""Streaming tracking (``MVTracker.open_stream``): push frame blocks as they arrive, get the tracks of the frames that became final.

The reference's window loop is causal (mvtracker.py:537-698): window w reads frames [w, w+S), carries coordinates, visibility
logits and features from window w - S/2, and what it writes is overwritten by later windows only in its second half.  So once
window w has run, frames [w, w + S/2) are final and no frame before w + S/2 is read again.  A session keeps the frames a window in
flight can read in a RING frame store of R = ring_blocks * S/2 slots (frame f in slot (f - base) mod R, base = the first window's
start, so every S/2-frame block is contiguous in the ring and the encoder / geometry kernels run unchanged on block views), runs
every window as soon as its S frames are there, and at ``finish()`` -- the clip length T known -- the remaining windows with the
reference's repeat-last-frame padding.  Device memory does not depend on the clip length.

The contract: for any push schedule and any accepted ``add_queries`` schedule, the emissions of the pushes and of ``finish()``
concatenated over the frames (earlier chunks zero-padded to the final number of queries) are bit for bit
``forward(whole clip, all queries concatenated in order of addition)``.

``StreamSchedule`` is the host half -- which frames go where in the ring, which windows run when, which frames are emitted --
and needs numpy only.  ``StreamSession`` executes its plan with the window loop of ``MVTracker._run_windows``, on one stream.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np


class StreamSchedule:
    """Pure host scheduler of a streaming session (numpy only).

    ``push(b)`` / ``finish()`` return (ops, (a, b)): the ordered operations of the step and the frames [a, b) that became final.
      ("encode", i0, i1, g)   frames [i0, i1) of the pushed block are clip frames [g, g + i1 - i0): into ring slots from
                              (g - base) mod R on, contiguous (an operation never crosses an S/2 block boundary of the ring)
      ("window", w, p1, hi)   run window w on the first p1 queries (stable sort by query frame), ``hi`` = last frame received
    The windows over all steps are ``backward.window_prefixes(sorted query frames, S, T)``, the emitted ranges tile [0, T)."""

    def __init__(self, S: int, ring_blocks: int = 3):
        if S < 2 or S % 2:
            raise ValueError(f"the window length must be even, got {S}")
        if ring_blocks < 3:
            raise ValueError(f"ring_blocks must be at least 3 (the window in flight is two S/2 blocks, plus the block arriving), got {ring_blocks}")
        self.S, self.half, self.R = S, S // 2, ring_blocks * (S // 2)
        self.qt = np.zeros(0, dtype=np.int64)  # query frames in order of addition
        self.received = 0    # frames pushed so far
        self.base = None     # start of the first window: fixed when the first frame is stored
        self.next_w = None   # start of the next window to run
        self.last_w = None   # start of the last window run
        self.emitted = 0     # frames [0, emitted) have been returned
        self.finished = False
        self.windows: List[Tuple[int, int]] = []  # every window run so far, (start, active prefix)

    def add_queries(self, qt) -> None:
        """Append queries with integer frames ``qt``.  ValueError -- and nothing changes -- for a query that ``forward`` on the whole
        clip would have treated differently from what the session has already done: one that a window already run would have
        admitted (t < w_last + S), or, before the first window, one whose frame has already been skipped."""
        qt = np.asarray(qt, dtype=np.int64).reshape(-1)
        if self.finished:
            raise ValueError("the session is finished")
        if qt.size == 0:
            raise ValueError("no queries")
        if qt.min() < 0:
            raise ValueError(f"query frames must not be negative, got {int(qt.min())}")
        if self.last_w is not None:
            if qt.min() < self.last_w + self.S:
                raise ValueError(f"query at frame {int(qt.min())}: window {self.last_w} has already run and would have admitted every "
                                 f"query before frame {self.last_w + self.S}; add queries before their window runs")
        elif self.qt.size:
            skipped = min(int(self.qt.min()), self.received)  # frames before the first window's start are dropped as they arrive
            if qt.min() < skipped:
                raise ValueError(f"query at frame {int(qt.min())}: frames before {skipped} have already been skipped (they lie before "
                                 f"the first window's start, frame {int(self.qt.min())}, as known when they arrived)")
        self.qt = np.concatenate([self.qt, qt])

    def _ready(self, hi: int, T=None):
        """Windows that can run with frames up to ``hi`` received: all S frames there, or (``T`` known) the reference's loop condition."""
        ops = []
        while self.next_w is not None and (self.next_w + self.S - 1 <= hi if T is None else self.next_w < T - self.half):
            w = self.next_w
            p1 = int(np.count_nonzero(self.qt < w + self.S))
            ops.append(("window", w, p1, hi))
            self.windows.append((w, p1))
            self.last_w, self.next_w = w, w + self.half
        return ops

    def push(self, b: int):
        if self.finished:
            raise ValueError("the session is finished")
        if b < 1 or not self.qt.size:
            raise ValueError("push needs at least one frame and one query")
        ops, i = [], 0
        while i < b:
            g = self.received + i
            if self.base is None:
                w0 = int(self.qt.min())
                if g < w0:  # before the first window's start: accepted and skipped
                    i += min(b - i, w0 - g)
                    continue
                self.base = self.next_w = w0
            n = min(b - i, self.half - (g - self.base) % self.half)
            assert g + n - 1 - self.next_w < self.R  # the ring holds [next_w, next_w + R)
            ops.append(("encode", i, i + n, g))
            i += n
            ops += self._ready(g + n - 1)
        self.received += b
        a = self.emitted
        if any(op[0] == "window" for op in ops):
            self.emitted = self.last_w + self.half  # the first half of the last window run is final
        return ops, (a, self.emitted)

    def finish(self):
        if self.finished:
            raise ValueError("the session is finished")
        T = self.received
        ops = self._ready(T - 1, T)
        self.finished = True
        a, self.emitted = self.emitted, T
        return ops, (a, T)

    def slot(self, f: int) -> int:
        """Ring slot of clip frame ``f``."""
        return (f - self.base) % self.R


class StreamSession:
    """``MVTracker.open_stream``: see the module docstring.  One HIP stream; encoding block k + 1 beside window k is left open."""

    def __init__(self, model, query_points, iters=4, ring_blocks=3):
        import torch
        from . import hip
        self.model, self.iters = model, iters
        self.sched = StreamSchedule(model.S, ring_blocks)
        hip.require_device(query_points)
        self.dev = query_points.device
        self.queries = torch.zeros(0, 4, device=self.dev)  # caller rows, in order of addition
        self.store = None     # the ring frame store (allocated by the first push, never reallocated)
        self.carry = {}       # what one window hands to the next (MVTracker._run_windows)
        self.feat = torch.zeros(0, model.latent_dim, device=self.dev)  # initial feature rows, sorted order
        self.nan_flag = torch.zeros(1, device=self.dev, dtype=torch.int32)
        self.add_queries(query_points)

    # ------------------------------------------------------------------ queries
    def add_queries(self, query_points):
        import torch
        from .tracker import _f32
        if query_points.dim() != 3 or query_points.shape[0] != 1 or query_points.shape[2] != 4 or query_points.shape[1] < 1:
            raise ValueError(f"query points must be (1, N, 4) with N >= 1, got {tuple(query_points.shape)}")
        qp = _f32(query_points[0], self.dev)
        self.sched.add_queries(qp[:, 0].long().cpu().numpy())  # (truncation toward zero, mvtracker.py:489; raises before any change)
        self.queries = torch.cat([self.queries, qp], 0)
        # the layout ``forward`` would use for all queries so far: stable sort by query frame (mvtracker.py:514).  The rows that
        # have entered a window are a prefix of it that later additions (all behind the windows run) cannot change.
        qt = self.sched.qt
        order = np.argsort(qt, kind="stable")
        self.qt_s = qt[order]
        self.order_d, self.qt_sd = self.model._upload_small(self.dev, order.astype(np.int64), self.qt_s.astype(np.int32))
        self.qxyz = self.queries[self.order_d, 1:].contiguous()
        feat = torch.zeros(len(qt), self.model.latent_dim, device=self.dev)
        entered = self.carry.get("p0", 0)
        feat[:entered] = self.feat[:entered]
        self.feat = feat

    # ------------------------------------------------------------------ the ring store
    def _allocate(self, V, H, W):
        import torch
        m, R, dev = self.model, self.sched.R, self.dev
        hs, ws, C, L = H // m.stride, W // m.stride, m.latent_dim, m.corr_n_levels
        sdt = m.store_dtype()
        P = [V * (hs >> l) * (ws >> l) for l in range(L)]
        nt = [(p + 63) // 64 for p in P]
        self.store = dict(
            fvec=[torch.zeros(R, V, hs >> l, ws >> l, C, device=dev, dtype=sdt) for l in range(L)],
            xyz=[torch.zeros(R, V, hs >> l, ws >> l, 4, device=dev) for l in range(L)],
            box=[torch.zeros(R, n, 8, device=dev) for n in nt],
            gbox=[torch.zeros(R, (n + 63) // 64, 8, device=dev) if n > 64 else None for n in nt],
            tile_grid=[((ws >> l), (hs >> l)) if ((ws >> l) % 8 == 0 and (hs >> l) % 8 == 0) else (0, 0) for l in range(L)],
            depth_s=torch.zeros(R, V, hs, ws, device=dev), P=P, T=R, ring=None)
        self.shape = (V, H, W)

    def _encode(self, rgbs, depths, intrs, extrs, i0, i1, g):
        """Frames [i0, i1) of the pushed block -> geometry and feature pyramid of ring slots [slot(g), slot(g) + i1 - i0)."""
        from . import hip
        m, st = self.model, self.store
        V, H, W = self.shape
        s0 = self.sched.slot(g)
        s1 = s0 + (i1 - i0)
        assert s1 <= self.sched.R
        m.store_geometry(depths[:, i0:i1].contiguous(), intrs[:, i0:i1].contiguous(), extrs[:, i0:i1].contiguous(), into=(st, s0))
        fv = st["fvec"]
        m.encode_frames(rgbs, i0, i1, images_per_chunk=m.encoder_chunk_images or max(16, V * (m.S // 2)), out=fv[0][s0:s1], out_t0=i0)
        hs, ws = H // m.stride, W // m.stride
        for lvl in range(1, m.corr_n_levels):
            hip.avgpool2(fv[lvl - 1][s0:s1], fv[lvl][s0:s1], (i1 - i0) * V, hs >> (lvl - 1), ws >> (lvl - 1), m.latent_dim)

    # ------------------------------------------------------------------ steps
    def _store_carried(self, out, a, b):
        """The carried window's slots inside frames [a, b) into the step's chunk, un-sorted to the caller's rows."""
        from . import hip
        c = self.carry
        if c and b > a:
            hip.window_store(c["coords"], c["vis"], self.order_d, c["p0"], self.model.S, c["w"], self.sched.received, out["traj"].shape[1],
                             out["traj"], out["vis_logit"], out["vis_prob"], frames=(a, b))

    def _step(self, ops, frames, clip=None):
        import torch
        m = self.model
        a, b = frames
        N = self.queries.shape[0]
        out = dict(traj=torch.zeros(b - a, N, 3, device=self.dev), vis_prob=torch.zeros(b - a, N, device=self.dev),
                   vis_logit=torch.zeros(b - a, N, device=self.dev), nan_flag=self.nan_flag)
        # frames of this chunk that the last window of an earlier step wrote (its second half) and no window of this step rewrites
        self._store_carried(out, a, b)
        for op in ops:
            if op[0] == "encode":
                self._encode(*clip, *op[1:])
                continue
            _, w, p1, hi = op
            self.store["ring"] = (self.sched.base, self.sched.R, w, hi)
            m._run_windows(self.store, [(w, p1)], [w], 1, (self.qxyz, self.qt_sd, self.feat), self.order_d, out, self.iters, None,
                           store_slots=False, enter_frames=self.qt_s, carry=self.carry, T=hi + 1)
            self._store_carried(out, a, b)
        return {"frames": (a, b), "traj_e": out["traj"][None], "vis_e": out["vis_prob"][None], "vis_logits": out["vis_logit"][None]}

    def push(self, rgbs, depths, intrs, extrs):
        """A block of frames (1,V,b,3,H,W) ..., any b >= 1, uint8 or float as ``forward`` accepts.  Returns {"frames": (a, b),
        "traj_e" (1, b-a, N_now, 3), "vis_e", "vis_logits"} for the frames that became final."""
        import torch
        from . import hip
        with torch.no_grad(), hip.device_guard(self.queries):
            rgbs, depths, intrs, extrs = self.model._normalise_inputs(rgbs, depths, intrs, extrs, False, False)
            V, _, _, H, W = rgbs.shape
            if self.store is None:
                self._allocate(V, H, W)
            elif self.shape != (V, H, W):
                raise ValueError(f"the session's frames are {self.shape} (views, height, width), got {(V, H, W)}")
            ops, frames = self.sched.push(rgbs.shape[1])
            return self._step(ops, frames, (rgbs, depths, intrs, extrs))

    def finish(self):
        """Run the remaining windows with the clip length now known; returns the last chunk, plus ``feat_init`` as ``forward``'s, and
        leaves ``last_windows`` / ``last_nan_flag`` on the model as ``forward`` does."""
        import torch
        from . import hip
        with torch.no_grad(), hip.device_guard(self.queries):
            ops, frames = self.sched.finish()
            res = self._step(ops, frames)
        m = self.model
        res["feat_init"] = self.feat[None, None].expand(1, m.S, -1, -1)
        m.last_windows = list(self.sched.windows)
        m.last_windows_backward = []
        m.last_nan_flag = self.nan_flag
        return res

    def check_finite(self):
        """Deferred NaN guard (reference mvtracker.py:401-404) of the windows run so far."""
        if int(self.nan_flag.item()) != 0:
            raise FloatingPointError("Got NaN values in coords, perhaps the training exploded")
