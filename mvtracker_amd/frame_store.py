"""The frame store of MVTracker (reference model_utils.py:420-482) and the plumbing around it: features and world-space points
of every pyramid level, frame-major; the second-stream encoder that fills it beside the refinement windows; the cached streams
and scratch buffers of a model.

``FrameStoreMixin`` reads these model attributes: S, stride, latent_dim, corr_n_levels, corr_neighbors, encoder_chunk_images,
wide_conv_shared, sync_debug; it owns _shared_gpu (set by ``_beside_windows``), _side (streams) and _scratch (buffers); and calls
encode_frames / store_dtype (encoder).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import hip
from .weights import _round_up


def nseg(P: int, K: int) -> int:
    """Segments (runs of 64-point tiles) scanned by different waves; none may be empty."""
    nt = (P + 63) // 64
    n = max(1, min(64 // K, P // 8192, 4))
    while n > 1 and ((nt + n - 1) // n) * (n - 1) >= nt:
        n -= 1
    return n


class FrameStoreMixin:
    # ------------------------------------------------------------------ cached scratch buffers and streams
    def _scratch_buffer(self, kind, dev, size):
        """The model's cached buffer of ``kind`` for this device and the CURRENT stream (single_point mode runs forwards on several
        streams at once).  Each kind has its own growth rule:
          "workspace"  device bytes for the composite entries (no state between calls), grown on demand in whole MiB;
          "pin_i64"    pinned host int64, at least 1024 (the asynchronous read-back of the query frames);
          "pin_bytes"  pinned host bytes, at least 64 KiB (the staging buffer of ``_upload_small``);
          "flow"       size = (rows, ld): the flow head's two hidden activations, ld = round_up(out_dim, 4) -- the GEMMs write
                       out_dim columns, the pad columns are read as K padding by the next layer and must be zero: zeroed once per
                       (rows, ld), then reused by every call.  More than 32 of them are dropped together; other kinds stay."""
        key = (kind, dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0)
        if kind == "flow":
            key += size
            if key not in self._scratch:
                flow = [k for k in self._scratch if k[0] == "flow"]
                for k in flow if len(flow) > 32 else ():
                    del self._scratch[k]
                self._scratch[key] = (torch.zeros(*size, device=dev), torch.zeros(*size, device=dev))
            return self._scratch[key]
        t = self._scratch.get(key)
        if t is None or t.numel() < size:
            if kind == "workspace":
                t = torch.empty(_round_up(size, 1 << 20), device=dev, dtype=torch.uint8)
            else:
                dtype, least = {"pin_i64": (torch.int64, 1024), "pin_bytes": (torch.uint8, 1 << 16)}[kind]
                t = torch.empty(max(size, least), dtype=dtype).pin_memory()
            self._scratch[key] = t
        return t

    def _workspace(self, nbytes, dev):
        return self._scratch_buffer("workspace", dev, nbytes)

    def _pinned_i64(self, dev, n):
        return self._scratch_buffer("pin_i64", dev, n)[:n]

    def _upload_small(self, dev, *arrays):
        """Host numpy arrays -> device tensors via one cached pinned buffer (non-blocking copies on the current stream)."""
        if dev.type != "cuda":
            return tuple(torch.from_numpy(a).to(dev) for a in arrays)
        pin = self._scratch_buffer("pin_bytes", dev, sum((a.nbytes + 15) // 16 * 16 for a in arrays))
        out, o = [], 0
        for a in arrays:
            view = pin[o:o + a.nbytes].view(torch.from_numpy(a).dtype)
            view.copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))
            out.append(view.to(dev, non_blocking=True).reshape(a.shape))
            o += (a.nbytes + 15) // 16 * 16
        return tuple(out)

    def _stream(self, kind, dev):
        """The model's second stream of ``kind`` on a device: "side" runs work beside the refinement windows (later frame blocks'
        encoder, the searches issued ahead), "helper" takes every other chunk of one encoder call."""
        key = (kind, dev.type, dev.index)
        if key not in self._side:
            self._side[key] = torch.cuda.Stream(device=dev)
        return self._side[key]

    def _helper_stream(self, dev):
        return self._stream("helper", dev)

    def _side_stream(self, dev):
        return self._stream("side", dev)

    def _handover(self, dev):
        """Debug hook at every point where one stream starts consuming what another produced (see ``sync_debug``)."""
        if self.sync_debug and dev.type == "cuda":
            torch.cuda.synchronize(dev)

    @contextlib.contextmanager
    def _beside_windows(self, short_workgroups=True):
        """Encoder calls issued inside run BESIDE the refinement windows: short-lived workgroups only (MVT_IO_SHORT_WG, the
        ``encoder_struct_shared`` weights; bit-identical results) unless ``short_workgroups`` is off (``wide_conv_shared``)."""
        self._shared_gpu = short_workgroups
        try:
            yield
        finally:
            self._shared_gpu = False

    # ------------------------------------------------------------------ frame store (model_utils.py:420-482)
    def _encode_on_side_stream(self, store, rgbs, firsts, pending, end=None):
        """Encode the S/2-frame blocks starting at ``firsts`` on the second HIP stream (ordered after everything enqueued on the
        caller's stream so far); ``pending`` receives (first frame, event) per block.  ``end``: the blocks stop at this frame
        (default: the clip's end)."""
        dev = rgbs.device
        S = self.S
        T = rgbs.shape[1] if end is None else min(end, rgbs.shape[1])
        # (the later blocks stay on ONE stream, in order: alternating them between two streams as encode_images does for the chunks
        #  of the first block measured +0.5 ms -- beside the updater their concurrency only adds contention)
        streams = [self._side_stream(dev)]
        for st in streams:
            st.wait_stream(torch.cuda.current_stream(dev))  # hand-over H3: the store (allocated / geometry written on the caller's stream)
        self._handover(dev)
        # these blocks run BESIDE the refinement windows: short-lived workgroups only, unless the encoder bounds the call anyway
        V = rgbs.shape[0]
        first_block = max(1, min(rgbs.shape[1], S)) * V
        side_images = sum(min(T, a + S // 2) - a for a in firsts) * V
        big = self.wide_conv_shared == "1" or (self.wide_conv_shared == "auto" and side_images > 2 * first_block)
        for i, a in enumerate(firsts):
            st = streams[i % len(streams)]
            with torch.cuda.stream(st):
                with self._beside_windows(short_workgroups=not big):
                    self.fill_frame_features(store, rgbs, a, min(T, a + S // 2))
                ev = torch.cuda.Event()
                ev.record(st)
                pending.append((a, ev))

    @hip.guarded
    def fill_frame_features(self, store, rgbs, a, b, level0=None, after_first_chunk=None):
        """Encode frames [a, b) into the store's feature pyramid (everything else in the store is geometry)."""
        V, T, _, H, W = rgbs.shape
        hs, ws = H // self.stride, W // self.stride
        fv = store["fvec"]
        if level0 is None:
            self.encode_frames(rgbs, a, b, images_per_chunk=self.encoder_chunk_images or max(16, V * (self.S // 2)), out=fv[0],
                               after_first_chunk=after_first_chunk)
        elif after_first_chunk is not None:
            after_first_chunk()
        for lvl in range(1, self.corr_n_levels):
            h, w = hs >> (lvl - 1), ws >> (lvl - 1)
            hip.avgpool2(fv[lvl - 1][a:b], fv[lvl][a:b], (b - a) * V, h, w, self.latent_dim)

    @hip.guarded
    def store_geometry(self, depths, intrs, extrs, into=None):
        """The query-independent half of the frame store: world-space points of every pyramid level, tile boxes.  A handful of small
        kernels; ``forward`` enqueues them BEFORE its one host sync (the query frames), so that the GPU has work while the host wakes up.
        ``into``: (store, first slot) -- the T frames go into slots [first, first + T) of that store's tensors (a block of a ring
        store: the kernels are the same, on block views), nothing is allocated but the camera inverses."""
        V, T, _, H, W = depths.shape
        dev = depths.device
        hs, ws = H // self.stride, W // self.stride
        # (the reference fails here too, inside its kNN -- pointops / topk with k above the number of points, mvtracker.py:26-90 --; say why)
        pmin = V * (hs >> (self.corr_n_levels - 1)) * (ws >> (self.corr_n_levels - 1))
        if pmin < self.corr_neighbors:
            raise ValueError(f"the coarsest level of the point-cloud pyramid has {pmin} points per frame ({V} views of "
                             f"{hs >> (self.corr_n_levels - 1)} x {ws >> (self.corr_n_levels - 1)}), fewer than corr_neighbors = "
                             f"{self.corr_neighbors}: frames of {H} x {W} are too small for {self.corr_n_levels} correlation levels")
        kinv = torch.empty(V * T, 9, device=dev)
        einv = torch.empty(V * T, 12, device=dev)
        hip.invert_cameras(intrs.reshape(V * T, 9), extrs.reshape(V * T, 12), kinv, einv, V * T)
        slots = None if into is None else slice(into[1], into[1] + T)
        ds = torch.empty(T, V, hs, ws, device=dev) if into is None else into[0]["depth_s"][slots]
        hip.depth_subsample(depths.reshape(V, T, H, W), ds, V, T, H, W, self.stride)
        xyz = []
        for lvl in range(self.corr_n_levels):
            o = torch.empty(T, V, hs >> lvl, ws >> lvl, 4, device=dev) if into is None else into[0]["xyz"][lvl][slots]
            hip.unproject(ds, kinv, einv, o, V, T, hs, ws, self.stride, lvl)
            xyz.append(o)
        P = [V * (hs >> lvl) * (ws >> lvl) for lvl in range(self.corr_n_levels)]
        # bounding boxes of the 64-point scan tiles (8x8 pixel patches where the grid allows it): the kNN scan culls with them
        # ... and the union boxes of 64 consecutive tiles, the coarse level the single-wave searches test first
        box, tgrid, gbox = [], [], []
        for lvl in range(self.corr_n_levels):
            h, w = hs >> lvl, ws >> lvl
            g = (w, h) if (w % 8 == 0 and h % 8 == 0) else (0, 0)
            nt = (P[lvl] + 63) // 64
            b = torch.empty(T, nt, 8, device=dev) if into is None else into[0]["box"][lvl][slots]
            hip.tile_aabb(xyz[lvl], P[lvl], T, b, g)
            gb = None
            if nt > 64:
                gb = torch.empty(T, (nt + 63) // 64, 8, device=dev) if into is None else into[0]["gbox"][lvl][slots]
                hip.tile_group_aabb(b, P[lvl], T, gb)
            box.append(b)
            tgrid.append(g)
            gbox.append(gb)
        if into is not None:
            return into[0]
        geo = {"xyz": xyz, "P": P, "T": T, "depth_s": ds, "box": box, "tile_grid": tgrid, "gbox": gbox}
        if dev.type == "cuda":
            geo["geo_event"] = torch.cuda.Event()
            geo["geo_event"].record(torch.cuda.current_stream(dev))
        return geo

    @hip.guarded
    def build_frame_store(self, rgbs, depths, intrs, extrs, t0=0, level0=None, t1=None, after_geometry=None, geometry=None):
        """Features and world-space points of every pyramid level, frame-major.

        rgbs (V,T,3,H,W), depths (V,T,1,H,W), intrs (V,T,3,3), extrs (V,T,3,4).  ``level0`` (T,V,H/4,W/4,C)
        may carry level-0 features encoded elsewhere (frames split across GPUs, mvtracker_amd.parallel).
        Features are computed for frames [t0, t1) only (``fill_frame_features`` adds more later); the geometry
        (points, tile boxes) covers every frame."""
        V, T, _, H, W = rgbs.shape
        dev = rgbs.device
        hs, ws = H // self.stride, W // self.stride
        C = self.latent_dim
        t1 = T if t1 is None else t1
        # (no memset of the 0.8 GB level-0 store: frames [t0, T) are written by the encoder before any window reads them --
        #  later frames possibly on the second stream, ordered by events -- and frames before t0 are never read)
        sdt = level0.dtype if level0 is not None else self.store_dtype()
        fv = [torch.empty(T, V, hs, ws, C, device=dev, dtype=sdt) if level0 is None else level0]
        for lvl in range(1, self.corr_n_levels):
            fv.append(torch.empty(T, V, hs >> lvl, ws >> lvl, C, device=dev, dtype=sdt))
        for f_ in fv[(1 if level0 is not None else 0):]:
            f_[:t0].zero_()
        # geometry first (a handful of small kernels), features after: what only needs the point clouds -- the first, unseeded
        # neighbour searches of new tracks -- can then run beside the encoder.  ``after_geometry(store)`` is called on the host as
        # soon as the FIRST encoder chunk has been enqueued (the GPU is busy from then on); work it issues on another stream
        # orders itself after store["geo_event"], not after the encoder.  ``geometry``: already enqueued by the caller (store_geometry).
        store = dict(geometry) if geometry is not None else self.store_geometry(depths, intrs, extrs)
        store["fvec"] = fv
        store["feat_t0"] = t0  # features exist for frames [t0, T) (backward tracking needs t0 == 0)
        self.fill_frame_features(store, rgbs, t0, t1, level0, after_first_chunk=(lambda: after_geometry(store)) if after_geometry else None)
        return store
