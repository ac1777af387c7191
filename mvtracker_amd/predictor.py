"""EvaluationPredictor on MI355X: the drop-in boundary of the tracking forward path.

Mirrors ``mvtracker.models.evaluation_predictor_3dpt.EvaluationPredictor`` (reference
evaluation_predictor_3dpt.py:17-414): same constructor, same ``forward`` keyword arguments
(``rgbs, depths, query_points_3d, intrs, extrs`` + ignored ``**kwargs``), same result dict
(``traj_e``, ``vis_e`` bool, ``vis_e_as_prob``), so ``demo.py`` and ``Evaluator.evaluate_sequence``
can drive it unchanged.  The heavy lifting is ``self.model`` (mvtracker_amd.tracker.MVTracker);
the resize runs in the HIP library, the support-grid synthesis is a few hundred points of
bookkeeping on device tensors.

``forward`` is a list of stages, each written once ("The predictor's stages"); a streaming session's ``push``
runs the same cast, clean, normalise and resize on every block, and the global support grid on the first.
"""
from __future__ import annotations

import contextlib
import logging
from typing import Optional, Tuple

import numpy as np
import torch

from . import hip

log = logging.getLogger(__name__)


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


def _bilinear_sample_depth(depth: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Four clamped taps with weights from the unclamped corners (reference model_utils.py:81-165).

    depth (H,W), x,y (M,) pixel coordinates -> (M,)."""
    H, W = depth.shape
    x0, y0 = torch.floor(x), torch.floor(y)
    x1, y1 = x0 + 1, y0 + 1
    cx0, cx1 = x0.clamp(0, W - 1).long(), x1.clamp(0, W - 1).long()
    cy0, cy1 = y0.clamp(0, H - 1).long(), y1.clamp(0, H - 1).long()
    flat = depth.reshape(-1)
    return ((x1 - x) * (y1 - y) * flat[cy0 * W + cx0] + (x - x0) * (y1 - y) * flat[cy0 * W + cx1]
            + (x1 - x) * (y - y0) * flat[cy1 * W + cx0] + (x - x0) * (y - y0) * flat[cy1 * W + cx1])


def _bilinear_sample_depth_multi(depths: torch.Tensor, v: torch.Tensor, t: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``_bilinear_sample_depth`` for points that live in different (view, frame) depth maps: depths (V,T,H,W), v,t,x,y (M,)."""
    V, T, H, W = depths.shape
    x0, y0 = torch.floor(x), torch.floor(y)
    x1, y1 = x0 + 1, y0 + 1
    cx0, cx1 = x0.clamp(0, W - 1).long(), x1.clamp(0, W - 1).long()
    cy0, cy1 = y0.clamp(0, H - 1).long(), y1.clamp(0, H - 1).long()
    flat = depths.reshape(-1)
    base = (v * T + t) * (H * W)
    return ((x1 - x) * (y1 - y) * flat[base + cy0 * W + cx0] + (x - x0) * (y1 - y) * flat[base + cy0 * W + cx1]
            + (x1 - x) * (y - y0) * flat[base + cy1 * W + cx0] + (x - x0) * (y - y0) * flat[base + cy1 * W + cx1])


def _lift(depths, vid, fid, x, y, kinv, einv):
    """The batched lift: pixels (x, y) of the depth maps (vid, fid) into the world.  depths (V,T,H,W), vid,fid,x,y (M,), kinv
    (V,T,3,3), einv (V,T,3,4) -> (M,4) rows (frame, world xyz).  (The global grid does NOT come through here: it keeps the
    per-camera matmul of ``_support_rows``, whose rounding the stream-equals-forward promise and the golden fixtures rest on.)"""
    z = _bilinear_sample_depth_multi(depths, vid, fid, x, y)
    cam = torch.einsum("mij,mj->mi", kinv[vid, fid], torch.stack([x, y, torch.ones_like(x)], 1)) * z[:, None]
    ei = einv[vid, fid]
    world = torch.einsum("mij,mj->mi", ei[:, :, :3], cam) + ei[:, :, 3]
    return torch.cat([fid[:, None].to(world.dtype), world], 1)


def get_uniformly_sampled_pts(size: int, num_frames: int, extent: Tuple[float, ...], device="cpu") -> torch.Tensor:
    """(1, size, 3) rows (t, a, b): t uniform in [0, num_frames), a uniform in [0, extent[1]), b in [0, extent[0]) -- reference
    evaluation_predictor_3dpt.py:417-429, the same draws in the same order (torch.randint, then torch.rand)."""
    time_points = torch.randint(low=0, high=num_frames, size=(size, 1), device=device)
    space_points = torch.rand(size, 2, device=device) * torch.tensor([extent[1], extent[0]], device=device)
    return torch.cat((time_points, space_points), dim=1)[None]


def points_on_a_grid(size: int, extent: Tuple[float, float], center=None, device="cpu") -> torch.Tensor:
    """(size*size, 2) pixel (x, y) grid with margin W/64 (reference model_utils.py:361-417)."""
    if size == 1:
        return torch.tensor([[extent[1] / 2, extent[0] / 2]], device=device)
    if center is None:
        center = [extent[0] / 2, extent[1] / 2]
    m = extent[1] / 64
    ys = torch.linspace(m - extent[0] / 2 + center[0], extent[0] / 2 + center[0] - m, size, device=device)
    xs = torch.linspace(m - extent[1] / 2 + center[1], extent[1] / 2 + center[1] - m, size, device=device)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    return torch.stack([gx, gy], dim=-1).reshape(-1, 2)


# ---- clip stages without state: ``forward`` and a streaming session's ``push`` run the same ones ----------------------------------
def _cast(rgbs, depths, intrs, extrs, interp_shape):
    """(uint8 frames stay uint8 unless they have to be resized: the encoder's first kernel converts them)"""
    if not (rgbs.dtype == torch.uint8 and interp_shape is None):
        rgbs = rgbs.to(torch.float32)
    return rgbs.contiguous(), _f32(depths), intrs.to(torch.float32), extrs.to(torch.float32)


def _clean(depths, intrs, extrs, depth_cleaning, depths_conf):
    """The raw clip's depths cleaned of outliers (the radius is in the caller's units).  None: not one launch."""
    if depth_cleaning is None:
        return depths
    from . import clean
    return clean.clean_depths(depths, intrs, extrs, depth_cleaning, depths_conf=depths_conf)[0]


def _normalise(xf, depths, extrs, query_points=None):
    """Depths, extrinsics and queries (``forward`` only: a stream transforms its queries once, when it is opened) of the raw-resolution
    clip in the normalised scene.  The support points are built from these, so they need nothing of their own."""
    if xf is None:
        return depths, extrs, query_points
    return xf.apply(depths=depths, extrs=extrs, query_points=query_points)[:3]


def _resize(rgbs, depths, intrs, interp_shape):
    """Frames and depths at ``interp_shape`` (nearest) with the intrinsics rescaled, evaluation_predictor_3dpt.py:72-87.  None: not one launch."""
    if interp_shape is None:
        return rgbs, depths, intrs
    dev = rgbs.device
    _, V, T, _, height_raw, width_raw = rgbs.shape
    height, width = interp_shape
    r = torch.empty(1, V, T, 3, height, width, device=dev)
    hip.resize_nearest(rgbs, r, V * T * 3, height_raw, width_raw, height, width)
    d = torch.empty(1, V, T, 1, height, width, device=dev)
    hip.resize_nearest(depths, d, V * T, height_raw, width_raw, height, width)
    rs = torch.tensor([[width / width_raw, 0, 0], [0, height / height_raw, 0], [0, 0, 1]], device=dev, dtype=intrs.dtype)
    return r, d, torch.einsum("ij,BVTjk->BVTik", rs, intrs)


class EvaluationPredictor(torch.nn.Module):
    def __init__(
            self,
            multiview_model: torch.nn.Module,
            interp_shape: Optional[Tuple[int, int]] = (384, 512),
            visibility_threshold=0.5,
            grid_size: int = 5,
            n_grids_per_view: int = 1,
            local_grid_size: int = 8,
            local_extent: int = 50,
            single_point: bool = False,
            sift_size: int = 0,
            num_uniformly_sampled_pts: int = 0,
            n_iters: int = 6,
            backward_tracking: bool = False,
    ) -> None:
        super().__init__()
        self.model = multiview_model
        self.interp_shape = interp_shape
        self.visibility_threshold = visibility_threshold
        self.grid_size = grid_size
        self.n_grids_per_view = n_grids_per_view
        self.local_grid_size = local_grid_size
        self.local_extent = local_extent
        self.single_point = single_point
        self.sift_size = sift_size
        self.num_uniformly_sampled_pts = num_uniformly_sampled_pts
        self.n_iters = n_iters
        # also track every query BEFORE its frame (MVTracker.forward(backward_tracking=True): a time-reversed pass over the same
        # frame store); not in the reference's constructor, off by default
        self.backward_tracking = bool(backward_tracking)
        self.single_point_streams = 8  # HIP streams the per-query forwards of single_point mode are spread over
        # single_point mode: consecutive queries per MVTracker.forward_grouped call (each keeps its own rows and softmax);
        # 1 = one forward per query.  (An attribute, not a constructor argument: the constructor mirrors the reference's.)
        self.single_point_group_size = 1
        self._stream_pool = {}
        self.last_scene_transform = None  # the SceneTransform of the last forward / open_stream (None: the scene went in as it was)
        self.last_camera_correction = None  # the CameraCorrection of the last forward (None: the cameras went in as they were)
        # the ReprojectionReport of the cameras the last forward tracked with, and of the uncorrected ones when it also aligned them
        self.last_reprojection_report = self.last_reprojection_report_before = None
        self.last_track_overlay = None  # (video (V,T,3,Hp,Wp) uint8, colors (N,3) uint8) of the last forward with track_overlay
        self.last_rigid_motion = None  # the RigidMotionResult of the last forward with rigid_motion
        self.model.eval()

    # ---- helpers -------------------------------------------------------------------------
    def _streams(self, dev, n):
        key = (dev.type, dev.index)
        pool = self._stream_pool.setdefault(key, [])
        while len(pool) < n:
            pool.append(torch.cuda.Stream(device=dev))
        return pool[:n]

    @staticmethod
    def _invert(intrs, extrs):
        """K^-1 (V,T,3,3) and rows 0..2 of [R|t]^-1 (V,T,3,4) through the library (fp64 closed form)."""
        V, T = intrs.shape[:2]
        kinv = torch.empty(V * T, 9, device=intrs.device)
        einv = torch.empty(V * T, 12, device=intrs.device)
        hip.invert_cameras(intrs.reshape(V * T, 9).contiguous(), extrs.reshape(V * T, 12).contiguous(), kinv, einv, V * T)
        return kinv.reshape(V, T, 3, 3), einv.reshape(V, T, 3, 4)

    @staticmethod
    def _unproject(pix, z, kinv, einv):
        ph = torch.cat([pix, torch.ones_like(pix[:, :1])], 1)
        cam = (ph @ kinv.t()) * z[:, None]
        return cam @ einv[:, :3].t() + einv[:, 3]

    @staticmethod
    def _scene_transform(scene_transform, auto_inputs=None):
        """``scene_transform`` of ``forward`` / ``open_stream`` as a SceneTransform or None.  ``"auto"``:
        ``auto_scene_normalization`` of ``auto_inputs`` = (depths, intrs, extrs, depths_conf)."""
        if scene_transform is None:
            return None
        from . import scene
        if isinstance(scene_transform, scene.SceneTransform):
            return scene_transform
        if isinstance(scene_transform, str) and scene_transform == "auto":
            if auto_inputs is None:
                raise ValueError('a streaming session cannot take scene_transform="auto": the normalisation is computed from a whole '
                                 "frame of all views before anything is tracked.  Call mvtracker_amd.auto_scene_normalization(depths, "
                                 "intrs, extrs) on the first frame and pass the SceneTransform it returns")
            depths, intrs, extrs, conf = auto_inputs
            return scene.auto_scene_normalization(depths, intrs, extrs, depths_conf=conf)
        raise ValueError(f'scene_transform must be None, a SceneTransform or "auto", got {scene_transform!r}')

    def _query_groups(self, query_groups, num_points):
        """``forward``'s ``query_groups`` -> the caller rows of every distinct id, in ascending id order."""
        if self.single_point:
            raise NotImplementedError("query_groups with single_point: every query is a forward of its own there (group them with "
                                      "single_point_group_size)")
        if self.backward_tracking:
            raise NotImplementedError("query_groups with backward_tracking: forward_grouped has no backward tracking")
        if not hasattr(self.model, "forward_grouped"):
            raise NotImplementedError("query_groups needs a model with forward_grouped")
        ids = torch.as_tensor(query_groups)
        if ids.dim() != 1 or ids.dtype.is_floating_point or ids.dtype == torch.bool or ids.shape[0] != num_points or num_points == 0:
            raise ValueError(f"query_groups must be ({num_points},) integers, one per query, got {tuple(ids.shape)} {ids.dtype}")
        ids = ids.cpu().numpy()
        return [np.nonzero(ids == g)[0] for g in np.unique(ids)]

    # ---- clip stages that leave a ``last_*`` attribute --------------------------------------------------------------------------
    def _align(self, depths, intrs, extrs, camera_alignment, depths_conf):
        """(corrected extrs, uncorrected extrs) of a ``CameraAlignment`` (refined here, on the cleaned raw clip) or a ready
        ``CameraCorrection``, kept as ``last_camera_correction``.  None: (extrs, None) and not one launch."""
        self.last_camera_correction = None
        if camera_alignment is None:
            return extrs, None
        from . import align
        if isinstance(camera_alignment, align.CameraCorrection):
            correction = camera_alignment
        elif isinstance(camera_alignment, align.CameraAlignment):
            correction = align.align_cameras(depths, intrs, extrs, camera_alignment, depths_conf=depths_conf)
        else:
            raise ValueError(f"camera_alignment must be None, a CameraAlignment or a CameraCorrection, got {camera_alignment!r}")
        self.last_camera_correction = correction
        return correction.apply(extrs), extrs

    def _reproject(self, rgbs, depths, intrs, extrs, extrs_uncorrected, reprojection_check, depths_conf):
        """``last_reprojection_report`` of the cameras the tracker is about to use and, after an alignment, ``..._before`` of the
        uncorrected ones; both on the cleaned depths at raw resolution.  None: not one launch."""
        self.last_reprojection_report = self.last_reprojection_report_before = None
        if reprojection_check is None:
            return
        from . import reproject
        if extrs_uncorrected is not None:
            self.last_reprojection_report_before = reproject.reprojection_report(rgbs, depths, intrs, extrs_uncorrected, reprojection_check,
                                                                                 depths_conf=depths_conf)
        self.last_reprojection_report = reproject.reprojection_report(rgbs, depths, intrs, extrs, reprojection_check, depths_conf=depths_conf)

    # ---- support points: rows (frame, world xyz) from the clip the model is about to see ------------------------------------------
    def _support_rows(self, depth, pix, kinv, einv, t):
        z = _bilinear_sample_depth(depth, pix[:, 0], pix[:, 1])
        world = self._unproject(pix, z, kinv, einv)
        return torch.cat([torch.full_like(world[:, :1], float(t)), world], 1)

    def _grid_rows(self, depths, kinv, einv, frames):
        """The global support grid (:101-120) of every view at ``frames`` (frame-major, then view), through the per-camera lift."""
        pix = points_on_a_grid(self.grid_size, tuple(depths.shape[-2:]), device=depths.device)
        return torch.cat([self._support_rows(depths[0, v, t, 0], pix, kinv[v, t], einv[v, t], t)
                          for t in frames for v in range(depths.shape[1])], 0)

    def _uniform_rows(self, depths, kinv, einv):
        """Uniformly sampled support points (:147-190): (t, y, x) rows from get_uniformly_sampled_pts -- the same two torch draws as
        the reference, from the global generator of the tensors' device -- lifted into the world through EVERY view's depth map
        (sample-major, then view), with the reference's argument order kept as it is: the column it calls y is scaled by the WIDTH
        and the one it calls x by the HEIGHT (:424-426), and out-of-map coordinates are clamped by the sampler."""
        _, V, T, _, height, width = depths.shape
        sp = get_uniformly_sampled_pts(self.num_uniformly_sampled_pts, T, (height, width), device=depths.device)[0]
        t_s, y_s, x_s = sp[:, 0].long(), sp[:, 1].float(), sp[:, 2].float()
        vid = torch.arange(V, device=depths.device).repeat(sp.shape[0])
        fid, xs, ys = t_s.repeat_interleave(V), x_s.repeat_interleave(V), y_s.repeat_interleave(V)
        return _lift(depths[0, :, :, 0], vid, fid, xs, ys, kinv, einv)

    def _local_grid_rows(self, queries, qt_d, qt, depths, intrs, extrs, kinv, einv):
        """Local support grids of ALL queries in one pass (:221-252): project every query into every view at its own frame (one
        device op, ONE readback instead of two .item() syncs per view and query), lay the grids out and clip them to the image on
        the host, then lift all surviving pixels at once on the device.  queries (N,4) with frames qt_d (device) = qt (host list)
        -> per query, the list of its views' rows (a view whose grid is wholly outside the image gives none)."""
        num_points, V, dev = queries.shape[0], depths.shape[1], queries.device
        height, width = depths.shape[-2:]
        local_rows = [[] for _ in range(num_points)]
        if not (self.local_grid_size > 0 and num_points > 0):
            return local_rows
        qh = torch.cat([queries[:, 1:], torch.ones(num_points, 1, device=dev)], 1)
        cam = torch.einsum("vnij,nj->vni", extrs[0][:, qt_d], qh)
        ph = torch.einsum("vnij,vnj->vni", intrs[0][:, qt_d], cam)
        centres = (ph[..., :2] / ph[..., 2:]).cpu()  # (V, N, 2) pixel (x, y)
        pix_l, vid_l, fid_l, counts = [], [], [], []
        for i in range(num_points):
            for v in range(V):
                px, py = centres[v, i, 0].item(), centres[v, i, 1].item()
                pix = points_on_a_grid(self.local_grid_size, (self.local_extent, self.local_extent), (py, px), "cpu")
                ok = (pix[:, 0] >= 0) & (pix[:, 0] < width) & (pix[:, 1] >= 0) & (pix[:, 1] < height)
                k = int(ok.sum())
                counts.append(k)
                if k:
                    pix_l.append(pix[ok])
                    vid_l.append(torch.full((k,), v, dtype=torch.long))
                    fid_l.append(torch.full((k,), qt[i], dtype=torch.long))
        if pix_l:
            pix_all = torch.cat(pix_l).to(dev)
            rows_all = _lift(depths[0, :, :, 0], torch.cat(vid_l).to(dev), torch.cat(fid_l).to(dev), pix_all[:, 0], pix_all[:, 1], kinv, einv)
            o = 0
            for j, k in enumerate(counts):  # (query-major, then view; empty grids have no rows)
                if k:
                    local_rows[j // V].append(rows_all[o:o + k])
                    o += k
        return local_rows

    # ---- dispatch: each mode returns (traj_e (1,T,N,3), vis_e (1,T,N), the model's NaN flags) ------------------------------------
    def _run_joint(self, rgbs, depths, queries, support, fwd):
        """One forward of [the queries; the support rows] (:341-360)."""
        n = queries.shape[0]
        res = self.model(rgbs, depths=depths, query_points=torch.cat([queries, support], 0)[None], **fwd)
        return res["traj_e"][:, :, :n, :], res["vis_e"][:, :, :n], [getattr(self.model, "last_nan_flag", None)]

    def _run_groups(self, rgbs, depths, queries, support, fwd, groups):
        """Joint mode per group: every id's queries with the support rows, all sets through one grouped forward."""
        T, dev = rgbs.shape[2], rgbs.device
        traj_e = torch.zeros(1, T, queries.shape[0], 3, device=dev)
        vis_e = torch.zeros(1, T, queries.shape[0], device=dev)
        rows = [torch.from_numpy(g).to(dev) for g in groups]
        qs = [torch.cat([queries[r], support], 0)[None] for r in rows]
        for r, res in zip(rows, self.model.forward_grouped(rgbs, depths, qs, **fwd)):
            traj_e[:, :, r] = res["traj_e"][:, :, :len(r)]
            vis_e[:, :, r] = res["vis_e"][:, :, :len(r)]
        return traj_e, vis_e, [getattr(self.model, "last_nan_flag", None)]

    def _run_single_point(self, rgbs, depths, queries, support, fwd, kinv, einv):
        """One forward per query (or per ``single_point_group_size`` queries) with its local grids (:191-339)."""
        T, dev, num_points = rgbs.shape[2], rgbs.device, queries.shape[0]
        intrs, extrs = fwd["intrs"], fwd["extrs"]
        traj_e = torch.zeros(1, T, num_points, 3, device=dev)
        vis_e = torch.zeros(1, T, num_points, device=dev)
        qt_d = queries[:, 0].long()
        qt = qt_d.cpu().tolist()
        # The N forwards differ only in their queries: encoder, feature pyramid and point clouds are built ONCE and
        # shared (the reference re-encodes the clip for every query).  Every forward reads
        # frames >= its own first query frame only, so one store from the earliest query frame serves them all.
        if hasattr(self.model, "build_frame_store"):
            # (the global support grid starts at frame 0; backward tracking reads every frame before a query's too)
            t_first = 0 if (self.grid_size > 0 or self.backward_tracking or not qt) else max(0, min(qt))
            r0 = rgbs[0].contiguous() if rgbs.dtype == torch.uint8 else _f32(rgbs[0])
            fwd = dict(fwd, frame_store=self.model.build_frame_store(r0, _f32(depths[0]), _f32(intrs[0]), _f32(extrs[0]), t0=t_first))
        local_rows = self._local_grid_rows(queries, qt_d, qt, depths, intrs, extrs, kinv, einv)
        # The per-query forwards are independent (each has its own 64 virtual tracks, :254-275) and tiny -- a few hundred
        # tracks, pure launch-latency chains -- so they are issued round-robin on a few HIP streams and overlap on the GPU.
        G = max(1, int(self.single_point_group_size))
        if G > 1 and not hasattr(self.model, "forward_grouped"):
            raise NotImplementedError("single_point_group_size > 1 needs a model with forward_grouped")
        n_calls = (num_points + G - 1) // G
        n_streams = max(1, min(self.single_point_streams, n_calls)) if dev.type == "cuda" else 1
        main = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
        streams = self._streams(dev, n_streams) if n_streams > 1 else []
        nan_flags = []
        for s_ in streams:
            s_.wait_stream(main)
        for c in range(n_calls):
            ctx = torch.cuda.stream(streams[c % n_streams]) if streams else contextlib.nullcontext()
            with ctx:  # (everything of a call, its input rows included, is enqueued on its own stream)
                ids = range(c * G, min((c + 1) * G, num_points))
                qs = [torch.cat([queries[i:i + 1]] + local_rows[i] + [support], 0)[None] for i in ids]
                if G == 1:
                    res_l = [self.model(rgbs, depths=depths, query_points=qs[0], **fwd)]
                else:  # G query sets through one launch sequence (MVTracker.forward_grouped)
                    res_l = self.model.forward_grouped(rgbs, depths, qs, **fwd)  # (the same options as the per-query calls)
                for i, res in zip(ids, res_l):
                    traj_e[:, :, i] = res["traj_e"][:, :, 0]
                    vis_e[:, :, i] = res["vis_e"][:, :, 0]
                nan_flags.append(getattr(self.model, "last_nan_flag", None))
        for s_ in streams:
            main.wait_stream(s_)
        return traj_e, vis_e, nan_flags

    def _nan_guard(self, flags):
        """Deferred NaN guard of the model (reference mvtracker.py:401-404 logs in the iteration where the NaN appears): the caller is
        about to copy the tracks to the host anyway, so ONE flag read at the end of ``forward`` / ``finish`` costs nothing."""
        flags = [f.reshape(()) for f in flags if f is not None]
        self.last_nan = bool(flags) and int(torch.stack(flags).max().item()) != 0
        if self.last_nan:
            log.error("Got NaN values in coords, perhaps the training exploded")

    # ---- forward ---------------------------------------------------------------------------
    @torch.no_grad()
    @hip.guarded
    def forward(
            self,
            rgbs,
            depths,
            query_points_3d,
            intrs,
            extrs,
            save_debug_logs=False,
            debug_logs_path="",
            query_points_view=None,
            scene_transform=None,
            depths_conf=None,
            depth_cleaning=None,
            camera_alignment=None,
            reprojection_check=None,
            track_overlay=None,
            query_groups=None,
            rigid_motion=None,
            **kwargs,
    ):
        """``rigid_motion``: a ``RigidMotion``: after the tracking, one rigid pose per object and frame is fitted to the tracks on the
        device (``mvtracker_amd.rigid_motion``) and the result is kept as ``last_rigid_motion`` (reset to None by every forward).  The
        objects are the ids of ``query_groups``; without ``query_groups`` every query belongs to object 0.  It runs on the caller's
        rows only (no support point takes part), in the caller's world (after the scene normalisation is undone), with the
        thresholded ``vis_e`` and the query frames of ``query_points_3d[..., 0]``.  Nothing the tracker reads is changed.  None: not
        one launch.
        ``query_groups``: (N,) integers, one per query (``mask_queries``' ``object_ids``): in joint mode the queries of every
        distinct id, in ascending id order, are a query set of their own -- [its queries; the support rows] -- and all sets go
        through ``MVTracker.forward_grouped``: per-object independent tracking in one encoder pass and one launch sequence, the
        results scattered back to the caller's rows.  Refused with ``single_point``, ``backward_tracking`` and a model without
        ``forward_grouped``.  None: the joint forward as it always was.
        ``track_overlay``: a ``TrackOverlay``: after the tracking, the tracks are drawn into every view's frames on the device
        (``mvtracker_amd.render_track_overlays``) and ``(video, colors)`` is kept as ``last_track_overlay``.  The overlay is drawn
        on the raw input frames, at the caller's resolution and in the caller's world: ``traj_e`` as returned, the thresholded
        ``vis_e``, the query frames of ``query_points_3d[..., 0]``, the raw ``intrs`` and the ``extrs`` the tracker used before any
        normalisation (after ``camera_alignment`` if given).  Nothing the tracker reads is changed; ``save_debug_logs`` stays
        accepted and ignored.  None: not one launch.  There is no stream form (``open_stream`` takes no overlay): a stream's tracks
        arrive one window after their frames, so a caller who kept the frames draws them with ``mvtracker_amd.open_track_overlay``.
        ``reprojection_check``: a ``ReprojectionCheck``: the cameras the tracker is about to use (after depth cleaning and camera
        alignment, before normalisation and resize) are judged by ``mvtracker_amd.reprojection_report`` and the report is kept as
        ``last_reprojection_report``; with ``camera_alignment`` the report of the uncorrected cameras is kept too, as
        ``last_reprojection_report_before``.  Nothing the tracker reads is changed.  None: not one launch.
        ``camera_alignment``: a ``CameraAlignment`` (the views are refined against each other by ``mvtracker_amd.align_cameras`` on
        the raw inputs after depth cleaning, so ``max_distance`` is in the caller's units) or a ready ``CameraCorrection``; everything
        below sees ``correction.apply(extrs)``, and the correction is kept as ``last_camera_correction``.  None: not one launch.
        ``depth_cleaning``: a ``DepthCleaning``: every (view, frame) depth map is cleaned of outliers first
        (``mvtracker_amd.clean_depths`` on the raw inputs, with ``depths_conf`` when given, so its radius is in the caller's units),
        and everything below sees the cleaned depths.  None: not one launch is issued.
        ``scene_transform``: a ``SceneTransform`` or ``"auto"`` (``auto_scene_normalization`` of the raw inputs, with
        ``depths_conf`` when given): depths, extrinsics and queries go to the model transformed, ``traj_e`` comes back in the
        caller's world, and the transform is kept as ``last_scene_transform``.  None: nothing is done."""
        batch_size, num_views, num_frames, _, height_raw, width_raw = rgbs.shape
        _, num_points, _ = query_points_3d.shape
        assert rgbs.shape == (batch_size, num_views, num_frames, 3, height_raw, width_raw)
        assert depths.shape == (batch_size, num_views, num_frames, 1, height_raw, width_raw)
        assert query_points_3d.shape == (batch_size, num_points, 4)
        assert intrs.shape == (batch_size, num_views, num_frames, 3, 3)
        assert extrs.shape == (batch_size, num_views, num_frames, 3, 4)
        if batch_size != 1:
            raise NotImplementedError
        if self.sift_size > 0:
            raise NotImplementedError
        groups = None if query_groups is None else self._query_groups(query_groups, num_points)
        hip.require_device(rgbs)
        self.last_track_overlay = None
        if track_overlay is not None:  # checked before anything is launched; drawn after the tracking
            from . import overlay
            overlay._check(track_overlay)
        self.last_rigid_motion = None
        if rigid_motion is not None:  # checked before anything is launched; fitted after the tracking
            from . import rigid
            rigid._check(rigid_motion)
        caller_rgbs, caller_query_frames = rgbs, query_points_3d[0, :, 0]  # the overlay is drawn on the caller's own frames
        # the clip stages, in the order the docstring promises; everything up to the resize works on the raw-resolution clip
        rgbs, depths, intrs, extrs = _cast(rgbs, depths, intrs, extrs, self.interp_shape)
        queries = query_points_3d.to(torch.float32)
        depths = _clean(depths, intrs, extrs, depth_cleaning, depths_conf)
        extrs, extrs_uncorrected = self._align(depths, intrs, extrs, camera_alignment, depths_conf)
        self._reproject(rgbs, depths, intrs, extrs, extrs_uncorrected, reprojection_check, depths_conf)
        caller_intrs, caller_extrs = intrs, extrs  # the overlay's cameras: before the normalisation and the resize
        xf = self.last_scene_transform = self._scene_transform(scene_transform, (depths, intrs, extrs, depths_conf))
        depths, extrs, queries = _normalise(xf, depths, extrs, queries)
        rgbs, depths, intrs = _resize(rgbs, depths, intrs, self.interp_shape)
        # support points, in the reference's order: grid rows, then uniform rows
        kinv, einv = self._invert(intrs[0], extrs[0])
        support = torch.zeros(0, 4, device=rgbs.device)
        if self.grid_size > 0:
            support = self._grid_rows(depths, kinv, einv, range(0, num_frames, max(1, num_frames // self.n_grids_per_view)))
        if self.num_uniformly_sampled_pts > 0:
            support = torch.cat([support, self._uniform_rows(depths, kinv, einv)], 0)
        # dispatch: the model's keyword arguments are the same in every mode
        fwd = dict(intrs=intrs, extrs=extrs, iters=self.n_iters, save_debug_logs=save_debug_logs,
                   debug_logs_path=debug_logs_path, query_points_view=query_points_view, **kwargs)
        if self.backward_tracking:
            if self.single_point and int(self.single_point_group_size) > 1:
                raise NotImplementedError("backward_tracking with single_point_group_size > 1: forward_grouped has no backward tracking "
                                          "(use group size 1)")
            fwd["backward_tracking"] = True
        if self.single_point:
            traj_e, vis_e, nan_flags = self._run_single_point(rgbs, depths, queries[0], support, fwd, kinv, einv)
        elif groups is not None:
            traj_e, vis_e, nan_flags = self._run_groups(rgbs, depths, queries[0], support, fwd, groups)
        else:
            traj_e, vis_e, nan_flags = self._run_joint(rgbs, depths, queries[0], support, fwd)
        self._nan_guard(nan_flags)
        if xf is not None:
            traj_e = xf.restore_tracks(traj_e)
        if track_overlay is not None:
            self.last_track_overlay = overlay.render_track_overlays(caller_rgbs[0], traj_e[0], vis_e[0] > self.visibility_threshold, caller_query_frames,
                                                                    caller_intrs[0], caller_extrs[0], track_overlay)
        if rigid_motion is not None:
            self.last_rigid_motion = self._rigid_motion(traj_e[0], vis_e[0] > self.visibility_threshold, caller_query_frames, query_groups,
                                                        rigid_motion)
        return {"traj_e": traj_e, "vis_e": vis_e > self.visibility_threshold, "vis_e_as_prob": vis_e}

    @staticmethod
    def _rigid_motion(tracks, visible, query_frames, query_groups, options):
        """The poses of the caller's rows: the objects are ``query_groups``' ids (their number is known from the host copy
        ``_query_groups`` already took, so nothing is read back here), or object 0 for every row."""
        from . import rigid
        n, dev = tracks.shape[1], tracks.device
        if query_groups is None:
            ids, num = torch.zeros(n, dtype=torch.int32, device=dev), 1
        else:
            host = torch.as_tensor(query_groups).cpu()
            ids, num = host.to(torch.int32).to(dev), max(int(host.max()) + 1, 0)
        return rigid.rigid_motion(tracks.contiguous(), visible.contiguous(), query_frames.to(torch.int32), ids, options, num_objects=num)

    @staticmethod
    def sample_queries(depths, intrs, extrs, spec=None, **kw):
        """Query points for a clip without labels (``mvtracker_amd.queries.sample_queries``; the evaluator's sampling,
        evaluation/evaluator_3dpt.py:286-388): a (1, N, 4) tensor for ``forward(query_points_3d=...)``, ``open_stream(...)`` or a
        session's ``add_queries(...)``.  The inputs are the clip as ``forward`` takes it; ``interp_shape`` plays no part (a nearest
        resize with rescaled intrinsics keeps world points, and the queries are in world space).  Keyword arguments go through as
        they are: ``region=`` / ``region_poses=`` put the queries on the thing at a pose, ``motion=`` / ``rgbs=`` / ``motion_keep=`` on
        what moves (or on the static background)."""
        from . import queries
        return queries.sample_queries(depths, intrs, extrs, queries.DEFAULT_SPEC if spec is None else spec, **kw)

    @staticmethod
    def mask_queries(labels, depths, intrs, extrs, options=None, **kw):
        """Query points per segmented object (``mvtracker_amd.masks.mask_queries``): ``(query_points (1, N, 4), object_ids (N,),
        report)`` from per-camera instance masks; ``forward(query_points_3d=query_points, query_groups=object_ids)`` then tracks
        every object on its own."""
        from . import masks
        return masks.mask_queries(labels, depths, intrs, extrs, masks.MaskQueries() if options is None else options, **kw)

    def open_stream(self, query_points_3d, ring_blocks=3, scene_transform=None, depth_cleaning=None):
        """Streaming form of ``forward`` in joint mode (``MVTracker.open_stream``): returns a session whose
        ``push(rgbs, depths, intrs, extrs)`` / ``finish()`` give {"frames": (a, b), "traj_e", "vis_e", "vis_e_as_prob"} for the
        frames that became final, the same bits as ``forward`` on the whole clip.  ``scene_transform``: a ``SceneTransform`` applied
        to the queries here, to every pushed block's depths and extrinsics, and undone on every returned chunk (``"auto"`` is
        refused: it needs a frame before the session has one).  ``depth_cleaning``: a ``DepthCleaning`` applied to every pushed block
        before anything else (``push(..., depths_conf=...)`` takes the block's confidence map); clouds are per (view, frame), so
        the streamed clip is cleaned exactly as the offline one."""
        if self.single_point:
            raise NotImplementedError("there is no streaming form of single_point mode (one forward per query, each with local "
                                      "support grids around the query): use forward")
        if self.backward_tracking:
            raise NotImplementedError("there is no streaming form of backward_tracking (inherently offline)")
        if self.sift_size > 0 or self.num_uniformly_sampled_pts > 0:
            raise NotImplementedError("streaming supports the support grid only: uniformly sampled support points are drawn over the "
                                      "whole clip, whose length a session does not know")
        if self.grid_size > 0 and self.n_grids_per_view != 1:
            raise NotImplementedError(f"streaming takes the support grid from the first pushed frame (n_grids_per_view == 1, the "
                                      f"reference's t = 0 grid); n_grids_per_view = {self.n_grids_per_view} places grids at frames that "
                                      f"depend on the clip length")
        if depth_cleaning is not None:
            from . import clean
            clean._check(depth_cleaning)
        xf = self.last_scene_transform = self._scene_transform(scene_transform)
        return _PredictorStream(self, query_points_3d, ring_blocks, xf, depth_cleaning)


class _PredictorStream:
    """``EvaluationPredictor.open_stream``: every pushed block goes through ``forward``'s own cast, clean, normalise and resize and
    comes back thresholded as there; the support grid is added as queries (behind the caller's) when the first frame arrives."""

    def __init__(self, predictor, query_points_3d, ring_blocks, scene_transform=None, depth_cleaning=None):
        self.p = predictor
        self.xf = scene_transform
        self.cleaning = depth_cleaning
        if query_points_3d.dim() != 3 or query_points_3d.shape[0] != 1 or query_points_3d.shape[2] != 4:
            raise ValueError(f"query points must be (1, N, 4), got {tuple(query_points_3d.shape)}")
        self.num_points = query_points_3d.shape[1]
        if self.xf is not None:
            query_points_3d = self.xf.apply(query_points=query_points_3d)[2]
        self.session = predictor.model.open_stream(query_points_3d.to(torch.float32), iters=predictor.n_iters, ring_blocks=ring_blocks)
        self.first = True

    def _result(self, res):
        vis = res["vis_e"][:, :, :self.num_points]
        traj = res["traj_e"][:, :, :self.num_points, :]
        if self.xf is not None:
            traj = self.xf.restore_tracks(traj)
        return {"frames": res["frames"], "traj_e": traj, "vis_e": vis > self.p.visibility_threshold, "vis_e_as_prob": vis}

    @torch.no_grad()
    def push(self, rgbs, depths, intrs, extrs, depths_conf=None):
        p = self.p
        with hip.device_guard(rgbs):
            hip.require_device(rgbs)
            rgbs, depths, intrs, extrs = _cast(rgbs, depths, intrs, extrs, p.interp_shape)
            depths = _clean(depths, intrs, extrs, self.cleaning, depths_conf)
            depths, extrs, _ = _normalise(self.xf, depths, extrs)
            rgbs, depths, intrs = _resize(rgbs, depths, intrs, p.interp_shape)
            if self.first and p.grid_size > 0:  # the reference's t = 0 support grid (:101-120), from the first pushed frame
                kinv, einv = p._invert(intrs[0, :, :1], extrs[0, :, :1])
                self.session.add_queries(p._grid_rows(depths, kinv, einv, [0])[None])
            self.first = False
            return self._result(self.session.push(rgbs, depths, intrs, extrs))

    @torch.no_grad()
    def finish(self):
        res = self.session.finish()
        self.p._nan_guard([self.session.nan_flag])
        return self._result(res)
