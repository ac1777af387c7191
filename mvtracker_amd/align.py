"""Camera alignment on the device ("Camera alignment"): point-to-plane ICP of every view's clouds onto the clouds
of the other views, so that extrinsics that are off by a few centimetres do not show up as a second copy of every surface in the
fused cloud the tracker searches.

The reference does this with Open3D (conversions/droid/utils/optimization.py ``run_icp_point_to_plane``: ``registration_icp`` with
``TransformationEstimationPointToPlane``, ``max_correspondence_distance=0.05``); here the same loop runs in
``mvt_clean_points`` -> ``mvt_align_normals`` -> ``mvt_tile_aabb`` -> ``mvt_tile_group_aabb`` and then, per view,
(``mvt_align_correspond`` -> ``mvt_align_solve``) x (max_iterations + 1) -> ``mvt_align_transform`` with no host read.

    a = CameraAlignment(max_distance=0.05, frames=(0,))
    c = align_cameras(depths, intrs, extrs, a)                      # CameraCorrection: one rigid transform per view
    extrs_fixed = c.apply(extrs)                                    # extrs @ inv(D_v)
    out = predictor(rgbs=..., depths=..., ..., camera_alignment=a)  # after depth cleaning, before normalisation and resize
    T, fitness, rmse = align_point_clouds(source, target, target_normals, 0.05, 30)   # registration_icp on point lists
    T, fitness, rmse = align_point_clouds(source, target, None, 0.05, 30)             # the target's normals by PCA (cloud.py)
    a = PcaCameraAlignment(max_distance=0.05, normal_radius=0.1)                      # PCA normals instead of the grid cross product
"""
from __future__ import annotations

import math

import torch

from . import hip
from .clip import MAX_POINTS, DepthClip, list_cloud


class CameraAlignment:
    """``max_distance``: the correspondence cap (Open3D's ``max_correspondence_distance``, strict), in the caller's units;
    ``max_iterations`` per ICP run; ``sweeps`` over the views; ``frames`` whose clouds are aligned (correspondences within a frame,
    one set of normal equations over all of them); ``anchor``: the view that stays fixed; ``sample_stride``: every s-th pixel row and
    column of the source view is a query; ``normal_max_edge``: a normal needs its four grid neighbours within this distance (None:
    ``max_distance``); ``conf_thresh``: with a confidence map only pixels with conf > conf_thresh enter the clouds."""

    def __init__(self, max_distance=0.05, max_iterations=30, sweeps=2, frames=(0,), anchor=0, sample_stride=1, normal_max_edge=None,
                 conf_thresh=None):
        if not (math.isfinite(float(max_distance)) and float(max_distance) > 0.0):
            raise ValueError(f"max_distance must be finite and positive, got {max_distance!r}")
        if int(max_iterations) != max_iterations or not 1 <= int(max_iterations) <= 1000:
            raise ValueError(f"max_iterations must be an integer in 1..1000, got {max_iterations!r}")
        if int(sweeps) != sweeps or not 1 <= int(sweeps) <= 100:
            raise ValueError(f"sweeps must be an integer in 1..100, got {sweeps!r}")
        try:
            fr = tuple(frames)
        except TypeError:
            raise ValueError(f"frames must be a sequence of frame indices, got {frames!r}") from None
        if not fr or any(int(f) != f or int(f) < 0 for f in fr) or len(set(int(f) for f in fr)) != len(fr):
            raise ValueError(f"frames must be distinct integers >= 0, at least one, got {frames!r}")
        if int(anchor) != anchor or int(anchor) < 0:
            raise ValueError(f"anchor must be an integer >= 0, got {anchor!r}")
        if int(sample_stride) != sample_stride or not 1 <= int(sample_stride) <= 64:
            raise ValueError(f"sample_stride must be an integer in 1..64, got {sample_stride!r}")
        if normal_max_edge is not None and not (math.isfinite(float(normal_max_edge)) and float(normal_max_edge) > 0.0):
            raise ValueError(f"normal_max_edge must be finite and positive, got {normal_max_edge!r}")
        if conf_thresh is not None and not math.isfinite(float(conf_thresh)):
            raise ValueError(f"conf_thresh must be finite, got {conf_thresh!r}")
        self.max_distance, self.max_iterations, self.sweeps = float(max_distance), int(max_iterations), int(sweeps)
        self.frames, self.anchor, self.sample_stride = tuple(int(f) for f in fr), int(anchor), int(sample_stride)
        self.normal_max_edge = self.max_distance if normal_max_edge is None else float(normal_max_edge)
        self.conf_thresh = None if conf_thresh is None else float(conf_thresh)

    def __repr__(self):
        return (f"CameraAlignment(max_distance={self.max_distance}, max_iterations={self.max_iterations}, sweeps={self.sweeps}, "
                f"frames={self.frames}, anchor={self.anchor}, sample_stride={self.sample_stride}, normal_max_edge={self.normal_max_edge}, "
                f"conf_thresh={self.conf_thresh})")


class PcaCameraAlignment(CameraAlignment):
    """A ``CameraAlignment`` whose target normals come from ``mvt_normals_estimate`` (a PCA over each point's ``normal_max_nn`` nearest
    points within ``normal_radius``; None: ``max_distance``), the reference's estimate_normals, instead of the cross product of
    grid neighbours: coarse or oblique views keep their normals.  ``normal_max_edge`` is unused."""

    def __init__(self, max_distance=0.05, max_iterations=30, sweeps=2, frames=(0,), anchor=0, sample_stride=1, normal_max_edge=None,
                 conf_thresh=None, normal_radius=None, normal_max_nn=30):
        super().__init__(max_distance, max_iterations, sweeps, frames, anchor, sample_stride, normal_max_edge, conf_thresh)
        from . import cloud
        r = self.max_distance if normal_radius is None else normal_radius
        self.normal_radius, self.normal_max_nn = cloud.check_normal_search(r, normal_max_nn)

    def __repr__(self):
        return f"Pca{super().__repr__()[:-1]}, normal_radius={self.normal_radius}, normal_max_nn={self.normal_max_nn})"


def _check(alignment):
    if not isinstance(alignment, CameraAlignment):
        raise ValueError(f"alignment must be a CameraAlignment, got {alignment!r}")
    return alignment


class CameraCorrection:
    """The result of ``align_cameras``: ``transforms`` (V,4,4) fp64 on the device, D_v moving view v's world points onto the other
    views' (identity for the anchor), and per view the last ICP run's ``fitness``, ``rmse`` (fp64), ``iterations`` and ``status``
    (int32; bits ``hip.ALIGN_FEW``, ``hip.ALIGN_SINGULAR``), all on the device."""

    def __init__(self, transforms, fitness=None, rmse=None, iterations=None, status=None):
        if transforms.dim() != 3 or tuple(transforms.shape[1:]) != (4, 4):
            raise ValueError(f"transforms must be (V, 4, 4), got {tuple(transforms.shape)}")
        V, dev = transforms.shape[0], transforms.device
        self.transforms = transforms.to(torch.float64)
        self.fitness = torch.zeros(V, dtype=torch.float64, device=dev) if fitness is None else fitness
        self.rmse = torch.zeros(V, dtype=torch.float64, device=dev) if rmse is None else rmse
        self.iterations = torch.zeros(V, dtype=torch.int32, device=dev) if iterations is None else iterations
        self.status = torch.zeros(V, dtype=torch.int32, device=dev) if status is None else status

    def inverse_transforms(self):
        """inv(D_v) (V,4,4) fp64, closed form (adjugate of the 3x3 block): D_v need not be exactly orthogonal."""
        R, t = self.transforms[:, :3, :3], self.transforms[:, :3, 3]
        c0, c1, c2 = (torch.linalg.cross(R[:, a], R[:, b]) for a, b in ((1, 2), (2, 0), (0, 1)))
        Ri = torch.stack([c0, c1, c2], -1) / (R[:, 0] * c0).sum(-1)[:, None, None]
        out = torch.zeros_like(self.transforms)
        out[:, :3, :3] = Ri
        out[:, :3, 3] = -(Ri * t[:, None, :]).sum(-1)
        out[:, 3, 3] = 1.0
        return out

    def apply(self, extrs):
        """World-to-camera extrinsics (..., V, T, 3, 4) of the corrected cameras: ``extrs @ inv(D_v)`` per view (a point D_v X of the
        corrected world lands where X landed), computed in fp64 and rounded to the dtype of ``extrs`` once."""
        if extrs.dim() < 4 or tuple(extrs.shape[-2:]) != (3, 4) or extrs.shape[-4] != self.transforms.shape[0]:
            raise ValueError(f"extrs must be (..., {self.transforms.shape[0]}, T, 3, 4), got {tuple(extrs.shape)}")
        inv = self.inverse_transforms().to(extrs.device)[:, None]  # (V, 1, 4, 4)
        e = extrs.to(torch.float64)
        prod = (e[..., :3].unsqueeze(-1) * inv[..., :3, :].unsqueeze(-3)).sum(-2)  # E_R [inv_R | inv_t], element-wise: no BLAS call
        rot, tr = prod[..., :3], prod[..., 3] + e[..., 3]
        return torch.cat([rot, tr[..., None]], -1).to(extrs.dtype)


def query_slots(n_points, grid=(0, 0), sample_stride=1):
    """Source point index of every query slot of ``mvt_align_correspond`` (int64, tiles * 64; -1: the slot holds no query)."""
    ntq, tpr = hip.align_queries(n_points, grid, sample_stride)
    slot = torch.arange(ntq * 64)
    if grid[0] == 0:
        return torch.where(slot < n_points, slot, torch.full_like(slot, -1))
    s = sample_stride
    ws, hs = (grid[0] + s - 1) // s, (grid[1] + s - 1) // s
    tile, lane = slot // 64, slot % 64
    sy, sx = (tile // tpr) * 8 + lane // 8, (tile % tpr) * 8 + lane % 8
    return torch.where((sy < hs) & (sx < ws), sy * s * grid[0] + sx * s, torch.full_like(slot, -1))


def cap_squared(max_distance):
    """cap2 of the search: fl(fl(cap) * fl(cap)) in fp32."""
    c = torch.tensor(float(max_distance), dtype=torch.float32)
    return float(c * c)


def build_search(xyz, n_clouds, n_points, grid, box, gbox):
    box, gbox = box.view(n_clouds, -1, 8), gbox.view(n_clouds, -1, 8)
    hip.tile_aabb(xyz, n_points, n_clouds, box, grid)
    hip.tile_group_aabb(box, n_points, n_clouds, gbox)


class IcpRun:
    """One ICP problem on the device: the source clouds ``src0`` (frames, P, 4) as they were before any correction, its transform
    ``D`` (12 doubles on the device, updated in place), and the target clouds (dicts of xyz, nrm, box, gbox, P, grid).  ``step``
    enqueues one (correspond, solve) pair; ``run`` the whole fixed sequence.  ``keep_queries``: keep the per-query index and d2."""

    def __init__(self, src0, n_points, grid, frames, targets, max_distance, sample_stride, D, max_iterations, result=None, keep_queries=False):
        if not 1 <= len(targets) <= hip.ALIGN_MAX_TARGETS:
            raise ValueError(f"an ICP run takes 1..{hip.ALIGN_MAX_TARGETS} target clouds, got {len(targets)}")
        dev = src0.device
        self.src0, self.P, self.grid, self.frames, self.targets = src0, n_points, grid, frames, targets
        self.cap2, self.stride, self.D, self.max_iterations = cap_squared(max_distance), sample_stride, D, max_iterations
        self.ntq = hip.align_queries(n_points, grid, sample_stride)[0]
        self.partial = torch.zeros(frames, self.ntq, hip.ALIGN_ROW, dtype=torch.float64, device=dev)
        self.istate = torch.zeros(4, dtype=torch.int32, device=dev)
        self.hist = torch.zeros(max_iterations + 1, hip.ALIGN_HIST, dtype=torch.float64, device=dev)
        self.sums = torch.zeros(hip.ALIGN_ROW, dtype=torch.float64, device=dev)
        self.result = torch.zeros(4, dtype=torch.float64, device=dev) if result is None else result
        self.q_idx = torch.full((frames, self.ntq * 64), -1, dtype=torch.int32, device=dev) if keep_queries else None
        self.q_d2 = torch.zeros(frames, self.ntq * 64, dtype=torch.float32, device=dev) if keep_queries else None
        ok = torch.isfinite(src0.reshape(frames, n_points, 4)[..., :3]).all(-1)
        if grid[0]:  # the sampled pixels
            ok = ok.reshape(frames, grid[1], grid[0])[:, ::sample_stride, ::sample_stride]
        self.n_queries = ok.sum().to(torch.float64).reshape(1)  # source points taking part: the divisor of fitness (stays on the device)

    def step(self, final=False):
        hip.align_correspond(self.src0, self.P, self.grid, self.stride, self.frames, self.D, self.cap2, self.targets, self.istate, self.partial,
                             self.q_idx, self.q_d2)
        hip.align_solve(self.partial, self.frames * self.ntq, self.n_queries, final, self.D, self.istate, self.hist, self.result, self.sums)

    def run(self):
        for i in range(self.max_iterations + 1):
            self.step(final=i == self.max_iterations)


def _rows12(T44):
    return T44[..., :3, :].reshape(*T44.shape[:-2], 12).contiguous()


def _eye_rows(n, dev):
    return _rows12(torch.eye(4, dtype=torch.float64, device=dev).expand(n, 4, 4))


def _to44(D):
    out = torch.zeros(*D.shape[:-1], 4, 4, dtype=torch.float64, device=D.device)
    out[..., :3, :] = D.reshape(*D.shape[:-1], 3, 4)
    out[..., 3, 3] = 1.0
    return out


class ClipAlignment:
    """The device state of ``align_cameras`` on a clip (V,T,1,H,W) with cameras (V,T,3,3) / (V,T,3,4): every view's clouds of the
    chosen frames as unprojected (``xyz0``) and as they stand now (``xyz``), their normals and boxes, all (V, F, ...) so that a view's
    part is contiguous, and the transforms ``D`` (V,12) fp64.  ``icp(v)`` is the ``IcpRun`` of view v against all other views as they
    stand; ``commit(v)`` moves view v's clouds by D[v] and rebuilds its normals and boxes."""

    def __init__(self, depths, intrs, extrs, alignment, depths_conf=None):
        a = self.alignment = _check(alignment)
        clip = DepthClip(depths, intrs, extrs, depths_conf)
        V, T, dev = clip.V, clip.T, clip.dev
        if not 2 <= V <= hip.ALIGN_MAX_TARGETS + 1:
            raise ValueError(f"camera alignment takes 2..{hip.ALIGN_MAX_TARGETS + 1} views, got {V}")
        if a.anchor >= V:
            raise ValueError(f"anchor {a.anchor} is not one of the {V} views")
        if max(a.frames) >= T:
            raise ValueError(f"frames {a.frames} reach past the clip's {T} frames")
        Hp, Wp, P = clip.padded_grid()
        F = len(a.frames)
        if V * P >= MAX_POINTS:
            raise ValueError(f"{V} clouds of {Hp} x {Wp} points are too large (the limit is 2^31 target points)")
        self.V, self.F, self.P, self.grid = V, F, P, (Wp, Hp)
        nt = P // 64
        self.xyz0 = torch.empty(V, F, P, 4, device=dev)
        for fi, t in enumerate(a.frames):
            self.xyz0[:, fi] = clip.clouds(t, 1, a.conf_thresh)
        self.xyz = self.xyz0.clone()  # (D = identity: the same bits)
        self.nrm = torch.empty(V, F, P, 4, device=dev)
        self.box = torch.empty(V, F, nt, 8, device=dev)
        self.gbox = torch.empty(V, F, (nt + 63) // 64, 8, device=dev)
        self.rebuild(self.xyz, V * F, self.nrm, self.box, self.gbox)
        self.D = _eye_rows(V, dev)
        self.results = torch.zeros(V, 4, dtype=torch.float64, device=dev)

    def rebuild(self, xyz, n_clouds, nrm, box, gbox):
        """Normals and boxes of clouds that have just been written: the grid cross product, then the boxes; for a
        ``PcaCameraAlignment`` the boxes first, since the PCA's neighbour search walks them."""
        a = self.alignment
        if isinstance(a, PcaCameraAlignment):
            from . import cloud
            build_search(xyz, n_clouds, self.P, self.grid, box, gbox)
            cloud.normals_of_clouds(xyz, n_clouds, self.P, self.grid, a.normal_radius, a.normal_max_nn, nrm=nrm, box=box, gbox=gbox)
        else:
            hip.align_normals(xyz, n_clouds, self.grid, a.normal_max_edge, nrm)
            build_search(xyz, n_clouds, self.P, self.grid, box, gbox)

    def targets(self, v):
        return [dict(xyz=self.xyz[u], nrm=self.nrm[u], box=self.box[u], gbox=self.gbox[u], P=self.P, grid=self.grid) for u in range(self.V) if u != v]

    def icp(self, v, keep_queries=False):
        a = self.alignment
        return IcpRun(self.xyz0[v], self.P, self.grid, self.F, self.targets(v), a.max_distance, a.sample_stride, self.D[v], a.max_iterations,
                      result=self.results[v], keep_queries=keep_queries)

    def commit(self, v):
        hip.align_transform(self.xyz0[v], self.D[v], self.F * self.P, self.xyz[v])  # the view as it stands now, for the views that follow
        self.rebuild(self.xyz[v], self.F, self.nrm[v], self.box[v], self.gbox[v])

    def run(self):
        for _ in range(self.alignment.sweeps):
            for v in range(self.V):
                if v != self.alignment.anchor:
                    self.icp(v).run()
                    self.commit(v)
        r = self.results
        return CameraCorrection(_to44(self.D), r[:, 0].clone(), r[:, 1].clone(), r[:, 2].to(torch.int32), r[:, 3].to(torch.int32))


def align_clip(depths, intrs, extrs, alignment, depths_conf=None):
    """``align_cameras`` on a clip (V,T,1,H,W) with cameras (V,T,3,3) / (V,T,3,4)."""
    return ClipAlignment(depths, intrs, extrs, alignment, depths_conf).run()


@hip.guarded
def align_cameras(depths, intrs, extrs, alignment, depths_conf=None):
    """Refines the cameras of a clip against each other.  depths (V,T,1,H,W) or (1,V,T,1,H,W) with intrs / extrs (and
    ``depths_conf``) of the same rank, as ``EvaluationPredictor.forward`` takes them.  The anchor view stays fixed; in every sweep
    each other view v, in view order, is aligned by point-to-plane ICP onto the union of all other views as they stand at that
    moment (their current corrections applied), after which its clouds are moved and its boxes and normals rebuilt.  There is one
    rigid correction per view for the whole clip.  Returns a ``CameraCorrection``; the inputs are not written."""
    return align_clip(depths, intrs, extrs, alignment, depths_conf)


def list_problem(source, target, target_normals, max_distance, max_iterations, init=None, keep_queries=False, normal_radius=0.05,
                 normal_max_nn=30):
    """The ``IcpRun`` of ``align_point_clouds`` (point lists: linear tiles)."""
    from . import cloud
    if not (math.isfinite(float(max_distance)) and float(max_distance) > 0.0):
        raise ValueError(f"max_distance must be finite and positive, got {max_distance!r}")
    if int(max_iterations) != max_iterations or not 1 <= int(max_iterations) <= 1000:
        raise ValueError(f"max_iterations must be an integer in 1..1000, got {max_iterations!r}")
    src = list_cloud(source, "source")
    tgt = list_cloud(target, "target")
    if target_normals is None:
        cloud.check_normal_search(normal_radius, normal_max_nn)
    elif tuple(target_normals.shape) != tuple(target.shape):
        raise ValueError(f"target_normals must have the shape of target, got {tuple(target_normals.shape)}")
    if init is not None and tuple(init.shape) != (4, 4):
        raise ValueError(f"init must be (4, 4), got {tuple(init.shape)}")
    dev = source.device
    M, N = source.shape[0], target.shape[0]
    if target_normals is None:
        target_normals = cloud.estimate_normals(target, normal_radius, normal_max_nn)
    nrm = list_cloud(target_normals, "target_normals")
    box, gbox = hip.cloud_boxes(tgt, 1, N, (0, 0))
    D = _eye_rows(1, dev)[0] if init is None else _rows12(init.to(device=dev, dtype=torch.float64))
    return IcpRun(src, M, (0, 0), 1, [dict(xyz=tgt, nrm=nrm, box=box, gbox=gbox, P=N, grid=(0, 0))], max_distance, 1, D, int(max_iterations),
                  keep_queries=keep_queries)


@hip.guarded
def align_point_clouds(source, target, target_normals, max_distance, max_iterations, init=None, *, normal_radius=0.05, normal_max_nn=30):
    """Open3D's ``registration_icp(source, target, max_distance, init, TransformationEstimationPointToPlane(),
    ICPConvergenceCriteria(max_iteration=max_iterations))`` on point lists: source (M,3), target (N,3) with normals (N,3), all on the
    device; rows that are not finite (and target rows without a finite normal) take no part.  Returns ``(transform, fitness, rmse)``:
    the 4x4 fp64 transform on the device that moves the source onto the target, and Open3D's two figures for it.
    ``target_normals=None``: they are ``estimate_normals(target, normal_radius, normal_max_nn)``, the reference's preparation."""
    run = list_problem(source, target, target_normals, max_distance, max_iterations, init, normal_radius=normal_radius, normal_max_nn=normal_max_nn)
    run.run()
    fitness, rmse = run.result[:2].tolist()
    return _to44(run.D), fitness, rmse
