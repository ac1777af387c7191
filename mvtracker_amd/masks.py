"""Mask queries on the device ("Mask queries"): per-camera 2-D instance masks (SAM2, HOISTFormer, ...) lifted to
world space through depth, the cameras' local ids matched into global object ids, and query points drawn per object.

The rules are those of the reference fork's explainers (MASK_LIFTING, GLOBAL_MASK_ID, AVERAGE_DISTANCE_MATCHING,
QUERY_POINTS_FROM_MASKS, PER_MASK_TRACKING), made exact: ``mvt_mask_stats`` keeps per (view, frame, label) the pixel counts and the
fixed-point coordinate sums of the valid pixels, ``mvt_mask_centroids`` / ``mvt_mask_match`` turn them into centroids and the greedy
"average distance" assignment, ``mvt_mask_relabel`` writes the clip in global ids and ``mvt_mask_pool`` compacts the pool of one
(object, frame) in ``frame_pool``'s order.  Everything summed is an integer: two runs give the same bits.  There is no CPU path.

    q, ids, report = mask_queries(labels, depths, intrs, extrs, MaskQueries(max_points_per_frame=256))
    res = predictor(rgbs, depths, q, intrs, extrs, query_groups=ids)        # every object tracked on its own, one launch sequence
    overlay = TrackOverlay(colors=object_colors(ids))
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Union

import numpy as np
import torch

from . import hip
from .clip import DepthClip

L = hip.MASK_LABELS


def _int(name, v, lo):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer)) or int(v) != v or int(v) < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return int(v)


@dataclass(frozen=True)
class MaskQueries:
    """``anchor``: "first" (an object's first frame with a valid pixel), a frame number for every object, or ``{(view, label): frame}``
    per camera and instance; the frames used are [anchor - frames_before, anchor + frames_after], clipped to the clip.  A labelled
    pixel is valid when its depth is finite, ``min_depth < depth <= max_depth`` and, with ``conf_thresh`` set, ``conf > conf_thresh``.
    A (view, frame, label) has a centroid from ``min_pixels`` valid pixels on.  ``match``: the cameras' ids are matched by their mean
    centroid distance over the common frames (at least ``min_common_frames`` of them), joined when it is strictly below
    ``distance_threshold``; False: label l is object l - 1 in every camera.  ``max_points_per_frame``: a larger pool is cut to that
    many rows by ``method`` "random" (a seeded permutation) or "kmeans" (the pool's k-means centres)."""
    anchor: Union[str, int, dict] = "first"
    frames_before: int = 3
    frames_after: int = 1
    min_depth: float = 1e-6
    max_depth: float = 10.0
    conf_thresh: Optional[float] = None
    min_pixels: int = 1
    match: bool = True
    distance_threshold: float = 0.15
    min_common_frames: int = 1
    max_points_per_frame: Optional[int] = None
    method: str = "random"

    def __post_init__(self):
        a = self.anchor
        if isinstance(a, dict):
            out = {}
            for key, f in a.items():
                if not (isinstance(key, tuple) and len(key) == 2):
                    raise ValueError(f"anchor keys must be (view, label), got {key!r}")
                v, l = _int("anchor view", key[0], 0), _int("anchor label", key[1], 1)
                if l > hip.MASK_MAX_LABEL:
                    raise ValueError(f"anchor label must be at most {hip.MASK_MAX_LABEL}, got {l}")
                out[(v, l)] = _int("anchor frame", f, 0)
            a = out
        elif isinstance(a, str):
            if a != "first":
                raise ValueError(f'anchor must be "first", a frame number or a dict {{(view, label): frame}}, got {a!r}')
        else:
            a = _int("anchor", a, 0)
        set_ = lambda k, v: object.__setattr__(self, k, v)
        set_("anchor", a)
        set_("frames_before", _int("frames_before", self.frames_before, 0))
        set_("frames_after", _int("frames_after", self.frames_after, 0))
        for k in ("min_depth", "max_depth", "distance_threshold"):
            if isinstance(getattr(self, k), bool) or not math.isfinite(float(getattr(self, k))):
                raise ValueError(f"{k} must be finite, got {getattr(self, k)!r}")
            set_(k, float(getattr(self, k)))
        if not self.min_depth < self.max_depth:
            raise ValueError(f"min_depth must be below max_depth, got {self.min_depth} and {self.max_depth}")
        if self.distance_threshold < 0:
            raise ValueError(f"distance_threshold must not be negative, got {self.distance_threshold}")
        if self.conf_thresh is not None:
            if isinstance(self.conf_thresh, bool) or not math.isfinite(float(self.conf_thresh)):
                raise ValueError(f"conf_thresh must be None or finite, got {self.conf_thresh!r}")
            set_("conf_thresh", float(self.conf_thresh))
        set_("min_pixels", _int("min_pixels", self.min_pixels, 1))
        set_("min_common_frames", _int("min_common_frames", self.min_common_frames, 1))
        if not isinstance(self.match, bool):
            raise ValueError(f"match must be a bool, got {self.match!r}")
        if self.max_points_per_frame is not None:
            set_("max_points_per_frame", _int("max_points_per_frame", self.max_points_per_frame, 1))
        if self.method not in ("random", "kmeans"):
            raise ValueError(f'method must be "random" or "kmeans", got {self.method!r}')
        if self.method == "kmeans" and self.max_points_per_frame is not None and self.max_points_per_frame > hip.KMEANS_MAX_K:
            raise ValueError(f"k-means draws at most {hip.KMEANS_MAX_K} points per frame, got {self.max_points_per_frame}")


def _check(options):
    if not isinstance(options, MaskQueries):
        raise ValueError(f"options must be a MaskQueries, got {options!r}")
    return options


def _readback(t):
    """The host copy of the tables: the one read of ``match_mask_ids`` / ``mask_queries``."""
    return t.cpu().numpy()


def labels_from_instances(masks):
    """(I,V,T,H,W) bool, or a dict name -> (V,T,H,W) bool in insertion order -> (V,T,H,W) uint8 labels: instance i becomes id i + 1,
    and where instances overlap the lowest i wins."""
    if isinstance(masks, dict):
        if not masks:
            raise ValueError("no instance masks")
        masks = torch.stack([torch.as_tensor(m) for m in masks.values()])
    masks = torch.as_tensor(masks)
    if masks.dim() != 5 or masks.dtype != torch.bool:
        raise ValueError(f"instance masks must be (I, V, T, H, W) bool, got {tuple(masks.shape)} {masks.dtype}")
    if not 1 <= masks.shape[0] <= hip.MASK_MAX_LABEL:
        raise ValueError(f"between 1 and {hip.MASK_MAX_LABEL} instances, got {masks.shape[0]}")
    out = torch.zeros(masks.shape[1:], dtype=torch.uint8, device=masks.device)
    for i in range(masks.shape[0] - 1, -1, -1):  # descending, so that the lowest instance is written last
        out = torch.where(masks[i], torch.full((), i + 1, dtype=torch.uint8, device=masks.device), out)
    return out


def _labels(labels):
    """(V,T,H,W) or (1,V,T,H,W), bool / uint8 / int16 / int32 / int64 with values 0..255 -> (V,T,H,W) uint8 contiguous, 16-byte
    aligned.  A wider type costs one read of its extremes."""
    if not isinstance(labels, torch.Tensor):
        raise ValueError(f"labels must be a tensor, got {type(labels).__name__}")
    if labels.dim() == 5:
        if labels.shape[0] != 1:
            raise ValueError(f"labels must be (V, T, H, W) or (1, V, T, H, W), got {tuple(labels.shape)}")
        labels = labels[0]
    if labels.dim() != 4 or min(labels.shape) < 1:
        raise ValueError(f"labels must be (V, T, H, W) or (1, V, T, H, W), got {tuple(labels.shape)}")
    if labels.dtype not in (torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f"labels must be bool, uint8, int16, int32 or int64, got {labels.dtype}")
    if labels.dtype not in (torch.bool, torch.uint8):
        lo, hi = (int(x) for x in torch.aminmax(labels))
        if lo < 0 or hi > hip.MASK_MAX_LABEL:
            raise ValueError(f"labels must lie in [0, {hip.MASK_MAX_LABEL}] (0 = background), got values from {lo} to {hi}")
    labels = labels.to(torch.uint8).contiguous()
    return labels.clone() if labels.data_ptr() % 16 else labels


class _Clip(DepthClip):
    """The checked inputs of one call: the depth clip (1,V,T,...) with its labels ``lab`` (V,T,H,W) uint8 and the options ``opt``."""

    def __init__(self, labels, depths, intrs, extrs, depths_conf, options):
        self.opt = _check(options)
        super().__init__(depths, intrs, extrs, depths_conf, batch="required")
        V, T, H, W = self.V, self.T, self.H, self.W
        self.lab = _labels(labels)
        if tuple(self.lab.shape) != (V, T, H, W):
            raise ValueError(f"labels {tuple(self.lab.shape)} and depths {tuple(depths.shape)} differ in (V, T, H, W)")
        if self.opt.conf_thresh is not None and depths_conf is None:
            raise ValueError("conf_thresh needs depths_conf")
        if V > hip.MASK_MAX_VIEWS or V * T > 65535 or H * W > 1 << 24 or V * H * W >= 1 << 31:
            raise ValueError(f"{V} views x {T} frames of {H} x {W} are too many for one call (at most {hip.MASK_MAX_VIEWS} views, 65535 "
                             f"images, 2^24 pixels per image)")
        if isinstance(self.opt.anchor, int) and self.opt.anchor >= T:
            raise ValueError(f"anchor frame {self.opt.anchor} is beyond the clip's {T} frames")
        if self.lab.device != self.dev:
            raise ValueError(f"labels on {self.lab.device}, depths on {self.dev}")
        self.kinv  # (inverted here: ahead of whatever the call launches, also when that is nothing)

    def pool_args(self, t):
        o = self.opt  # (the confidence map is read only under a threshold)
        return (self.lab, self.d, self.conf(o.conf_thresh), self.kinv, self.einv, self.V, self.T, int(t), self.H, self.W, o.min_depth, o.max_depth,
                0.0 if o.conf_thresh is None else o.conf_thresh)


class _Tables:
    """One int64 buffer for everything the host reads: the statistics (V,T,256,6) int64, the centroids (V,T,256,3) fp64, the
    winning distances (V,256) fp64, the id table (V,256) int32 and (objects, present ids) int32 -- one copy brings them all."""

    def __init__(self, V, T, dev):
        self.V, self.T = V, T
        self.sizes = (V * T * L * hip.MASK_STAT_WORDS, V * T * L * 3, V * L, V * L // 2, 1)
        self.buf = torch.zeros(sum(self.sizes), dtype=torch.int64, device=dev)
        s, c, d, g, st = self.parts(self.buf)
        self.stats = s.view(V, T, L, hip.MASK_STAT_WORDS)
        self.centroid = c.view(torch.float64).view(V, T, L, 3)
        self.distance = d.view(torch.float64).view(V, L)
        self.global_id = g.view(torch.int32).view(V, L)
        self.state = st.view(torch.int32)

    def parts(self, buf):
        out, o = [], 0
        for n in self.sizes:
            out.append(buf[o:o + n])
            o += n
        return out

    def host(self):
        V, T = self.V, self.T
        s, c, d, g, st = self.parts(_readback(self.buf))
        s = s.reshape(V, T, L, hip.MASK_STAT_WORDS)
        return {"stats": s, "centroid": c.view(np.float64).reshape(V, T, L, 3), "distance": d.view(np.float64).reshape(V, L),
                "global_id": g.view(np.int32).reshape(V, L), "num_objects": int(st.view(np.int32)[0]), "present": int(st.view(np.int32)[1])}


class MaskStatistics:
    """Per (view, frame, label), on the device: ``pixels`` (V,T,256) int64 labelled pixels, ``count`` (V,T,256) int64 valid pixels that
    entered the sums, ``sums`` (V,T,256,3) int64 their coordinates in fixed point (20 fractional bits), ``centroid`` (V,T,256,3) fp64
    (NaN below ``min_pixels``); ``out_of_range``: the valid pixels left out (a non-finite coordinate or one of 2^18 and more)."""

    def __init__(self, tables, min_pixels):
        self._tables, self.min_pixels = tables, min_pixels
        s = tables.stats
        self.pixels, self.count, self.sums = s[..., hip.MASK_PIXELS], s[..., hip.MASK_COUNT], s[..., hip.MASK_SUM:hip.MASK_SUM + 3]
        self.out_of_range_table = s[..., hip.MASK_OUT_OF_RANGE]
        self.centroid = tables.centroid

    @property
    def out_of_range(self):
        return int(self.out_of_range_table.sum().item())  # (a host read of its own)


def _statistics(clip):
    tables = _Tables(clip.V, clip.T, clip.dev)
    o = clip.opt
    hip.mask_stats(clip.lab, clip.d, clip.conf(o.conf_thresh), clip.kinv, clip.einv, clip.V, clip.T, clip.H, clip.W, o.min_depth, o.max_depth,
                   0.0 if o.conf_thresh is None else o.conf_thresh, tables.stats)
    hip.mask_centroids(tables.stats, clip.V, clip.T, o.min_pixels, tables.centroid)
    return MaskStatistics(tables, o.min_pixels)


@hip.guarded
def mask_statistics(labels, depths, intrs, extrs, options=MaskQueries(), depths_conf=None):
    """The statistics of a labelled clip: labels (V,T,H,W) or (1,V,T,H,W) (bool, uint8, int16, int32, int64; 0 = background, 1..255 a
    camera's local ids), depths (1,V,T,1,H,W), intrs (1,V,T,3,3), extrs (1,V,T,3,4), ``depths_conf`` like depths.  Two launches,
    nothing read back."""
    return _statistics(_Clip(labels, depths, intrs, extrs, depths_conf, options))


class MaskMatching:
    """``global_id`` (V,256) int32 on the device: the object of every (view, label), -1 where absent; ``distance`` (V,256) fp64: the
    mean centroid distance it joined its object at, NaN where it opened a new one; ``num_objects``; ``members``: {object: [(view,
    label), ...]}.  ``host``: the tables of the one read (statistics, centroids, ids) as numpy arrays."""

    def __init__(self, tables, host):
        self._tables, self.host = tables, host
        self.global_id, self.distance = tables.global_id, tables.distance
        self.num_objects = host["num_objects"]
        gid = host["global_id"]
        self.members = {g: [] for g in range(self.num_objects)}
        for v, l in zip(*np.nonzero(gid >= 0)):
            self.members[int(gid[v, l])].append((int(v), int(l)))
        s = host["stats"]
        self.valid = s[..., hip.MASK_COUNT] + s[..., hip.MASK_OUT_OF_RANGE]  # (V,T,256): the valid pixels, the pools' sizes
        self.out_of_range = int(s[..., hip.MASK_OUT_OF_RANGE].sum())

    def object_valid(self, g):
        """(T,) valid pixels of object g per frame, over its members in all views."""
        T = self.valid.shape[1]
        return sum((self.valid[v, :, l] for v, l in self.members[g]), np.zeros(T, np.int64))

    def summary(self):
        n = sum(len(m) for m in self.members.values())
        joined = int(np.isfinite(self.host["distance"]).sum())
        return (f"{n} instance ids of {self.valid.shape[0]} cameras -> {self.num_objects} objects ({joined} joined an earlier camera's object"
                + (f", {self.out_of_range} valid pixels out of range" if self.out_of_range else "") + ")")

    def table(self):
        rows = [f"{'object':>6} {'view':>4} {'label':>5} {'distance':>10} {'frames':>6} {'valid px':>9}"]
        for g, mem in self.members.items():
            for v, l in mem:
                d = self.host["distance"][v, l]
                frames = int(np.isfinite(self.host["centroid"][v, :, l, 0]).sum())
                rows.append(f"{g:>6} {v:>4} {l:>5} {('new' if np.isnan(d) else f'{d:.4f}'):>10} {frames:>6} {int(self.valid[v, :, l].sum()):>9}")
        return "\n".join(rows)


def _matching(stats, options):
    tb = stats._tables
    ids = torch.empty(tb.V * L, dtype=torch.int32, device=tb.buf.device)
    hip.mask_match(tb.centroid, tb.V, tb.T, options.min_common_frames, options.distance_threshold, options.match, ids, tb.global_id,
                   tb.distance, tb.state)
    return MaskMatching(tb, tb.host())


def match_mask_ids(stats, options=MaskQueries()):
    """The cameras' local ids of ``stats`` (a MaskStatistics) matched into global object ids: one launch, one read."""
    if not isinstance(stats, MaskStatistics):
        raise ValueError(f"stats must be a MaskStatistics, got {stats!r}")
    _check(options)
    with hip.device_guard(stats._tables.buf):
        return _matching(stats, options)


def _check_matching(matching, V):
    if not isinstance(matching, MaskMatching):
        raise ValueError(f"matching must be a MaskMatching, got {matching!r}")
    if matching.global_id.shape[0] != V:
        raise ValueError(f"the matching is of {matching.global_id.shape[0]} views, the labels of {V}")
    return matching


@hip.guarded
def global_masks(labels, matching):
    """labels (V,T,H,W) in the cameras' local ids -> (V,T,H,W) int32 in global object ids, -1 = background (and ids the matching
    does not know)."""
    lab = _labels(labels)
    V, T, H, W = lab.shape
    _check_matching(matching, V)
    hip.require_device(lab)
    out = torch.empty(V, T, H, W, dtype=torch.int32, device=lab.device)
    hip.mask_relabel(lab, matching.global_id.contiguous(), V, T, H, W, out)
    return out


def _pools(clip, matching, jobs):
    """The pools of ``jobs`` = [(object, frame, size)] in one allocation: (points (M,3), pixel (M,) int32, offsets)."""
    off = np.concatenate([[0], np.cumsum([m for _, _, m in jobs])]).astype(np.int64)
    M = int(off[-1])
    pts = torch.empty(M, 3, device=clip.dev)
    pix = torch.empty(M, dtype=torch.int32, device=clip.dev)
    count = torch.empty(max(len(jobs), 1), dtype=torch.int32, device=clip.dev)
    blocks = torch.empty((clip.V * clip.H * clip.W + 255) // 256, dtype=torch.int32, device=clip.dev)
    table = matching.global_id.contiguous()
    for j, (g, t, m) in enumerate(jobs):
        hip.mask_pool(*clip.pool_args(t), table, int(g), pts[off[j]:off[j + 1]], pix[off[j]:off[j + 1]], count[j:j + 1], blocks)
    return pts, pix, off


@hip.guarded
def lift_masks(labels, depths, intrs, extrs, frame, matching=None, options=MaskQueries(), depths_conf=None):
    """Every object of frame ``frame`` in world space: (points (M,3), object_id (M,) int32, pixel (M,) int32), grouped by object in
    ascending id, inside an object in raster order (view, row, column); ``pixel`` = (v * H + y) * W + x.  ``matching``: a
    MaskMatching of this clip under these options (None: computed here)."""
    clip = _Clip(labels, depths, intrs, extrs, depths_conf, options)
    frame = _int("frame", frame, 0)
    if frame >= clip.T:
        raise ValueError(f"frame {frame} is beyond the clip's {clip.T} frames")
    matching = _matching(_statistics(clip), clip.opt) if matching is None else _check_matching(matching, clip.V)
    jobs = [(g, frame, int(matching.object_valid(g)[frame])) for g in range(matching.num_objects)]
    jobs = [j for j in jobs if j[2] > 0]
    pts, pix, _ = _pools(clip, matching, jobs)
    oid = np.concatenate([np.full(m, g, np.int32) for g, _, m in jobs] + [np.zeros(0, np.int32)])
    return pts, torch.from_numpy(oid).to(clip.dev), pix


class MaskQueryReport:
    """``objects``: per object a dict (object, members, anchors, frames_used, frames_skipped, pool_sizes, rows); ``matching``."""

    def __init__(self, objects, matching):
        self.objects, self.matching = objects, matching

    def split(self, query_points):
        """(1,N,4) rows of ``mask_queries`` -> [(1,N_g,4)] per object that has rows, ready for ``MVTracker.forward_grouped``."""
        sizes = [o["rows"] for o in self.objects if o["rows"] > 0]
        if query_points.dim() != 3 or query_points.shape[1] != sum(sizes):
            raise ValueError(f"query points must be the (1, {sum(sizes)}, 4) rows of this report, got {tuple(query_points.shape)}")
        return list(torch.split(query_points, sizes, dim=1))

    def summary(self):
        rows = sum(o["rows"] for o in self.objects)
        skipped = sum(len(o["frames_skipped"]) for o in self.objects)
        return f"{self.matching.summary()}; {rows} query points on {sum(o['rows'] > 0 for o in self.objects)} objects, {skipped} frames skipped"

    def table(self):
        rows = [f"{'object':>6} {'members':<24} {'anchors':<12} {'frames':<16} {'skipped':<10} {'pool':>8} {'rows':>6}"]
        for o in self.objects:
            mem = " ".join(f"{v}:{l}" for v, l in o["members"])
            rows.append(f"{o['object']:>6} {mem:<24} {','.join(map(str, o['anchors'])):<12} {','.join(map(str, o['frames_used'])):<16} "
                        f"{','.join(map(str, o['frames_skipped'])):<10} {sum(o['pool_sizes']):>8} {o['rows']:>6}")
        return "\n".join(rows)


def object_frames(valid, members, options, T):
    """Rule 4 for one object: ``valid`` (T,) its valid pixels per frame -> (anchors, frames used, frames skipped)."""
    first = [int(np.nonzero(valid > 0)[0][0])] if (valid > 0).any() else []
    if isinstance(options.anchor, dict):
        anchors = [options.anchor[m] for m in members if m in options.anchor] or first
    else:
        anchors = first if options.anchor == "first" else [options.anchor]
    frames = sorted({t for a in anchors for t in range(max(a - options.frames_before, 0), min(a + options.frames_after, T - 1) + 1)})
    return anchors, [t for t in frames if valid[t] > 0], [t for t in frames if valid[t] <= 0]


@hip.guarded
def mask_queries(labels, depths, intrs, extrs, options=MaskQueries(), depths_conf=None, seed=0):
    """Query points per segmented object: (query_points (1,N,4) = (t, x, y, z), object_ids (N,) int32, MaskQueryReport).  Rows are
    ordered by object, then frame, then the pool's raster order (or the draw's).  Statistics, centroids and matching run on the
    device and are read once; every pool's size follows from that read, so the pools are allocated exactly.  ``method="random"``
    draws with one CPU generator seeded with ``seed``, consumed in (object, frame) order; ``"kmeans"`` takes
    ``kmeans_centres(pool, max_points_per_frame, seed=seed + k)`` for the k-th pool."""
    clip = _Clip(labels, depths, intrs, extrs, depths_conf, options)
    o = clip.opt
    matching = _matching(_statistics(clip), o)
    objects, jobs = [], []
    for g in range(matching.num_objects):
        mem = matching.members[g]
        if not mem:  # (match=False: a label no camera shows)
            continue
        valid = matching.object_valid(g)
        anchors, used, skipped = object_frames(valid, mem, o, clip.T)
        objects.append(dict(object=g, members=mem, anchors=anchors, frames_used=used, frames_skipped=skipped,
                            pool_sizes=[int(valid[t]) for t in used], rows=0))
        jobs += [(g, t, int(valid[t])) for t in used]
    if not jobs:
        raise ValueError("no object yields a query point: the masks are empty, or no labelled pixel has a depth inside "
                         f"({o.min_depth}, {o.max_depth}] (and a confidence above conf_thresh): check the masks and widen the depth bounds")
    pts, _, off = _pools(clip, matching, jobs)
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    by_object = {ob["object"]: ob for ob in objects}
    out, ids = [], []
    for k, (g, t, m) in enumerate(jobs):
        pool = pts[off[k]:off[k + 1]]
        if o.max_points_per_frame is not None and m > o.max_points_per_frame:
            if o.method == "random":
                pool = pool[torch.randperm(m, generator=gen)[:o.max_points_per_frame].to(clip.dev)]
            else:
                from . import queries
                pool = queries.kmeans_centres(pool, o.max_points_per_frame, seed=int(seed) + k)[0]
        out.append(torch.cat([torch.full((pool.shape[0], 1), float(t), device=clip.dev), pool], 1))
        ids.append(np.full(pool.shape[0], g, np.int32))
        by_object[g]["rows"] += int(pool.shape[0])
    return torch.cat(out, 0)[None], torch.from_numpy(np.concatenate(ids)).to(clip.dev), MaskQueryReport(objects, matching)


def object_colors(object_ids):
    """(N,) object ids -> (N,3) uint8: one gist_rainbow colour per object, spread over the map, for ``TrackOverlay(colors=...)``."""
    from .overlay import GIST_RAINBOW
    ids = torch.as_tensor(object_ids)
    if ids.dim() != 1 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise ValueError(f"object_ids must be (N,) integers, got {tuple(ids.shape)} {ids.dtype}")
    h = ids.cpu().numpy().astype(np.int64)
    if h.size and h.min() < 0:
        raise ValueError("object ids must not be negative")
    n = int(h.max()) + 1 if h.size else 1
    lut = np.frombuffer(GIST_RAINBOW, np.uint8).reshape(256, 3)
    return torch.from_numpy(lut[((2 * h + 1) * 256) // (2 * n)].copy()).to(ids.device)
