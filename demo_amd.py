#!/usr/bin/env python3
"""Offline demo of the MI355X tracker: the reference's demo.py flow (load a sample NPZ -> track -> save the result NPZ) without
its remote pieces (torch.hub / HuggingFace downloads, Rerun logging, depth estimators).

    python demo_amd.py --sample-path data_sample.npz --checkpoint mvtracker_200000_june2025.pth --save-npz tracks.npz
    python demo_amd.py --synthetic --precision bf16            # seeded synthetic clip, seeded random weights (no files needed)
    python demo_amd.py --synthetic --query-masks bands --per-mask-tracking --print-masks   # queries per segmented object, tracked apart
    python demo_amd.py --synthetic --query-masks bands --per-mask-tracking --rigid-motion --print-rigid   # and how every object moved

Mirrors reference demo.py: sample layout :650, 922-929; temporal / spatial subsampling :905-944 (``--temporal_stride``,
``--spatial_downsample``); ``--random_query_points`` :967-993 (512 queries drawn from the depth of frame 0 inside a cylinder);
``--sample-queries`` = the evaluator's sampling for unlabelled clips (evaluation/evaluator_3dpt.py:286-388, on the device);
``--normalize-scene auto`` = the dataset's scene normalisation for a user's own recording (datasets/generic_scene_dataset.py:288-358,
on the device: queries are sampled and tracks saved in the recording's own world, the model sees the normalised scene);
the predictor call :1004-1010 (bf16 = the demo's autocast arithmetic); the result file :1086-1121.  The wall time of the predictor
call is reported with the evaluator's convention (frames / second, evaluation/evaluator_3dpt.py:496-523)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def random_queries(depths, intrs, extrs, num_queries=512, t0=0, xy_radius=12.0, z_min=-1.0, z_max=10.0, seed=0):
    """demo.py:967-993: unproject every pixel of frame t0 (all views), keep the points inside the cylinder, draw num_queries."""
    from mvtracker_amd.queries import sample_queries
    try:  # demo.py's rule: valid depth (no confidence map), x^2 + y^2 <= r^2
        return sample_queries(depths, intrs, extrs, [(t0, z_min, z_max, xy_radius, num_queries, "")], seed=seed, radius_inclusive=True)
    except ValueError:
        raise AssertionError("cylinder mask removed all points; increase the radius or the z range") from None


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--sample-path", help="sample NPZ (rgbs, depths, intrs, extrs[, query_points])")
    src.add_argument("--synthetic", action="store_true", help="seeded synthetic clip (4 views x 24 frames x 384x512, 256 queries)")
    ap.add_argument("--checkpoint", help="reference checkpoint (.pth, read with weights_only=True); default: seeded random weights")
    ap.add_argument("--precision", choices=["fp32", "bf16x3", "bf16"], default="bf16", help="bf16 = the demo's autocast arithmetic")
    ap.add_argument("--temporal_stride", type=int, default=1)
    ap.add_argument("--spatial_downsample", type=int, default=1)
    ap.add_argument("--random_query_points", action="store_true")
    ap.add_argument("--sample-queries", choices=["random", "kmeans"], default=None,
                    help="sample the queries from the depth of frame 0 like the reference's evaluator does for unlabelled clips "
                         "(mvtracker_amd.sample_queries): a random draw or the k-means centres of the points inside --region")
    ap.add_argument("--num-queries", type=int, default=1000, metavar="N", help="queries drawn by --sample-queries")
    ap.add_argument("--region", type=float, nargs=3, default=(2.1, -0.1, 4.2), metavar=("R", "ZMIN", "ZMAX"),
                    help="cylinder of --sample-queries around the z axis: radius and z range")
    ap.add_argument("--query-region-box", type=float, nargs=6, default=None, metavar=("XLO", "XHI", "YLO", "YHI", "ZLO", "ZHI"),
                    help="with --sample-queries: draw the queries from the largest cluster of points inside this box around "
                         "--query-region-pose, per view (mvtracker_amd.region_masks, the reference's classify_gripper_points on the device)")
    ap.add_argument("--query-region-pose", type=float, nargs=16, default=None, metavar="M",
                    help="world_T_region, 16 numbers row by row (default: the identity)")
    ap.add_argument("--query-region-pose-key", default=None, metavar="NAME",
                    help="name of an array (T, 4, 4) or (4, 4) world_T_region in the sample NPZ, instead of --query-region-pose")
    ap.add_argument("--query-region-eps", type=float, default=0.03, help="DBSCAN neighbourhood radius, in the clip's own units")
    ap.add_argument("--query-region-min-samples", type=int, default=12, help="DBSCAN: neighbours (itself included) of a core point")
    ap.add_argument("--query-motion", choices=["moving", "static"], default=None,
                    help="with --sample-queries: draw the queries from the pixels that move (or from the static background), found from "
                         "the frames alone (mvtracker_amd.motion_masks, the reference's _static_bg_mask_from_window on the device)")
    ap.add_argument("--query-motion-window", type=int, default=None, metavar="W",
                    help="frames to either side of the query frame whose differences count (default: the whole clip)")
    ap.add_argument("--query-motion-radius", type=int, default=None, metavar="R", help="a pixel moves when one within R pixels does (default 7)")
    ap.add_argument("--query-motion-thresh", type=float, default=None, metavar="D",
                    help="channel-mean frame difference from which a pixel moves, in the frames' own units (default 10, for 0..255 frames)")
    ap.add_argument("--query-masks", default=None, metavar="KEY",
                    help="queries on segmented objects (mvtracker_amd.mask_queries): KEY names the (V, T, H, W) label map (0 = background, "
                         "1..255 a camera's instance ids) or the (I, V, T, H, W) stack of boolean instance masks in the sample NPZ; with "
                         "--synthetic any KEY gives depth bands per view")
    ap.add_argument("--mask-frames-before", type=int, default=None, metavar="N", help="frames before an object's anchor frame (default 3)")
    ap.add_argument("--mask-frames-after", type=int, default=None, metavar="N", help="frames after it (default 1)")
    ap.add_argument("--mask-anchor", default=None, metavar="first|INT", help="an object's first frame with a valid pixel (default) or one frame for all")
    ap.add_argument("--mask-distance-threshold", type=float, default=None, metavar="D",
                    help="two cameras' ids are one object when their mean centroid distance is below D (default 0.15, in the clip's units)")
    ap.add_argument("--mask-no-match", action="store_true", help="the label ids are global already: label l is object l - 1 in every camera")
    ap.add_argument("--mask-max-points", type=int, default=256, metavar="N", help="query points per object and frame")
    ap.add_argument("--mask-method", choices=["random", "kmeans"], default=None, help="how a larger pool is cut to --mask-max-points (default random)")
    ap.add_argument("--per-mask-tracking", action="store_true",
                    help="track every object's queries as a query set of its own (EvaluationPredictor.forward(query_groups=...))")
    ap.add_argument("--print-masks", action="store_true", help="print the mask query report (matching table, frames, pools, rows)")
    ap.add_argument("--rigid-motion", action="store_true",
                    help="fit one rigid pose per object and frame to the tracks on the device (mvtracker_amd.rigid_motion): the objects are "
                         "those of --query-masks, or one object of all queries; the saved NPZ gains object_poses, rigid_inliers, rigid_status")
    ap.add_argument("--rigid-threshold", type=float, default=None, metavar="C",
                    help="a track moves with its object within this distance of where the pose puts it (default 0.02, in the clip's units)")
    ap.add_argument("--rigid-iterations", type=int, default=None, metavar="K", help="fits per object and frame (default 3)")
    ap.add_argument("--rigid-min-points", type=int, default=None, metavar="P", help="members a fit needs (default 4)")
    ap.add_argument("--rigid-fill", action="store_true",
                    help="put every occluded track point where its object's pose says it is (mvtracker_amd.fill_tracks) before saving")
    ap.add_argument("--print-rigid", action="store_true", help="print the per-object table of the rigid motion")
    ap.add_argument("--print-motion", action="store_true",
                    help="print the clip's motion report (static share per view and frame, mean frame differences) and its static "
                         "prefix: the leading frames before anything moves (the reference demo's _detect_static_prefix_frames)")
    ap.add_argument("--normalize-scene", choices=["none", "auto"], default="none",
                    help="auto: centre the scene, lift its floor to z = 0 and rescale it to the size the weights were trained on "
                         "(mvtracker_amd.auto_scene_normalization on frame 0); tracks are saved in the clip's own world")
    ap.add_argument("--target-radius", type=float, default=6.3, help="median camera distance after --normalize-scene auto")
    ap.add_argument("--norm-conf-thresh", type=float, default=4.8,
                    help="confidence above which a pixel counts for --normalize-scene auto (clips with a depths_conf entry only)")
    ap.add_argument("--single_point", action="store_true")
    ap.add_argument("--grid-size", type=int, default=5)
    ap.add_argument("--n-iters", type=int, default=4)
    ap.add_argument("--interp-shape", type=int, nargs=2, default=None, metavar=("H", "W"), help="resize like the evaluator (e.g. 384 512)")
    ap.add_argument("--backward-tracking", action="store_true",
                    help="also track every query before its frame (a time-reversed pass over the same frame store)")
    ap.add_argument("--streaming", action="store_true",
                    help="feed the clip block by block through a streaming session (EvaluationPredictor.open_stream): the same result, "
                         "from a ring frame store whose size does not depend on the clip length")
    ap.add_argument("--block-frames", type=int, default=6, metavar="B", help="frames per pushed block with --streaming")
    ap.add_argument("--save-npz", help="result file (tracks_3d, visibilities, query_points, camera data)")
    ap.add_argument("--save-overlay", metavar="DIR", default=None,
                    help="draw the tracks into every view's frames on the device (mvtracker_amd.render_track_overlays, the reference's "
                         "visualizer_mp4 drawing rules) and write view{v}_frame{t:04d}.png into DIR (one view{v}.npy per view without PIL)")
    ap.add_argument("--overlay-trail", type=int, default=None, metavar="L", help="segments a track leaves behind: -1 all (default), 0 none")
    ap.add_argument("--overlay-linewidth", type=int, default=None, metavar="W", help="line width 1..8 (default 2); markers have twice the radius")
    ap.add_argument("--overlay-pad", type=int, default=None, metavar="P", help="white border of P pixels, 0..64 (default 0)")
    ap.add_argument("--overlay-min-depth", type=float, default=None, metavar="D",
                    help="draw a point only when its camera depth exceeds D (default: no test, as the reference)")
    ap.add_argument("--overlay-max-tracks", type=int, default=None, metavar="M", help="draw only the first M tracks (the reference draws 36)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--clean-depths", choices=["statistical", "radius"], default=None,
                    help="remove outliers from every (view, frame) depth map before tracking (mvtracker_amd.clean_depths, the reference "
                         "demo's --clean_pointcloud on the device); the saved NPZ gains the keep mask")
    ap.add_argument("--pc-clean-nb-neighbors", type=int, default=20, help="statistical: neighbours of the mean distance")
    ap.add_argument("--pc-clean-std-ratio", type=float, default=2.0, help="statistical: threshold = mean + ratio * deviation")
    ap.add_argument("--pc-clean-radius", type=float, default=0.05, help="radius: search radius, in the clip's own units")
    ap.add_argument("--pc-clean-min-points", type=int, default=5, help="radius: a point needs more neighbours than this")
    ap.add_argument("--align-cameras", action="store_true",
                    help="refine the views' extrinsics against each other by point-to-plane ICP of their clouds before tracking "
                         "(mvtracker_amd.align_cameras, the reference's run_icp_point_to_plane on the device); the saved NPZ holds the "
                         "corrected extrinsics and the per-view corrections")
    ap.add_argument("--align-max-distance", type=float, default=0.05, help="correspondence cap, in the clip's own units")
    ap.add_argument("--align-iterations", type=int, default=30, help="ICP iterations per view and sweep")
    ap.add_argument("--align-sweeps", type=int, default=2, help="passes over the views")
    ap.add_argument("--align-frames", type=int, nargs="+", default=[0], metavar="F", help="frames whose clouds are aligned")
    ap.add_argument("--align-anchor", type=int, default=0, help="the view that stays fixed")
    ap.add_argument("--align-sample-stride", type=int, default=1, help="every s-th pixel row and column of a view is a query")
    ap.add_argument("--align-normal-max-edge", type=float, default=None,
                    help="a normal needs its four grid neighbours within this distance (default: --align-max-distance)")
    ap.add_argument("--align-normals", choices=("grid", "pca"), default="grid",
                    help="target normals: the cross product of grid neighbours, or a PCA over the nearest points "
                         "(mvtracker_amd.estimate_normals, the reference's estimate_normals)")
    ap.add_argument("--align-normal-radius", type=float, default=None, help="PCA normals: neighbour radius (default: --align-max-distance)")
    ap.add_argument("--align-normal-max-nn", type=int, default=30, help="PCA normals: neighbours per point, at most")
    ap.add_argument("--reprojection-check", action="store_true",
                    help="render every view from the other views' depth maps and score the render against the view's own frame and depth "
                         "(mvtracker_amd.reprojection_report, the reference's reproject_depth_into_videos.py and "
                         "compare_photometric_error.py on the device); with --align-cameras both tables and their difference are printed")
    ap.add_argument("--reproject-frames", type=int, nargs="+", default=[0], metavar="F", help="frames that are rendered and scored")
    ap.add_argument("--reproject-sources", choices=("others", "all"), default="others",
                    help="a view is rendered from every other view, or from every view (what the reference script renders)")
    ap.add_argument("--reproject-splat", type=int, choices=(1, 3, 5), default=1, help="side of the depth-tested sprite a point is drawn as")
    ap.add_argument("--reproject-depth-tol", type=float, default=0.05,
                    help="a rendered depth within this of the view's own depth counts as close, in the clip's own units")
    return ap


def depth_cleaning_from_args(args):
    """The DepthCleaning of --clean-depths and the --pc-clean-* flags, or None."""
    if args.clean_depths is None:
        return None
    from mvtracker_amd import DepthCleaning
    return DepthCleaning(method=args.clean_depths, nb_neighbors=args.pc_clean_nb_neighbors, std_ratio=args.pc_clean_std_ratio,
                         radius=args.pc_clean_radius, min_points=args.pc_clean_min_points)


def camera_alignment_from_args(args):
    """The CameraAlignment of --align-cameras and the --align-* flags, or None."""
    if not args.align_cameras:
        return None
    from mvtracker_amd import CameraAlignment, PcaCameraAlignment
    kw = dict(max_distance=args.align_max_distance, max_iterations=args.align_iterations, sweeps=args.align_sweeps,
              frames=tuple(args.align_frames), anchor=args.align_anchor, sample_stride=args.align_sample_stride,
              normal_max_edge=args.align_normal_max_edge)
    if args.align_normals == "pca":
        return PcaCameraAlignment(normal_radius=args.align_normal_radius, normal_max_nn=args.align_normal_max_nn, **kw)
    return CameraAlignment(**kw)


def reprojection_check_from_args(args):
    """The ReprojectionCheck of --reprojection-check and the --reproject-* flags, or None."""
    if not args.reprojection_check:
        return None
    from mvtracker_amd import ReprojectionCheck
    return ReprojectionCheck(frames=tuple(args.reproject_frames), sources=args.reproject_sources, splat=args.reproject_splat,
                             depth_tol=args.reproject_depth_tol)


def query_region_from_args(args, temporal_stride=1):
    """(RegionCluster, world_T_region poses) of the --query-region-* flags, or (None, None)."""
    given = args.query_region_box is not None or args.query_region_pose is not None or args.query_region_pose_key is not None
    if not given:
        return None, None
    if args.sample_queries is None:
        raise SystemExit("--query-region-* flags need --sample-queries")
    if args.query_region_box is None:
        raise SystemExit("--query-region-pose / --query-region-pose-key need --query-region-box")
    if args.query_region_pose is not None and args.query_region_pose_key is not None:
        raise SystemExit("give --query-region-pose or --query-region-pose-key, not both")
    from mvtracker_amd import RegionCluster
    b = args.query_region_box
    region = RegionCluster(box=((b[0], b[1]), (b[2], b[3]), (b[4], b[5])), eps=args.query_region_eps, min_samples=args.query_region_min_samples)
    if args.query_region_pose_key is not None:
        if not args.sample_path:
            raise SystemExit("--query-region-pose-key needs --sample-path")
        with np.load(args.sample_path) as f:
            if args.query_region_pose_key not in f.files:
                raise SystemExit(f"{args.sample_path} has no array {args.query_region_pose_key!r}")
            poses = np.asarray(f[args.query_region_pose_key], np.float64)
        if poses.ndim == 3:
            poses = poses[::temporal_stride]
    else:
        poses = np.eye(4) if args.query_region_pose is None else np.asarray(args.query_region_pose, np.float64).reshape(4, 4)
    return region, poses


def query_motion_from_args(args):
    """(MotionMask, which side the queries are drawn from) of the --query-motion* flags, or (None, "moving")."""
    details = (args.query_motion_window, args.query_motion_radius, args.query_motion_thresh)
    if args.query_motion is None:
        if any(v is not None for v in details):
            raise SystemExit("--query-motion-window / -radius / -thresh need --query-motion")
        return None, "moving"
    if args.sample_queries is None:
        raise SystemExit("--query-motion needs --sample-queries")
    from mvtracker_amd import MotionMask
    kw = {k: v for k, v in zip(("window", "patch_radius", "diff_thresh"), details) if v is not None}
    try:
        return MotionMask(**kw), args.query_motion
    except ValueError as e:
        raise SystemExit(str(e)) from None


def query_masks_from_args(args):
    """The MaskQueries of --query-masks and the --mask-* flags, or None."""
    details = (args.mask_frames_before, args.mask_frames_after, args.mask_anchor, args.mask_distance_threshold, args.mask_method)
    if args.query_masks is None:
        if any(d is not None for d in details) or args.mask_no_match or args.per_mask_tracking or args.print_masks:
            raise SystemExit("--mask-* flags, --per-mask-tracking and --print-masks need --query-masks")
        return None
    if args.sample_queries is not None or args.random_query_points:
        raise SystemExit("--query-masks replaces --sample-queries / --random-query-points: give one of them")
    if args.per_mask_tracking and (args.streaming or args.single_point or args.backward_tracking):
        raise SystemExit("--per-mask-tracking runs in joint mode only (no --streaming, --single-point or --backward-tracking)")
    from mvtracker_amd import MaskQueries
    kw = {k: v for k, v in zip(("frames_before", "frames_after", "anchor", "distance_threshold", "method"), details) if v is not None}
    if "anchor" in kw and kw["anchor"] != "first":
        try:
            kw["anchor"] = int(kw["anchor"])
        except ValueError:
            raise SystemExit(f"--mask-anchor must be 'first' or a frame number, got {kw['anchor']!r}") from None
    try:
        return MaskQueries(match=not args.mask_no_match, max_points_per_frame=args.mask_max_points, **kw)
    except ValueError as e:
        raise SystemExit(str(e)) from None


def rigid_motion_from_args(args):
    """The RigidMotion of --rigid-motion and the --rigid-* flags, or None."""
    details = (args.rigid_threshold, args.rigid_iterations, args.rigid_min_points)
    if not args.rigid_motion:
        if any(d is not None for d in details) or args.rigid_fill or args.print_rigid:
            raise SystemExit("--rigid-threshold, --rigid-iterations, --rigid-min-points, --rigid-fill and --print-rigid need --rigid-motion")
        return None
    from mvtracker_amd import RigidMotion
    kw = {k: v for k, v in zip(("inlier_threshold", "iterations", "min_points"), details) if v is not None}
    try:
        return RigidMotion(live_before_query=bool(args.backward_tracking), **kw)
    except ValueError as e:
        raise SystemExit(str(e)) from None


def mask_labels(args, s):
    """The label map of --query-masks: from the sample NPZ, or (--synthetic) three depth bands per view, numbered from the far band
    in odd views so that the cameras' ids differ."""
    if args.synthetic:
        d = s["depths"][0, :, :, 0]
        lab = torch.bucketize(d, torch.tensor([0.5, 2.5, 3.5, 4.5], device=d.device)).clamp(max=4) % 4
        lab[1::2] = torch.where(lab[1::2] > 0, 4 - lab[1::2], lab[1::2])
        return lab.to(torch.uint8)
    with np.load(args.sample_path) as z:
        if args.query_masks not in z:
            raise SystemExit(f"--query-masks: no array {args.query_masks!r} in {args.sample_path}")
        m = torch.from_numpy(z[args.query_masks])
    st = args.temporal_stride
    if m.dtype == torch.bool:
        from mvtracker_amd import labels_from_instances
        m = labels_from_instances(m[:, :, ::st] if m.dim() == 5 else m[None, :, ::st])
    else:
        m = (m[0] if m.dim() == 5 else m)[:, ::st]
    if args.spatial_downsample > 1:
        m = m[..., ::args.spatial_downsample, ::args.spatial_downsample]
    return m.to(s["depths"].device)


def track_overlay_from_args(args):
    """The TrackOverlay of --save-overlay and the --overlay-* flags, or None."""
    names = ("trail", "linewidth", "pad", "min_depth", "max_tracks")
    details = {k: getattr(args, "overlay_" + k) for k in names if getattr(args, "overlay_" + k) is not None}
    if args.save_overlay is None:
        if details:
            raise SystemExit("--overlay-trail / -linewidth / -pad / -min-depth / -max-tracks need --save-overlay")
        return None
    from mvtracker_amd import TrackOverlay
    try:
        return TrackOverlay(**details)
    except ValueError as e:
        raise SystemExit(str(e)) from None


def save_overlay(video, directory):
    """video (V, T, 3, Hp, Wp) uint8 -> view{v}_frame{t:04d}.png in ``directory`` with PIL when it imports, else one view{v}.npy
    (T, 3, Hp, Wp) per view; the list of files written."""
    os.makedirs(directory, exist_ok=True)
    frames = video.cpu().numpy()
    files = []
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for v in range(frames.shape[0]):
        if Image is None:
            files.append(os.path.join(directory, f"view{v}.npy"))
            np.save(files[-1], frames[v])
            continue
        for t in range(frames.shape[1]):
            files.append(os.path.join(directory, f"view{v}_frame{t:04d}.png"))
            Image.fromarray(np.ascontiguousarray(frames[v, t].transpose(1, 2, 0))).save(files[-1])
    return files


def main():
    args = build_parser().parse_args()
    track_overlay = track_overlay_from_args(args)
    region, region_poses = query_region_from_args(args, args.temporal_stride)  # (flag errors before any work)
    motion, motion_keep = query_motion_from_args(args)
    rigid_options = rigid_motion_from_args(args)
    mask_options = query_masks_from_args(args)
    if not torch.cuda.is_available():
        raise SystemExit("demo_amd.py needs an MI355X: the tracker has no CPU path")
    from mvtracker_amd import sample_io, synth
    from mvtracker_amd.factory import load_mvtracker

    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    predictor = load_mvtracker(checkpoint=args.checkpoint, device=dev, interp_shape=tuple(args.interp_shape) if args.interp_shape else None,
                               grid_size=args.grid_size, n_iters=args.n_iters, single_point=args.single_point,
                               backward_tracking=args.backward_tracking)
    model = predictor.model
    if args.checkpoint is None:
        print("no --checkpoint: seeded random weights (results are meaningless as tracks, the pipeline is the real one)")
        sd = synth.make_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=0)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        model.to(dev)
    model.precision = args.precision
    if args.synthetic:
        clip = synth.make_clip(3, V=4, T=24, H=384, W=512, N=256, late_queries=True, rgb_dtype=np.uint8)
        s = {k: torch.from_numpy(v)[:, :, ::args.temporal_stride].to(dev) if k != "query_points" else torch.from_numpy(v).to(dev)
             for k, v in clip.items()}
        s["query_points_3d"] = s.pop("query_points")
        if args.temporal_stride > 1:
            s["query_points_3d"][..., 0] = torch.floor(s["query_points_3d"][..., 0] / args.temporal_stride)
    else:
        s = sample_io.load_sample(args.sample_path, device=dev, temporal_stride=args.temporal_stride, spatial_downsample=args.spatial_downsample)
    # cleaning and camera alignment first, in the predictor's order (clean, then align on the cleaned depths): the queries below are
    # sampled, the saved mask is cleaned and the scene is normalised with the corrected cameras, which are also what is saved
    cleaning, alignment, keep = depth_cleaning_from_args(args), camera_alignment_from_args(args), None
    norm_depths = s["depths"]
    check, before = reprojection_check_from_args(args), None
    if cleaning is not None and (alignment is not None or check is not None):  # (the check reports on what the predictor would track with)
        from mvtracker_amd import clean_depths
        norm_depths = clean_depths(s["depths"].float(), s["intrs"], s["extrs"], cleaning)[0]
    if check is not None and alignment is not None:  # the reference's "no ICP" side
        from mvtracker_amd import reprojection_report
        before = reprojection_report(s["rgbs"], norm_depths.float(), s["intrs"], s["extrs"], check, depths_conf=s.get("depths_conf"))
        print(before.table("no_icp"))
    if alignment is not None:  # once, here: the warm-up and the timed call both get the corrected cameras
        from mvtracker_amd import align_cameras
        correction = align_cameras(norm_depths.float(), s["intrs"], s["extrs"], alignment, depths_conf=s.get("depths_conf"))
        s["extrs"] = correction.apply(s["extrs"])
        s["camera_corrections"] = correction.transforms.cpu().numpy()
        print(f"camera alignment: fitness {np.round(correction.fitness.cpu().numpy(), 3).tolist()}, rmse "
              f"{np.round(correction.rmse.cpu().numpy(), 4).tolist()}, iterations {correction.iterations.cpu().tolist()}")
    if check is not None:
        from mvtracker_amd import compare_reports, reprojection_report
        report = reprojection_report(s["rgbs"], norm_depths.float(), s["intrs"], s["extrs"], check, depths_conf=s.get("depths_conf"))
        print(report.table("icp" if before is not None else "reprojection"))
        if before is not None:
            print("improvement (positive = the corrected cameras are better)")
            print(compare_reports(before, report))
    if cleaning is not None:  # (the predictor cleans the raw depths itself; this call is for the saved mask and the normalisation)
        from mvtracker_amd import clean_depths
        norm_depths, keep = clean_depths(s["depths"].float(), s["intrs"], s["extrs"], cleaning)
        print(f"depth cleaning ({args.clean_depths}): {int((~keep & (s['depths'] > 0)).sum())} of {int((s['depths'] > 0).sum())} valid pixels removed")
    if args.print_motion:
        from mvtracker_amd import MotionMask, motion_masks
        report = motion_masks(s["rgbs"], motion if motion is not None else MotionMask())[1]
        print("motion:", report.summary())
        print(report.table())
        print("static prefix frames:", report.static_prefix_frames())
    if args.sample_queries is not None:
        from mvtracker_amd import sample_queries
        r, zmin, zmax = args.region
        spec = [(0, zmin, zmax, r, args.num_queries, "kmeans" if args.sample_queries == "kmeans" else "")]
        reports, motion_reports = {}, {}
        s["query_points_3d"] = sample_queries(s["depths"], s["intrs"], s["extrs"], spec, region=region, region_poses=region_poses,
                                              region_reports=reports, motion=motion, rgbs=s["rgbs"] if motion is not None else None,
                                              motion_keep=motion_keep, motion_reports=motion_reports)
        for t, report in sorted(reports.items()):
            print(f"query region, frame {t}:", report.summary())
            print(report.table())
        for report in motion_reports.values():
            print(f"query motion ({motion_keep} pixels):", report.summary())
    elif mask_options is not None:
        from mvtracker_amd import mask_queries
        s["query_points_3d"], object_ids, report = mask_queries(mask_labels(args, s), s["depths"], s["intrs"], s["extrs"], mask_options,
                                                                depths_conf=s.get("depths_conf") if mask_options.conf_thresh is not None else None)
        print("mask queries:", report.summary())
        if args.print_masks:
            print(report.matching.table())
            print(report.table())
    elif args.random_query_points or s["query_points_3d"].shape[1] == 0:
        s["query_points_3d"] = random_queries(s["depths"].float(), s["intrs"], s["extrs"])
    xf = None
    if args.normalize_scene == "auto":  # (after the queries: sampling stays in the clip's own world)
        from mvtracker_amd import auto_scene_normalization
        xf = auto_scene_normalization(norm_depths, s["intrs"], s["extrs"], depths_conf=s.get("depths_conf"), conf_thresh=args.norm_conf_thresh,
                                      target_radius=args.target_radius)
        print(f"scene normalisation: scale {xf.scale:.4f}, translation {np.round(xf.translation, 4).tolist()}")
    V, T = s["rgbs"].shape[1:3]
    print(f"clip: {V} views x {T} frames x {tuple(s['rgbs'].shape[-2:])}, {s['query_points_3d'].shape[1]} queries, precision {args.precision}")
    call = lambda: predictor(rgbs=s["rgbs"], depths=s["depths"], intrs=s["intrs"], extrs=s["extrs"], query_points_3d=s["query_points_3d"],
                             scene_transform=xf, depth_cleaning=cleaning, query_groups=object_ids if args.per_mask_tracking else None)
    if args.streaming:
        if args.block_frames < 1:
            raise SystemExit("--block-frames must be at least 1")

        def call():
            st = predictor.open_stream(s["query_points_3d"], scene_transform=xf, depth_cleaning=cleaning)
            outs = [st.push(*(s[k][:, :, t:t + args.block_frames] for k in ("rgbs", "depths", "intrs", "extrs")))
                    for t in range(0, T, args.block_frames)]
            outs.append(st.finish())
            return {k: torch.cat([o[k] for o in outs], 1) for k in ("traj_e", "vis_e")}
    call()  # warm-up (weight packing, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = s["query_points_3d"].shape[1]
    print(f"{'streaming session' if args.streaming else 'predictor call'}: {1e3 * dt:.1f} ms = {T / dt:.1f} frames/s = {n * T / dt:.0f} query-points*frames/s; "
          f"{int(out['vis_e'].sum())} of {out['vis_e'].numel()} track points visible; NaN guard {'TRIPPED' if predictor.last_nan else 'clean'}")
    if rigid_options is not None:  # after the timed call, from what it returned: the streaming path has the same tracks
        from mvtracker_amd import fill_tracks, rigid_motion
        n_q = s["query_points_3d"].shape[1]
        ids = object_ids if mask_options is not None else torch.zeros(n_q, dtype=torch.int32, device=out["traj_e"].device)
        tracks, visible = out["traj_e"][0].float().contiguous(), out["vis_e"][0].bool().contiguous()
        rigid = rigid_motion(tracks, visible, s["query_points_3d"][0, :, 0].to(torch.int32), ids, rigid_options)
        print("rigid motion:", rigid.summary())
        if args.print_rigid:
            print(rigid.table())
        if args.rigid_fill:
            filled, where = fill_tracks(tracks, visible, rigid)
            out["traj_e"] = filled[None]
            print(f"rigid fill: {int(where.sum())} occluded track points put where their object's pose says they are")
        s["object_poses"], s["rigid_inliers"], s["rigid_status"] = (x.cpu().numpy() for x in (rigid.poses, rigid.inliers, rigid.status))
    if args.save_npz:
        if keep is not None:
            s["keep"] = keep[0].cpu().numpy()
        sample_io.save_result(args.save_npz, out["traj_e"], out["vis_e"], s, temporal_stride=args.temporal_stride,
                              spatial_downsample=args.spatial_downsample)
        print("saved", args.save_npz)
    if track_overlay is not None:  # after the timed call, from what it returned: the streaming path has the same tracks
        from mvtracker_amd import render_track_overlays
        if mask_options is not None:  # one colour per object
            import dataclasses
            from mvtracker_amd import object_colors
            track_overlay = dataclasses.replace(track_overlay, colors=object_colors(object_ids))
        video, _ = render_track_overlays(s["rgbs"][0], out["traj_e"][0], out["vis_e"][0], s["query_points_3d"][0, :, 0], s["intrs"][0], s["extrs"][0],
                                         track_overlay)
        files = save_overlay(video, args.save_overlay)
        print(f"track overlay: {tuple(video.shape)} drawn on the device, {len(files)} files in {args.save_overlay}")


if __name__ == "__main__":
    main()
