"""MI355X-native multi-view point-tracking forward path (drop-in for mvtracker.models' predictor).

    from mvtracker_amd import MVTracker, EvaluationPredictor, load_mvtracker, sample_queries, auto_scene_normalization, DepthCleaning, clean_depths, CameraAlignment, align_cameras, estimate_normals, voxel_downsample, ReprojectionCheck, reprojection_report, RegionCluster, region_masks, cluster_points, MotionMask, motion_masks, TrackOverlay, render_track_overlays, MaskQueries, mask_queries, RigidMotion, rigid_motion, move_points, fill_tracks

``synth`` (numpy only) can be imported without the HIP library; everything else loads
libmvtracker_hip.so on import and raises if it is missing -- there is no CPU fallback.
"""
__all__ = ["MVTracker", "EvaluationPredictor", "load_mvtracker", "hip", "synth", "sample_io", "adapter", "geometry", "parallel", "queries",
           "sample_queries", "kmeans_centres", "DEFAULT_SPEC", "scene", "SceneTransform", "auto_scene_normalization", "clean", "DepthCleaning", "clean_depths",
           "clean_point_cloud", "align", "CameraAlignment", "PcaCameraAlignment", "CameraCorrection", "align_cameras", "align_point_clouds", "cloud",
           "estimate_normals", "voxel_downsample", "reproject", "ReprojectionCheck", "ReprojectionReport", "reprojection_report", "reproject_views",
           "render_point_cloud", "compare_reports", "cluster", "RegionCluster", "RegionReport", "cluster_points", "select_region_points",
           "region_masks", "motion", "MotionMask", "MotionReport", "motion_masks", "overlay", "TrackOverlay", "TrackOverlaySession", "project_tracks",
           "render_track_overlays", "open_track_overlay", "stack_views", "masks", "MaskQueries", "MaskStatistics", "MaskMatching",
           "MaskQueryReport", "labels_from_instances", "mask_statistics", "match_mask_ids", "global_masks", "lift_masks", "mask_queries",
           "object_colors", "rigid", "RigidMotion", "RigidMotionResult", "rigid_motion", "move_points", "fill_tracks"]


def __getattr__(name):
    if name == "MVTracker":
        from .tracker import MVTracker
        return MVTracker
    if name == "EvaluationPredictor":
        from .predictor import EvaluationPredictor
        return EvaluationPredictor
    if name == "load_mvtracker":
        from .factory import load_mvtracker
        return load_mvtracker
    if name in ("sample_queries", "kmeans_centres", "DEFAULT_SPEC"):
        from . import queries
        return getattr(queries, name)
    if name in ("SceneTransform", "auto_scene_normalization"):
        from . import scene
        return getattr(scene, name)
    if name in ("DepthCleaning", "clean_depths", "clean_point_cloud"):
        from . import clean
        return getattr(clean, name)
    if name in ("CameraAlignment", "PcaCameraAlignment", "CameraCorrection", "align_cameras", "align_point_clouds"):
        from . import align
        return getattr(align, name)
    if name in ("estimate_normals", "voxel_downsample"):
        from . import cloud
        return getattr(cloud, name)
    if name in ("ReprojectionCheck", "ReprojectionReport", "reprojection_report", "reproject_views", "render_point_cloud", "compare_reports"):
        from . import reproject
        return getattr(reproject, name)
    if name in ("RegionCluster", "RegionReport", "cluster_points", "select_region_points", "region_masks"):
        from . import cluster
        return getattr(cluster, name)
    if name in ("MotionMask", "MotionReport", "motion_masks"):
        from . import motion
        return getattr(motion, name)
    if name in ("TrackOverlay", "TrackOverlaySession", "project_tracks", "render_track_overlays", "open_track_overlay", "stack_views"):
        from . import overlay
        return getattr(overlay, name)
    if name in ("MaskQueries", "MaskStatistics", "MaskMatching", "MaskQueryReport", "labels_from_instances", "mask_statistics", "match_mask_ids",
                "global_masks", "lift_masks", "mask_queries", "object_colors"):
        from . import masks
        return getattr(masks, name)
    if name in ("RigidMotion", "RigidMotionResult", "rigid_motion", "move_points", "fill_tracks"):
        from . import rigid
        return getattr(rigid, name)
    if name in ("hip", "synth", "sample_io", "adapter", "geometry", "parallel", "queries", "scene", "clean", "align", "cloud", "reproject", "cluster", "motion", "overlay", "masks", "rigid"):
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError(name)
