"""Golden vectors of the reprojection check: the reference's ``render_dense_pointcloud`` (conversions/droid/
reproject_depth_into_videos.py:38-120) and ``compute_mse`` / ``compute_psnr`` / ``compute_mae`` (conversions/droid/debug/
compare_photometric_error.py:48-103) on ``camera_align_cases.scene(3, 24, 40)``, each view rendered from the other two, generated
from /root/reference in the build container.

The render script refuses to be imported (it raises NotImplementedError on line 19, before its functions are defined, and imports
the ZED SDK), so the function's own definition is compiled from the file's syntax tree into a namespace that holds numpy and the
reference's ``transform_points`` / ``invert_transform`` (utils/transforms.py, loaded by path: the package's __init__ imports Open3D,
cv2 and the ZED SDK); ``cv2`` and ``pytransform3d`` are absent here and registered as stubs, as make_golden_evaluate3dpt.py does
(``invert_transform`` of a rigid 4x4 is the stub's closed form [R^T | -R^T t]; cv2 is never called by the three score functions).
Data only: the scene, seeded colours, the fp32 point lists and the reference's results.

The restatement tests/reproject_ref.py differs from the reference's render in 0 of the 960 pixels of each of the three views on this
case (coverage 0.43-0.46), which the generator asserts before it writes.  (On scene(4, 36, 52) the reference alone differs from the
rule in 3-9 pixels per view: its symmetric cameras put points within 1e-9 of pixel borders, where the reference's matmul and
pytransform3d's inverse round differently from the rule's written-out sums.)"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/conversions/droid"
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _stub(name, **attrs):
    if name in sys.modules:
        return sys.modules[name]
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _invert_rigid(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_stub("cv2")
pkg = _stub("pytransform3d")
pkg.__path__ = []
pkg.transformations = _stub("pytransform3d.transformations", invert_transform=_invert_rigid)
transforms = _load(os.path.join(REF, "utils", "transforms.py"), "_ref_droid_transforms")
scores = _load(os.path.join(REF, "debug", "compare_photometric_error.py"), "_ref_compare_photometric_error")

path = os.path.join(REF, "reproject_depth_into_videos.py")
tree = ast.parse(open(path).read(), path)
node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "render_dense_pointcloud"]
ns = {"np": np, "transform_points": transforms.transform_points, "invert_transform": transforms.invert_transform}
exec(compile(ast.Module(body=node, type_ignores=[]), path, "exec"), ns)
render_dense_pointcloud = ns["render_dense_pointcloud"]

import camera_align_cases as cases  # noqa: E402
import reproject_ref as R  # noqa: E402

V, H, W = 3, 24, 40
clip = cases.scene(V, H, W)
pts = cases.unproject(clip["depths"], clip["intrs"], clip["extrs"])[:, 0].astype(np.float32)  # (V,H,W,3), frame 0
valid = clip["depths"][0, :, 0, 0] > 0
colors = np.random.default_rng(20240611).integers(1, 256, size=(V, 3, H, W), dtype=np.uint8)  # non-zero: an empty pixel is told apart
out = dict(depths=clip["depths"], intrs=clip["intrs"], extrs=clip["extrs"], colors=colors, min_depth=np.array([0.01]))
flat = np.arange(V * H * W).reshape(V, H, W)
for tv in range(V):
    others = [sv for sv in range(V) if sv != tv]
    p = np.concatenate([pts[sv][valid[sv]] for sv in others]).astype(np.float32)
    c = np.concatenate([colors[sv].transpose(1, 2, 0)[valid[sv]] for sv in others])
    src = np.concatenate([flat[sv][valid[sv]] for sv in others]).astype(np.int32)
    K, E = clip["intrs"][0, tv, 0].astype(np.float64), clip["extrs"][0, tv, 0].astype(np.float64)
    world_T_cam = _invert_rigid(np.vstack([E, [0, 0, 0, 1]]))
    bgr = render_dense_pointcloud(W, H, p, c, K, world_T_cam, 0.01)
    ref_color = np.ascontiguousarray(bgr[..., ::-1].transpose(2, 0, 1))  # planar R, G, B
    mine = R.render_points(p, c, clip["intrs"][0, tv, 0], clip["extrs"][0, tv, 0], H, W, 0.01)
    differ = int((mine[0] != ref_color).any(0).sum())
    coverage = float((mine[2] >= 0).mean())
    print(f"view {tv}: {len(p)} points, coverage {coverage:.3f}, restatement differs from the reference in {differ} of {H * W} pixels")
    assert differ == 0
    own = np.ascontiguousarray(colors[tv].transpose(1, 2, 0))
    ren = np.ascontiguousarray(ref_color.transpose(1, 2, 0))
    out[f"points_{tv}"], out[f"point_colors_{tv}"], out[f"point_source_{tv}"], out[f"color_{tv}"] = p, c, src, ref_color
    out[f"scores_{tv}"] = np.array([scores.compute_mse(ren, own), scores.compute_psnr(ren, own), scores.compute_mae(ren, own)], np.float64)
np.savez_compressed(os.path.join(HERE, "reproject_render.npz"), **out)
print("reproject_render.npz", os.path.getsize(os.path.join(HERE, "reproject_render.npz")) / 1024, "KiB")
