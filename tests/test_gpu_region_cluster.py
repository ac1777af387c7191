"""Region clustering on the device against the fp64 restatement tests/cluster_ref.py and sklearn's recorded labels
(tests/golden/cluster_dbscan.npz).  Every comparison is exact: the lattice inputs make every d2 and r2 exact in fp32 (with pairs
exactly at eps), and the other inputs are asserted to keep every pair and every box face beyond the stated margins."""
import os

import numpy as np
import pytest
import torch

import cluster_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_dbscan.npz")
LEPS = 3.0 / 64.0  # the lattice's eps: coordinates are multiples of 1/64, so every d2 is a multiple of 2^-12 and r2 = 9 / 4096 exact
MARGIN = 1e-5
# (points, grid): 1 tile; 7 tiles (beyond the +-2 ring); 130 tiles in 3 groups; organised clouds of 3 x 5 and 9 x 10 patches
SIZES = {"list40": (40, (0, 0)), "list448": (448, (0, 0)), "list8320": (8320, (0, 0)), "grid24x40": (960, (40, 24)), "grid72x80": (5760, (80, 72))}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def rows4(p):
    out = np.zeros((len(p), 4), np.float32)
    out[:, :3] = np.asarray(p, np.float32)[:, :3]
    return out


def run(clouds, grid, eps, ms, poses=None, box=None):
    """clouds (C, P, 3 or 4) float32 -> numpy dict of the device's results."""
    from mvtracker_amd import cluster
    x = np.stack([rows4(c) for c in clouds])
    C, P = x.shape[:2]
    rtw = None if box is None else cluster.invert_poses(np.stack(poses), C).cuda()
    bounds = None if box is None else tuple(v for pair in box for v in pair)
    r = cluster.cluster_clouds(dev(x), C, P, grid, eps, ms, rtw, bounds)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def state_dict(row):
    return dict(zip(R.STATE_FIELDS, (int(v) for v in row)))


def lattice_cloud(P, seed, nan_frac=0.1):
    """P rows in multiples of 1/64: blobs dense enough for cores at min_samples 12, a sparse haze for borders and noise, some NaN
    rows, in shuffled order so that clusters span far tiles and groups."""
    rng = np.random.default_rng(seed)
    side = max(8, int(round((P / 0.06) ** (1 / 3))))
    n_blob = max(1, P // 150)
    centres = rng.integers(0, side, (n_blob, 3))
    pts = np.concatenate([centres[rng.integers(0, n_blob, P // 2)] + rng.integers(-3, 4, (P // 2, 3)), rng.integers(0, side, (P - P // 2, 3))])
    pts = pts[rng.permutation(P)].astype(np.float32) / 64.0
    pts[rng.random(P) < nan_frac] = np.nan
    return pts


@pytest.fixture(scope="module")
def lattice():
    """name -> (cloud, grid, {min_samples: restatement}) computed once."""
    out = {}
    for k, (name, (P, grid)) in enumerate(SIZES.items()):
        pts = lattice_cloud(P, 100 + k)
        out[name] = (pts, grid, {ms: R.dbscan(pts, LEPS, ms) for ms in (1, 2, 4, 12)})
    return out


@pytest.mark.parametrize("name", list(SIZES))
def test_lattice_labels_and_core_flags(lattice, name):
    pts, grid, ref = lattice[name]
    for ms in (1, 2, 4, 12):
        got = run([pts], grid, LEPS, ms)
        exp = ref[ms]
        n_lab, n_core = int((got["labels"][0] != exp["labels"]).sum()), int(((got["core"][0] != 0) != exp["core"]).sum())
        print(f"{name} min_samples {ms}: clusters {exp['labels'].max() + 1} core {int(exp['core'].sum())} border "
              f"{int(((exp['labels'] >= 0) & ~exp['core']).sum())} label mismatches {n_lab} core mismatches {n_core} status {got['state'][0, 7]}")
        assert n_lab == 0 and n_core == 0 and got["state"][0, 7] == 0
        assert got["state"][0, 2] == exp["labels"].max() + 1 and got["state"][0, 1] == exp["core"].sum()
        again = run([pts], grid, LEPS, ms)
        assert all(np.array_equal(got[k], again[k]) for k in got), "two runs differ"


def bit_reversed(P):
    bits = max(1, int(P - 1).bit_length())
    key = [int(format(i, f"0{bits}b")[::-1], 2) for i in range(P)]
    return np.argsort(np.asarray(key), kind="stable")


@pytest.mark.parametrize("P", [448, 8320])
@pytest.mark.parametrize("order", ["ascending", "reversed", "bit_reversed"])
def test_chains(P, order):
    """P collinear points at spacing exactly eps: the deepest union-find the size allows."""
    pos = {"ascending": np.arange(P), "reversed": np.arange(P)[::-1], "bit_reversed": bit_reversed(P)}[order]
    pts = np.zeros((P, 3), np.float32)
    pts[:, 0] = pos.astype(np.float32) * np.float32(LEPS)  # k * 3 / 64: exact
    ends = (pos == 0) | (pos == P - 1)
    for ms in (2, 3, 4):
        got = run([pts], (0, 0), LEPS, ms)
        lab, core, st = got["labels"][0], got["core"][0] != 0, state_dict(got["state"][0])
        print(f"chain {P} {order} min_samples {ms}: labels {np.unique(lab).tolist()} core {int(core.sum())} state {st}")
        assert st["status"] == 0
        if ms == 2:
            assert (lab == 0).all() and core.all() and st["clusters"] == 1 and st["chosen_size"] == P
        elif ms == 3:
            assert (lab == 0).all() and np.array_equal(core, ~ends) and st["clusters"] == 1 and st["noise"] == 0
        else:
            assert (lab == -1).all() and not core.any() and st["clusters"] == 0 and st["fallback"] == R.NONE and got["select"][0].all()


def test_border_point_takes_the_lower_cluster():
    """A non-core point within eps of core points of two clusters gets the lower id, whichever cluster comes first."""
    a = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float64)
    b = a + [7, 0, 0]
    bridge = np.array([[4, 0, 0]], np.float64)
    rng = np.random.default_rng(5)
    for first, second in ((a, b), (b, a)):
        pts = np.concatenate([first, bridge, second]) / 64.0
        d2 = ((pts[:, None] - pts[None]) ** 2).sum(-1)
        adj = d2 <= LEPS ** 2
        core = adj.sum(1) >= 4
        assert not core[4] and core[:4].all() and core[5:].all()  # the bridge is not core ...
        assert (adj[4, :4] & core[:4]).any() and (adj[4, 5:] & core[5:]).any()  # ... and reaches a core point of both clusters
        assert not adj[:4, 5:].any()  # which the core graph does not join
        slots = np.sort(rng.permutation(448)[:9])  # scattered over 7 tiles, the order kept
        cloud = np.full((448, 3), np.nan, np.float32)
        cloud[slots] = pts
        got = run([cloud], (0, 0), LEPS, 4)
        lab = got["labels"][0][slots]
        print("border labels", lab.tolist())
        assert lab.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]
        assert np.array_equal(got["labels"][0], R.dbscan(cloud, LEPS, 4)["labels"])


def test_degenerate_inputs(lattice):
    from mvtracker_amd import cluster
    nan = np.full((448, 3), np.nan, np.float32)
    got = run([nan], (0, 0), LEPS, 1)
    assert (got["labels"] == -1).all() and not got["core"].any() and not got["select"].any()
    assert state_dict(got["state"][0]) == dict(candidates=0, core=0, clusters=0, chosen=-1, chosen_size=0, noise=0, fallback=R.EMPTY, status=0)
    # NaN rows interleaved: the labels of the finite rows are those of the compact cloud
    pts = lattice["list448"][0]
    ok = R.valid_rows(pts)
    wide = np.full((2 * ok.sum(), 3), np.nan, np.float32)
    wide[1::2] = pts[ok]
    for ms in (2, 12):
        a, b = run([wide], (0, 0), LEPS, ms), run([pts[ok]], (0, 0), LEPS, ms)
        assert np.array_equal(a["labels"][0][1::2], b["labels"][0]) and (a["labels"][0][0::2] == -1).all()
        assert np.array_equal(b["labels"][0], R.dbscan(pts[ok], LEPS, ms)["labels"])
    # one point
    lab, info = cluster.cluster_points(dev([[0.25, 0.5, 1.0]]), LEPS, 1, return_info=True)
    assert lab.tolist() == [0] and info["clusters"] == 1 and info["core"].tolist() == [True] and info["status"] == 0
    assert cluster.cluster_points(dev([[0.25, 0.5, 1.0]]), LEPS, 2).tolist() == [-1]
    assert cluster.cluster_points(dev([[float("nan"), 0.5, 1.0], [0.0, 0.0, float("inf")]]), LEPS, 1).tolist() == [-1, -1]
    # duplicated points: 12 copies are each other's neighbours
    dup = np.tile(np.array([[0.5, 0.25, 0.125]], np.float32), (12, 1))
    assert cluster.cluster_points(dev(dup), LEPS, 12).tolist() == [0] * 12
    assert cluster.cluster_points(dev(dup), LEPS, 13).tolist() == [-1] * 12
    both = np.concatenate([dup, dup + np.float32(1.0), dup[:3]])
    assert cluster.cluster_points(dev(both), LEPS, 12).tolist() == [0] * 12 + [1] * 12 + [0] * 3
    # min_samples above every count: above the number of points (the reference's "few" rule) and at it (clustered: no cluster)
    for ms, fb in ((10 ** 6, R.FEW), (int(ok.sum()), R.NONE)):
        got = run([pts], (0, 0), LEPS, ms)
        print("min_samples", ms, "state", state_dict(got["state"][0]))
        assert (got["labels"] == -1).all() and not got["core"].any() and got["state"][0, 6] == fb
        assert np.array_equal(got["select"][0] != 0, ok)


def test_batch_equals_single_runs():
    clouds = [lattice_cloud(448, s, nan_frac=f) for s, f in ((7, 0.0), (8, 0.5), (9, 0.1))]
    clouds[1][:200] = np.nan  # whole tiles without a point
    for ms in (2, 12):
        got = run(clouds, (0, 0), LEPS, ms)
        for c, cloud in enumerate(clouds):
            one = run([cloud], (0, 0), LEPS, ms)
            for k in got:
                assert np.array_equal(got[k][c], one[k][0]), (ms, c, k)
            assert np.array_equal(got["labels"][c], R.dbscan(cloud, LEPS, ms)["labels"])


def test_fixture_clouds_give_sklearn_labels():
    from mvtracker_amd import cluster
    g = np.load(GOLDEN)
    names = sorted(k[:-len("_points")] for k in g.files if k.endswith("_points"))
    assert len(names) >= 3
    for name in names:
        pts = g[name + "_points"]
        for eps, ms, lab in zip(g[name + "_eps"], g[name + "_min_samples"], g[name + "_labels"]):
            got = cluster.cluster_points(dev(pts), float(eps), int(ms)).cpu().numpy()
            print(f"{name} eps {eps} min_samples {ms}: clusters {lab.max() + 1} mismatches {int((got != lab).sum())}")
            assert np.array_equal(got, lab)


def axis_pose(perm, signs, t):
    """world_T_region whose rotation is a signed axis permutation and whose translation is dyadic: inverse and crop are exact."""
    m = np.eye(4)
    m[:3, :3] = 0
    for r, (p, s) in enumerate(zip(perm, signs)):
        m[r, p] = s
    m[:3, 3] = t
    return m


def check_region(pts, pose, box, eps, ms, grid=(0, 0)):
    exp = R.select(pts, pose, box, eps, ms)
    got = run([pts], grid, eps, ms, [pose], box)
    st = state_dict(got["state"][0])
    print("region state", st, "expected", exp["state"], "selected", int(got["select"].sum()))
    assert np.array_equal(got["select"][0] != 0, exp["select"]) and np.array_equal(got["labels"][0], exp["labels"])
    assert st == exp["state"]
    return exp


def test_region_faces_and_axis_poses():
    """Dyadic points, many of them exactly on the planes of the box's faces: excluded, as the reference's strict test excludes them."""
    rng = np.random.default_rng(11)
    box = ((-0.5, 0.5), (-0.25, 0.25), (-0.125, 0.375))
    pts = (rng.integers(-40, 41, (8320, 3)) / 64.0).astype(np.float32)
    for perm, signs, t in (((0, 1, 2), (1, 1, 1), (0, 0, 0)), ((1, 2, 0), (1, -1, 1), (0.25, -0.5, 0.125)), ((2, 0, 1), (-1, 1, -1), (-1.5, 2.0, 0.75))):
        pose = axis_pose(perm, signs, t)
        world = (pts.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)  # region coordinates pts, exactly
        assert np.array_equal(R.region_coords(world, pose), pts.astype(np.float64))
        on_face = int(((np.abs(pts[:, 0]) == 0.5) | (np.abs(pts[:, 1]) == 0.25) | (pts[:, 2] == -0.125) | (pts[:, 2] == 0.375)).sum())
        exp = check_region(world, pose, box, LEPS, 4)
        print("points on a face plane", on_face, "kept", exp["state"]["candidates"])
        assert on_face > 500 and 0 < exp["state"]["candidates"] < len(pts)
        c = pts[R.crop(world, pose, box)]
        assert (np.abs(c[:, 0]) < 0.5).all() and (np.abs(c[:, 1]) < 0.25).all() and (c[:, 2] > -0.125).all() and (c[:, 2] < 0.375).all()


def general_case(seed, n, eps, box, spread):
    from camera_align_cases import rigid
    rng = np.random.default_rng(seed)
    pose = rigid(rng.uniform(-180, 180), rng.normal(size=3), rng.uniform(-1, 1, 3))
    lo, hi = np.asarray(box)[:, 0], np.asarray(box)[:, 1]
    local = np.concatenate([rng.uniform(lo - spread, hi + spread, (n // 2, 3)),
                            rng.normal(size=(n - n // 2, 3)) * 0.02 + rng.uniform(lo, hi, (4, 3))[rng.integers(0, 4, n - n // 2)]])
    world = (local @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)
    return pose, world


def test_region_general_poses():
    from mvtracker_amd import cluster
    box = cluster.DEFAULT_BOX
    done = 0
    for seed in range(20, 40):
        pose, world = general_case(seed, 448 if done % 2 else 2000, 0.03, box, 0.05)
        if R.face_margin(world, pose, box) < MARGIN or R.min_pair_gap(world, 0.03) <= MARGIN:
            continue  # (the next fixed seed: the comparison is exact only beyond the margins)
        assert R.face_margin(world, pose, box) >= MARGIN and R.min_pair_gap(world, 0.03) > MARGIN
        exp = check_region(world, pose, box, 0.03, 12)
        sel = cluster.select_region_points(dev(world), dev(pose, torch.float64), cluster.RegionCluster()).cpu().numpy()
        assert np.array_equal(sel, exp["select"])
        done += 1
        if done == 3:
            break
    assert done == 3


def test_region_fallbacks_and_equal_sizes():
    pose = axis_pose((0, 1, 2), (1, 1, 1), (0.5, 0.25, 0.0))
    box = ((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0))
    blob = np.array([[x, y, 0] for x in range(4) for y in range(3)], np.float64) / 64.0  # a 4 x 3 patch: one cluster at min_samples 4
    far = np.array([[10.0, 10.0, 10.0]])
    def world(local):
        return (np.asarray(local, np.float64) + pose[:3, 3]).astype(np.float32)
    # fewer than min_samples candidates: all of them
    exp = check_region(world(np.concatenate([blob[:5], far])), pose, box, LEPS, 12)
    assert exp["state"]["fallback"] == R.FEW and exp["select"].tolist() == [True] * 5 + [False]
    # enough candidates and no cluster: all of them
    spread = np.array([[i * 4, 0, 0] for i in range(14)], np.float64) / 64.0  # 4 > 3 lattice units apart, all inside the box
    exp = check_region(world(np.concatenate([spread, far])), pose, box, LEPS, 3)
    assert exp["state"]["fallback"] == R.NONE and exp["select"].tolist() == [True] * 14 + [False]
    # nothing inside
    exp = check_region(world(np.concatenate([far, far + 1])), pose, box, LEPS, 3)
    assert exp["state"]["fallback"] == R.EMPTY and not exp["select"].any()
    # two clusters of the same size: the lower id; a larger third one: that one
    two = np.concatenate([blob + [0.5, 0, 0], blob])
    exp = check_region(world(two), pose, box, LEPS, 4)
    assert exp["state"]["clusters"] == 2 and exp["state"]["chosen"] == 0 and exp["select"].tolist() == [True] * 12 + [False] * 12
    three = np.concatenate([two, blob + [0, 0.5, 0], blob[:6] + [0, 0.5, 1 / 64]])
    exp = check_region(world(three), pose, box, LEPS, 4)
    assert exp["state"]["clusters"] == 3 and exp["state"]["chosen"] == 2 and exp["state"]["chosen_size"] == 18


CLIP = dict(V=3, T=2, H=48, W=64, eps=0.12, min_samples=6, box=((-0.45, 0.45), (-0.45, 0.45), (-0.45, 0.45)))


@pytest.fixture(scope="module")
def clip():
    """A rendered scene with a compact object (the second sphere) at the pose; the second frame's pose is moved half off it."""
    import camera_align_cases as cases
    from mvtracker_amd import clean
    s = cases.scene(CLIP["V"], CLIP["H"], CLIP["W"], CLIP["T"])
    t = {k: torch.from_numpy(v).cuda() for k, v in s.items()}
    poses = np.stack([cases.rigid(20.0, (0.2, 0.4, 1.0), cases.SPHERES[1][0]), cases.rigid(-30.0, (1.0, 0.1, 0.3), np.add(cases.SPHERES[1][0], (0.3, 0.1, 0.02)))])
    pts = clean.clean_clip(t["depths"][0], t["intrs"][0], t["extrs"][0], clean.DepthCleaning(), details=True)[3].cpu().numpy()  # the clouds' points
    return t, poses, pts


def test_clip_masks_equal_the_restatement(clip):
    from mvtracker_amd import cluster
    t, poses, pts = clip
    region = cluster.RegionCluster(CLIP["box"], CLIP["eps"], CLIP["min_samples"])
    mask, report = cluster.region_masks(t["depths"], t["intrs"], t["extrs"], dev(poses, torch.float64), region)
    assert mask.shape == t["depths"].shape and mask.dtype == torch.bool
    m = mask[0, :, :, 0].cpu().numpy()
    print(report.table())
    for v in range(CLIP["V"]):
        for f in range(CLIP["T"]):
            cloud = pts[v, f].reshape(-1, 4)
            inside = np.where(R.crop(cloud, poses[f], CLIP["box"])[:, None], cloud[:, :3], np.nan)
            fm, gap = R.face_margin(cloud, poses[f], CLIP["box"]), R.min_pair_gap(inside, CLIP["eps"])
            print(f"view {v} frame {f}: face margin {fm:.3g} pair gap {gap:.3g}")
            assert fm >= MARGIN and gap > MARGIN
            exp = R.select(cloud, poses[f], CLIP["box"], CLIP["eps"], CLIP["min_samples"])
            assert np.array_equal(m[v, f].reshape(-1), exp["select"])
            for k in R.STATE_FIELDS:
                assert int(getattr(report, k)[v, f]) == exp["state"][k], (v, f, k)
            assert int(report.selected[v, f]) == int(exp["select"].sum())
    assert report.candidates.min() > 0 and report.clusters.max() >= 1 and m.any()
    assert {R.FEW, R.NONE} <= set(report.fallback.reshape(-1).tolist()) and (report.fallback == 0).any()  # both fallbacks occur, and neither
    # unbatched input, a single pose for every frame, details
    out = cluster.region_masks(t["depths"][0], t["intrs"][0], t["extrs"][0], poses[0], region, details=True)
    assert torch.equal(out[0][:, 0], mask[0][:, 0]) and out[2].shape == (CLIP["V"], CLIP["T"], CLIP["H"], CLIP["W"])
    exp = R.select(pts[0, 1].reshape(-1, 4), poses[0], CLIP["box"], CLIP["eps"], CLIP["min_samples"])
    assert np.array_equal(out[2][0, 1].cpu().numpy().reshape(-1), exp["labels"]) and np.array_equal(out[3][0, 1].cpu().numpy().reshape(-1), exp["core"])


def test_sample_queries_in_a_region(clip):
    from mvtracker_amd import cluster, queries
    t, poses, pts = clip
    region = cluster.RegionCluster(CLIP["box"], CLIP["eps"], CLIP["min_samples"])
    mask = cluster.region_masks(t["depths"], t["intrs"], t["extrs"], poses, region)[0][0, :, :, 0].cpu().numpy()
    spec = [(0, -10.0, 10.0, 100.0, 40, ""), (1, -10.0, 10.0, 100.0, 10 ** 6, ""), (1, -10.0, 10.0, 100.0, 8, "kmeans")]
    q = queries.sample_queries(t["depths"], t["intrs"], t["extrs"], spec, region=region, region_poses=poses, seed=2)
    again = queries.sample_queries(t["depths"], t["intrs"], t["extrs"], spec, region=region, region_poses=poses, seed=2)
    assert torch.equal(q, again)
    q = q[0].cpu().numpy()
    n1 = int(mask[:, 1].sum())
    print("pool sizes", int(mask[:, 0].sum()), n1, "queries", q.shape)
    assert q.shape == (40 + n1 + 8, 4) and (q[:40, 0] == 0).all() and (q[40:, 0] == 1).all()
    # the expected pool, by the arithmetic that defines it: the unrestricted pool of frame f (every pixel with depth > 0, in view,
    # row, column order: the cylinder and z range of the spec hold the whole scene) and of its rows those whose pixel is in the mask
    from mvtracker_amd import hip
    V, T = CLIP["V"], CLIP["T"]
    d = t["depths"][0].float().contiguous()
    kinv, einv = torch.empty(V * T, 9, device="cuda"), torch.empty(V * T, 12, device="cuda")
    hip.invert_cameras(t["intrs"][0].float().reshape(V * T, 9).contiguous(), t["extrs"][0].float().reshape(V * T, 12).contiguous(), kinv, einv, V * T)
    pools = {}
    for f in (0, 1):
        full = queries.frame_pool(d, kinv, einv, f, None, 0.9, (0.0, 0.0), 100.0, -10.0, 10.0).cpu().numpy()
        valid = (d[:, f, 0] > 0).cpu().numpy()
        assert len(full) == int(valid.sum()) and not (mask[:, f] & ~valid).any()
        pools[f] = full[mask[:, f][valid]]
        cloud = pts[:, f][mask[:, f]][:, :3]
        print("frame", f, "pool", len(pools[f]), "largest difference between the pool kernel's and the cloud kernel's points",
              float(np.abs(pools[f] - cloud).max()))
    assert len(pools[1]) == n1
    for f, rows in ((0, q[:40]), (1, q[40:40 + n1])):
        pool = {tuple(p) for p in pools[f].tolist()}
        got = [tuple(r) for r in rows[:, 1:].tolist()]
        assert all(g in pool for g in got) and len(set(got)) == len(got), f  # pool points bit for bit, none twice
    assert {tuple(r) for r in q[40:40 + n1, 1:].tolist()} == {tuple(p) for p in pools[1].tolist()} and len(pools[1]) == len({tuple(p) for p in pools[1].tolist()})  # a count above the pool: the pool whole
    lo, hi = pools[1].min(0), pools[1].max(0)
    assert ((q[40 + n1:, 1:] >= lo) & (q[40 + n1:, 1:] <= hi)).all()  # k-means centres lie in the pool's box
    plain = queries.sample_queries(t["depths"], t["intrs"], t["extrs"], spec[:1], seed=2)
    assert not torch.equal(plain, torch.from_numpy(q[None, :40]).cuda())
