"""Writes tests/golden/rigid_umeyama.npz: the reference's ``align_umeyama(model=Q, data=P, known_scale=True)``
(mvtracker/datasets/utils.py) on unweighted clouds, for tests/test_rigid_host.py::test_restatement_equals_align_umeyama.  Run where
the reference checkout is (see _ref_import.py); nothing imports this module at test time.

The file that holds the function imports third-party modules that are absent here and that the function never touches (png,
torchvision); they are stubbed the way _ref_import.py stubs easydict.  Cases: 4 general clouds, then near-planar clouds with noise
(in-plane extent 0.2, off-plane sigma 1e-4, noise sigma 2e-4) drawn until three of them take the determinant correction and three do
not.  The clouds are fp32 numbers held in fp64, so that a test can put them through the fp32 interface unchanged."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import rigid_ref as R  # noqa: E402
from _ref_import import REF_ROOT  # noqa: E402


def load_align_umeyama():
    sys.path.insert(0, REF_ROOT)
    for name in ("png", "torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except ImportError:
                m = types.ModuleType(name)
                m.__path__ = []
                sys.modules[name] = m
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    spec = importlib.util.spec_from_file_location("_ref_datasets_utils", os.path.join(REF_ROOT, "mvtracker", "datasets", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.align_umeyama


def cloud(rng, n, planar):
    if planar:
        P = np.concatenate([rng.uniform(-0.1, 0.1, size=(n, 2)), rng.normal(scale=1e-4, size=(n, 1))], 1)
        noise = 2e-4
    else:
        P = rng.uniform(-0.15, 0.15, size=(n, 3))
        noise = 1e-3
    P = P @ R.rotation(rng.normal(size=3), rng.uniform(-3, 3)).T + rng.uniform(-1, 1, size=3)
    Q = P @ R.rotation(rng.normal(size=3), rng.uniform(-2, 2)).T + rng.uniform(-0.5, 0.5, size=3) + rng.normal(scale=noise, size=(n, 3))
    return P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)


def main():
    align_umeyama = load_align_umeyama()
    rng = np.random.default_rng(0)
    cases = [cloud(rng, n, False) for n in (4, 9, 40, 200)]
    want = {True: 3, False: 3}
    while any(want.values()):
        P, Q = cloud(rng, 8, True)
        f = R.kabsch(P, Q)[2]["flipped"]
        if want[f]:
            want[f] -= 1
            cases.append((P, Q))
    nmax = max(len(P) for P, _ in cases)
    out = dict(n=np.array([len(P) for P, _ in cases], np.int32), P=np.zeros((len(cases), nmax, 3)), Q=np.zeros((len(cases), nmax, 3)),
               R=np.zeros((len(cases), 3, 3)), t=np.zeros((len(cases), 3)), flipped=np.zeros(len(cases), bool))
    for k, (P, Q) in enumerate(cases):
        s, Rm, tv = align_umeyama(model=Q, data=P, known_scale=True)
        assert s == 1
        out["P"][k, :len(P)], out["Q"][k, :len(P)], out["R"][k], out["t"][k] = P, Q, Rm, tv
        out["flipped"][k] = np.linalg.det(np.linalg.svd((Q - Q.mean(0)).T @ (P - P.mean(0)))[0]) * \
            np.linalg.det(np.linalg.svd((Q - Q.mean(0)).T @ (P - P.mean(0)))[2]) < 0
        print(k, len(P), "flipped" if out["flipped"][k] else "", "det", np.linalg.det(Rm))
    np.savez_compressed(os.path.join(HERE, "rigid_umeyama.npz"), **out)
    print("wrote rigid_umeyama.npz:", len(cases), "cases,", int(out["flipped"].sum()), "with the determinant correction")


if __name__ == "__main__":
    main()
