"""Launch-sequence recording shared by tests/test_launch_sequence_host.py and tests/golden/make_launch_sequence.py -- TEST
INFRASTRUCTURE ONLY.

``record(monkeypatch, case)`` installs tests/hip_mock.py, wraps every entry the mock patched so that each call appends
(entry name, every int / float / bool positional argument in order), runs one case of ``CASES`` and returns what the fixture
holds for it: the entry names in call order, a SHA-256 of the full records and a SHA-256 of the result tensors' bytes.  The host
code decides every one of those scalars (sizes, strides, leading dimensions, frame numbers, flags), so a refactor of the host
code that changes a launch, its order or one of its scalar arguments changes the digest.
"""
import hashlib
import json

import numpy as np
import torch

from mvtracker_amd import synth

import hip_mock


def _model(precision, **switches):
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.precision = precision
    m.fold_downsample = False  # (the mock has no folded-downsample entry)
    for k, v in switches.items():
        setattr(m, k, v)
    return m


def _forward(precision, backward=False):
    def run():
        m = _model(precision)
        clip = {k: torch.from_numpy(v) for k, v in synth.make_clip(7, V=2, T=14, H=96, W=128, N=5).items()}
        kw = {}
        if backward:  # query frames late enough that the reversed pass has windows to run
            clip["query_points"][0, :, 0] = torch.tensor([0.0, 5.0, 9.0, 12.0, 13.0])
            kw["backward_tracking"] = True
        r = m(clip["rgbs"], clip["depths"], clip["query_points"], clip["intrs"], clip["extrs"], iters=2, **kw)
        if backward:
            assert m.last_windows_backward
        return [r[k] for k in sorted(r)] + [m.last_vis_logits]
    return run


def _update_former(precision, tracks, **switches):
    def run():
        m = _model(precision, **switches)
        x = np.random.default_rng(11).standard_normal((1, tracks, m.S, m.updateformer_input_dim)).astype(np.float32)
        return [m.update_former(torch.from_numpy(x))]
    return run


CASES = {
    "forward_fp32": _forward("fp32"),
    "forward_bf16x3": _forward("bf16x3"),
    "forward_bf16": _forward("bf16"),
    "forward_backward_fp32": _forward("fp32", backward=True),
    "update_former_fp32": _update_former("fp32", 3),
    "update_former_bf16": _update_former("bf16", 3),
    "update_former_bf16_unfused": _update_former("bf16", 3, fuse_blocks=False),
    "update_former_bf16_unfused_280": _update_former("bf16", 280, fuse_blocks=False),  # rows >= 4096: mlp_fused_bf16
}


def _scalars(args):
    out = []
    for a in args:
        if isinstance(a, (bool, np.bool_)):
            out.append(bool(a))
        elif isinstance(a, (int, np.integer)):
            out.append(int(a))
        elif isinstance(a, (float, np.floating)):
            out.append(float(a))
    return out


def record(monkeypatch, case):
    """Run ``CASES[case]`` on the mocked library -> dict(names, records_sha256, results_sha256)."""
    from mvtracker_amd import hip
    hip_mock.install(monkeypatch)
    records = []

    def wrap(name, fn):
        def entry(*args, **kwargs):
            records.append([name, _scalars(args)])
            return fn(*args, **kwargs)
        return entry

    for name in dir(hip_mock):
        fn = getattr(hip_mock, name)
        if callable(fn) and not name.startswith("_") and getattr(hip, name, None) is fn:  # patched by ``install``
            monkeypatch.setattr(hip, name, wrap(name, fn))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (one reduction order for the result digest, whatever the machine's core count)
    try:
        results = CASES[case]()
    finally:
        torch.set_num_threads(threads)
    h = hashlib.sha256()
    for t in results:
        h.update(t.detach().contiguous().numpy().tobytes())
    return dict(names=[r[0] for r in records], records_sha256=hashlib.sha256(json.dumps(records).encode()).hexdigest(),
                results_sha256=h.hexdigest())
