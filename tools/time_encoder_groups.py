"""One mvt_encoder_forward_rgb call alone on the chip per value of MVT_ENC_GROUP (groups of the half-resolution section): n = 24,
512 x 512, bf16 rows, HIP events, 30 calls after 5 warm-ups per value, the values interleaved round-robin, short_workgroups off
and on; every value must leave the rows of the first.  Run on the GPU box from the repo root:
    python tools/time_encoder_groups.py [out.json]      (prints the table; writes it as JSON when a path is given)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import hip, synth  # noqa: E402
from mvtracker_amd.tracker import MVTracker  # noqa: E402

dev = torch.device("cuda:0")
model = MVTracker(hidden_size=256).eval()
sd = synth.make_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=0)
model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
model.to(dev)
model.precision = "bf16"
model.composite_encoder = True
pk = model._pack(dev)
V, T, H, W, n, C = 4, 24, 512, 512, 24, model.latent_dim
rgbs = (torch.rand(V, T, 3, H, W, device=dev) * 255).contiguous()
rows = torch.empty(n * (H // 4) * (W // 4), C, dtype=torch.bfloat16, device=dev)
ws = torch.empty(hip.encoder_workspace_bytes(n, H, W, C), dtype=torch.uint8, device=dev)

groups = (24, 12, 8, 6, 4, 3, 2)
res = {}
for swg in (0, 1):
    w = pk["encoder_struct_shared" if swg else "encoder_struct"]
    times = {g: [] for g in groups}
    ref = None
    for it in range(35):
        for g in groups:
            os.environ["MVT_ENC_GROUP"] = str(g)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip.encoder_forward_rgb(w, rgbs, V, T, 8, n, H, W, rows, C, ws)
            e1.record()
            torch.cuda.synchronize()
            if it == 0:
                if ref is None:
                    ref = rows.clone()
                assert torch.equal(ref, rows), g
            if it >= 5:
                times[g].append(e0.elapsed_time(e1))
    for g in groups:
        t = np.array(times[g])
        res[f"short_workgroups {swg} / groups of {g}"] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), mean_ms=float(t.mean()))
        print(f"short_workgroups {swg}, groups of {g:2d}: median {np.median(t):.4f} min {t.min():.4f} mean {t.mean():.4f} ms", flush=True)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
    json.dump(res, open(sys.argv[1], "w"), indent=1)
