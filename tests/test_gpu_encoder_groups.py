"""The composite encoder's image groups (`encoder_run`, MVT_ENC_GROUP): a grouped call leaves exactly what an ungrouped call leaves.

The half-resolution section (stem, layer 1) may be issued for a few images at a time, so that its maps stay in the last-level cache
between the launch that writes them and the launch that reads them.  No kernel changes, every image keeps its slice of every
buffer, so everything here is `torch.equal`: no bar.

 * grouped = ungrouped: forced group sizes 1, 2 (n is odd: a short last group), n and n + 2 against MVT_ENC_GROUP = n + 5 (one
   pass): the rows, and every activation buffer left in the workspace.  The workspace starts as 0xFF bytes with a poisoned guard
   behind it and behind the rows; the guards, the gaps between the plan's buffers and the ldo padding stay untouched.
   n = 5 at 32 x 48 and n = 3 at 64 x 64 (a stem map of more than one column tile and several row tiles), latent_dim 128 and 160,
   both entry points (x4; the clip as fp32 and as uint8, starting inside a frame), fp32 and bf16 rows, short_workgroups 0 / 1.
 * statistics are per image: image i of the grouped n = 5 call = the n = 1 call on that image alone (a slice of a statistics
   table or of the partial sums read after another group wrote it would show here).
 * the override is read on every call: two calls of one process with different values both equal the reference, and the rule
   (unset, 0) leaves these shapes in one pass; a negative value is an argument error.

The layout (`plan`), the weights and the workspace checks are those of test_gpu_encoder_wiring.py; the clip is two of its clips
one after the other (its own has room for three images only).
"""
import functools
import os

import pytest
import torch

import encoder_wiring_ref as R
import test_gpu_encoder_wiring as Wr
from test_gpu_encoder_wiring import hip  # noqa: F401  (fixture)

gpu = pytest.mark.gpu
ENV = "MVT_ENC_GROUP"

Case = Wr.Case
A, B = (5, 32, 48), (3, 64, 64)
CASES = [
    Case(*A, 128, 0, "x4", True, 0),
    Case(*A, 128, 1, "rgb-u8", False, 8),
    Case(*A, 128, 0, "rgb-f32", True, 8),
    Case(*A, 160, 0, "x4", False, 0),
    Case(*B, 128, 0, "x4", False, 8),
    Case(*B, 128, 1, "rgb-f32", True, 0),
    Case(*B, 128, 0, "rgb-u8", True, 0),
]


class group:
    """MVT_ENC_GROUP for the calls inside (None: unset), restored afterwards."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop(ENV, None)
        if self.value is not None:
            os.environ[ENV] = str(self.value)

    def __exit__(self, *exc):
        os.environ.pop(ENV, None)
        if self.old is not None:
            os.environ[ENV] = self.old


V, T, IMG0 = R.V_CLIP, 2 * R.T_CLIP, R.IMG0  # two of the wiring suite's clips, one after the other: room for 5 images from IMG0


@functools.lru_cache(maxsize=None)
def clip_of(H, W):
    return torch.cat([R.make_clip(H, W, 0), R.make_clip(H, W, 1)], 1).contiguous()


def source(form, H, W, n):
    """The call's input on the device: x4 [n][H][W][4] fp32, or the clip (V, T, 3, H, W) as fp32 / uint8."""
    clip = clip_of(H, W)
    if form == "x4":
        return R.x4_of(R.normalised(R.clip_images(clip, n, IMG0))).to(Wr.DEV)
    return (clip if form == "rgb-u8" else clip.float()).contiguous().to(Wr.DEV)


def call(hip, dv, n, H, W, form, swg, out_bf16, ldo_extra, src=None):
    """`call` of the wiring suite on this file's clip: one call in a fresh workspace of 0xFF bytes with a poisoned guard behind it
    and behind the rows -> (rows [n][H/4][W/4][C] on the CPU, the workspace bytes on the CPU)."""
    C, ldo = dv.C, dv.C + ldo_extra
    total = hip.encoder_workspace_bytes(n, H, W, C)
    assert total == Wr.plan(n, H, W, C)["total"]
    ws = torch.full((total + Wr.GUARD,), 0xFF, dtype=torch.uint8, device=Wr.DEV)
    M = n * (H // 4) * (W // 4)
    rows = torch.full((M * ldo + Wr.GUARD,), Wr.NAN, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=Wr.DEV)
    w = dv.comp["encoder_struct_shared" if swg else "encoder_struct"]
    assert w.latent_dim == C and w.short_workgroups == swg
    src = source(form, H, W, n) if src is None else src
    try:
        if form == "x4":
            hip.encoder_forward(w, src, n, H, W, rows, ldo, ws[:total])
        else:
            hip.encoder_forward_rgb(w, src, V, T, IMG0, n, H, W, rows, ldo, ws[:total])
    finally:
        torch.cuda.synchronize()
    r = rows.cpu()
    body = r[:M * ldo].view(M, ldo)
    assert bool(torch.isnan(r[M * ldo:]).all()), "the guard behind the rows was written"
    assert bool(torch.isnan(body[:, C:]).all()), "the ldo padding was written"
    return body[:, :C].reshape(n, H // 4, W // 4, C).clone(), ws.cpu()


def run(hip, c, g, src=None, n=None):
    """One call of case c under MVT_ENC_GROUP = g -> (rows, the activation tensors left behind), guards and gaps checked."""
    n = c.n if n is None else n
    with group(g):
        rows, wsb = call(hip, Wr.device(c.C), n, c.H, c.W, c.form, c.swg, c.out_bf16, c.ldo_extra, src=src)
    return rows, Wr.check_workspace(wsb, n, c.H, c.W, c.C)


@functools.lru_cache(maxsize=None)
def reference(hip, c):
    """The ungrouped call of case c (computed once, shared)."""
    return run(hip, c, c.n + 5)


def assert_equal_calls(got, want, what):
    Wr.assert_same(got[0], want[0], f"{what}: rows")
    for name in Wr.ACTIVATIONS:
        a, b = got[1][name], want[1][name]
        assert bool(torch.isfinite(a).all()), (what, name)
        assert torch.equal(a, b), f"{what}: {name}: {int((a != b).sum())} of {a.numel()} elements differ"


def test_cases_cover_what_they_should():
    """(CPU) the shapes have a short last group at g = 2, more than one tile of the stem map, and every option appears."""
    for c in CASES:
        assert c.n % 2 == 1 and c.n > 2 and c.H % 4 == 0 and c.W % 4 == 0
    assert {c.form for c in CASES} == {"x4", "rgb-f32", "rgb-u8"} and {c.swg for c in CASES} == {0, 1}
    assert {c.out_bf16 for c in CASES} == {False, True} and {c.C for c in CASES} == {128, 160}
    assert (B[1] // 2 + 7) // 8 > 1 and (A[2] // 2 + 31) // 32 == 1 and (B[2] // 2) % 32 == 0
    assert IMG0 % V != 0 and IMG0 + A[0] <= V * T and (IMG0 + A[0] - 1) // V > IMG0 // V


@gpu
@pytest.mark.parametrize("c", CASES, ids=Wr.case_id)
def test_grouped_equals_ungrouped(hip, c):
    want = reference(hip, c)
    for g in (1, 2, c.n, c.n + 2):
        assert_equal_calls(run(hip, c, g), want, f"groups of {g}")


@gpu
@pytest.mark.parametrize("g", [1, 2])
def test_statistics_are_per_image(hip, g):
    c = CASES[0]
    x4 = source("x4", c.H, c.W, c.n)
    rows, Tn = run(hip, c, g, src=x4)
    for i in range(c.n):
        r1, T1 = run(hip, c, c.n + 5, src=x4[i:i + 1].contiguous(), n=1)
        Wr.assert_same(r1[0], rows[i], f"image {i}: rows")
        for name in Wr.ACTIVATIONS:
            assert torch.equal(T1[name][0], Tn[name][i]), (i, name)


@gpu
def test_override_is_read_per_call(hip):
    c = CASES[1]
    want = reference(hip, c)
    for g in (2, c.n + 5, 1, None, 0, 3):  # (None, 0: the rule, one pass at this size)
        assert_equal_calls(run(hip, c, g), want, f"MVT_ENC_GROUP={g}")


@gpu
@pytest.mark.parametrize("form", ["x4", "rgb-f32"])
def test_negative_override_is_an_argument_error(hip, form):
    from mvtracker_amd.hip import HipError
    c = CASES[0]._replace(form=form)
    with pytest.raises(HipError, match="arguments rejected"):
        run(hip, c, -1)
    assert_equal_calls(run(hip, c, 2), reference(hip, CASES[0]), "after the rejected call")
