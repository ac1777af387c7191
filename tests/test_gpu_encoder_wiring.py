"""The composite encoder (`mvt_encoder_forward`, `mvt_encoder_forward_rgb`) stage by stage: its wiring and its workspace.

The entry has no kernels of its own -- every kernel it launches has an exact suite -- but it decides which table normalises
which tensor, which buffer a launch reads and writes, which image a row of a table belongs to, and how large each buffer of the
shared workspace is.  An end-to-end bar cannot see that: the summation order of the convolutions alone moves the final output by
about 1 % of its RMS (one bf16 rounding flip reaches nine pixels of every output channel of the next convolution).  So the tests
read the tensors a call LEAVES BEHIND in its workspace and compare segment by segment, each segment fed with the device's own
input ("teacher forced"), against the fp64 reference of `encoder_wiring_ref.py`, which lists the rounding points.

GPU tests carry the `gpu` marker; the others are the CPU checks of the reference, of the restated plan, of the bars' conditions
and of the probes.  Weights are the test's own: bf16-representable, every one of the 22 convolutions different, every bias
non-zero, packed by `MVTracker._pack` (the layout is the kernel suites' subject), images with different statistics.

Cases (section "cases" below).  3 x 36 x 68 is ragged everywhere: stem map 18 x 34 (row tiles 8, 8, 2; columns 32 + 2), pyramid
9 x 17, 5 x 9, 3 x 5, features 9 x 17, stride-2 tiles of 4, 4, 1 rows.  2 x 32 x 64 has whole tiles.  latent_dim 128 (conv2 on the
256-channel big tile unless short_workgroups) and 32 (row tiles), short_workgroups 0 / 1, fp32 and bf16 rows, ldo = C + 8, the x4
entry and the rgb entry (fp32 and uint8 clip, V = 3, T = 2, img0 = 2: the run starts inside a frame and crosses into the next).
1 x 16 x 16, the smallest the entry accepts, only runs the invariants: its last stage is 1 x 1, and InstanceNorm over one pixel
multiplies the bf16 rounding of that pixel by 1 / sqrt(eps) = 316 -- two fp32 summation orders differ there by more than the
signal, so the reference pair cannot hold any useful bar.

One call per case: workspace filled with 0xFF bytes (NaN as bf16 and as fp32), rows NaN, a poisoned guard behind both.  After
it: the guards, the gaps between the plan's activation buffers and the ldo padding are untouched, every compared tensor is finite.

 * One-step segments (image -> raw stem, s[0..3] -> cat, cat -> raw c2, s[2] -> d, z0 -> y): element by element,
   |got - want| <= one bf16 ulp of the larger magnitude + the fp32 accumulation bound of that element
   ((K + 1) 2^-23 (sum |w x| + |b|), `Encoder.acc_bound`; for the resize the bar derived in test_gpu_encoder_norm_exact.py);
   and the share of elements that differ at all is capped.
 * Multi-step segments (image -> s[0], s[l-1] -> s[l], cat -> rows): mean |d| / RMS, and the largest per-pixel channel-RMS of d
   over the RMS (it localises an edge pixel).

No bar is a constant.  For each (shape, latent_dim, segment, metric) the measure is the largest distance of either fp32-order
reference ("f32a", "f32b", "f32c") from the fp64 reference over the eight seeds SEEDS, every segment fed with the intermediate tensors of
an "f32a" run (the stand-in for the device's), computed here on the CPU from the references only -- never from the device.  The
bar is FACTOR = 4 times the measure: the device is a third summation order, and the maximum over a few samples of a flip process
fluctuates by a small factor.  The cap on the differing share is set the same way (4 x the references' largest share, at least
four elements).  `test_reference_conditions` asserts on the CPU that the references keep the element-wise bound themselves and
that the caps stay below 1 %.  A device outside a bar is a finding: a rounding point the reference misses, or a defect.

`plan()` restates the workspace layout of `encoder_forward.hip`: A CHANGE TO THE PLAN THERE MUST BE MADE HERE TOO.  Its total is
asserted equal to `mvt_encoder_workspace_bytes` for every case.

Invariants (torch.equal, no bar): a call does not depend on what its workspace held; image i of an n = 3 call equals the n = 1
call on it (`encode_images` chunks by 16); x4 = rgb fp32 = rgb uint8; short_workgroups 0 = 1; the bf16 rows are the fp32 rows
rounded to nearest even; 16 x 16 runs inside its guards; the composite equals the Python-sequenced path; latent_dim 160 (conv2
has 320 > 256 channels: the statistics tables and partials are sized from max(256, 2C)) keeps its guards and equals the Python
sequence at 2 x 16 x 16 and 3 x 36 x 68.

Probes (CPU): each fault of `encoder_wiring_ref.FAULTS`, planted in the reference's wiring, leaves the bar of a segment it acts
in by a factor of 2 at least, on the GPU tests' own weights and images.  Out of reach, by construction: a bias in front of an
InstanceNorm cancels exactly (only conv3's bias is visible), and a wrong eps (it showed only 3 - 10 x the noise in a prototype).

The switches a process reads once (MVT_FOLD_DOWNSAMPLE, MVT_ROWS_NW8, MVT_APPLY_GENERIC, MVT_CONCAT_GENERIC) are set by
tests/test_gpu_tuning_switches.py, which runs cases of this file in a child process per value.  Not switched: MVT_CONV_BIG.
"""
import collections
import functools

import pytest
import torch

import encoder_wiring_ref as R

gpu = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
GUARD = 4096          # poisoned bytes behind the workspace, poisoned elements behind the rows
FACTOR = 4.0          # bar = FACTOR x the references' own distance (docstring)
SEEDS = tuple(range(8))
V, T, IMG0 = R.V_CLIP, R.T_CLIP, R.IMG0

Case = collections.namedtuple("Case", "n H W C swg form out_bf16 ldo_extra")
RAGGED, WHOLE = (3, 36, 68), (2, 32, 64)
CASES = [
    Case(*RAGGED, 128, 0, "x4", False, 8),
    Case(*RAGGED, 128, 1, "x4", True, 8),
    Case(*RAGGED, 128, 0, "rgb-u8", False, 0),
    Case(*RAGGED, 32, 0, "rgb-f32", True, 8),
    Case(*WHOLE, 128, 0, "x4", True, 0),
    Case(*WHOLE, 128, 1, "rgb-u8", False, 8),
    Case(*WHOLE, 32, 0, "x4", False, 8),
]
SHAPES = sorted({(c.n, c.H, c.W, c.C) for c in CASES})
ONE_STEP = ("stem", "cat", "c2", "d", "y")
MULTI_STEP = ("s0", "stage1", "stage2", "stage3", "out32", "out16")


def case_id(c):
    return f"{c.n}x{c.H}x{c.W}-C{c.C}-swg{c.swg}-{c.form}-{'bf16' if c.out_bf16 else 'fp32'}-ldo+{c.ldo_extra}"


# ================================================================== the plan, restated

def plan(n, H, W, C):
    """encoder_forward.hip `plan()`: name -> (byte offset, bytes), "total", and the [h][w][c] of what each activation buffer holds
    when a call returns.  A change to the plan there must be made here too."""
    h2, w2, hs, ws = H // 2, W // 2, H // 4, W // 4
    P, o = {}, 0

    def take(name, nbytes):
        nonlocal o
        P[name] = (o, nbytes)
        o += (nbytes + 255) & ~255

    for name in ("stem", "z0", "y"):
        take(name, n * h2 * w2 * 64 * 2)
    hh, ww, dims = h2, w2, []
    for l, c in enumerate(R.COUTS):
        if l:
            hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
        take(f"s{l}", n * hh * ww * c * 2)
        dims.append((hh, ww, c))
    take("d", n * hs * ws * 96 * 2)
    take("cat", n * hs * ws * 416 * 2)
    take("c2", n * hs * ws * 2 * C * 2)
    slots_max = ((h2 + 7) // 8) * ((w2 + 31) // 32)
    st_ch = max(256, 2 * C)
    take("part", n * slots_max * st_ch * 2 * 4)
    take("st", 8 * n * st_ch * 2 * 4)
    P["total"] = o
    last = dims[3]  # z0, y and d hold layer 4's tensors when the call returns
    P["holds"] = dict(stem=(h2, w2, 64), z0=last, y=last, d=last, cat=(hs, ws, 416), c2=(hs, ws, 2 * C),
                      **{f"s{l}": dims[l] for l in range(4)})
    return P


ACTIVATIONS = ("stem", "z0", "y", "s0", "s1", "s2", "s3", "d", "cat", "c2")


def test_plan_is_laid_out_as_restated():
    """Pure arithmetic of the restatement: buffers in order, 256-byte aligned, nothing overlaps, C <= 128 keeps 256-channel tables."""
    for (n, H, W, C) in SHAPES + [(1, 16, 16, 128), (2, 16, 16, 160), (3, 36, 68, 160)]:
        P = plan(n, H, W, C)
        end = 0
        for name in ACTIVATIONS + ("part", "st"):
            off, nb = P[name]
            assert off % 256 == 0 and off >= end and nb > 0
            end = off + nb
        assert P["total"] >= end and P["total"] % 256 == 0
        for name, (h, w, c) in P["holds"].items():
            assert n * h * w * c * 2 <= P[name][1], name
        assert P["st"][1] == 8 * n * max(256, 2 * C) * 8
        # conv2's partials (2C channels, one slot per 8 x 32 tile of the H/4 map) fit `part`, its table fits one ring slot
        assert n * ((H // 4 + 7) // 8) * ((W // 4 + 31) // 32) * 2 * C * 8 <= P["part"][1] and n * 2 * C * 8 <= P["st"][1] // 8


def test_plan_total_matches_library():
    """The restated total is the library's for every shape the tests run (host-side entry: no GPU needed)."""
    from mvtracker_amd import hip
    for (n, H, W, C) in SHAPES + [(1, 16, 16, 128), (1, 16, 16, 32), (2, 16, 16, 160), (3, 36, 68, 160), (3, 40, 72, 128), (1, 36, 68, 128),
                                   (3, 36, 68, 256), (16, 128, 128, 128)]:
        assert hip.encoder_workspace_bytes(n, H, W, C) == plan(n, H, W, C)["total"], (n, H, W, C)


# ================================================================== references, measures and bars (CPU)

@functools.lru_cache(maxsize=None)
def weights_of(C, seed):
    return R.make_weights(C, seed)


@functools.lru_cache(maxsize=None)
def clip_of(H, W, seed):
    return R.make_clip(H, W, seed)


def inputs(H, W, C, seed):
    return weights_of(C, seed), clip_of(H, W, seed)


def run_segments(enc, x, Tin, H, W):
    """Every segment of `enc` on the inputs of Tin (the tensors a call left behind) -> name -> (tensor, extra) with extra = the
    element-wise allowance of a one-step segment."""
    out = {}
    want, _, acc = enc.seg_stem(x)
    out["stem"] = (want, acc)
    out["s0"] = (enc.seg_s0(x), None)
    for l in (1, 2, 3):
        out[f"stage{l}"] = (enc.seg_stage(l + 1, Tin["s"][l - 1]), None)
    out["cat"] = enc.seg_cat(Tin["s"], H // 4, W // 4)
    c2, st, acc = enc.seg_c2(Tin["cat"])
    out["c2"] = (c2, acc)
    v = enc.seg_out(Tin["cat"], (c2, st))
    out["out32"], out["out16"] = (R.out_rows(v, False), None), (R.out_rows(v, True), None)
    out["d"] = enc.seg_d(Tin["s"][2])
    out["y"] = enc.seg_y(Tin["z0"])
    return out


def got_of(T):
    """The tensors of a call (or of Encoder.run) under the segments' names."""
    g = {"stem": T["stem"], "s0": T["s"][0], "cat": T["cat"], "c2": T["c2"], "d": T["d"], "y": T["y"]}
    g.update({f"stage{l}": T["s"][l] for l in (1, 2, 3)})
    return g


@functools.lru_cache(maxsize=None)
def stand_in(n, H, W, C, seed):
    """(x, the tensors of an "f32a" run, the fp64 segments on them): the CPU's stand-in for a device call."""
    Wt, clip = inputs(H, W, C, seed)
    x = R.Encoder(Wt, C).images(clip, n)
    Ta = R.Encoder(Wt, C, "f32a").run(x)
    return x, Ta, run_segments(R.Encoder(Wt, C), x, Ta, H, W)


@functools.lru_cache(maxsize=None)
def measures(n, H, W, C):
    """name -> the references' own figures over SEEDS: (segment, "mean") / (segment, "pix") for the multi-step segments,
    (segment, "ratio") / (segment, "share") for the one-step ones."""
    M = collections.defaultdict(float)
    for seed in SEEDS:
        x, Ta, want = stand_in(n, H, W, C, seed)
        for mode in R.MODES[1:]:
            got = run_segments(R.Encoder(inputs(H, W, C, seed)[0], C, mode), x, Ta, H, W)
            for seg in MULTI_STEP:
                dm, dp = R.distances(got[seg][0], want[seg][0])
                M[seg, "mean"], M[seg, "pix"] = max(M[seg, "mean"], dm), max(M[seg, "pix"], dp)
            for seg in ONE_STEP:
                ratio, share = R.elementwise(got[seg][0], want[seg][0], want[seg][1])
                M[seg, "ratio"], M[seg, "share"] = max(M[seg, "ratio"], ratio), max(M[seg, "share"], share)
    return dict(M)


def bars(n, H, W, C):
    M = measures(n, H, W, C)
    B = {k: FACTOR * v for k, v in M.items() if k[1] in ("mean", "pix")}
    for seg in ONE_STEP:
        numel = stand_in(n, H, W, C, 0)[2][seg][0].numel()
        B[seg, "share"] = max(FACTOR * M[seg, "share"], 4.0 / numel)
    return B


REACHED = collections.defaultdict(float)  # the largest fraction of each kind of bar a device call reached (printed)


def check_segments(got, want, B, out_seg, what, reached=None):
    """The assertions of one call: got / want name -> tensor / (tensor, extra); out_seg: "out32" or "out16" (got["out"])."""
    fails = []
    for seg in ONE_STEP:
        w, extra = want[seg]
        assert bool(torch.isfinite(got[seg]).all()), f"{what}: {seg} holds a value that is not finite"
        ratio, share = R.elementwise(got[seg], w, extra)
        if reached is not None:
            reached["element", seg] = max(reached["element", seg], ratio)
            reached["share", seg] = max(reached["share", seg], share / B[seg, "share"])
        if ratio > 1.0 or share > B[seg, "share"]:
            fails.append(f"{seg}: worst element at {ratio:.3g} of its bound, {share:.3g} of the elements differ (cap {B[seg, 'share']:.3g})")
    for seg in MULTI_STEP:
        if seg.startswith("out") and seg != out_seg:
            continue
        g = got["out"] if seg == out_seg else got[seg]
        assert bool(torch.isfinite(g).all()), f"{what}: {seg} holds a value that is not finite"
        dm, dp = R.distances(g, want[seg][0])
        if reached is not None:
            reached["mean", seg] = max(reached["mean", seg], dm / B[seg, "mean"])
            reached["pix", seg] = max(reached["pix", seg], dp / B[seg, "pix"])
        if dm > B[seg, "mean"] or dp > B[seg, "pix"]:
            fails.append(f"{seg}: mean {dm:.3g} (bar {B[seg, 'mean']:.3g}), pixel {dp:.3g} (bar {B[seg, 'pix']:.3g})")
    return fails


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_conditions(shape):
    """The conditions the bars rest on: all fp32-order references keep the element-wise bound of every one-step segment on every
    seed (largest ratio <= 1), their differing shares leave caps below 1 %, every multi-step measure is positive (a bar of zero would
    ask for bit equality) and small against a wiring fault (< 1e-2 mean); and a stand-in call passes the device's assertions."""
    n, H, W, C = shape
    M, B = measures(*shape), bars(*shape)
    print({f"{k[0]}.{k[1]}": float(f"{v:.3g}") for k, v in sorted(M.items())})
    for seg in ONE_STEP:
        assert M[seg, "ratio"] <= 1.0, (seg, M[seg, "ratio"])
        assert B[seg, "share"] <= 1e-2, (seg, B[seg, "share"])
    for seg in MULTI_STEP:
        assert 0 < M[seg, "mean"] < 1e-2 / FACTOR and 0 < M[seg, "pix"], (seg, M[seg, "mean"], M[seg, "pix"])
    x, Ta, want = stand_in(n, H, W, C, 0)
    for out_seg in ("out32", "out16"):
        got = dict(got_of(Ta), out=R.out_rows(R.Encoder(inputs(H, W, C, 0)[0], C, "f32a").seg_out(Ta["cat"]), out_seg == "out16"))
        assert check_segments(got, want, B, out_seg, "stand-in") == []


def test_reference_self_checks():
    """The weights are what the issue asks for; the reference's pieces agree with plain torch where they must."""
    import torch.nn.functional as F
    Wt, clip = inputs(36, 68, 128, 0)
    assert len(Wt) == 22
    flat = [w.reshape(-1) for w, _ in Wt.values()]
    for i, a in enumerate(flat):
        assert torch.equal(a, a.float().bfloat16().double()) and float(a.abs().max()) > 0
        for b in flat[:i]:
            assert a.numel() != b.numel() or not torch.equal(a, b)
    assert all(bool((b != 0).all()) and torch.equal(b, b.float().double()) for _, b in Wt.values())
    enc = R.Encoder(Wt, 128)
    x = enc.images(clip, 3)
    assert x.shape == (3, 36, 68, 3) and x.dtype == torch.float32 and float(x.min()) >= -1 and float(x.max()) <= 1
    m = x.reshape(3, -1).double().mean(1)
    assert float((m[0] - m[1]).abs()) > 1e-2 and float((m[1] - m[2]).abs()) > 1e-2  # the images' statistics differ
    # frame-major numbering: image i of the run is view (IMG0 + i) % V of frame (IMG0 + i) // V
    assert torch.equal(R.clip_images(clip, 3)[1], clip[(IMG0 + 1) % V, (IMG0 + 1) // V].permute(1, 2, 0))
    assert (IMG0 % V != 0) and (IMG0 + 3 - 1) // V > IMG0 // V  # starts inside a frame, crosses into the next
    # the whole chain without any rounding = InstanceNorm / ReLU / conv of plain torch (the wiring of blocks.py:214-284)
    T = enc.run(x)
    assert T["stem"].shape == (3, 18, 34, 64) and [tuple(s.shape[1:]) for s in T["s"]] == [(18, 34, 64), (9, 17, 96), (5, 9, 128), (3, 5, 128)]
    assert T["cat"].shape == (3, 9, 17, 416) and T["c2"].shape == (3, 9, 17, 256) and T["out"].shape == (3, 9, 17, 128) and len(T["tables"]) == 21

    def torch_encoder(xin):
        conv = lambda name, t, s: F.conv2d(t, Wt[name][0], Wt[name][1], stride=s, padding=Wt[name][0].shape[-1] // 2)
        inorm = lambda t: F.instance_norm(t, eps=R.EPS)
        t = F.relu(inorm(conv("fnet.conv1", xin.double().permute(0, 3, 1, 2), 2)))
        stages = []
        for li in (1, 2, 3, 4):
            for blk in (0, 1):
                p, s = f"fnet.layer{li}.{blk}", (R.STRIDES[li - 1] if blk == 0 else 1)
                y = F.relu(inorm(conv(p + ".conv1", t, s)))
                y = F.relu(inorm(conv(p + ".conv2", y, 1)))
                if blk == 0 and li > 1:
                    t = inorm(conv(p + ".downsample.0", t, s))
                t = F.relu(t + y)
            stages.append(t)
        cat = torch.cat([F.interpolate(s, size=(9, 17), mode="bilinear", align_corners=True) for s in stages], 1)
        return conv("fnet.conv3", F.relu(inorm(conv("fnet.conv2", cat, 1))), 1).permute(0, 2, 3, 1)

    plain = torch_encoder(x)
    dm, dp = R.distances(T["out"], plain)
    print(f"reference (bf16 rounding points) against plain fp64 torch: mean {dm:.3g}, pixel {dp:.3g}")
    assert dm < 3e-2 and dp < 1e-1  # bf16 activations through 23 convolutions: a percent; a wiring error in the reference: 0.1 - 1
    # a segment fed with the chain's own tensor reproduces the chain's next tensor bit for bit (fp64, same rounding points)
    for l in (1, 2, 3):
        assert torch.equal(enc.seg_stage(l + 1, T["s"][l - 1]), T["s"][l])
    assert torch.equal(enc.seg_s0(x), T["s"][0]) and torch.equal(enc.seg_cat(T["s"], 9, 17)[0], T["cat"])
    assert torch.equal(enc.seg_c2(T["cat"])[0], T["c2"]) and torch.equal(enc.seg_d(T["s"][2])[0], T["d"]) and torch.equal(enc.seg_y(T["z0"])[0], T["y"])


# ================================================================== probes (CPU)

def faulty(fault, seg, n, H, W, C):
    """The segment `seg` of the reference with `fault` planted, on the stand-in's inputs (seed 0, the GPU tests' own)."""
    Wt, clip = inputs(H, W, C, 0)
    _, Ta, _ = stand_in(n, H, W, C, 0)
    enc = R.Encoder(Wt, C, fault=fault, stale=Ta["tables"][10])
    x = enc.images(clip, n)
    if seg == "stem":
        return enc.seg_stem(x)[0]
    if seg == "s0":
        return enc.seg_s0(x)
    if seg.startswith("stage"):
        return enc.seg_stage(int(seg[-1]) + 1, Ta["s"][int(seg[-1]) - 1])
    if seg == "cat":
        return enc.seg_cat(Ta["s"], H // 4, W // 4)[0]
    assert seg == "out"
    return enc.seg_out(Ta["cat"])


@pytest.mark.parametrize("fault", sorted(R.FAULTS))
def test_probe(fault):
    """Each planted wiring fault leaves the bar of every segment it acts in by a factor of 2 at least (one-step: the worst
    element is at twice its bound at least), at every shape and latent_dim of the cases."""
    for (n, H, W, C) in SHAPES:
        if fault in ("short_row", "short_col") and (n, H, W) != RAGGED:
            continue  # (a ragged tile's fault)
        B = bars(n, H, W, C)
        _, _, want = stand_in(n, H, W, C, 0)
        for seg in R.FAULTS[fault]:
            bad = faulty(fault, seg, n, H, W, C)
            if seg in ONE_STEP:
                ratio, _ = R.elementwise(bad, *want[seg])
                assert ratio >= 2.0, (fault, seg, (n, H, W, C), ratio)
                continue
            for out_seg, b16 in ((seg, None),) if seg != "out" else (("out32", False), ("out16", True)):
                g = bad if b16 is None else R.out_rows(bad, b16)
                dm, dp = R.distances(g, want[out_seg][0])
                assert max(dm / B[out_seg, "mean"], dp / B[out_seg, "pix"]) >= 2.0, (fault, out_seg, (n, H, W, C), dm, dp, B[out_seg, "mean"], B[out_seg, "pix"])


# ================================================================== the device

@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


class Device:
    """An MVTracker whose encoder holds the test's weights (bf16 mode), and both of its packings: `comp` with the composite
    entry's weight structs, `seq` for the Python-sequenced path.  Only fnet.* is used: latent_dim is set on the instance, so that
    values the tracker as a whole does not take (160) still reach the encoder entry, which accepts any multiple of 32."""

    def __init__(self, C, seed=0):
        from mvtracker_amd.tracker import MVTracker
        m = MVTracker(hidden_size=256).eval().to(DEV)
        m.precision, m.latent_dim = "bf16", C
        params = dict(m.named_parameters())
        for name, (w, b) in weights_of(C, seed).items():
            params[name + ".weight"].data = w.float().to(DEV)
            params[name + ".bias"].data = b.float().to(DEV)
        self.m, self.C = m, C
        m.composite_encoder = True
        self.comp = m._pack(torch.device(DEV))
        assert "encoder_struct" in self.comp
        m.composite_encoder = False
        self.seq = m._pack(torch.device(DEV))
        assert "encoder_struct" not in self.seq

    def sequenced(self, x4, n, H, W, dtype):
        out = torch.full((n, H // 4, W // 4, self.C), NAN, device=DEV, dtype=dtype)
        self.m._encode(self.seq, x4, n, H, W, out)
        torch.cuda.synchronize()
        return out.cpu()


@functools.lru_cache(maxsize=None)
def device(C):
    return Device(C)


def source(form, H, W, n, seed=0):
    """The call's input on the device: x4 [n][H][W][4] fp32, or the clip (V, T, 3, H, W) as fp32 / uint8."""
    clip = clip_of(H, W, seed)
    if form == "x4":
        return R.x4_of(R.normalised(R.clip_images(clip, n))).to(DEV)
    return (clip if form == "rgb-u8" else clip.float()).contiguous().to(DEV)


def call(hip, dv, n, H, W, form="x4", swg=0, out_bf16=False, ldo_extra=0, src=None, ws=None):
    """One call of the composite entry -> (rows [n][H/4][W/4][C] on the CPU, the workspace bytes on the CPU).  ws: a byte buffer
    to run in as it is (its first `total` bytes are handed over); default: a fresh one of 0xFF bytes with a guard behind it."""
    C, ldo = dv.C, dv.C + ldo_extra
    total = hip.encoder_workspace_bytes(n, H, W, C)
    assert total == plan(n, H, W, C)["total"]
    if ws is None:
        ws = torch.full((total + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    assert ws.numel() >= total + GUARD and ws.data_ptr() % 256 == 0
    M = n * (H // 4) * (W // 4)
    rows = torch.full((M * ldo + GUARD,), NAN, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=DEV)
    w = dv.comp["encoder_struct_shared" if swg else "encoder_struct"]
    assert w.latent_dim == C and w.short_workgroups == swg
    src = source(form, H, W, n) if src is None else src
    if form == "x4":
        hip.encoder_forward(w, src, n, H, W, rows, ldo, ws[:total])
    else:
        hip.encoder_forward_rgb(w, src, V, T, IMG0, n, H, W, rows, ldo, ws[:total])
    torch.cuda.synchronize()
    r = rows.cpu()
    body = r[:M * ldo].view(M, ldo)
    assert bool(torch.isnan(r[M * ldo:]).all()), "the guard behind the rows was written"
    assert bool(torch.isnan(body[:, C:]).all()), "the ldo padding was written"
    return body[:, :C].reshape(n, H // 4, W // 4, C).clone(), ws.cpu()


def check_workspace(wsb, n, H, W, C, fresh=True):
    """On a fresh (0xFF) workspace: the guard and the gaps between the activation buffers are intact.  -> the tensors left behind."""
    P = plan(n, H, W, C)
    if fresh:
        assert bool((wsb[P["total"]:P["total"] + GUARD] == 0xFF).all()), "the guard behind the workspace was written"
    names = ACTIVATIONS + ("part",)
    Tn = {}
    for i, name in enumerate(ACTIVATIONS):
        off, nb = P[name]
        if fresh:
            assert bool((wsb[off + nb:P[names[i + 1]][0]] == 0xFF).all()), f"the gap behind {name} was written"
        h, w, c = P["holds"][name]
        Tn[name] = wsb[off:off + n * h * w * c * 2].view(torch.bfloat16).reshape(n, h, w, c).double()
    Tn["s"] = [Tn[f"s{l}"] for l in range(4)]
    return Tn


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_segments(hip, c):
    """One call; every segment of the fp64 reference applied to the device's own input, against what the device left behind."""
    dv = device(c.C)
    rows, wsb = call(hip, dv, c.n, c.H, c.W, c.form, c.swg, c.out_bf16, c.ldo_extra)
    Tn = check_workspace(wsb, c.n, c.H, c.W, c.C)
    Wt, clip = inputs(c.H, c.W, c.C, 0)
    enc = R.Encoder(Wt, c.C)
    want = run_segments(enc, enc.images(clip, c.n), Tn, c.H, c.W)
    reached = collections.defaultdict(float)
    fails = check_segments(dict(got_of(Tn), out=rows.double()), want, bars(c.n, c.H, c.W, c.C), "out16" if c.out_bf16 else "out32",
                           case_id(c), reached)
    print(case_id(c), {f"{k[0]}.{k[1]}": float(f"{v:.3g}") for k, v in sorted(reached.items())})
    for k, v in reached.items():
        REACHED[k[0]] = max(REACHED[k[0]], v)
    print("largest fraction of a bar so far:", {k: float(f"{v:.3g}") for k, v in sorted(REACHED.items())})
    assert not fails, fails


# ---------------------------------------------------------------- invariants (torch.equal)

def assert_same(a, b, what):
    assert bool(torch.isfinite(a.float()).all()) and float(a.float().abs().max()) > 0, what
    assert a.dtype == b.dtype and torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


@gpu
@pytest.mark.parametrize("C", [128, 32])
def test_workspace_contents_do_not_matter(hip, C):
    """The same call in a workspace of 0xFF bytes and in one a larger-shape call has just used: identical rows and tensors."""
    dv = device(C)
    n, H, W = RAGGED
    first, ws1 = call(hip, dv, n, H, W, out_bf16=True)
    big = torch.full((hip.encoder_workspace_bytes(n, H + 4, W + 4, C) + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    call(hip, dv, n, H + 4, W + 4, out_bf16=True, ws=big)
    second, ws2 = call(hip, dv, n, H, W, out_bf16=True, ws=big)
    assert_same(first, second, "rows")
    T1, T2 = check_workspace(ws1, n, H, W, C), check_workspace(ws2, n, H, W, C, fresh=False)
    for name in ACTIVATIONS:
        assert torch.equal(T1[name], T2[name]), name


@gpu
def test_images_are_independent(hip):
    """Image i of an n = 3 call = the n = 1 call on that image (rows and every tensor left behind)."""
    dv = device(128)
    n, H, W = RAGGED
    x4 = source("x4", H, W, n)
    rows, wsb = call(hip, dv, n, H, W, src=x4, out_bf16=True)
    Tn = check_workspace(wsb, n, H, W, 128)
    for i in range(n):
        r1, w1 = call(hip, dv, 1, H, W, src=x4[i:i + 1].contiguous(), out_bf16=True)
        assert_same(r1[0], rows[i], f"image {i}")
        T1 = check_workspace(w1, 1, H, W, 128)
        for name in ACTIVATIONS:
            assert torch.equal(T1[name][0], Tn[name][i]), (i, name)


@gpu
@pytest.mark.parametrize("C,out_bf16", [(128, False), (32, True)])
def test_input_forms_agree(hip, C, out_bf16):
    """x4 = the fp32 clip = the uint8 clip, images IMG0 .. of V = 3 views x T = 2 frames."""
    dv = device(C)
    n, H, W = RAGGED
    outs = [call(hip, dv, n, H, W, form, out_bf16=out_bf16)[0] for form in ("x4", "rgb-f32", "rgb-u8")]
    assert_same(outs[0], outs[1], "x4 against the fp32 clip")
    assert_same(outs[0], outs[2], "x4 against the uint8 clip")


@gpu
@pytest.mark.parametrize("shape", [RAGGED, WHOLE])
def test_short_workgroups_same_rows(hip, shape):
    dv = device(128)
    a, b = (call(hip, dv, *shape, swg=s)[0] for s in (0, 1))
    assert_same(a, b, "short_workgroups 0 against 1")


@gpu
@pytest.mark.parametrize("C", [128, 32])
def test_bf16_rows_are_rounded_fp32_rows(hip, C):
    dv = device(C)
    f, b = (call(hip, dv, *RAGGED, out_bf16=o, ldo_extra=8)[0] for o in (False, True))
    assert_same(f.bfloat16(), b, "bf16 rows against the fp32 rows rounded to nearest even")


@gpu
@pytest.mark.parametrize("n,C", [(1, 128), (1, 32), (2, 160)])
def test_smallest_image(hip, n, C):
    """16 x 16: the last stage is one pixel.  It runs, stays inside its guards and does not depend on its workspace's contents.
    (No bar here: InstanceNorm over one pixel amplifies that pixel's bf16 rounding by 316.)"""
    dv = device(C)
    src = source("x4", 16, 16, n)
    for out_bf16 in (False, True):
        first, ws1 = call(hip, dv, n, 16, 16, src=src, out_bf16=out_bf16, ldo_extra=8)
        check_workspace(ws1, n, 16, 16, C)
        big = torch.full((hip.encoder_workspace_bytes(n, 32, 32, C) + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        call(hip, dv, n, 32, 32, out_bf16=out_bf16, ws=big)
        second, _ = call(hip, dv, n, 16, 16, src=src, out_bf16=out_bf16, ldo_extra=8, ws=big)
        assert_same(first, second, "16 x 16 in a used workspace")


@gpu
@pytest.mark.parametrize("n,H,W,C", [(*RAGGED, 128), (*RAGGED, 32), (2, 16, 16, 160), (*RAGGED, 160)])
def test_equals_python_sequence(hip, n, H, W, C):
    """The composite against the same kernels sequenced from Python (MVTracker._encode without the weight struct), fp32 and bf16
    rows; at latent_dim 160 conv2's 320-channel table and partials are wider than the 256 the plan used to assume."""
    dv = device(C)
    x4 = source("x4", H, W, n)
    for out_bf16 in (False, True):
        rows, wsb = call(hip, dv, n, H, W, src=x4, out_bf16=out_bf16)
        check_workspace(wsb, n, H, W, C)
        assert_same(rows, dv.sequenced(x4, n, H, W, rows.dtype), f"composite against the Python sequence ({rows.dtype})")
