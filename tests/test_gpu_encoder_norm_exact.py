"""The encoder's InstanceNorm chain and its resize / concat / repack kernels on inputs whose right answer is exact.

GPU tests (`-m gpu`) go through `mvtracker_amd.hip`; the tests without the marker are the CPU-only checks of the dispatch
restatement, of the reference-side conditions and of the probes.  Every output, partials and statistics buffer is poisoned (NaN)
before the launch, has a guard region behind its last element and a padded leading dimension where the entry has one; what the
kernel must not write has to stay poisoned.  Input padding columns (`ldx > C`) and the region behind the last input element hold
NaN: a read of either shows in the result.  Every call has at least two images with different data and different statistics.

The principle.  Inputs are small integers.  Planted statistics are integer means, of both signs inside every group of four
channels, and rstd in {0.5, 1, 2}; a channel with rstd 0.5 holds mean + even integers, so relu((x - mean) * rstd) is a small
non-negative INTEGER, exact in bf16, and so are the residual sums.  No comparison in this file is measured:

 * torch.equal, for every output, and for the statistics partials summed over their slots in fp64 on the CPU;
 * the one-ulp bar on rstd (A, C): the reference is float32(1 / sqrt(SS / HW - mean^2 + 1e-5)) evaluated in fp64 from the exact
   integer sums.  The device evaluates the same expression in fp64 but may contract `ss / HW - mean * mean` into an fma, which can
   move the last fp64 bit of the variance; relative to var + 1e-5 that is at most 2^-52 * mean^2 / (var + 1e-5) < 1e-8 here (the
   tests assert mean^2 <= 2^15 and var >= 1, or |x| <= 16 where var may be 0), below half an fp32 ulp (3e-8), so the only
   effect is the direction of one fp32 rounding: |got - want| <= one fp32 ulp of want.  The mean has no such freedom: S / HW is ONE
   correctly rounded fp64 division of exact operands and one rounding to fp32, so it is compared with torch.equal.
 * the derived bar of the one non-dyadic bilinear case (D): (2^-22 * max(Hs, Ws) + 8 * 2^-24) * max|x|.  The source coordinate
   ratio * index carries two fp32 roundings (the ratio, the product) of a quantity below max(Hs, Ws): an error of at most
   2^-23 * max(Hs, Ws) in the fractional weight l, and the result a + l (b - a) moves by that times the largest neighbour
   difference, 2 max|x|: 2^-22 * max(Hs, Ws) * max|x|.  The blend is seven fp32 roundings (four products, three sums) of
   quantities <= max|x|: bounded by 8 * 2^-24 * max|x|.

A. Statistics written by the convolutions (mvt_conv2d_bf16 with out_partial in bf16 and bf16x3 mode, mvt_conv3x3s2_down_bf16 with
   part3 / partd).  Operands are integers with |Y| <= 180 asserted of the fp64 reference: any 512 pixels then have sum(Y^2) < 2^24,
   so every fp32 slot sum is exact in any order and the per-(image, channel) sums over all slots equal the reference's exactly,
   whatever the slot layout.  (Weights are +-1 at a density of min(1, 300 / K): zeros are fine here, dropped product terms are
   the matmul suite's subject.)  `conv_variant` / `epilogue_form` restate the host dispatch; `test_cases_reach_every_form` asserts
   on the CPU that the cases reach every kernel form and every epilogue form.  In bf16x3 mode only the 3x3 / stride-1 halo kernel
   cuts an image into slots at any size; the im2col kernels need Ho * Wo % 256 == 0 and the entry refuses out_partial otherwise
   (asserted).
B. Normalise-on-load (3x3 / stride 1 with in_stats, fp32 and bf16 tensors): torch.equal against the fp64 convolution of the
   explicitly normalised tensor, zero-padded AFTER the normalisation, and bit for bit against instnorm_apply + the plain
   convolution.  `test_normalised_padding_differs` shows on the CPU that normalising the padding changes every case (the negative
   means).
C. mvt_instnorm_stats, mvt_instnorm_finish_slots, mvt_instnorm_apply (generic fp32, the 16-byte bf16 kernel in its three template
   forms, the generic bf16 fallback at C = 12) in the four forms: no skip, skip, skip with statistics, the same with skip_relu.
D. mvt_resize_nearest, mvt_resize_bilinear_ac, mvt_concat_resize_bilinear_ac, the three RGB repack entries.  Bilinear sources
   are 64 * {-3..3}: at dyadic size ratios (weights are multiples of 1/8 per axis) every result is an integer <= 192, exact in
   fp32 and in bf16, and equals the fp64 formula.
E. Probes (CPU): planted faults in a Python restatement of the kernels' rules must break the assertions above on the cases' inputs.

MVT_ROWS_NW8, MVT_APPLY_GENERIC and MVT_CONCAT_GENERIC are read once per process: tests/test_gpu_tuning_switches.py runs cases
of this file in a child process per value.  `rows_tile` / `tile_rows` / `stat_slots` / `apply_kernel` / `concat_kernel` take the
switch values as arguments and default to the process's environment, so the slot-count assertion of `run_conv` follows the switch.
"""
import collections
import functools
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_gpu_matmul_exact import conv_out, env_int, rows_staged_fits, rows_tile  # the one definition of these restatements

gpu = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
YMAX = 180  # |Y| bound of A: 512 * 180^2 < 2^24
EPS = 1e-5


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


def cdiv(a, b):
    return (a + b - 1) // b


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def rint(g, lo, hi, *shape):
    """Integers in [lo, hi] as fp64."""
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def dt(ch):
    return torch.bfloat16 if ch == "b" else torch.float32


def guarded(t, dtype, guard=64, ld=None, fill=NAN):
    """`t` ([rows][cols] or flat) on the device in a NaN buffer: padded to `ld` columns, `guard` poisoned elements behind."""
    if ld is not None:
        rows, cols = t.shape
        buf = torch.full((rows * ld + guard,), fill, dtype=dtype)
        buf[:rows * ld].view(rows, ld)[:, :cols] = t.to(dtype)
    else:
        buf = torch.full((t.numel() + guard,), fill, dtype=dtype)
        buf[:t.numel()] = t.reshape(-1).to(dtype)
    return buf.to(DEV)


def poisoned(numel, dtype=torch.float32, guard=64):
    return torch.full((numel + guard,), NAN, dtype=dtype, device=DEV)


def taken(buf, rows, cols, ld, what):
    """The [rows][cols] result of a poisoned [rows][ld] + guard buffer; everything else must still be NaN."""
    torch.cuda.synchronize()
    b = buf.double().cpu()
    body = b[:rows * ld].view(rows, ld)
    assert bool(torch.isnan(body[:, cols:]).all()), f"{what}: columns past {cols} written"
    assert bool(torch.isnan(b[rows * ld:]).all()), f"{what}: guard written"
    return body[:, :cols].clone()


def assert_equal(got, want, what):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = ~(got == want)
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {i}: got {got[tuple(i)].item()} want {want[tuple(i)].item()}")


def breaks(check, *args):
    try:
        check(*args, "probe")
    except AssertionError:
        return True
    return False


REACHED = collections.defaultdict(float)  # the fraction of each derived bar the device reached (printed by the tests that own one)


def ulps_off(got, want):
    """|got - want| in fp32 ulps of want (both fp32 tensors)."""
    want = want.float()
    ulp = (torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()).double()
    return (got.double() - want.double()).abs() / ulp


def check_mean_rstd(mr, S, SS, HW, what):
    """mr [n][C][2] fp32 from the device; S, SS the exact fp64 sums [n][C]."""
    mean64 = S / HW
    var = (SS / HW - mean64 * mean64).clamp_min(0.0)
    assert float((mean64 * mean64).max()) <= 2 ** 15
    assert float(var.min()) >= 1.0 or float(S.abs().max()) <= 16 * HW, what  # the condition of the one-ulp bar (docstring)
    assert_equal(mr[..., 0], mean64.float(), what + " mean")
    off = ulps_off(mr[..., 1].float(), (1.0 / torch.sqrt(var + EPS)).float())
    REACHED["rstd ulps"] = max(REACHED["rstd ulps"], float(off.max()))
    assert float(off.max()) <= 1.0, f"{what}: rstd {float(off.max())} ulps off"


# ================================================================== planted statistics and the formulas (CPU, fp64)

def planted_stats(g, n, C):
    """(mean, rstd, step) [n][C]: integer means 1..5 in magnitude whose signs alternate with the channel (both signs inside every
    group of four) and flip from image to image, rstd in {0.5, 1, 2}, step = the spacing of x - mean that keeps (x - mean) * rstd an
    integer."""
    sign = 1.0 - 2.0 * ((torch.arange(C)[None, :] + torch.arange(n)[:, None]) % 2).double()
    mean = sign * rint(g, 1, 5, n, C)
    rstd = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n, C), generator=g)]
    step = torch.where(rstd == 0.5, 2.0, 1.0)
    for q in range(0, C - 3, 4):
        assert bool(((mean[:, q:q + 4] > 0).any(1) & (mean[:, q:q + 4] < 0).any(1)).all())
    return mean, rstd, step


def planted_tensor(g, mean, rstd, step, *space):
    """x [n][*space][C] = mean + step * d, d in {-2..2} ({-1..1} at rstd 2): (x - mean) * rstd is an integer in [-2, 2]."""
    n, C = mean.shape
    d = rint(g, -2, 2, n, *space, C)
    bc = lambda t: t.view(n, *([1] * len(space)), C)
    d = torch.where(bc(rstd) == 2.0, d.clamp(-1, 1), d)
    return bc(mean) + bc(step) * d


def normalise(x, mean, rstd, relu=True):
    n, C = mean.shape
    bc = lambda t: t.view(n, *([1] * (x.dim() - 2)), C)
    z = (x.double() - bc(mean)) * bc(rstd)
    return F.relu(z) if relu else z


def stats_tensor(mean, rstd):
    return torch.stack([mean, rstd], dim=-1).float().contiguous()


# ================================================================== A: the host dispatch, restated

# one convolution case; io = element types of (input, output): "f" fp32, "b" bf16; norm: with planted in_stats
Conv = collections.namedtuple("Conv", "prec io Cin Cout k s ldo_extra norm big", defaults=(0, False, True))


def conv_variant(c, Ho=None, nw8=None):
    """The kernel mvt_conv2d_bf16 launches for case c (conv_plan.h plan_conv); the row tile, and with it the staged epilogue,
    follows MVT_ROWS_NW8 (rows_tile)."""
    stem = c.Cin == 4
    inb, outb = c.io[0] == "b", c.io[1] == "b"
    ldo = c.Cout + c.ldo_extra
    st_ok = outb and c.Cout % 8 == 0 and ldo % 8 == 0
    if c.prec == "bf16x3":
        return ("halo",) if (c.k == 3 and c.s == 1 and not stem) else ("im2col",)
    if stem:
        return ("stem", 1 if c.Cout <= 32 else 2, st_ok)
    n96 = c.Cout % 64 != 0 and c.Cout % 96 == 0
    tm, nw = rows_tile(c.k, c.s, Ho, nw8)
    # (every call of this file takes statistics: the big tile, whose slots are its own 8-row tiles, only where the row tile has 8 too)
    if c.k == 3 and c.s == 1 and not c.norm and inb and st_ok and c.Cout % 256 == 0 and c.big and tm * nw == 8:
        return ("big",)
    tn = 3 if n96 else 2
    return ("rows", c.k, c.s, tn, st_ok and rows_staged_fits(tm, c.k, c.s, nw, tn))


def epilogue_form(c, Ho=None, nw8=None):
    """The form of epilogue_rows (conv_rows.hip) case c runs: staged transposed / staged by pixel / quad / pair / scalar."""
    v = conv_variant(c, Ho, nw8)
    ldo = c.Cout + c.ldo_extra
    if v[0] in ("halo", "im2col"):
        return "gemm"
    if v[0] == "big":
        return "staged-tr"
    tn, staged = (v[1], v[2]) if v[0] == "stem" else (v[3], v[4])
    if staged:
        return "staged-tr" if tn * 32 * 36 <= 32 * (tn * 32 + 8) else "staged-px"
    quads_compiled = v[0] == "stem" or tn == 3
    if quads_compiled and (c.Cout | ldo) % 4 == 0:
        return "quad"
    return "pair" if (c.Cout | ldo) % 2 == 0 else "scalar"


def tile_rows(c, Ho=None, nw8=None):
    """Output rows of one statistics slot (conv_plan.h tile_rows): the stem and the big tile keep 8."""
    if conv_variant(c, Ho, nw8)[0] == "rows":
        tm, nw = rows_tile(c.k, c.s, Ho, nw8)
        return tm * nw
    return 4 if (c.k == 3 and c.s == 2) else 8


def stat_slots(c, H, W, nw8=None):
    """mvt_conv2d_stat_slots."""
    Ho, Wo = conv_out(H, W, c.k, c.s)
    v = conv_variant(c, Ho, nw8)
    if v[0] == "halo":
        return cdiv(Ho, 8) * cdiv(Wo, 16) * 4
    if v[0] == "im2col":
        return Ho * Wo // 32 if (Ho * Wo) % 256 == 0 else 0
    return cdiv(Ho, tile_rows(c, Ho, nw8)) * cdiv(Wo, 32)


def apply_kernel(io, C, generic=None):
    """mvt_instnorm_apply on 16-byte aligned tensors: the 16-byte bf16 kernel or the generic one (generic = MVT_APPLY_GENERIC is set)."""
    generic = ("MVT_APPLY_GENERIC" in os.environ) if generic is None else generic
    return ("apply", "bf16-16B") if (io == "b" and C % 8 == 0 and C <= 2048 and not generic) else ("apply", "generic", io)


def concat_kernel(io, ctot, generic=None):
    """mvt_concat_resize_bilinear_ac: the row kernel of bf16 tensors or the generic one (generic = MVT_CONCAT_GENERIC is set)."""
    generic = ("MVT_CONCAT_GENERIC" in os.environ) if generic is None else generic
    return ("concat", "rows-bf16") if (io == "b" and not generic and ctot // 8 <= 256) else ("concat", "generic", io)


# output sizes against the 8 x 32 tile: smaller than one tile, exactly one, one row and one column over, ragged in both directions
OUT_S1 = [(5, 20), (8, 32), (9, 33), (13, 45)]
OUT_S2 = [(3, 20), (4, 32), (5, 33), (7, 45)]  # 4 x 32 tiles (3x3 / stride 2, the fused downsample)
N_IMG = 2


def in_size(ho, wo, s, i):
    """An input size with that output size; for stride 2, odd and even inputs alternate."""
    return (ho, wo) if s == 1 else (2 * ho - (i % 2), 2 * wo - ((i + 1) % 2))


def conv_geos(c):
    v = conv_variant(c)
    if v[0] == "im2col":  # slots only where Ho * Wo % 256 == 0
        return [in_size(8, 32, c.s, 0), in_size(16, 48, c.s, 1)]
    if c.Cin == 416:
        return [(9, 33)]
    outs = OUT_S2 if (c.k == 3 and c.s == 2) else OUT_S1
    return [in_size(ho, wo, c.s, i) for i, (ho, wo) in enumerate(outs)]


CONV_CASES = [
    # 1x1, stride 1 and 2
    Conv("bf16", "fb", 32, 64, 1, 1), Conv("bf16", "bf", 64, 96, 1, 1), Conv("bf16", "ff", 96, 34, 1, 1),
    Conv("bf16", "bb", 64, 72, 1, 2), Conv("bf16", "ff", 32, 33, 1, 2), Conv("bf16", "fb", 96, 96, 1, 2, ldo_extra=2),
    # 3x3 stride 1 without in_stats: every epilogue form
    Conv("bf16", "bb", 64, 64, 3, 1), Conv("bf16", "fb", 32, 96, 3, 1), Conv("bf16", "ff", 96, 96, 3, 1, ldo_extra=4),
    Conv("bf16", "ff", 32, 64, 3, 1, ldo_extra=2), Conv("bf16", "ff", 64, 96, 3, 1, ldo_extra=1), Conv("bf16", "bf", 32, 65, 3, 1),
    Conv("bf16", "bb", 96, 64, 3, 1, ldo_extra=4), Conv("bf16", "fb", 64, 96, 3, 1, ldo_extra=1), Conv("bf16", "bb", 32, 72, 3, 1),
    Conv("bf16", "bb", 64, 128, 3, 1, ldo_extra=8),
    # 3x3 stride 1 with in_stats (B): fp32 and bf16 tensors (the packed-arithmetic path)
    Conv("bf16", "ff", 32, 64, 3, 1, norm=True), Conv("bf16", "bb", 64, 64, 3, 1, norm=True), Conv("bf16", "bb", 96, 96, 3, 1, norm=True),
    Conv("bf16", "fb", 64, 72, 3, 1, norm=True, ldo_extra=1), Conv("bf16", "bf", 32, 96, 3, 1, norm=True),
    Conv("bf16", "bb", 32, 256, 3, 1, norm=True),
    # 3x3 stride 2
    Conv("bf16", "bb", 64, 96, 3, 2), Conv("bf16", "ff", 32, 64, 3, 2), Conv("bf16", "fb", 96, 66, 3, 2), Conv("bf16", "bf", 32, 31, 3, 2),
    # the 7x7 stem: Cout <= 32 and 64
    Conv("bf16", "ff", 4, 32, 7, 2), Conv("bf16", "fb", 4, 24, 7, 2), Conv("bf16", "fb", 4, 64, 7, 2), Conv("bf16", "fb", 4, 64, 7, 2, ldo_extra=2),
    Conv("bf16", "ff", 4, 31, 7, 2),
    # the 256-channel big tile and the row tiles it replaces
    Conv("bf16", "bb", 32, 256, 3, 1), Conv("bf16", "bb", 32, 256, 3, 1, big=False), Conv("bf16", "bb", 416, 256, 3, 1),
    Conv("bf16", "bb", 416, 256, 3, 1, big=False),
    # bf16x3: the halo kernel (any size), the im2col kernels (Ho * Wo % 256 == 0)
    Conv("bf16x3", "ff", 32, 64, 3, 1), Conv("bf16x3", "ff", 64, 96, 3, 1, ldo_extra=3), Conv("bf16x3", "ff", 96, 72, 3, 1, norm=True),
    Conv("bf16x3", "ff", 32, 64, 1, 1), Conv("bf16x3", "ff", 64, 96, 3, 2, ldo_extra=1), Conv("bf16x3", "ff", 96, 33, 1, 2),
    Conv("bf16x3", "ff", 4, 64, 7, 2),
]
DOWN_CASES = [(32, 64, 8), (64, 96, 0), (96, 64, 0), (32, 160, 8)]  # (Cin, Cout, ldo - Cout): 64- and 96-channel tiles


def conv_id(c):
    return (f"{c.prec}-{c.io}-cin{c.Cin}-cout{c.Cout}-k{c.k}s{c.s}" + (f"-ldo{c.ldo_extra}" if c.ldo_extra else "") +
            ("-norm" if c.norm else "") + ("" if c.big else "-nobig"))


def test_cases_reach_every_form():
    """The parametrised cases reach every kernel form and every epilogue form the issue names, each with partials."""
    kernels = {conv_variant(c)[:3] if conv_variant(c)[0] == "rows" else conv_variant(c)[:2] for c in CONV_CASES}
    for want in [("rows", 1, 1), ("rows", 1, 2), ("rows", 3, 1), ("rows", 3, 2), ("stem", 1), ("stem", 2), ("big",), ("halo",), ("im2col",)]:
        assert want in kernels, want
    assert any(c.norm and conv_variant(c)[0] == "rows" and c.io[0] == "f" for c in CONV_CASES)
    assert any(c.norm and conv_variant(c)[0] == "rows" and c.io[0] == "b" for c in CONV_CASES)
    assert any(c.norm and conv_variant(c)[0] == "halo" for c in CONV_CASES)
    # the row tiles that the big tile replaces: the same case with MVT_CONV_BIG=0
    for c in CONV_CASES:
        if conv_variant(c)[0] == "big":
            assert c._replace(big=False) in CONV_CASES and conv_variant(c._replace(big=False))[0] == "rows"
    assert {c.Cin for c in CONV_CASES if conv_variant(c)[0] == "rows"} >= {32, 64, 96, 416}
    assert any(c.Cin == 416 and conv_variant(c)[0] == "big" for c in CONV_CASES)
    forms = collections.defaultdict(list)
    for c in CONV_CASES:
        forms[epilogue_form(c)].append(c)
    assert set(forms) >= {"staged-tr", "staged-px", "quad", "pair", "scalar"}
    ldo = lambda c: c.Cout + c.ldo_extra
    assert any(c.Cout % 4 == 2 for c in forms["pair"]) and any(ldo(c) % 4 == 2 and c.Cout % 4 == 0 for c in forms["pair"])
    assert any(c.Cout % 2 == 1 for c in forms["scalar"]) and any(ldo(c) % 2 == 1 and c.Cout % 2 == 0 for c in forms["scalar"])
    assert all(c.io[1] == "f" for c in forms["quad"]) and any(c.Cin == 4 for c in forms["quad"]) and any(c.Cin != 4 for c in forms["quad"])
    for f in ("pair", "scalar"):  # a non-staged bf16 output (ldo % 8 != 0), in both forms
        assert any(c.io[1] == "b" and ldo(c) % 8 != 0 for c in forms[f]), f
    assert any(c.Cout == 72 for c in forms["staged-tr"]) and any(c.Cout == 72 for c in forms["pair"] + forms["scalar"])  # partial last block
    assert {c.io[0] for c in CONV_CASES} == {"f", "b"}
    assert {down_tile(co) for _, co, _ in DOWN_CASES} == {2, 3}
    # the sizes sit on both sides of every tile edge
    for outs, tr in ((OUT_S1, 8), (OUT_S2, 4)):
        assert any(h < tr and w < 32 for h, w in outs) and (tr, 32) in outs and (tr + 1, 33) in outs
        assert any(h % tr not in (0, 1) and w % 32 not in (0, 1) and h > tr and w > 32 for h, w in outs)


def down_tile(Cout):
    return 3 if (Cout % 64 != 0 and Cout % 96 == 0) else 2


# ================================================================== A / B: operands and references (CPU)

def conv_ref(z, w, b, k, s):
    """fp64 F.conv2d with zero padding, NHWC in and out."""
    return F.conv2d(z.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), b.double(), stride=s, padding=k // 2).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def conv_data(Cin, Cout, k, s, norm, H, W, seed=0):
    """x [n][H][W][cin] (integers; mean + step * d with planted statistics for `norm`), w [Cout][k][k][cin] in {-1, 0, 1} at density
    min(1, 300 / K), b in [-3, 3], z = what the convolution multiplies, Y = its fp64 result."""
    g = gen("conv", Cin, Cout, k, s, norm, H, W, seed)
    n, cin = N_IMG, (3 if Cin == 4 else Cin)
    K = k * k * cin
    if norm:
        mean, rstd, step = planted_stats(g, n, cin)
        x = planted_tensor(g, mean, rstd, step, H, W)
        z = normalise(x, mean, rstd)
    else:
        mean = rstd = None
        x = rint(g, -2, 2, n, H, W, cin) + torch.arange(n).double().view(n, 1, 1, 1)  # (image i is shifted by i: distinct sums)
        z = x
    w = rint(g, 0, 1, Cout, k, k, cin) * 2 - 1
    w = w * (torch.rand(Cout, k, k, cin, generator=g) < min(1.0, 300.0 / K)).double()
    b = rint(g, -3, 3, Cout)
    return dict(x=x, w=w, b=b, mean=mean, rstd=rstd, z=z, Y=conv_ref(z, w, b, k, s))


def case_data(c, H, W, seed=0):
    return conv_data(c.Cin, c.Cout, c.k, c.s, c.norm, H, W, seed)


def exact_sums(Y):
    """(sum Y, sum Y^2) [n][C] in fp64: integers below 2^53."""
    n, C = Y.shape[0], Y.shape[-1]
    y = Y.reshape(n, -1, C)
    return y.sum(1), (y * y).sum(1)


@pytest.mark.parametrize("c", CONV_CASES, ids=conv_id)
def test_reference_stays_inside(c):
    """|Y| <= 180 on every reference of A: fp32 slot sums of up to 512 pixels are then exact in any order; and integers."""
    for (H, W) in conv_geos(c):
        Y = case_data(c, H, W)["Y"]
        assert float(Y.abs().max()) <= YMAX and torch.equal(Y, Y.round())
        assert 512 * YMAX ** 2 < 2 ** 24


def check_partials(part, Y, what):
    """part [n][slots][C][2] (fp32 from the device): finite, and summed over the slots in fp64 exactly the reference's sums."""
    assert bool(torch.isfinite(part).all()), f"{what}: a partial was not written"
    S, SS = exact_sums(Y)
    got = part.double().sum(1)
    assert_equal(got[..., 0], S, what + " sum y")
    assert_equal(got[..., 1], SS, what + " sum y^2")


# ================================================================== A / B on the device

def weights_bf16(hip, w):
    """[N][K] integers -> (bf16 hi, bf16 lo) zero padded to a multiple of 64 columns, on the device."""
    N, K = w.shape
    wp = torch.zeros(N, cdiv(K, 64) * 64)
    wp[:, :K] = w.float()
    wp = wp.to(DEV)
    hi, lo = torch.empty(wp.shape, device=DEV, dtype=torch.int16), torch.empty(wp.shape, device=DEV, dtype=torch.int16)
    hip.split_bf16(wp, hi, lo, wp.numel())
    return hi, lo


def run_conv(hip, c, H, W, x, w, b, in_stats, want_partial=True):
    """-> (out [n][Ho][Wo][Cout] fp64, partials [n][slots][Cout][2] fp32, mean_rstd [n][Cout][2] fp32), all on the CPU."""
    n = N_IMG
    stem = c.Cin == 4
    Ho, Wo = conv_out(H, W, c.k, c.s)
    if stem:  # [n][H][W][4] fp32 input, weight row = [kh][8][4] with kw < 7, c < 3
        x4 = torch.zeros(n, H, W, 4, dtype=torch.float64)
        x4[..., :3] = x
        wt = torch.zeros(c.Cout, 7, 8, 4, dtype=torch.float64)
        wt[:, :, :7, :3] = w
        x, w = x4, wt
    xd = guarded(x, dt(c.io[0]))
    hi, lo = weights_bf16(hip, w.reshape(c.Cout, -1))
    ldo, M = c.Cout + c.ldo_extra, n * Ho * Wo
    out = poisoned(M * ldo, dt(c.io[1]))
    slots = hip.conv2d_stat_slots(H, W, c.Cin, c.k, c.k, c.s, c.k // 2, split=c.prec == "bf16x3")
    assert slots == stat_slots(c, H, W) and slots > 0, (slots, stat_slots(c, H, W))
    part = poisoned(n * slots * c.Cout * 2) if want_partial else None
    st = stats_tensor(*in_stats).to(DEV) if in_stats is not None else None
    hip.conv2d_bf16(xd, hi, lo if c.prec == "bf16x3" else None, b.float().to(DEV), out, n, H, W, c.Cin, c.Cout, c.k, c.k, c.s, c.k // 2, ldo,
                    in_stats=st, out_partial=part)
    what = f"{conv_id(c)} {H}x{W} -> {conv_variant(c)} {epilogue_form(c)}"
    o = taken(out, M, c.Cout, ldo, what).reshape(n, Ho, Wo, c.Cout)
    if not want_partial:
        return o, None, None
    mr = poisoned(n * c.Cout * 2)
    hip.instnorm_finish_slots(part, slots, mr, n, Ho * Wo, c.Cout)
    p = taken(part, n * slots, c.Cout * 2, c.Cout * 2, what + " partials").float().reshape(n, slots, c.Cout, 2)
    m = taken(mr, n, c.Cout * 2, c.Cout * 2, what + " mean_rstd").float().reshape(n, c.Cout, 2)
    return o, p, m


@gpu
@pytest.mark.parametrize("c", CONV_CASES, ids=conv_id)
def test_conv_statistics_exact(hip, c, monkeypatch):
    """A (and the first half of B for the `norm` cases): output, partials summed over slots, finished statistics."""
    monkeypatch.setenv("MVT_CONV_BIG", "1" if c.big else "0")
    for (H, W) in conv_geos(c):
        d = case_data(c, H, W)
        Y = d["Y"]
        assert float(Y.abs().max()) <= YMAX
        out, part, mr = run_conv(hip, c, H, W, d["x"], d["w"], d["b"], (d["mean"], d["rstd"]) if c.norm else None)
        what = f"{conv_id(c)} {H}x{W}"
        assert_equal(out, Y.to(dt(c.io[1])), what + " output")
        check_partials(part, Y, what)
        S, SS = exact_sums(Y)
        check_mean_rstd(mr, S, SS, Y.shape[1] * Y.shape[2], what)
    print(f"rstd: at most {REACHED['rstd ulps']:.3f} of the one-ulp bar so far")


@gpu
def test_im2col_refuses_partials_it_cannot_slot(hip):
    """bf16x3 outside the halo kernel: Ho * Wo % 256 != 0 has no slot layout; the entry must refuse, not write."""
    c = Conv("bf16x3", "ff", 32, 64, 1, 1)
    assert hip.conv2d_stat_slots(9, 33, 32, 1, 1, 1, 0, split=True) == 0 == stat_slots(c, 9, 33)
    d = case_data(c, 9, 33)
    hi, lo = weights_bf16(hip, d["w"].reshape(64, -1))
    out, part = poisoned(N_IMG * 9 * 33 * 64), poisoned(4096)
    with pytest.raises(hip.HipError):
        hip.conv2d_bf16(guarded(d["x"], torch.float32), hi, lo, d["b"].float().to(DEV), out, N_IMG, 9, 33, 32, 64, 1, 1, 1, 0, 64, out_partial=part)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(part).all())


@gpu
def test_wide_stem_shape_refuses_partials(hip):
    """The stem shape with more than 64 output channels runs the im2col GEMM kernel, whose slots are 32-pixel blocks, while
    mvt_conv2d_stat_slots answers the stem's 8 x 32 tiles (conv_plan.h plan_conv: statistics only where the family that runs writes
    the slots the caller sized by): with out_partial the entry must refuse, not write; without, the call runs."""
    n, H, W, Cout = N_IMG, 16, 64, 96
    assert hip.conv2d_stat_slots(H, W, 4, 7, 7, 2, 3) == 1 and (H // 2) * (W // 2) // 32 == 8
    g = gen("wide-stem")
    x4 = torch.zeros(n, H, W, 4, dtype=torch.float64)
    x4[..., :3] = rint(g, -2, 2, n, H, W, 3)
    wt = torch.zeros(Cout, 7, 8, 4, dtype=torch.float64)
    wt[:, :, :7, :3] = rint(g, -1, 1, Cout, 7, 7, 3)
    hi, _ = weights_bf16(hip, wt.reshape(Cout, -1))
    b = torch.zeros(Cout, device=DEV)
    M = n * (H // 2) * (W // 2)
    out, part = poisoned(M * Cout), poisoned(n * 1 * Cout * 2)
    with pytest.raises(hip.HipError):
        hip.conv2d_bf16(guarded(x4, torch.float32), hi, None, b, out, n, H, W, 4, Cout, 7, 7, 2, 3, Cout, out_partial=part)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(part).all())
    hip.conv2d_bf16(guarded(x4, torch.float32), hi, None, b, out, n, H, W, 4, Cout, 7, 7, 2, 3, Cout)
    want = conv_ref(x4[..., :3], wt[:, :, :7, :3], torch.zeros(Cout, dtype=torch.float64), 7, 2)
    assert_equal(taken(out, M, Cout, Cout, "wide stem shape").reshape(n, H // 2, W // 2, Cout), want, "wide stem shape without statistics")


@gpu
@pytest.mark.parametrize("Cin,Cout,ldo_extra", DOWN_CASES)
def test_down_statistics_exact(hip, Cin, Cout, ldo_extra):
    """mvt_conv3x3s2_down_bf16 with part3 / partd: both outputs, both partials, both finished statistics."""
    n, ldo = N_IMG, Cout + ldo_extra
    for i, (ho, wo) in enumerate(OUT_S2):
        H, W = in_size(ho, wo, 2, i)
        d3, dd = conv_data(Cin, Cout, 3, 2, False, H, W), conv_data(Cin, Cout, 1, 2, False, H, W, seed=1)
        x = d3["x"]
        Y3, Yd = d3["Y"], conv_ref(x, dd["w"], dd["b"], 1, 2)
        assert float(Y3.abs().max()) <= YMAX and float(Yd.abs().max()) <= YMAX and Y3.shape == Yd.shape == (n, ho, wo, Cout)
        h3, _ = weights_bf16(hip, d3["w"].reshape(Cout, -1))
        hd, _ = weights_bf16(hip, dd["w"].reshape(Cout, -1))
        M = n * ho * wo
        o3, od = poisoned(M * ldo, torch.bfloat16), poisoned(M * ldo, torch.bfloat16)
        slots = hip.conv2d_stat_slots(H, W, Cin, 3, 3, 2, 1)
        assert slots == cdiv(ho, 4) * cdiv(wo, 32)
        p3, pd = poisoned(n * slots * Cout * 2), poisoned(n * slots * Cout * 2)
        hip.conv3x3s2_down_bf16(guarded(x, torch.bfloat16), h3, d3["b"].float().to(DEV), hd, dd["b"].float().to(DEV), o3, od, n, H, W, Cin, Cout,
                                ldo, part3=p3, partd=pd)
        for name, o, p, Y in (("3x3", o3, p3, Y3), ("1x1", od, pd, Yd)):
            what = f"down cin={Cin} cout={Cout} {H}x{W} ({name})"
            assert_equal(taken(o, M, Cout, ldo, what).reshape(Y.shape), Y, what + " output")
            mr = poisoned(n * Cout * 2)
            hip.instnorm_finish_slots(p, slots, mr, n, ho * wo, Cout)
            check_partials(taken(p, n * slots, Cout * 2, Cout * 2, what).float().reshape(n, slots, Cout, 2), Y, what)
            check_mean_rstd(taken(mr, n, Cout * 2, Cout * 2, what).float().reshape(n, Cout, 2), *exact_sums(Y), ho * wo, what)


NORM_CASES = [c for c in CONV_CASES if c.norm]


def normalised_padding_ref(d, k=3):
    """The fault of B: the zero padding goes through relu((0 - mean) * rstd) as well."""
    xp = F.pad(d["x"], (0, 0, 1, 1, 1, 1))
    zp = normalise(xp, d["mean"], d["rstd"])
    return F.conv2d(zp.permute(0, 3, 1, 2), d["w"].permute(0, 3, 1, 2), d["b"], stride=1, padding=0).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("c", NORM_CASES, ids=conv_id)
def test_normalised_padding_differs(c):
    """Probe: a kernel that normalised its zero padding fails the output AND the statistics assertion of every B case and size
    (negative means in every channel piece make relu((0 - mean) * rstd) > 0), and only at the border pixels."""
    for (H, W) in conv_geos(c):
        d = case_data(c, H, W)
        bad = normalised_padding_ref(d)
        assert breaks(assert_equal, bad, d["Y"])
        assert torch.equal(bad[:, 1:-1, 1:-1], d["Y"][:, 1:-1, 1:-1])
        S, SS = exact_sums(bad)
        part = torch.stack([S, SS], -1)[:, None].float()
        assert breaks(check_partials, part, d["Y"])


@gpu
@pytest.mark.parametrize("c", NORM_CASES, ids=conv_id)
def test_normalise_on_load_equals_two_steps(hip, c):
    """B: the convolution with in_stats gives the bits of instnorm_apply followed by the plain convolution (and both the reference)."""
    n = N_IMG
    for (H, W) in conv_geos(c):
        d = case_data(c, H, W)
        fused, pf, _ = run_conv(hip, c, H, W, d["x"], d["w"], d["b"], (d["mean"], d["rstd"]))
        xd = guarded(d["x"], dt(c.io[0]))
        yd = poisoned(n * H * W * c.Cin, dt(c.io[0]))
        hip.instnorm_apply(xd, stats_tensor(d["mean"], d["rstd"]).to(DEV), None, None, yd, n, H * W, c.Cin)
        z = taken(yd, n * H * W, c.Cin, c.Cin, "apply").reshape(n, H, W, c.Cin)
        assert_equal(z, d["z"], f"{conv_id(c)} {H}x{W} instnorm_apply")
        two, pt, _ = run_conv(hip, c._replace(norm=False, big=True), H, W, z, d["w"], d["b"], None)
        assert_equal(fused, two, f"{conv_id(c)} {H}x{W} fused against two steps")
        assert_equal(fused, d["Y"].to(dt(c.io[1])), f"{conv_id(c)} {H}x{W} against the reference")
        assert_equal(pf.double().sum(1), pt.double().sum(1), f"{conv_id(c)} {H}x{W} statistics, fused against two steps")


# ================================================================== C: instnorm_stats / finish_slots / apply

IN_SLABS = 64  # MVT_IN_SLABS
STATS_HW = (1, 5, 63, 64, 65, 999)
STATS_C = (4, 8, 32, 96, 128, 256)


@functools.lru_cache(maxsize=None)
def stats_data(HW, C):
    """x [n][HW][C]: integers, |x| <= 11, a different offset per (image, channel)."""
    g = gen("stats", HW, C)
    return rint(g, -8, 8, 2, 1, C) + rint(g, -3, 3, 2, HW, C)


@gpu
@pytest.mark.parametrize("ld_extra", [0, 4], ids=["ldx=C", "ldx>C"])
@pytest.mark.parametrize("io", ["f", "b"])
def test_instnorm_stats_exact(hip, io, ld_extra):
    for HW in STATS_HW:
        for C in STATS_C:
            x = stats_data(HW, C)
            n, ldx = x.shape[0], C + ld_extra
            xd = guarded(x.reshape(n * HW, C), dt(io), ld=ldx)
            ws = torch.full((n * IN_SLABS * C * 2 + 16,), NAN, dtype=torch.float64, device=DEV)
            mr = poisoned(n * C * 2)
            hip.instnorm_stats(xd, ldx, ws, mr, n, HW, C)
            what = f"instnorm_stats {io} HW={HW} C={C} ldx={ldx}"
            got = taken(mr, n, C * 2, C * 2, what).float().reshape(n, C, 2)
            assert bool(torch.isnan(ws[n * IN_SLABS * C * 2:]).all()) and bool(torch.isfinite(ws[:n * IN_SLABS * C * 2]).all()), what
            check_mean_rstd(got, x.sum(1), (x * x).sum(1), HW, what)


FINISH_SLOTS = (1, 2, 127, 128, 129, 1000)
FINISH_C = (4, 12, 64, 96, 100)


@functools.lru_cache(maxsize=None)
def finish_data(slots, C, n=3):
    """Planted integer partials [n][slots][C][2] of 32-pixel slots: |s| <= 64, ss >= s^2 / 32 + 32 (so the variance is >= 1)."""
    g = gen("finish", slots, C)
    s = rint(g, -40, 40, n, slots, C) + 8.0 * (torch.arange(n).double().view(n, 1, 1) - 1)
    ss = torch.floor(s * s / 32) + 32 + rint(g, 0, 1000, n, slots, C)
    return torch.stack([s, ss], -1)


@gpu
def test_instnorm_finish_slots_exact(hip):
    for slots in FINISH_SLOTS:
        for C in FINISH_C:
            p = finish_data(slots, C)
            n, HW = p.shape[0], 32 * slots
            mr = poisoned(n * C * 2)
            hip.instnorm_finish_slots(guarded(p, torch.float32), slots, mr, n, HW, C)
            what = f"finish_slots slots={slots} C={C}"
            check_mean_rstd(taken(mr, n, C * 2, C * 2, what).float().reshape(n, C, 2), p[..., 0].sum(1), p[..., 1].sum(1), HW, what)


APPLY_HW = (1, 3, 21, 22, 85, 960)
APPLY_PATHS = [("f", (4, 12, 96)), ("b", (8, 64, 96, 256, 416)), ("b", (12,))]  # generic fp32; 16-byte bf16; generic bf16
APPLY_FORMS = ["plain", "skip", "skip-stats", "skip-stats-relu"]


@functools.lru_cache(maxsize=None)
def apply_data(HW, C, n=3):
    g = gen("apply", HW, C)
    m, r, st = planted_stats(g, n, C)
    km, kr, kst = planted_stats(g, n, C)
    return dict(m=m, r=r, km=km, kr=kr, x=planted_tensor(g, m, r, st, HW), kraw=rint(g, -4, 4, n, HW, C), kx=planted_tensor(g, km, kr, kst, HW))


def apply_ref(d, form, fault=None):
    """relu((x - m) r) [+ skip' then relu]; skip' = skip | (skip - km) kr | relu of that.  fp64; faults for the probes."""
    m, r, km, kr = d["m"], d["r"], d["km"], d["kr"]
    if fault == "image0":  # every image normalised with image 0's statistics
        m, r, km, kr = (t[:1].expand_as(t) for t in (m, r, km, kr))
    if fault == "octet":   # the statistics of the next channel octet
        m, r, km, kr = (torch.roll(t, -8, dims=1) for t in (m, r, km, kr))
    o = normalise(d["x"], m, r)
    if form == "plain":
        return o
    if form == "skip":
        return F.relu(d["kraw"] + o)
    relu = (form == "skip-stats-relu") != (fault == "flip_skip_relu")
    return F.relu(normalise(d["kx"], km, kr, relu=relu) + o)


@gpu
@pytest.mark.parametrize("form", APPLY_FORMS)
@pytest.mark.parametrize("path", range(len(APPLY_PATHS)), ids=["fp32", "bf16-16B", "bf16-generic"])
def test_instnorm_apply_exact(hip, path, form):
    io, Cs = APPLY_PATHS[path]
    for C in Cs:
        for HW in APPLY_HW:
            d = apply_data(HW, C)
            n = d["x"].shape[0]
            want = apply_ref(d, form)
            assert float(want.abs().max()) <= 8 and torch.equal(want, want.round())
            skip = None if form == "plain" else guarded(d["kraw"] if form == "skip" else d["kx"], dt(io))
            kst = stats_tensor(d["km"], d["kr"]).to(DEV) if form.startswith("skip-stats") else None
            y = poisoned(n * HW * C, dt(io))
            hip.instnorm_apply(guarded(d["x"], dt(io)), stats_tensor(d["m"], d["r"]).to(DEV), skip, kst, y, n, HW, C, skip_relu=form == "skip-stats-relu")
            what = f"instnorm_apply {io} {form} C={C} HW={HW}"
            assert_equal(taken(y, n * HW, C, C, what).reshape(want.shape), want.to(dt(io)), what)


# ================================================================== D: resize, concat, repack

NEAREST = [((5, 7), (10, 14)), ((10, 14), (5, 7)), ((7, 5), (3, 11)), ((1, 1), (4, 3)), ((6, 9), (1, 1)), ((3, 1), (1, 5)), ((13, 17), (29, 23))]


@gpu
def test_resize_nearest_exact(hip):
    for (Hi, Wi), (Ho, Wo) in NEAREST:
        planes = 5
        x = rint(gen("nearest", Hi, Wi, Ho, Wo), -99, 99, planes, Hi, Wi).float()
        out = poisoned(planes * Ho * Wo)
        hip.resize_nearest(guarded(x, torch.float32), out, planes, Hi, Wi, Ho, Wo)
        what = f"nearest {Hi}x{Wi} -> {Ho}x{Wo}"
        want = F.interpolate(x[None], size=(Ho, Wo), mode="nearest")[0]
        assert_equal(taken(out, planes * Ho, Wo, Wo, what).reshape(planes, Ho, Wo), want, what)


def bilinear_ref(src, Hd, Wd, unclamped=False):
    """fp64 align_corners=True bilinear resize of src [n][Hs][Ws][C], the kernel's formula; `unclamped`: the +1 taps are read
    past the last row / column of a FLAT buffer with a NaN guard behind the last image, as the device would."""
    n, Hs, Ws, C = src.shape
    flat = torch.cat([src.double().reshape(-1), torch.full((Ws * C + C,), NAN, dtype=torch.float64)])
    rh = (Hs - 1) / (Hd - 1) if Hd > 1 else 0.0
    rw = (Ws - 1) / (Wd - 1) if Wd > 1 else 0.0
    fy, fx = torch.arange(Hd).double() * rh, torch.arange(Wd).double() * rw
    y0, x0 = fy.floor().long(), fx.floor().long()
    yp = torch.ones_like(y0) if unclamped else (y0 < Hs - 1).long()
    xp = torch.ones_like(x0) if unclamped else (x0 < Ws - 1).long()
    ly, lx = (fy - y0).view(1, Hd, 1, 1), (fx - x0).view(1, 1, Wd, 1)
    img = torch.arange(n).view(n, 1, 1, 1)
    ch = torch.arange(C).view(1, 1, 1, C)
    at = lambda yy, xx: flat[((img * Hs + yy.view(1, Hd, 1, 1)) * Ws + xx.view(1, 1, Wd, 1)) * C + ch]
    return (1 - ly) * ((1 - lx) * at(y0, x0) + lx * at(y0, x0 + xp)) + ly * ((1 - lx) * at(y0 + yp, x0) + lx * at(y0 + yp, x0 + xp))


# dyadic ratios (Hs-1)/(Hd-1): 5->9, 9->5, 4->13, equal; and sizes of 1 on either side, in either direction
BILINEAR = [((5, 4), (9, 13)), ((9, 5), (5, 9)), ((4, 9), (13, 5)), ((6, 7), (6, 7)), ((5, 4), (1, 13)), ((5, 4), (9, 1)), ((1, 4), (9, 13)),
            ((5, 1), (9, 13)), ((1, 1), (3, 3)), ((5, 9), (1, 1)), ((2, 2), (9, 9))]


@functools.lru_cache(maxsize=None)
def bilinear_src(n, Hs, Ws, C, tag=0):
    return 64.0 * rint(gen("bilinear", n, Hs, Ws, C, tag), -3, 3, n, Hs, Ws, C)


def run_bilinear(hip, src, Hd, Wd, io, ldd, c_off, dst=None):
    n, Hs, Ws, C = src.shape
    dst = poisoned(n * Hd * Wd * ldd, dt(io)) if dst is None else dst
    hip.resize_bilinear_ac(guarded(src, dt(io), guard=Ws * C + C), dst, n, Hs, Ws, C, Hd, Wd, ldd, c_off)
    return dst


def slice_taken(dst, rows, c_off, C, ldd, what):
    torch.cuda.synchronize()
    b = dst.double().cpu()
    body = b[:rows * ldd].view(rows, ldd)
    assert bool(torch.isnan(body[:, :c_off]).all()) and bool(torch.isnan(body[:, c_off + C:]).all()) and bool(torch.isnan(b[rows * ldd:]).all()), f"{what}: wrote outside its slice"
    return body[:, c_off:c_off + C].clone()


@gpu
@pytest.mark.parametrize("io", ["f", "b"])
def test_resize_bilinear_exact(hip, io):
    for i, ((Hs, Ws), (Hd, Wd)) in enumerate(BILINEAR):
        n, C = 2, (12, 8, 32)[i % 3]
        c_off, ldd = ((0, C), (4, C + 12), (8, C + 8))[i % 3]
        src = bilinear_src(n, Hs, Ws, C)
        want = bilinear_ref(src, Hd, Wd)
        assert torch.equal(want, want.round()) and float(want.abs().max()) <= 192
        what = f"bilinear {io} {Hs}x{Ws} -> {Hd}x{Wd} C={C} c_off={c_off} ldd={ldd}"
        got = slice_taken(run_bilinear(hip, src, Hd, Wd, io, ldd, c_off), n * Hd * Wd, c_off, C, ldd, what)
        assert_equal(got.reshape(want.shape), want, what)


@gpu
def test_resize_bilinear_non_dyadic_within_derived_bar(hip):
    """37x53 -> 64x96 against fp64 F.interpolate(align_corners=True); the bar is derived in the module docstring."""
    n, Hs, Ws, C, Hd, Wd = 2, 37, 53, 8, 64, 96
    src = rint(gen("nondyadic"), -7, 7, n, Hs, Ws, C)
    want = F.interpolate(src.permute(0, 3, 1, 2), size=(Hd, Wd), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    bar = (2.0 ** -22 * max(Hs, Ws) + 8 * 2.0 ** -24) * float(src.abs().max())
    got = slice_taken(run_bilinear(hip, src, Hd, Wd, "f", C + 4, 0), n * Hd * Wd, 0, C, C + 4, "non-dyadic").reshape(want.shape)
    err = float((got - want).abs().max())
    print(f"non-dyadic bilinear: max error {err:.3e}, {err / bar:.3f} of the bar {bar:.3e}")
    assert err <= bar


# (dims per source (Hs, Ws, C)), destination size; all ratios dyadic.  fp32 needs C % 4, bf16 C % 8
CONCAT = [("fb", [(9, 9, 64), (5, 5, 96), (3, 3, 128), (2, 2, 128)], (9, 9)),     # the encoder's own 64 + 96 + 128 + 128
          ("f", [(5, 4, 4), (3, 7, 12)], (9, 13)),                                 # small fp32: 4 + 12
          ("b", [(5, 4, 8), (3, 7, 16)], (9, 13)),
          ("fb", [(4, 9, 32), (1, 1, 8), (7, 3, 24)], (13, 5)),
          ("fb", [(5, 9, 64)], (9, 5)),
          ("fb", [(2, 3, 8), (1, 5, 8), (3, 1, 8), (5, 9, 8)], (1, 1))]


@gpu
@pytest.mark.parametrize("case", range(len(CONCAT)))
def test_concat_resize_exact(hip, case):
    ios, dims, (Hd, Wd) = CONCAT[case]
    n, ctot = 2, sum(d[2] for d in dims)
    ldd = ctot + 8
    for io in ios:
        srcs = [bilinear_src(n, hs, ws, c, tag=k) for k, (hs, ws, c) in enumerate(dims)]
        want = torch.cat([bilinear_ref(s, Hd, Wd) for s in srcs], dim=-1)
        assert torch.equal(want, want.round()) and float(want.abs().max()) <= 192
        dst = poisoned(n * Hd * Wd * ldd, dt(io))
        hip.concat_resize_bilinear_ac([guarded(s, dt(io), guard=s.shape[2] * s.shape[3] + s.shape[3]) for s in srcs], dims, dst, n, Hd, Wd, ldd)
        what = f"concat {io} {dims} -> {Hd}x{Wd}"
        got = taken(dst, n * Hd * Wd, ctot, ldd, what)
        assert_equal(got.reshape(want.shape), want, what)
        sep = poisoned(n * Hd * Wd * ldd, dt(io))
        c0 = 0
        for s in srcs:  # the same through separate launches into channel slices: bit-identical
            run_bilinear(hip, s, Hd, Wd, io, ldd, c0, dst=sep)
            c0 += s.shape[3]
        assert_equal(taken(sep, n * Hd * Wd, ctot, ldd, what + " (separate)"), got, what + " against separate launches")


@functools.lru_cache(maxsize=None)
def rgb_clip():
    """(V, T, 3, H, W) uint8 with every byte value present."""
    V, T, H, W = 3, 4, 5, 11
    vals = (torch.arange(V * T * 3 * H * W) % 256)[torch.randperm(V * T * 3 * H * W, generator=gen("rgb"))]
    assert set(vals.tolist()) == set(range(256))
    return vals.to(torch.uint8).reshape(V, T, 3, H, W)


def repack_ref(u8, imgs):
    """[len(imgs)][H][W][4] fp32: 2 (x / 255) - 1 in fp32, channel 3 zero; image i = frame i // V, view i % V."""
    V = u8.shape[0]
    out = torch.zeros(len(imgs), u8.shape[3], u8.shape[4], 4)
    for j, i in enumerate(imgs):
        out[j, ..., :3] = (2.0 * (u8[i % V, i // V].float() / 255.0) - 1.0).permute(1, 2, 0)
    return out


@gpu
def test_rgb_repack_exact(hip):
    u8 = rgb_clip()
    V, T, _, H, W = u8.shape
    for dtype in (torch.uint8, torch.float32):
        clip = guarded(u8, dtype, fill=255 if dtype == torch.uint8 else NAN)
        for t0, nt in ((1, T - 1), (2, 2), (0, T)):
            out = poisoned(nt * V * H * W * 4)
            hip.rgb_to_nhwc4(clip[:u8.numel()].view(u8.shape), out, V, T, H, W, t0, nt)
            what = f"rgb_to_nhwc4 {dtype} t0={t0} nt={nt}"
            assert_equal(taken(out, nt * V * H * W, 4, 4, what).reshape(nt * V, H, W, 4), repack_ref(u8, range(t0 * V, (t0 + nt) * V)), what)
        for img0, nimg in ((1, 4), (2, V * T - 2), (5, 1), (0, V * T)):  # ranges that start and end inside a frame
            out = poisoned(nimg * H * W * 4)
            hip.rgb_images_to_nhwc4(clip[:u8.numel()].view(u8.shape), out, V, T, H, W, img0, nimg)
            what = f"rgb_images_to_nhwc4 {dtype} img0={img0} nimg={nimg}"
            assert_equal(taken(out, nimg * H * W, 4, 4, what).reshape(nimg, H, W, 4), repack_ref(u8, range(img0, img0 + nimg)), what)


# ================================================================== E: probes (CPU)

def slot_partials(z, w, b, k, s, trows, count_cols=False, count_rows=False):
    """The row-tile kernels' statistics rule restated: the image is cut into trows x 32 output tiles, a tile's accumulators cover the
    whole tile (taps outside the image read zeros), and only pixels inside Ho x Wo are counted.  -> [n][slots][C][2] fp32.
    count_cols / count_rows: the faults -- pixels of a ragged tile beyond Wo / Ho are counted too."""
    n, H, W, _ = z.shape
    Ho, Wo = conv_out(H, W, k, s)
    ty, tx = cdiv(Ho, trows), cdiv(Wo, 32)
    He, We = s * (ty * trows - 1) + k - 2 * (k // 2), s * (tx * 32 - 1) + k - 2 * (k // 2)  # input extent that covers whole tiles
    ze = F.pad(z.double(), (0, 0, 0, max(0, We - W), 0, max(0, He - H)))
    Ye = conv_ref(ze, w, b, k, s)[:, :ty * trows, :tx * 32]
    valid = torch.zeros(ty * trows, tx * 32, dtype=torch.bool)
    valid[:ty * trows if count_rows else Ho, :tx * 32 if count_cols else Wo] = True
    Ym = Ye * valid[None, :, :, None]
    C = Ym.shape[-1]
    t = Ym.reshape(n, ty, trows, tx, 32, C)
    return torch.stack([t.sum((2, 4)), (t * t).sum((2, 4))], -1).reshape(n, ty * tx, C, 2).float()


PROBE_CONV = [c for c in CONV_CASES if conv_variant(c)[0] in ("rows", "stem", "big") and c.Cin <= 96]


@pytest.mark.parametrize("c", PROBE_CONV, ids=conv_id)
def test_probe_ragged_tile_statistics(c):
    """The restated rule passes the partials assertion on every size; counting the columns beyond Wo or the rows beyond Ho of a
    ragged tile breaks it on every size that has such a tile."""
    for (H, W) in conv_geos(c):
        d = case_data(c, H, W)
        Ho, Wo = conv_out(H, W, c.k, c.s)
        args = (d["z"], d["w"], d["b"], c.k, c.s, tile_rows(c))
        good = slot_partials(*args)
        assert good.shape[1] == stat_slots(c, H, W)
        check_partials(good, d["Y"], "restated rule")
        assert breaks(check_partials, slot_partials(*args, count_cols=True), d["Y"]) == (Wo % 32 != 0)
        assert breaks(check_partials, slot_partials(*args, count_rows=True), d["Y"]) == (Ho % tile_rows(c) != 0)


def test_probe_apply_faults():
    """Image 0's statistics for image 1, statistics shifted by a channel octet, skip_relu ignored / applied without the flag: each
    breaks the apply assertion at every shape where it can act."""
    for io, Cs in APPLY_PATHS:
        for C in Cs:
            for HW in APPLY_HW:
                d = apply_data(HW, C)
                for form in APPLY_FORMS:
                    want = apply_ref(d, form)
                    assert breaks(assert_equal, apply_ref(d, form, "image0"), want), (C, HW, form)
                    if C > 8:
                        assert breaks(assert_equal, apply_ref(d, form, "octet"), want), (C, HW, form)
                    if form.startswith("skip-stats") and HW * C >= 32:  # (both directions: ignored with the flag, applied without)
                        assert breaks(assert_equal, apply_ref(d, form, "flip_skip_relu"), want), (C, HW, form)


def test_probe_conv_uses_image0_statistics():
    for c in NORM_CASES:
        H, W = conv_geos(c)[0]
        d = case_data(c, H, W)
        z = normalise(d["x"], d["mean"][:1].expand_as(d["mean"]), d["rstd"][:1].expand_as(d["rstd"]))
        assert breaks(assert_equal, conv_ref(z, d["w"], d["b"], c.k, c.s), d["Y"])


def test_probe_finish_drops_slots_from_128():
    for slots in FINISH_SLOTS:
        for C in FINISH_C:
            p = finish_data(slots, C)
            S, SS, HW = p[..., 0].sum(1), p[..., 1].sum(1), 32 * slots
            Sd, SSd = p[:, :128, :, 0].sum(1), p[:, :128, :, 1].sum(1)
            mean, var = Sd / HW, (SSd / HW - (Sd / HW) ** 2).clamp_min(0)
            mr = torch.stack([mean, 1 / torch.sqrt(var + EPS)], -1).float()
            check_mean_rstd(torch.stack([S / HW, 1 / torch.sqrt(SS / HW - (S / HW) ** 2 + EPS)], -1).float(), S, SS, HW, "restated")
            assert breaks(check_mean_rstd, mr, S, SS, HW) == (slots > 128)


def test_probe_unclamped_bilinear_tap():
    """Without the yp / xp clamp the last output row of the last image reads the NaN guard (weight 0 * NaN) wherever it sits on the
    last source row, i.e. unless Hd = 1 < Hs (there the extra tap stays inside the image and has weight 0)."""
    for (Hs, Ws), (Hd, Wd) in BILINEAR:
        src = bilinear_src(2, Hs, Ws, 8)
        hit = breaks(assert_equal, bilinear_ref(src, Hd, Wd, unclamped=True), bilinear_ref(src, Hd, Wd))
        assert hit == (Hd > 1 or Hs == 1), ((Hs, Ws), (Hd, Wd))


def test_probe_concat_boundary_source_map():
    """A channel piece at a source boundary resized with the previous source's map (`ch > c0[k]` for `ch >= c0[k]`) differs."""
    for _, dims, (Hd, Wd) in CONCAT:
        if len(dims) < 2:
            continue
        srcs = [bilinear_src(2, hs, ws, c, tag=k) for k, (hs, ws, c) in enumerate(dims)]
        want = torch.cat([bilinear_ref(s, Hd, Wd) for s in srcs], dim=-1)
        bad, c0 = want.clone(), 0
        for k, s in enumerate(srcs):
            if k > 0:  # the first piece of source k comes from source k - 1 at channel offset C[k-1]: the next pixel's first channels
                prev = srcs[k - 1]
                flat = torch.cat([prev.reshape(-1)[prev.shape[3]:], torch.full((prev.shape[3],), NAN, dtype=torch.float64)])
                bad[..., c0:c0 + 4] = bilinear_ref(flat.reshape(prev.shape)[..., :4], Hd, Wd)
            c0 += s.shape[3]
        assert breaks(assert_equal, bad, want), dims
