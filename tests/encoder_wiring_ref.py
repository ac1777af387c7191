"""CPU reference of the composite encoder's wiring (`tests/test_gpu_encoder_wiring.py`): BasicEncoder.forward in fp64, split
into segments, rounded exactly where the device rounds.  No GPU, no library.

The reference restates the RULES of the kernels, each read from the kernel that owns it; it does not follow the control flow of
`encoder_forward.hip` (no workspace, no ring of tables, no partials: a tensor is a tensor and a table belongs to its convolution).

Rounding points (every other operation is fp64):

 1. Stem input (`stem7x7` in conv_rows.hip): the planar clip is normalised as 2 * (c / 255) - 1 in fp32 (one division, one exact
    doubling, one subtraction: three fp32 operations that the CPU's fp32 arithmetic reproduces bit for bit), the x4 entry gets that
    fp32 tensor as it is; the kernel converts its patch to bf16 before the matrix cores see it.
 2. A convolution (`epilogue_rows`): fp32 accumulators + bias = the value v.  v is stored as bf16 (or, for conv3, as fp32 when the
    caller's rows are fp32).  The reference computes v in fp64 and rounds once.
 3. Statistics (`epilogue_rows`, `instnorm_finish_slots_kernel`): sum v and sum v^2 are taken from v BEFORE its bf16 conversion;
    mean = S / HW, var = max(SS / HW - mean^2, 0), rstd = 1 / sqrt(var + 1e-5) in fp64, both stored as fp32.
 4. Normalise-on-load (`store_patch` in conv_rows.hip): relu((x - mean) * rstd) with x bf16, two fp32 operations, rounded to
    bf16; the zero padding is applied after it.  The reference does the two operations in fp32 (they are IEEE operations with no
    freedom: a subtraction followed by a multiplication cannot contract into an fma).
 5. The residual pass (`instnorm_apply_bf16_kernel`): o = relu((x - m) * r) in fp32, NOT rounded to bf16; the skip is taken as
    it is (no skip statistics: layer x.1), as (k - km) * kr (skip statistics: the downsample branch, no ReLU, blocks.py:112-128),
    or as relu of that (MVT_APPLY_SKIP_RELU: the stem under layer1.0, whose InstanceNorm + ReLU was never materialised);
    relu(k + o) in fp32, rounded to bf16.  All in fp32 here as well.
 6. The concat (`concat_resize_rows_bf16_kernel`): align_corners bilinear resize of the bf16 stage outputs, blended in fp32,
    rounded to bf16.  The device's blend may contract into fmas and its source coordinate carries two fp32 roundings, so this
    one is NOT bit-exact: the reference is the fp64 formula and the test allows the bar derived in
    test_gpu_encoder_norm_exact.py plus the bf16 rounding.
 7. conv3 writes fp32 (v itself) or bf16 (v rounded to nearest even).

Rounding fp64 -> bf16 goes through fp32 here (torch has no direct conversion).  The double rounding can differ from a direct one
only when the fp32 rounding lands exactly on a bf16 tie, i.e. for v within 2^-24 relative of a tie: that is inside the accumulation
bound the element-wise checks allow anyway.

Modes.  "fp64" is the reference.  "f32a", "f32b" and "f32c" accumulate the convolutions and the statistics sums in fp32 in
different orders (plain; input channels reversed, or permuted, and the statistics summed in pieces of 32, or 8, pixels from the
last pixel backwards) and blend the resize in the kernel's own fp32 arithmetic: what they show against "fp64" on the same input is
what summation order alone does, and the only source of the tests' bars.

Faults (`Encoder(fault=...)`) are the probes' planted wiring errors; FAULTS lists them with the segments they act in.
"""
import zlib

import torch
import torch.nn.functional as F

EPS = 1e-5
COUTS = (64, 96, 128, 128)
STRIDES = (1, 2, 2, 2)
V_CLIP, T_CLIP, IMG0 = 3, 2, 2  # the clip every case reads: the run starts inside frame 0 and crosses into frame 1


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def f32(x):
    return x.float().double()


def bf(x):
    return x.float().bfloat16().double()


def bf16_ulp(x):
    """One bf16 ulp at |x| (8 significand bits): 2^(e - 8) with |x| = m 2^e, m in [0.5, 1)."""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


# ================================================================== weights and images

def conv_shapes(C):
    """name -> (Cout, Cin, k) of the 22 convolutions, in the order of the weight struct (slot 3, layer 1's missing downsample, left out)."""
    s = {"fnet.conv1": (64, 3, 7)}
    cin = 64
    for li, cout in enumerate(COUTS, start=1):
        s[f"fnet.layer{li}.0.conv1"] = (cout, cin, 3)
        s[f"fnet.layer{li}.0.conv2"] = (cout, cout, 3)
        if li > 1:
            s[f"fnet.layer{li}.0.downsample.0"] = (cout, cin, 1)
        s[f"fnet.layer{li}.1.conv1"] = (cout, cout, 3)
        s[f"fnet.layer{li}.1.conv2"] = (cout, cout, 3)
        cin = cout
    s["fnet.conv2"] = (2 * C, 416, 3)
    s["fnet.conv3"] = (C, 2 * C, 1)
    return s


def make_weights(C, seed):
    """name -> (w [Cout][Cin][k][k], b [Cout]) fp64: bf16-representable He-scaled normal weights, every bias non-zero (0.1 .. 0.5 in
    magnitude, random sign, an fp32 value), every convolution drawn on its own."""
    g = gen("weights", C, seed)
    W = {}
    for name, (co, ci, k) in conv_shapes(C).items():
        w = bf(torch.randn(co, ci, k, k, generator=g, dtype=torch.float64) * (2.0 / (ci * k * k)) ** 0.5)
        sign = 1.0 - 2.0 * torch.randint(0, 2, (co,), generator=g).double()
        b = f32(sign * (0.1 + 0.4 * torch.rand(co, generator=g, dtype=torch.float64)))
        W[name] = (w, b)
    return W


def make_clip(H, W, seed):
    """(V, T, 3, H, W) uint8: smooth random structure plus noise, a different gain and offset per image (their statistics differ)."""
    g = gen("clip", H, W, seed)
    V, T = V_CLIP, T_CLIP
    coarse = torch.rand(V, T, 3, (H + 7) // 8 + 1, (W + 7) // 8 + 1, generator=g)
    smooth = F.interpolate(coarse.reshape(V * T, 3, *coarse.shape[-2:]), size=(H, W), mode="bilinear", align_corners=True).reshape(V, T, 3, H, W)
    gain = 0.35 + 0.6 * torch.rand(V, T, 1, 1, 1, generator=g)
    off = 0.3 * torch.rand(V, T, 3, 1, 1, generator=g)
    x = (off + gain * (0.7 * smooth + 0.3 * torch.rand(V, T, 3, H, W, generator=g))).clamp(0, 1)
    return (x * 255).round().to(torch.uint8)


def clip_images(clip, n, img0=IMG0, view_major=False):
    """Images img0 .. img0 + n - 1 of the clip, frame-major (image i = view i % V of frame i // V) -> [n][H][W][3] uint8."""
    V, T = clip.shape[:2]
    out = []
    for gi in range(img0, img0 + n):
        v, t = (gi // T, gi % T) if view_major else (gi % V, gi // V)
        out.append(clip[v, t].permute(1, 2, 0))
    return torch.stack(out)


def normalised(u8, minus_one=True):
    """Rounding point 1: 2 * (c / 255) - 1 in fp32 -> [n][H][W][3] fp32."""
    x = 2.0 * (u8.float() / 255.0)
    return x - 1.0 if minus_one else x


def x4_of(x):
    """The x4 entry's input: [n][H][W][4] fp32, channel 3 zero."""
    return torch.cat([x, torch.zeros_like(x[..., :1])], -1).contiguous()


# ================================================================== the kernels' rules

def norm_load(x, st, relu=True):
    """Rounding points 4 / 5: (x - mean) * rstd in fp32 (x [n][..][C], st = (mean, rstd) [n][C]); not rounded to bf16 here."""
    n, C = st[0].shape
    shape = (n,) + (1,) * (x.dim() - 2) + (C,)
    z = (x.float() - st[0].float().view(shape)) * st[1].float().view(shape)
    return F.relu(z) if relu else z


def bilinear_ac(src, Hd, Wd, align_corners=True):
    """fp64 bilinear resize of [n][Hs][Ws][C]; align_corners=True is the kernel's formula (src = dst * (in - 1) / (out - 1))."""
    return F.interpolate(src.double().permute(0, 3, 1, 2), size=(Hd, Wd), mode="bilinear", align_corners=align_corners).permute(0, 2, 3, 1).contiguous()


def bilinear_f32(src, Hd, Wd, by_columns):
    """The kernel's own arithmetic in fp32 (ratio, source coordinate, weights, blend; no fma), blended rows first as the kernel
    writes it or columns first: what fp32 does to a non-dyadic size ratio (the fp32 modes of seg_cat)."""
    n, Hs, Ws, C = src.shape
    s = src.float()

    def taps(So, Sd):
        r = (torch.tensor(float(So - 1)) / torch.tensor(float(Sd - 1))) if Sd > 1 else torch.tensor(0.0)
        f = r * torch.arange(Sd, dtype=torch.float32)
        i0 = f.floor().long()
        return i0, i0 + (i0 < So - 1).long(), f - i0.float()

    y0, y1, ly = taps(Hs, Hd)
    x0, x1, lx = taps(Ws, Wd)
    ly, lx = ly.view(1, Hd, 1, 1), lx.view(1, 1, Wd, 1)
    hy, hx = 1.0 - ly, 1.0 - lx
    a00, a01, a10, a11 = s[:, y0][:, :, x0], s[:, y0][:, :, x1], s[:, y1][:, :, x0], s[:, y1][:, :, x1]
    if by_columns:
        return (hx * (hy * a00 + ly * a10) + lx * (hy * a01 + ly * a11)).double()
    return (hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11)).double()


def out_rows(v, out_bf16):
    """Rounding point 7: conv3's v as the caller's rows hold it."""
    return bf(v) if out_bf16 else f32(v)


FAULTS = {
    # fault: the segments it acts in ("s0" = image -> s[0]; "stage1..3" = s[l-1] -> s[l]; "stem", "cat", "c2", "out")
    "swap_conv1_down_tables": ("stage1", "stage2", "stage3"),
    "conv2_with_conv1_table": ("s0", "stage1", "stage2", "stage3"),
    "no_skip_relu_layer1_0": ("s0",),
    "skip_relu_on_downsample": ("stage1", "stage2", "stage3"),
    "skip_dropped": ("s0", "stage1", "stage2", "stage3"),
    "stale_table": ("stage3",),
    "image0_statistics": ("s0", "stage1", "stage2", "stage3", "out"),
    "swap_layer3_1_layer4_1": ("stage2", "stage3"),
    "swap_layer1_0_conv1_conv2": ("s0",),
    "swap_stages_3_4": ("cat",),
    "align_corners_off": ("cat",),
    "conv3_bias_dropped": ("out",),
    "no_relu_before_conv3": ("out",),
    "img0_off_by_one": ("stem", "s0"),
    "view_major": ("stem", "s0"),
    "u8_without_minus_one": ("stem", "s0"),
    "short_row": ("stem", "s0"),
    "short_col": ("stem", "s0"),
}


MODES = ("fp64", "f32a", "f32b", "f32c")


class Encoder:
    """BasicEncoder.forward (spatracker/blocks.py:214-284) by the rules above.  Activations are [n][H][W][C] fp64 tensors holding
    bf16 values; a statistics table is (mean, rstd), each [n][C] fp64 holding fp32 values."""

    def __init__(self, weights, C, mode="fp64", fault=None, stale=None):
        assert mode in MODES and (fault is None or fault in FAULTS)
        self.W, self.C, self.mode, self.fault, self.stale = weights, C, mode, fault, stale
        self.tables = []  # every statistics table in the order the composite allocates them (the probes' stale table comes from here)

    # ---------------------------------------------------------------- primitives
    def _name(self, name):
        if self.fault == "swap_layer3_1_layer4_1" and (".layer3.1." in name or ".layer4.1." in name):
            return name.replace(".layer3.1.", ".layer#.1.").replace(".layer4.1.", ".layer3.1.").replace(".layer#.1.", ".layer4.1.")
        if self.fault == "swap_layer1_0_conv1_conv2" and ".layer1.0." in name:
            return name.replace("conv1", "conv#").replace("conv2", "conv1").replace("conv#", "conv2")
        return name

    def conv(self, name, x, stride, in_stats=None, bias=True):
        """-> v [n][Ho][Wo][Cout]: accumulators + bias, unrounded (rounding point 2).  x holds bf16 values."""
        w, b = self.W[self._name(name)]
        if in_stats is not None:
            x = bf(norm_load(x, in_stats))  # rounding point 4; F.conv2d's zero padding comes after it
        k = w.shape[-1]
        xc, wc = x.permute(0, 3, 1, 2), w
        if self.mode == "f32b":
            xc, wc = xc.flip(1), wc.flip(1)
        if self.mode == "f32c":
            perm = torch.randperm(xc.shape[1], generator=gen("f32c", xc.shape[1]))
            xc, wc = xc[:, perm], wc[:, perm]
        if self.mode != "fp64":
            xc, wc, b = xc.float(), wc.float(), b.float()
        v = F.conv2d(xc.contiguous(), wc.contiguous(), b if bias else None, stride=stride, padding=k // 2)
        return v.double().permute(0, 2, 3, 1).contiguous()

    def acc_bound(self, name, x, stride, in_stats=None):
        """The fp32 accumulation bound of every element of conv(): (K + 1) * 2^-23 * (sum |w x| + |b|) over the element's
        receptive field, K = k * k * Cin products.  K + 1 additions (the bias is one), each off by at most one fp32 ulp --
        2^-23 relative, which covers an adder that truncates as well as one that rounds to nearest -- of a partial sum that is
        at most sum |w x| + |b| in magnitude; the products of two bf16 values are exact in fp32."""
        if self.mode != "fp64":
            return None  # (only the reference's elements carry an allowance)
        w, b = self.W[self._name(name)]
        if in_stats is not None:
            x = bf(norm_load(x, in_stats))
        k = w.shape[-1]
        a = F.conv2d(x.double().abs().permute(0, 3, 1, 2), w.abs(), b.abs(), stride=stride, padding=k // 2).permute(0, 2, 3, 1)
        return (w[0].numel() + 1) * 2.0 ** -23 * a

    def stats(self, v, HW=None):
        """Rounding point 3: (mean, rstd) of v [n][H][W][C] over its pixels, stored as fp32.  HW: the divisor, if not v's pixels."""
        n, C = v.shape[0], v.shape[-1]
        y = v.reshape(n, -1, C)
        HW = HW or y.shape[1]
        if self.mode == "fp64":
            S, SS = y.sum(1), (y * y).sum(1)
        elif self.mode == "f32a":
            yf = y.float()
            S, SS = yf.sum(1).double(), (yf * yf).sum(1).double()
        else:  # pieces of 32 (f32b) or 8 (f32c) pixels from the last pixel backwards, fp32 inside a piece, fp64 across the pieces
            q = 32 if self.mode == "f32b" else 8
            yf = F.pad(y.float().flip(1), (0, 0, 0, -y.shape[1] % q)).reshape(n, -1, q, C)
            S, SS = yf.sum(2).double().sum(1), (yf * yf).sum(2).double().sum(1)
        mean = S / HW
        var = (SS / HW - mean * mean).clamp_min(0.0)
        st = (f32(mean), f32(1.0 / torch.sqrt(var + EPS)))
        if self.fault == "image0_statistics":
            st = tuple(t[:1].expand_as(t).contiguous() for t in st)
        self.tables.append(st)
        return st

    def apply(self, z, st, skip, skip_st, skip_relu):
        """Rounding point 5: relu(skip' + relu((z - m) r)) in fp32 -> bf16."""
        o = norm_load(z, st)
        if skip is None:
            return bf(o)
        k = skip.float() if skip_st is None else norm_load(skip, skip_st, relu=skip_relu)
        return bf(F.relu(k + o))

    # ---------------------------------------------------------------- blocks (blocks.py:84-128)
    def block(self, p, x, x_st, stride, down, keep=None):
        """ResidualBlock `p` on x (a finished activation, or a raw convolution output with its table x_st) -> its output."""
        f = self.fault
        v1 = self.conv(p + ".conv1", x, stride, in_stats=x_st)
        st1 = self.stats(v1)
        y = bf(v1)
        d = sd = None
        if down:
            vd = self.conv(p + ".downsample.0", x, stride)
            sd = self.stats(vd)
            d = bf(vd)
            if f == "swap_conv1_down_tables":
                st1, sd = sd, st1
        in2 = st1
        if f == "stale_table" and p == "fnet.layer4.1":  # allocation 18 (layer4.1.conv1's table) read from allocation 10's slot
            in2 = self.stale
        v2 = self.conv(p + ".conv2", y, 1, in_stats=in2)
        st2 = self.stats(v2)
        z = bf(v2)
        if keep is not None:
            keep.update(y=y, d=d)
        st_z = st1 if f == "conv2_with_conv1_table" else st2
        if f == "skip_dropped" and p.endswith(".1"):
            return self.apply(z, st_z, None, None, False)
        if down:
            return self.apply(z, st_z, d, sd, f == "skip_relu_on_downsample")
        return self.apply(z, st_z, x, x_st, x_st is not None and not (f == "no_skip_relu_layer1_0" and p == "fnet.layer1.0"))

    def stage(self, li, x, x_st=None, keep=None):
        """layer `li` (1..4): two blocks.  keep: receives z0 (the first block's output), y and d (what the workspace holds last)."""
        k0, k1 = {}, {}
        z0 = self.block(f"fnet.layer{li}.0", x, x_st, STRIDES[li - 1], li > 1, k0)
        out = self.block(f"fnet.layer{li}.1", z0, None, 1, False, k1)
        if keep is not None:
            keep.update(z0=z0, y=k1["y"], d=k0["d"])
        return out

    # ---------------------------------------------------------------- segments
    def images(self, clip, n):
        """clip -> the stem's fp32 input [n][H][W][3] (rounding point 1)."""
        f = self.fault
        u8 = clip_images(clip, n, IMG0 + (1 if f == "img0_off_by_one" else 0), view_major=f == "view_major")
        return normalised(u8, minus_one=f != "u8_without_minus_one")

    def seg_stem(self, x):
        """fp32 image [n][H][W][3] -> (raw stem output as stored, its table, v's accumulation bound)."""
        xb = bf(x)
        v = counted = self.conv("fnet.conv1", xb, 2)
        if self.fault == "short_row":  # the last row / column of the ragged map: not computed (stored as zeros), not counted
            counted, v = v[:, :-1], torch.cat([v[:, :-1], torch.zeros_like(v[:, -1:])], 1)
        if self.fault == "short_col":
            counted, v = v[:, :, :-1], torch.cat([v[:, :, :-1], torch.zeros_like(v[:, :, -1:])], 2)
        st = self.stats(counted, HW=v.shape[1] * v.shape[2])
        return bf(v), st, self.acc_bound("fnet.conv1", xb, 2)

    def seg_s0(self, x):
        """fp32 image -> s[0]: the stem and layer 1."""
        stem, st, _ = self.seg_stem(x)
        return self.stage(1, stem, st)

    def seg_stage(self, li, s_prev):
        """s[li - 2] -> s[li - 1] (layer li = 2..4)."""
        return self.stage(li, s_prev)

    def seg_cat(self, stages, hs, ws):
        """s[0..3] -> (cat [n][hs][ws][416] bf16, the resize's bar per element without the bf16 rounding)."""
        if self.fault == "swap_stages_3_4":
            stages = [stages[0], stages[1], stages[3], stages[2]]
        ac = self.fault != "align_corners_off"
        parts, bars = [], []
        for s in stages:
            r = bilinear_ac(s, hs, ws, ac) if self.mode == "fp64" else bilinear_f32(s, hs, ws, self.mode != "f32a")
            parts.append(r)
            bar = (2.0 ** -22 * max(s.shape[1], s.shape[2]) + 8 * 2.0 ** -24) * float(s.abs().max())
            bars.append(torch.full(r.shape, bar, dtype=torch.float64))
        return bf(torch.cat(parts, -1)), torch.cat(bars, -1)

    def seg_c2(self, cat):
        """cat -> (raw conv2 output as stored, its table, the accumulation bound)."""
        v = self.conv("fnet.conv2", cat, 1)
        return bf(v), self.stats(v), self.acc_bound("fnet.conv2", cat, 1)

    def seg_out(self, cat, c2_st=None):
        """cat -> conv3's v, unrounded: the caller's rows hold out_rows(v, out_bf16).  c2_st: seg_c2(cat), if the caller has it."""
        c2, st = (c2_st or self.seg_c2(cat))[:2]
        if self.fault == "no_relu_before_conv3":
            return self.conv("fnet.conv3", bf(norm_load(c2, st, relu=False)), 1)
        return self.conv("fnet.conv3", c2, 1, in_stats=st, bias=self.fault != "conv3_bias_dropped")

    def seg_d(self, s2):
        """s[2] -> layer 4's downsample branch as stored (the folded launch's second output), and its accumulation bound."""
        return bf(self.conv("fnet.layer4.0.downsample.0", s2, 2)), self.acc_bound("fnet.layer4.0.downsample.0", s2, 2)

    def seg_y(self, z0):
        """layer 4's z0 -> layer4.1.conv1's raw output as stored, and its accumulation bound."""
        return bf(self.conv("fnet.layer4.1.conv1", z0, 1)), self.acc_bound("fnet.layer4.1.conv1", z0, 1)

    # ---------------------------------------------------------------- the whole chain
    def run(self, x, out_bf16=False):
        """fp32 image -> every tensor a call leaves behind: stem, s[0..3], z0, y, d (layer 4's), cat, c2, out; and `tables`."""
        n, H, W, _ = x.shape
        self.tables = []
        T = {}
        T["stem"], st, _ = self.seg_stem(x)
        keep = {}
        s = [self.stage(1, T["stem"], st)]
        for li in (2, 3, 4):
            s.append(self.stage(li, s[-1], None, keep))
        T.update(s=s, z0=keep["z0"], y=keep["y"], d=keep["d"])
        T["cat"], _ = self.seg_cat(s, H // 4, W // 4)
        c2_st = self.seg_c2(T["cat"])
        T["c2"] = c2_st[0]
        T["out"] = out_rows(self.seg_out(T["cat"], c2_st), out_bf16)
        T["tables"] = list(self.tables)
        return T


# ================================================================== distances and checks

def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def distances(got, want):
    """(mean |d| / RMS(want), max over pixels of the channel-RMS of d / RMS(want)) of [n][H][W][C] tensors."""
    d = got.double() - want.double()
    r = rms(want)
    return float(d.abs().mean()) / r, float(d.pow(2).mean(-1).sqrt().max()) / r


def elementwise(got, want, extra):
    """One-step check: (max over elements of |got - want| / (one bf16 ulp of the larger magnitude + extra), the share of elements
    that differ at all).  The first must be <= 1: got and want are each within half a bf16 ulp of their unrounded values, which
    are `extra` apart at most."""
    got, want = got.double(), want.double()
    d = (got - want).abs()
    bound = bf16_ulp(torch.maximum(got.abs(), want.abs())) + extra
    return float((d / bound).max()), float((d > 0).double().mean())
