"""Parity of every entry point of libmvtracker_hip.so against the oracle / plain torch fp32-fp64
references on identical inputs.  Runs on the MI355X box only (`-m gpu`); all calls go through the C ABI.
(The GEMM / conv / fused-MLP kernels variant by variant, on integer inputs with exact answers: test_gpu_matmul_exact.py.)"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (test_oracle_golden helpers)

from mvtracker_amd import synth  # noqa: E402
from oracle import mvt_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.asarray(a))


def G(a):
    return (a if isinstance(a, torch.Tensor) else T(a)).to(DEV).contiguous()


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def pad_w(w, mult=64):
    n, k = w.shape
    wp = torch.zeros(n, (k + mult - 1) // mult * mult)
    wp[:, :k] = w
    return wp


def split(hip, wp, lo=True):
    """fp32 [N][Kp] on device -> (bf16 hi, bf16 lo | None) int16 tensors through the library."""
    hi = torch.empty(wp.shape, device=DEV, dtype=torch.int16)
    l = torch.empty(wp.shape, device=DEV, dtype=torch.int16) if lo else None
    hip.split_bf16(wp, hi, l, wp.numel())
    return hi, l


PREC_TOL = {"fp32": 2e-6, "bf16x3": 2e-5, "bf16": 2e-2}


# ----------------------------------------------------------------------------------------- GEMM / conv
@pytest.mark.parametrize("M,N,K,act,res", [(300, 256, 581, 0, False), (1000, 131, 256, 1, False), (768, 288, 256, 0, False),
                                           (517, 1024, 256, 2, False), (400, 256, 1024, 0, True), (130, 128, 128, 3, True),
                                           (64, 64, 32, 0, False), (2000, 864, 256, 0, False), (33, 131, 131, 1, False)])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
def test_gemm(hip, M, N, K, act, res, prec):
    g = torch.Generator().manual_seed(M + N + K)
    lda = (K + 3) // 4 * 4
    A = torch.zeros(M, lda)
    A[:, :K] = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    R = torch.randn(M, N, generator=g) if res else None
    ref = A[:, :K].double() @ W.double().t() + b.double()
    ref = [lambda x: x, F.relu, lambda x: F.gelu(x, approximate="tanh"), F.gelu][act](ref)
    if res:
        ref = ref + R.double()
    ldc = N + 5
    C = torch.full((M, ldc), 7.0, device=DEV)
    Wp = G(pad_w(W))
    if prec == "fp32":
        hip.gemm(G(A), lda, Wp, Wp.shape[1], G(b), G(R) if res else None, N, C, ldc, M, N, K, act)
    else:
        hi, lo = split(hip, Wp, prec == "bf16x3")
        hip.gemm_bf16(G(A), lda, hi, lo, Wp.shape[1], G(b), G(R) if res else None, N, C, ldc, M, N, K, act)
    torch.cuda.synchronize()
    assert rel_err(C[:, :N], ref) < PREC_TOL[prec]
    assert bool((C[:, N:] == 7.0).all())  # nothing written outside the N columns


CONVS = [  # n, H, W, Cin, Cout, k, stride, pad
    (2, 64, 96, 3, 64, 7, 2, 3), (2, 33, 47, 64, 64, 3, 1, 1), (1, 33, 47, 64, 96, 3, 2, 1), (2, 30, 30, 96, 128, 1, 2, 0),
    (1, 16, 24, 416, 256, 3, 1, 1), (3, 9, 11, 256, 128, 1, 1, 0), (1, 20, 20, 128, 128, 3, 2, 1), (1, 20, 37, 96, 96, 3, 1, 1),
    (2, 17, 16, 128, 128, 3, 1, 1), (1, 8, 16, 64, 64, 3, 1, 1)]


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("cfg", CONVS)
def test_conv2d(hip, cfg, prec):
    n, H, W, Cin, Cout, k, s, p = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn(n, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p)
    if Cin == 3:
        x4 = torch.zeros(n, H, W, 4)
        x4[..., :3] = x.permute(0, 2, 3, 1)
        wt = torch.zeros(Cout, 7, 8, 4)
        wt[:, :, :7, :3] = w.permute(0, 2, 3, 1)
        xin, wt, cin = x4, wt.reshape(Cout, 224), 4
    else:
        xin, wt, cin = x.permute(0, 2, 3, 1).contiguous(), w.permute(0, 2, 3, 1).contiguous(), Cin
    Ho, Wo = ref.shape[-2:]
    out = torch.empty(n, Ho, Wo, Cout, device=DEV)
    wp = G(pad_w(wt.reshape(Cout, -1)))
    if prec == "fp32":
        hip.conv2d(G(xin), wp, G(b), out, n, H, W, cin, Cout, k, k, s, p, Cout)
    else:
        hi, lo = split(hip, wp, prec == "bf16x3")
        hip.conv2d_bf16(G(xin), hi, lo, G(b), out, n, H, W, cin, Cout, k, k, s, p, Cout)
    torch.cuda.synchronize()
    assert rel_err(out.permute(0, 3, 1, 2), ref) < PREC_TOL[prec]


@pytest.mark.parametrize("cfg", [(2, 24, 40, 64, 96, 3, 1, 1), (3, 17, 21, 32, 64, 3, 1, 1), (2, 32, 64, 64, 96, 3, 2, 1),
                                 (2, 24, 40, 64, 64, 3, 1, 1), (3, 17, 21, 64, 64, 3, 1, 1), (5, 64, 96, 64, 64, 3, 1, 1),
                                 (2, 32, 32, 96, 128, 1, 2, 0), (1, 64, 64, 3, 64, 7, 2, 3)])
@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
def test_conv2d_fused_instnorm(hip, cfg, prec):
    """statistics from the conv epilogue == InstanceNorm of the conv output; in_stats == relu(IN(x)) applied up front."""
    n, H, W, Cin, Cout, k, s, p = cfg
    g = torch.Generator().manual_seed(sum(cfg) + 1)
    x = torch.randn(n, H, W, Cin, generator=g) * 1.5 + 0.3
    w = torch.randn(Cout, k, k, Cin, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    if Cin == 3:
        x4 = torch.zeros(n, H, W, 4)
        x4[..., :3] = x
        wt = torch.zeros(Cout, 7, 8, 4)
        wt[:, :, :7, :3] = w
        x, w, cin = x4, wt.reshape(Cout, 224), 4
    else:
        cin = Cin
    hi, lo = split(hip, G(pad_w(w.reshape(Cout, -1))), prec == "bf16x3")
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    halo = k == 3 and s == 1
    slots = hip.conv2d_stat_slots(H, W, cin, k, k, s, p, prec == "bf16x3")
    if prec == "bf16":  # row-tile kernels: one slot per workgroup tile (8 rows x 32 pixels; 4 rows for the stride-2 3x3 kernel)
        tr = 4 if (k == 3 and s == 2) else 8
        assert slots == ((Ho + tr - 1) // tr) * ((Wo + 31) // 32)
    else:
        assert slots == (((Ho + 7) // 8) * ((Wo + 15) // 16) * 4 if halo else Ho * Wo // 32)
    xin = G(x)
    in_st = None
    if halo:  # normalise-on-load against an explicit normalise pass
        in_st = torch.empty(n, cin, 2, device=DEV)
        part64 = torch.empty(n * hip.IN_SLABS * cin * 2, device=DEV, dtype=torch.float64)
        hip.instnorm_stats(xin, cin, part64, in_st, n, H * W, cin)
        xn = torch.empty_like(xin)
        hip.instnorm_apply(xin, in_st, None, None, xn, n, H * W, cin)
    else:
        xn = xin
    ref = torch.empty(n, Ho, Wo, Cout, device=DEV)
    hip.conv2d_bf16(xn, hi, lo, G(b), ref, n, H, W, cin, Cout, k, k, s, p, Cout)
    out = torch.empty(n, Ho, Wo, Cout, device=DEV)
    part = torch.full((n * slots * Cout * 2,), float("nan"), device=DEV)
    hip.conv2d_bf16(xin, hi, lo, G(b), out, n, H, W, cin, Cout, k, k, s, p, Cout, in_stats=in_st, out_partial=part)
    st = torch.empty(n, Cout, 2, device=DEV)
    hip.instnorm_finish_slots(part, slots, st, n, Ho * Wo, Cout)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)  # same arithmetic on the same values
    y = ref.double().reshape(n, Ho * Wo, Cout)
    mean, var = y.mean(1), y.var(1, unbiased=False)
    assert (st[..., 0].double() - mean).abs().max() < 1e-5
    assert ((st[..., 1].double() * torch.sqrt(var + 1e-5)) - 1).abs().max() < 1e-5


@pytest.mark.parametrize("cfg", [(2, 24, 40, 64, 96, 3, 1, 1), (2, 32, 64, 64, 96, 3, 2, 1), (2, 32, 32, 96, 128, 1, 2, 0),
                                 (2, 24, 40, 64, 64, 3, 1, 1), (3, 17, 21, 64, 64, 3, 1, 1), (9, 64, 96, 64, 64, 3, 1, 1),
                                 (1, 64, 64, 3, 64, 7, 2, 3), (1, 16, 24, 416, 256, 3, 1, 1)])
def test_conv2d_bf16_activation_tensors(hip, cfg):
    """bf16 activation tensors (bf16 mode): same arithmetic as fp32 tensors holding the bf16 values, output rounded
    to nearest even, statistics untouched."""
    n, H, W, Cin, Cout, k, s, p = cfg
    g = torch.Generator().manual_seed(sum(cfg) + 3)
    x = (torch.randn(n, H, W, Cin, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    w = torch.randn(Cout, k, k, Cin, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    stem = Cin == 3
    if stem:  # the stem reads fp32 RGB, only its output is bf16
        x4 = torch.zeros(n, H, W, 4)
        x4[..., :3] = x.float()
        wt = torch.zeros(Cout, 7, 8, 4)
        wt[:, :, :7, :3] = w
        xin_f, w, cin = G(x4), wt.reshape(Cout, 224), 4
        xin_b = xin_f
    else:
        cin = Cin
        xin_f, xin_b = G(x.float()), G(x)
    hi, _ = split(hip, G(pad_w(w.reshape(Cout, -1))), False)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    halo = k == 3 and s == 1
    slots = hip.conv2d_stat_slots(H, W, cin, k, k, s, p, False)
    in_st = None
    if halo:
        in_st = G(torch.stack([torch.randn(n, cin, generator=g) * 0.2, torch.rand(n, cin, generator=g) + 0.5], -1))
    outs, parts = [], []
    for xin, dt in ((xin_f, torch.float32), (xin_b, torch.bfloat16)):
        out = torch.empty(n, Ho, Wo, Cout, device=DEV, dtype=dt)
        part = torch.full((n * max(slots, 1) * Cout * 2,), float("nan"), device=DEV)
        hip.conv2d_bf16(xin, hi, None, G(b), out, n, H, W, cin, Cout, k, k, s, p, Cout, in_stats=in_st, out_partial=part if slots else None)
        outs.append(out)
        parts.append(part)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].to(torch.bfloat16), outs[1])
    if slots:
        assert torch.equal(parts[0], parts[1])


@pytest.mark.parametrize("cfg", [(2, 16, 32, 416, 256), (1, 45, 80, 416, 256), (3, 21, 37, 64, 512), (1, 128, 128, 96, 256), (2, 8, 32, 32, 256)])
def test_conv_big_tile_bit_identical(hip, cfg, monkeypatch):
    """conv3x3_big_bf16 (one 512-thread workgroup per 8 x 32 pixel tile and 256-channel block, LDS-DMA staging, swizzled 64-B slots)
    against the 64-channel row tiles it replaces on the wide 3 x 3 / stride-1 layers without normalise-on-load (BasicEncoder.conv2,
    spatracker/blocks.py:246): same accumulation order, same epilogue -> identical outputs and InstanceNorm partials, bit for bit.
    Image sizes that leave partial tiles in both directions (45 x 80 is the C5 shard's feature map), one tile exactly, two channel
    blocks; and the values themselves against an fp64 convolution of the same bf16 operands."""
    n, H, W, Cin, Cout = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = (torch.randn(n, H, W, Cin, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) / math.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g)
    hi, _ = split(hip, G(pad_w(w.reshape(Cout, -1))), False)
    slots = hip.conv2d_stat_slots(H, W, Cin, 3, 3, 1, 1, False)
    xin, bias = G(x), G(b)
    outs, parts = [], []
    for big in ("1", "0"):
        monkeypatch.setenv("MVT_CONV_BIG", big)
        out = torch.full((n, H, W, Cout), float("nan"), device=DEV, dtype=torch.bfloat16)
        part = torch.full((n * slots * Cout * 2,), float("nan"), device=DEV)
        hip.conv2d_bf16(xin, hi, None, bias, out, n, H, W, Cin, Cout, 3, 3, 1, 1, Cout, out_partial=part)
        torch.cuda.synchronize()
        outs.append(out)
        parts.append(part)
    assert bool(torch.isfinite(outs[0].float()).all()) and bool(torch.isfinite(parts[0]).all())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(parts[0], parts[1])
    wb = w.to(torch.bfloat16).double().permute(0, 3, 1, 2)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), wb, b.double(), padding=1).permute(0, 2, 3, 1)
    assert rel_err(outs[0].float(), ref) < 6e-3  # (the output's own bf16 rounding)
    # the fused statistics: sums over the tiles' slots = sums over the image
    ps = parts[0].reshape(n, slots, Cout, 2).double().sum(1).cpu()
    assert (ps[..., 0] - ref.sum((1, 2))).abs().max() / ref.sum((1, 2)).abs().max() < 1e-4


@pytest.mark.parametrize("cfg", [(2, 64, 96, 64, 96), (1, 90, 160, 96, 128), (3, 33, 41, 128, 128), (2, 32, 32, 64, 64)])
def test_conv3x3s2_with_downsample_branch(hip, cfg):
    """mvt_conv3x3s2_down_bf16: conv1 (3x3 / stride 2) and downsample[0] (1x1 / stride 2) of a strided ResidualBlock
    (spatracker/blocks.py:84-128) in one launch -- the downsample as the centre tap of the 3x3 window -- against the two separate
    launches: both output tensors identical, bit for bit; conv1's statistics partials identical; the downsample's statistics (cut into
    4-row instead of 8-row tiles: another fixed summation order) equal after the slot reduction to fp32 rounding.  Odd sizes (a
    ragged last tile in both directions), 64- and 96-channel tiles."""
    n, H, W, Cin, Cout = cfg
    g = torch.Generator().manual_seed(sum(cfg) + 11)
    x = G((torch.randn(n, H, W, Cin, generator=g) * 1.5 + 0.3).to(torch.bfloat16))
    w3 = torch.randn(Cout, 3, 3, Cin, generator=g) / math.sqrt(Cin * 9)
    wd = torch.randn(Cout, 1, 1, Cin, generator=g) / math.sqrt(Cin)
    b3, bd = G(torch.randn(Cout, generator=g)), G(torch.randn(Cout, generator=g))
    h3, _ = split(hip, G(pad_w(w3.reshape(Cout, -1))), False)
    hd, _ = split(hip, G(pad_w(wd.reshape(Cout, -1))), False)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    s3 = hip.conv2d_stat_slots(H, W, Cin, 3, 3, 2, 1, False)
    sd = hip.conv2d_stat_slots(H, W, Cin, 1, 1, 2, 0, False)
    o3 = torch.full((n, Ho, Wo, Cout), float("nan"), device=DEV, dtype=torch.bfloat16)
    od, f3, fd = o3.clone(), o3.clone(), o3.clone()
    p3 = torch.full((n * s3 * Cout * 2,), float("nan"), device=DEV)
    pd = torch.full((n * sd * Cout * 2,), float("nan"), device=DEV)
    q3, qd = p3.clone(), torch.full((n * s3 * Cout * 2,), float("nan"), device=DEV)
    hip.conv2d_bf16(x, h3, None, b3, o3, n, H, W, Cin, Cout, 3, 3, 2, 1, Cout, out_partial=p3)
    hip.conv2d_bf16(x, hd, None, bd, od, n, H, W, Cin, Cout, 1, 1, 2, 0, Cout, out_partial=pd)
    hip.conv3x3s2_down_bf16(x, h3, b3, hd, bd, f3, fd, n, H, W, Cin, Cout, Cout, q3, qd)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(f3.float()).all()) and bool(torch.isfinite(fd.float()).all())
    assert torch.equal(f3, o3) and torch.equal(fd, od)
    assert torch.equal(q3, p3)
    a = pd.reshape(n, sd, Cout, 2).double().sum(1)
    b = qd.reshape(n, s3, Cout, 2).double().sum(1)
    assert bool(torch.isfinite(qd).all()) and ((a - b).abs().max() / a.abs().max()).item() < 1e-6


def test_encoder_elementwise_bf16_tensors(hip):
    g = torch.Generator().manual_seed(77)
    n, Hh, Ww, C = 2, 12, 20, 96
    x = (torch.randn(n, Hh * Ww, C, generator=g) * 2).to(torch.bfloat16)
    sk = torch.randn(n, Hh * Ww, C, generator=g).to(torch.bfloat16)
    st = G(torch.stack([torch.randn(n, C, generator=g) * 0.2, torch.rand(n, C, generator=g) + 0.5], -1))
    sst = G(torch.stack([torch.randn(n, C, generator=g) * 0.2, torch.rand(n, C, generator=g) + 0.5], -1))
    for skip, skst in ((None, None), (sk, None), (sk, sst)):
        yf = torch.empty(n, Hh * Ww, C, device=DEV)
        yb = torch.empty(n, Hh * Ww, C, device=DEV, dtype=torch.bfloat16)
        hip.instnorm_apply(G(x.float()), st, None if skip is None else G(skip.float()), skst, yf, n, Hh * Ww, C)
        hip.instnorm_apply(G(x), st, None if skip is None else G(skip), skst, yb, n, Hh * Ww, C)
        torch.cuda.synchronize()
        assert torch.equal(yf.to(torch.bfloat16), yb)
    # statistics of a bf16 tensor
    part = torch.empty(n * hip.IN_SLABS * C * 2, device=DEV, dtype=torch.float64)
    s1, s2 = torch.empty(n, C, 2, device=DEV), torch.empty(n, C, 2, device=DEV)
    hip.instnorm_stats(G(x.float()), C, part, s1, n, Hh * Ww, C)
    hip.instnorm_stats(G(x), C, part, s2, n, Hh * Ww, C)
    torch.cuda.synchronize()
    assert torch.equal(s1, s2)
    # resize into a channel slice
    df = torch.zeros(n, 24, 40, 128, device=DEV)
    db = torch.zeros(n, 24, 40, 128, device=DEV, dtype=torch.bfloat16)
    hip.resize_bilinear_ac(G(x.float()), df, n, Hh, Ww, C, 24, 40, 128, 32)
    hip.resize_bilinear_ac(G(x), db, n, Hh, Ww, C, 24, 40, 128, 32)
    torch.cuda.synchronize()
    assert torch.equal(df.to(torch.bfloat16), db)


def test_split_bf16(hip):
    x = torch.randn(4096) * 3
    hi = torch.empty(4096, device=DEV, dtype=torch.int16)
    lo = torch.empty(4096, device=DEV, dtype=torch.int16)
    hip.split_bf16(G(x), hi, lo, 4096)
    h = x.to(torch.bfloat16)
    assert torch.equal(hi.cpu().view(torch.bfloat16), h)
    assert torch.equal(lo.cpu().view(torch.bfloat16), (x - h.float()).to(torch.bfloat16))


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("M,N,K", [(1000, 864, 256), (130, 96, 128), (12288, 576, 256)])
def test_ln_gemm_bf16(hip, M, N, K, affine, prec):
    g = torch.Generator().manual_seed(M + N)
    A = torch.randn(M, K, generator=g) * 2 + 0.5
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    lw = torch.randn(K, generator=g) if affine else None
    lb = torch.randn(K, generator=g) if affine else None
    ref = F.layer_norm(A.double(), (K,), lw.double() if affine else None, lb.double() if affine else None, 1e-5) @ W.double().t() + b.double()
    Wp = G(pad_w(W))
    hi, lo = split(hip, Wp, prec == "bf16x3")
    C = torch.empty(M, N, device=DEV)
    hip.ln_gemm_bf16(G(A), K, G(lw) if affine else None, G(lb) if affine else None, 1e-5, hi, lo, Wp.shape[1], G(b), None, 0, C, N, M, N, K, 0)
    torch.cuda.synchronize()
    assert rel_err(C, ref) < PREC_TOL[prec]


@pytest.mark.parametrize("M,with_att,n_next", [(768, True, 2), (1000, True, 1), (12288, True, 2), (130, False, 0), (128, True, 0)])
def test_block_fused_bf16(hip, M, with_att, n_next):
    g = torch.Generator().manual_seed(M + n_next)
    C, H, Ko = 256, 1024, 288
    bf = lambda t: t.to(torch.bfloat16).double()
    x = torch.randn(M, C, generator=g) * 1.5 + 0.2
    att = torch.randn(M, Ko, generator=g)
    Wo, bo = torch.randn(C, Ko, generator=g) / 17, torch.randn(C, generator=g) * 0.1
    W1, b1 = torch.randn(H, C, generator=g) / 16, torch.randn(H, generator=g) * 0.1
    W2, b2 = torch.randn(C, H, generator=g) / 32, torch.randn(C, generator=g) * 0.1
    Ns = [576, 864][:n_next]
    Wn = [torch.randn(N, C, generator=g) / 16 for N in Ns]
    bn = [torch.randn(N, generator=g) * 0.1 for N in Ns]
    lnw, lnb = torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.1
    # reference (bf16 operands where the kernel rounds them, fp64 accumulation)
    xr = x.double()
    if with_att:
        xr = xr + bf(att) @ bf(Wo).t() + bo.double()
    hid = F.gelu(bf(F.layer_norm(xr, (C,), None, None, 1e-6).float()) @ bf(W1).t() + b1.double(), approximate="tanh")
    xr = xr + bf(hid.float()) @ bf(W2).t() + b2.double()
    yr = []
    for i, N in enumerate(Ns):
        ln = F.layer_norm(xr, (C,), lnw.double(), lnb.double(), 1e-5) if i == 0 else F.layer_norm(xr, (C,), None, None, 1e-6)
        yr.append(bf(ln.float()) @ bf(Wn[i]).t() + bn[i].double())
    xg, ys = G(x), [torch.full((M, N + 4), 3.0, device=DEV) for N in Ns]
    def hw(w):
        hi = split(hip, G(pad_w(w)), False)[0]
        fr = torch.empty((w.shape[0] + 31) // 32 * 32 * w.shape[1], device=DEV, dtype=torch.int16)
        hip.pack_frag_bf16(hi, hi.shape[1], w.shape[0], w.shape[1], fr)
        return fr

    who, wh1, wh2, whn = hw(Wo), hw(W1), hw(W2), [hw(w) for w in Wn]
    nexts = []
    for i, N in enumerate(Ns):
        d = dict(w=whn[i], ldw=C, b=G(bn[i]), N=N, y=ys[i], ldy=N + 4, eps=1e-5 if i == 0 else 1e-6)
        if i == 0:
            d.update(lnw=G(lnw), lnb=G(lnb))
        nexts.append(d)
    hip.block_fused_bf16(xg, C, G(att) if with_att else None, Ko, Ko, who, Ko, G(bo), wh1, C, G(b1), wh2, H, G(b2), H, nexts, M, C)
    torch.cuda.synchronize()
    assert rel_err(xg, xr) < 3e-3
    for i, N in enumerate(Ns):
        assert rel_err(ys[i][:, :N], yr[i]) < 6e-3
        assert bool((ys[i][:, N:] == 3.0).all())


@pytest.mark.parametrize("M,n_next", [(768, 2), (1000, 1), (50, 0), (768, 3)])
def test_block_fused_split_path(hip, M, n_next):
    """The two-launch path for small M (chunks of the MLP / column slices over separate workgroups) against the one-workgroup
    kernel: x and every projection agree to fp32 summation order (the partial fc2 sums are added in a different order)."""
    g = torch.Generator().manual_seed(M + n_next)
    C, H, Ko = 256, 1024, 288
    x = torch.randn(M, C, generator=g)
    att = torch.randn(M, Ko, generator=g)

    def hw(nn_, k):
        w = torch.randn(nn_, k, generator=g) / math.sqrt(k)
        hi = split(hip, G(pad_w(w)), False)[0]
        fr = torch.empty((nn_ + 31) // 32 * 32 * k, device=DEV, dtype=torch.int16)
        hip.pack_frag_bf16(hi, hi.shape[1], nn_, k, fr)
        return fr

    who, wh1, wh2 = hw(C, Ko), hw(H, C), hw(C, H)
    bo, b1, b2 = (G(torch.randn(k_, generator=g) * 0.1) for k_ in (C, H, C))
    Ns = [576, 864, 288][:n_next]
    wn = [hw(N, C) for N in Ns]
    bn = [G(torch.randn(N, generator=g) * 0.1) for N in Ns]
    lnw, lnb = G(torch.randn(C, generator=g) * 0.3 + 1), G(torch.randn(C, generator=g) * 0.1)
    res = []
    for ws in (None, torch.full((5 * M * C,), float("nan"), device=DEV)):
        xg = G(x)
        ys = [torch.full((M, N), 5.0, device=DEV) for N in Ns]
        nexts = [dict(w=wn[i], ldw=C, b=bn[i], N=N, y=ys[i], ldy=N, eps=1e-5 if i == 0 else 1e-6, **(dict(lnw=lnw, lnb=lnb) if i == 0 else {}),
                      **(dict(rows=(32, M - 7)) if i == 2 else {})) for i, N in enumerate(Ns)]
        hip.block_fused_bf16(xg, C, G(att), Ko, Ko, who, Ko, bo, wh1, C, b1, wh2, H, b2, H, nexts, M, C, ws=ws)
        torch.cuda.synchronize()
        res.append((xg, ys))
    assert rel_err(res[1][0], res[0][0].double().cpu()) < 1e-6
    for a, b in zip(res[0][1], res[1][1]):
        assert rel_err(b, a.double().cpu()) < 2e-3  # LayerNorm output is re-rounded to bf16: one-ulp flips of single operands
        assert torch.equal(a == 5.0, b == 5.0)


@pytest.mark.parametrize("M", [13056, 100])
def test_ln_proj_bf16(hip, M):
    g = torch.Generator().manual_seed(M)
    C, N = 256, 864
    bf = lambda t: t.to(torch.bfloat16).double()
    x = torch.randn(M, C, generator=g) * 1.3 + 0.1
    w = torch.randn(N, C, generator=g) / 16
    b = torch.randn(N, generator=g) * 0.1
    hi = split(hip, G(pad_w(w)), False)[0]
    fr = torch.empty((N + 31) // 32 * 32 * C, device=DEV, dtype=torch.int16)
    hip.pack_frag_bf16(hi, hi.shape[1], N, C, fr)
    xg = G(x)
    for dt, tol in ((torch.float32, 6e-3), (torch.bfloat16, 1.2e-2)):
        y = torch.full((M, N), 3.0, device=DEV, dtype=dt)
        hip.ln_proj_bf16(xg, C, [dict(w=fr, ldw=C, b=G(b), N=N, y=y, ldy=N, eps=1e-6)], M, C)
        torch.cuda.synchronize()
        ref = bf(F.layer_norm(x.double(), (C,), None, None, 1e-6).float()) @ bf(w).t() + b.double()
        assert rel_err(y.float(), ref) < tol
    assert torch.equal(xg.cpu(), x)  # x is only read


@pytest.mark.parametrize("M,cut", [(13056, 12288), (1000, 333), (200, 0)])
def test_block_fused_row_ranges(hip, M, cut):
    """Three follow-up projections restricted to row ranges (one launch over point + virtual rows): rows outside a range
    keep their old contents, rows inside equal the unrestricted result bit for bit."""
    g = torch.Generator().manual_seed(M)
    C, H, Ko = 256, 1024, 288
    x = torch.randn(M, C, generator=g)
    att = torch.randn(M, Ko, generator=g)

    def hw(n, k):
        w = torch.randn(n, k, generator=g) / math.sqrt(k)
        hi = split_(w)
        fr = torch.empty((n + 31) // 32 * 32 * k, device=DEV, dtype=torch.int16)
        hip.pack_frag_bf16(hi, hi.shape[1], n, k, fr)
        return fr

    split_ = lambda w: split(hip, G(pad_w(w)), False)[0]
    who, wh1, wh2 = hw(C, Ko), hw(H, C), hw(C, H)
    bo, b1, b2 = G(torch.randn(C, generator=g)), G(torch.randn(H, generator=g)), G(torch.randn(C, generator=g))
    Ns = [576, 288, 288]
    wn = [hw(N, C) for N in Ns]
    bn = [G(torch.randn(N, generator=g)) for N in Ns]
    ranges = [(0, cut), (0, cut), (cut, M)] if cut else [(0, M), (0, 0), (5, 70)]

    def run(restrict):
        xg = G(x)
        ys = [torch.full((M, N), 7.0, device=DEV) for N in Ns]
        nexts = [dict(w=wn[i], ldw=C, b=bn[i], N=N, y=ys[i], ldy=N, eps=1e-6, rows=ranges[i] if restrict else (0, 0))
                 for i, N in enumerate(Ns)]
        hip.block_fused_bf16(xg, C, G(att), Ko, Ko, who, Ko, bo, wh1, C, b1, wh2, H, b2, H, nexts, M, C)
        torch.cuda.synchronize()
        return xg, ys

    xf, yf = run(False)
    xr, yr = run(True)
    assert torch.equal(xf, xr)
    for i, (lo, hi) in enumerate(ranges):
        hi = hi or M
        assert torch.equal(yr[i][lo:hi], yf[i][lo:hi])
        assert bool((yr[i][:lo] == 7.0).all()) and bool((yr[i][hi:] == 7.0).all())


@pytest.mark.parametrize("M", [128, 1000, 13056])
def test_mlp_fused_bf16(hip, M):
    g = torch.Generator().manual_seed(M)
    C, H = 256, 1024
    x = torch.randn(M, C, generator=g) * 2 + 0.3
    W1 = torch.randn(H, C, generator=g) / 16
    b1 = torch.randn(H, generator=g) * 0.1
    W2 = torch.randn(C, H, generator=g) / 32
    b2 = torch.randn(C, generator=g) * 0.1
    h1, _ = split(hip, G(W1), False)
    h2, _ = split(hip, G(W2), False)
    xg = G(x)
    hip.mlp_fused_bf16(xg, C, h1, C, G(b1), h2, H, G(b2), M, C, H, 1e-6)
    torch.cuda.synchronize()
    bf = lambda t: t.to(torch.bfloat16).double()
    ln = F.layer_norm(x.double(), (C,), None, None, 1e-6)
    hid = F.gelu(bf(ln.float()) @ bf(W1).t() + b1.double(), approximate="tanh")
    ref = x.double() + bf(hid.float()) @ bf(W2).t() + b2.double()
    assert rel_err(xg, ref) < 2e-3  # bf16 operands; the hidden tile is re-rounded to bf16 between the two GEMMs
    exact = x.double() + F.gelu(ln @ W1.double().t() + b1.double(), approximate="tanh") @ W2.double().t() + b2.double()
    assert rel_err(xg, exact) < 2e-2


def test_conv2d_rejects_bad_args(hip):
    x = torch.zeros(1, 8, 8, 48, device=DEV)
    with pytest.raises(hip.HipError):
        hip.conv2d(x, x, None, x, 1, 8, 8, 48, 16, 3, 3, 1, 1, 16)  # Cin % 32 != 0


# ----------------------------------------------------------------------------------------- encoder-side kernels
def test_rgb_to_nhwc4(hip):
    V, Tn, H, W = 2, 5, 12, 20
    rgb = torch.randint(0, 256, (V, Tn, 3, H, W)).float()
    out = torch.empty(3, V, H, W, 4, device=DEV)
    hip.rgb_to_nhwc4(G(rgb), out, V, Tn, H, W, 1, 3)
    ref = (2 * (rgb[:, 1:4] / 255.0) - 1.0).permute(1, 0, 3, 4, 2)
    assert torch.equal(out[..., :3].cpu(), ref) and float(out[..., 3].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [(480, 640, 384, 512), (37, 53, 64, 96), (128, 128, 128, 128)])
def test_resize_nearest(hip, shape):
    Hi, Wi, Ho, Wo = shape
    x = torch.randn(6, Hi, Wi)
    out = torch.empty(6, Ho, Wo, device=DEV)
    hip.resize_nearest(G(x), out, 6, Hi, Wi, Ho, Wo)
    assert torch.equal(out.cpu(), F.interpolate(x[None], (Ho, Wo), mode="nearest")[0])


@pytest.mark.parametrize("C,HW", [(64, 32 * 48), (96, 16 * 24), (128, 999), (256, 64)])
def test_instnorm(hip, C, HW):
    n = 3
    x = torch.randn(n, HW, C) * 2 + 0.5
    skip = torch.randn(n, HW, C)
    xg = G(x)
    partial = torch.empty(n * hip.IN_SLABS * C * 2, device=DEV, dtype=torch.float64)
    st = torch.empty(n, C, 2, device=DEV)
    hip.instnorm_stats(xg, C, partial, st, n, HW, C)
    y = torch.empty_like(xg)
    hip.instnorm_apply(xg, st, None, None, y, n, HW, C)
    ref = F.relu(F.instance_norm(x.permute(0, 2, 1).double(), eps=1e-5)).permute(0, 2, 1)
    assert (y.cpu().double() - ref).abs().max() < 1e-5
    hip.instnorm_apply(xg, st, G(skip), None, y, n, HW, C)
    assert (y.cpu().double() - F.relu(skip.double() + ref)).abs().max() < 1e-5
    hip.instnorm_apply(xg, st, G(skip), st, y, n, HW, C)  # skip normalised with (here: the same) statistics
    sk = (skip.double() - st.cpu()[:, None, :, 0].double()) * st.cpu()[:, None, :, 1].double()
    assert (y.cpu().double() - F.relu(sk + ref)).abs().max() < 1e-4
    hip.instnorm_apply(xg, st, G(skip), st, y, n, HW, C, skip_relu=True)  # the skip is a raw conv output: relu(IN(skip))
    assert (y.cpu().double() - F.relu(F.relu(sk) + ref)).abs().max() < 1e-4


@pytest.mark.parametrize("Hs,Ws,Hd,Wd", [(32, 48, 16, 24), (8, 12, 16, 24), (16, 24, 16, 24), (4, 6, 16, 24)])
def test_resize_bilinear_ac(hip, Hs, Ws, Hd, Wd):
    n, C = 2, 64
    x = torch.randn(n, C, Hs, Ws)
    dst = torch.zeros(n, Hd, Wd, 160, device=DEV)
    hip.resize_bilinear_ac(G(x.permute(0, 2, 3, 1)), dst, n, Hs, Ws, C, Hd, Wd, 160, 32)
    ref = F.interpolate(x, (Hd, Wd), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert (dst[..., 32:96].cpu() - ref).abs().max() < 1e-5
    assert float(dst[..., :32].abs().max()) == 0 and float(dst[..., 96:].abs().max()) == 0


# ----------------------------------------------------------------------------------------- frame store
def test_frame_store_kernels(hip, golden):
    g = golden("pyramid_small")
    fm, ds_ref = T(g["fmaps"]), T(g["depths_strided"])  # (1,2,3,8,16,16), (1,2,3,1,16,16)
    V, Tn, C = 2, 3, 8
    clip = synth.make_clip(int(g["clip_seed"]), V=2, T=3, H=64, W=64, N=4, invalid_frac=0.02)
    ds = torch.empty(Tn, V, 16, 16, device=DEV)
    hip.depth_subsample(G(clip["depths"][0]), ds, V, Tn, 64, 64, 4)
    assert torch.equal(ds.cpu(), ds_ref[0, :, :, 0].permute(1, 0, 2, 3))
    kinv = torch.empty(V * Tn, 9, device=DEV)
    einv = torch.empty(V * Tn, 12, device=DEV)
    hip.invert_cameras(G(g["intrs"]).reshape(-1, 9), G(g["extrs"]).reshape(-1, 12), kinv, einv, V * Tn)
    f = G(fm[0].permute(1, 0, 3, 4, 2))  # (T,V,h,w,C)
    h = 16
    for lvl in range(3):
        if lvl > 0:
            nxt = torch.empty(Tn, V, h // 2, h // 2, C, device=DEV)
            hip.avgpool2(f, nxt, Tn * V, h, h, C)
            f, h = nxt, h // 2
        xyz = torch.empty(Tn, V, h, h, 4, device=DEV)
        hip.unproject(ds, kinv, einv, xyz, V, Tn, 16, 16, 4, lvl)
        torch.cuda.synchronize()
        assert np.abs(xyz[..., :3].reshape(Tn, -1, 3).cpu().numpy() - g[f"xyz{lvl}"]).max() < 2e-5
        assert np.abs(f.reshape(Tn, -1, C).cpu().numpy() - g[f"fvec{lvl}"]).max() < 1e-6


# ----------------------------------------------------------------------------------------- kNN + correlation
def _run_corr(hip, xyz, fvec, targets, coords, K, nseg, seed=None):
    B, P, C = fvec.shape
    M = targets.shape[1]
    x4 = torch.zeros(B, P, 4)
    x4[..., :3] = xyz
    # library layout: tracks major -> use N = M, S = B (slot s reads frame s)
    tg = G(targets.permute(1, 0, 2))
    cd = G(coords.permute(1, 0, 2))
    x4g, fg = G(x4), G(fvec)
    keys = torch.empty(M * B * nseg * K, device=DEV, dtype=torch.int64)
    hip.knn_scan(x4g, P, cd, M, B, 0, 1, B, K, nseg, keys, **(seed or {}))
    idx = torch.empty(M, B, K, device=DEV, dtype=torch.int32)
    hip.knn_merge(keys, M, B, K, nseg, P, idx)
    out = torch.zeros(M, B, K * 4, device=DEV)
    hip.corr_gather_dot([x4g], [fg], [P], [idx], C, tg, cd, M, B, 0, 1, B, K, out, K * 4, 0)
    torch.cuda.synchronize()
    return out.reshape(M, B, K, 4).permute(1, 0, 2, 3).cpu(), idx.permute(1, 0, 2).cpu().long(), keys


def test_corr_sample_golden(hip, golden):
    g = golden("corr_sample_small")
    out, idx, _ = _run_corr(hip, T(g["xyz"]), T(g["fvec"]), T(g["targets"]), T(g["coords"]), 16, 1)
    assert np.array_equal(idx.numpy(), g["idx_exact"])  # integer indices bit-exact vs the reference
    assert np.abs(out.numpy() - g["out_exact"]).max() < 2e-5


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("G_,off,xyz_", [(4, True, True), (2, False, False), (1, True, True), (16, True, False), (1, False, True)])
def test_corr_gather_dot_options(hip, golden, bf, G_, off, xyz_):
    """mvt_corr_gather_dot_opts: grouped dots / no offsets / neighbour coordinates (mvtracker.py:832-846) against the oracle on random
    clouds, fp32 and bf16 rows; the (k = 8, 4 groups, offsets + coordinates) case additionally against the reference fixture."""
    g = torch.Generator().manual_seed(100 + G_)
    B, P, M, K, C = 2, 3000, 37, 16, 128
    xyz = torch.rand(B, P, 3, generator=g) * 2 - 1
    fvec = torch.randn(B, P, C, generator=g)
    if bf:
        fvec = fvec.bfloat16().float()
    tg, cd = torch.randn(B, M, C, generator=g), torch.rand(B, M, 3, generator=g) * 2 - 1
    ref, ridx = O.corr_sample(xyz, fvec, tg, cd, K, G_, off, xyz_, "exact", return_idx=True)
    x4 = torch.zeros(B, P, 4)
    x4[..., :3] = xyz
    OW = G_ + 3 * off + 3 * xyz_
    out = torch.zeros(M, B, 2 + K * OW, device=DEV)
    hip.corr_gather_dot_opts([G(x4)], [G(fvec.bfloat16() if bf else fvec)], [P], [G(ridx.permute(1, 0, 2).int())], C, G(tg.permute(1, 0, 2)),
                             G(cd.permute(1, 0, 2)), M, B, 0, 1, B, K, G_, off, xyz_, out, 2 + K * OW, 2)
    torch.cuda.synchronize()
    assert float(out[..., :2].abs().max()) == 0.0
    got = out[..., 2:].reshape(M, B, K, OW).permute(1, 0, 2, 3).cpu()
    assert (got - ref).abs().max() < 2e-5
    if (G_, off, xyz_) == (4, True, True) and not bf:
        gg = golden("corr_sample_small")
        xyz, fvec, tg, cd = T(gg["xyz"]), T(gg["fvec"]), T(gg["targets"]), T(gg["coords"])
        B, P, C = fvec.shape
        M = tg.shape[1]
        _, ridx = O.corr_sample(xyz, fvec, tg, cd, 8, 4, True, True, "exact", return_idx=True)
        x4 = torch.zeros(B, P, 4)
        x4[..., :3] = xyz
        out = torch.zeros(M, B, 8 * 10, device=DEV)
        hip.corr_gather_dot_opts([G(x4)], [G(fvec)], [P], [G(ridx.permute(1, 0, 2).int())], C, G(tg.permute(1, 0, 2)), G(cd.permute(1, 0, 2)), M, B,
                                 0, 1, B, 8, 4, True, True, out, 80, 0)
        torch.cuda.synchronize()
        assert np.abs(out.reshape(M, B, 8, 10).permute(1, 0, 2, 3).cpu().numpy() - gg["out_exact_k8_g4_xyz"]).max() < 2e-5


@pytest.mark.parametrize("P,K,nseg,M", [(20000, 16, 2, 37), (65536, 16, 4, 16), (5000, 1, 1, 20), (40000, 1, 4, 9), (16, 16, 1, 5),
                                        (1000, 8, 1, 64)])
def test_knn_exact_vs_oracle(hip, P, K, nseg, M):
    g = torch.Generator().manual_seed(P + K)
    B, C = 2, 128
    xyz = torch.rand(B, P, 3, generator=g) * 4 - 2
    fvec = torch.randn(B, P, C, generator=g)
    tg = torch.randn(B, M, C, generator=g)
    cd = torch.rand(B, M, 3, generator=g) * 4 - 2
    out, idx, keys = _run_corr(hip, xyz, fvec, tg, cd, K, nseg)
    ref, ridx = O.corr_sample(xyz, fvec, tg, cd, K, 1, True, False, "exact", return_idx=True)
    assert torch.equal(idx, ridx)
    assert (out - ref).abs().max() < 2e-5
    kv = keys.reshape(M, B, nseg, K).cpu()
    assert bool((kv[..., 1:] > kv[..., :-1]).all())  # every per-segment list strictly ascending (sortedness)


def test_knn_seeded_scan_is_exact(hip):
    """A seed only prunes: neighbours of moved queries, seeded with the neighbours of the old positions
    (same level) or with the coarser level's neighbours, equal the unseeded oracle result bit for bit."""
    g = torch.Generator().manual_seed(11)
    V, h, w, K, M, B = 2, 32, 48, 16, 40, 3
    P = V * h * w
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    base = torch.stack([xs * 0.05, ys * 0.05, torch.zeros_like(xs)], -1).reshape(1, 1, h * w, 3)
    xyz = (base + torch.rand(B, V, h * w, 3, generator=g) * 0.02 + torch.arange(V).view(1, V, 1, 1) * 0.013).reshape(B, P, 3)
    q0 = torch.rand(B, M, 3, generator=g) * torch.tensor([2.0, 1.4, 0.02])
    fv, tg = torch.randn(B, P, 128, generator=g), torch.randn(B, M, 128, generator=g)
    _, idx0, _ = _run_corr(hip, xyz, fv, tg, q0, K, 2)
    q1 = q0 + torch.randn(B, M, 3, generator=g) * 0.01
    seed0 = G(idx0.permute(1, 0, 2).int())
    out1, idx1, _ = _run_corr(hip, xyz, fv, tg, q1, K, 2, seed=dict(seed_idx=seed0, seed_k=K))
    ref_out, ref = O.corr_sample(xyz, fv, tg, q1, K, 1, True, False, "exact", return_idx=True)
    assert torch.equal(idx1, ref) and (out1 - ref_out).abs().max() < 2e-5
    # coarse level = every second pixel of the same grid; its neighbours seed the fine scan
    hc, wc = h // 2, w // 2
    xc = xyz.reshape(B, V, h, w, 3)[:, :, ::2, ::2].reshape(B, V * hc * wc, 3)
    _, idxc, _ = _run_corr(hip, xc, fv[:, :V * hc * wc], tg, q1, K, 1)
    seedc = G(idxc.permute(1, 0, 2).int())
    _, idx2, _ = _run_corr(hip, xyz, fv, tg, q1, K, 2, seed=dict(seed_idx=seedc, seed_k=K, seed_dims=(wc, hc, w, h)))
    assert torch.equal(idx2, ref)


@pytest.mark.parametrize("patch", [False, True])
@pytest.mark.parametrize("nseg", [1, 3])
def test_knn_tile_culling_is_exact(hip, patch, nseg):
    """Bounding-box culling (linear and 8x8-patch tiles), with and without a seed, with NaN points and NaN / far queries:
    neighbour indices equal the oracle's bit for bit."""
    g = torch.Generator().manual_seed(21 + nseg)
    V, h, w, K, M, B = 3, 24, 40, 16, 45, 2
    P = V * h * w
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    base = torch.stack([xs * 0.05, ys * 0.05, 0.3 * torch.sin(xs * 0.2) + 0.1 * ys], -1).reshape(1, 1, h * w, 3)
    xyz = (base + torch.rand(B, V, h * w, 3, generator=g) * 0.02 + torch.arange(V).view(1, V, 1, 1) * 0.017).reshape(B, P, 3)
    xyz[0, 100:180] = float("nan")        # invalid points, including one whole linear tile (128..191 partially) ...
    xyz[1, 64 * 5:64 * 6] = float("nan")  # ... and exactly one all-NaN linear tile
    q = torch.rand(B, M, 3, generator=g) * torch.tensor([2.0, 1.2, 2.5])
    q[:, 0] = torch.tensor([50.0, -30.0, 9.0])  # far outside every box
    x4 = torch.zeros(B, P, 4)
    x4[..., :3] = xyz
    x4g, cd = G(x4), G(q.permute(1, 0, 2))
    grid = (w, h) if patch else (0, 0)
    box = torch.empty(B, (P + 63) // 64, 8, device=DEV)
    hip.tile_aabb(x4g, P, B, box, grid)
    torch.cuda.synchronize()
    if not patch:  # boxes against a direct evaluation
        t = xyz[:, :(P // 64) * 64].reshape(B, P // 64, 64, 3)
        lo = torch.where(torch.isnan(t), torch.full_like(t, float("inf")), t).amin(2)
        hi = torch.where(torch.isnan(t), torch.full_like(t, float("-inf")), t).amax(2)
        assert torch.equal(box[:, :P // 64, 0:3].cpu(), lo) and torch.equal(box[:, :P // 64, 4:7].cpu(), hi)
    _, ref = O.knn_exact(K, torch.where(torch.isnan(xyz), torch.full_like(xyz, 1e18), xyz), q)

    def run(**kw):
        keys = torch.empty(M * B * nseg * K, device=DEV, dtype=torch.int64)
        hip.knn_scan(x4g, P, cd, M, B, 0, 1, B, K, nseg, keys, box=box, grid=grid, **kw)
        idx = torch.empty(M, B, K, device=DEV, dtype=torch.int32)
        hip.knn_merge(keys, M, B, K, nseg, P, idx)
        torch.cuda.synchronize()
        return idx

    idx = run()
    assert torch.equal(idx.permute(1, 0, 2).cpu().long(), ref)
    q2 = q + torch.randn(B, M, 3, generator=g) * 0.01
    cd = G(q2.permute(1, 0, 2))
    _, ref2 = O.knn_exact(K, torch.where(torch.isnan(xyz), torch.full_like(xyz, 1e18), xyz), q2)
    idx2 = run(seed_idx=idx, seed_k=K)
    assert torch.equal(idx2.permute(1, 0, 2).cpu().long(), ref2)
    # single-wave search (scan + merge in one launch), with and without the coarse group boxes
    gbox = torch.empty(B, ((P + 63) // 64 + 63) // 64, 8, device=DEV)
    hip.tile_group_aabb(box, P, B, gbox)
    torch.cuda.synchronize()
    nt = (P + 63) // 64
    bc = box.cpu()
    for gi in range(gbox.shape[1]):
        assert torch.equal(gbox[:, gi, 0:3].cpu(), bc[:, 64 * gi:64 * gi + 64, 0:3].amin(1))
        assert torch.equal(gbox[:, gi, 4:7].cpu(), bc[:, 64 * gi:64 * gi + 64, 4:7].amax(1))
    for gb in (None, gbox):
        for kw, want in ((dict(), ref2), (dict(seed_idx=idx, seed_k=K), ref2)):
            out = torch.empty(M, B, K, device=DEV, dtype=torch.int32)
            hip.knn_search(x4g, P, cd, M, B, 0, 1, B, K, out, box, grid=grid, gbox=gb, **kw)
            torch.cuda.synchronize()
            assert torch.equal(out.permute(1, 0, 2).cpu().long(), want)


@pytest.mark.parametrize("invalid", [False, True])
def test_knn_search_group_boxes_c3_scale(hip, invalid):
    """The single-wave search at the scale the benchmark runs it: V*h*w = 4*128*128 points = 1 024 8x8-patch tiles in 16 group
    boxes.  Unseeded, seeded with the neighbours of the previous positions (tight bound), and seeded with K arbitrary distinct
    points (a valid but very loose bound: hundreds of survivors, the radix-select path): indices equal the oracle's bit for bit.
    ``invalid``: 2 % of the points collapsed onto one location (zero depth unprojects to the camera centre) plus NaN points."""
    g = torch.Generator().manual_seed(77 + int(invalid))
    V, h, w, K, M, B = 4, 128, 128, 16, 96, 2
    P = V * h * w
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    views = []
    for v in range(V):  # four overlapping, slightly rotated sheets of one smooth surface (what fused multi-view depth looks like)
        ang = 0.1 * v
        x_ = xs * 0.02 * np.cos(ang) - ys * 0.02 * np.sin(ang) + 0.1 * v
        y_ = xs * 0.02 * np.sin(ang) + ys * 0.02 * np.cos(ang)
        z_ = 0.3 * torch.sin(x_ * 2.0) + 0.2 * torch.cos(y_ * 3.0)
        views.append(torch.stack([x_, y_, z_], -1).reshape(h * w, 3))
    base = torch.stack(views, 0)[None].repeat(B, 1, 1, 1)
    xyz = (base + (torch.rand(B, V, h * w, 3, generator=g) - 0.5) * 0.02).reshape(B, P, 3)
    if invalid:
        bad = torch.rand(B, P, generator=g) < 0.02
        xyz[bad] = torch.tensor([0.5, 0.5, -3.0])
        xyz[0, 5000:5100] = float("nan")
    pick = torch.randint(0, P, (B, M), generator=g)
    q = torch.gather(torch.nan_to_num(xyz, nan=0.0), 1, pick[..., None].expand(B, M, 3)) + torch.randn(B, M, 3, generator=g) * 0.01
    q[:, 0] = torch.tensor([9.0, -7.0, 3.0])   # far outside every box
    if invalid:
        q[:, 1] = torch.tensor([0.5, 0.5, -3.0])  # exactly on the collapsed cluster: > K equidistant candidates, lowest indices win
    x4 = torch.zeros(B, P, 4)
    x4[..., :3] = xyz
    x4g = G(x4)
    box = torch.empty(B, P // 64, 8, device=DEV)
    hip.tile_aabb(x4g, P, B, box, (w, h))
    gbox = torch.empty(B, P // 64 // 64, 8, device=DEV)
    hip.tile_group_aabb(box, P, B, gbox)
    assert gbox.shape[1] == 16
    clean = torch.where(torch.isnan(xyz), torch.full_like(xyz, 1e18), xyz)

    def search(qq, **kw):
        out = torch.empty(M, B, K, device=DEV, dtype=torch.int32)
        hip.knn_search(x4g, P, G(qq.permute(1, 0, 2)), M, B, 0, 1, B, K, out, box, grid=(w, h), gbox=gbox, **kw)
        torch.cuda.synchronize()
        return out

    _, ref = O.knn_exact(K, clean, q)
    idx = search(q)
    assert torch.equal(idx.permute(1, 0, 2).cpu().long(), ref)
    q2 = q + torch.randn(B, M, 3, generator=g) * 0.004
    _, ref2 = O.knn_exact(K, clean, q2)
    assert torch.equal(search(q2, seed_idx=idx, seed_k=K).permute(1, 0, 2).cpu().long(), ref2)
    loose = torch.stack([torch.randperm(P, generator=g)[:K] for _ in range(M * B)]).reshape(M, B, K).int()
    if invalid:  # a NaN seed point must not poison the bound
        loose[:, 0, 3] = 5050
    assert torch.equal(search(q2, seed_idx=G(loose), seed_k=K).permute(1, 0, 2).cpu().long(), ref2)
    # the all-levels launch, in place (idx_out aliases seed_idx), as MVTracker._refine issues it
    inpl = idx.clone()
    hip.knn_search_levels([dict(xyz=x4g, P=P, seed_idx=inpl, box=box, grid=(w, h), idx_out=inpl, gbox=gbox)], G(q2.permute(1, 0, 2)), M, B, 0, 1, B,
                          K, seed_k=K)
    torch.cuda.synchronize()
    assert torch.equal(inpl.permute(1, 0, 2).cpu().long(), ref2)


def test_knn_levels_one_launch(hip):
    """mvt_knn_scan_levels / mvt_knn_merge_levels == the per-level calls (seeded and unseeded)."""
    g = torch.Generator().manual_seed(31)
    B, M, K = 2, 37, 16
    grids = [(16, 24), (8, 16), (8, 8)]
    V = 2
    clouds, boxes = [], []
    for (h, w) in grids:
        ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
        sc = 32.0 / w
        base = torch.stack([xs * 0.05 * sc, ys * 0.05 * sc, 0.2 * torch.sin(xs * 0.3)], -1).reshape(1, 1, h * w, 3)
        x = torch.zeros(B, V * h * w, 4)
        x[..., :3] = (base + torch.rand(B, V, h * w, 3, generator=g) * 0.02).reshape(B, V * h * w, 3)
        xg = G(x)
        bx = torch.empty(B, (V * h * w + 63) // 64, 8, device=DEV)
        hip.tile_aabb(xg, V * h * w, B, bx, (w, h))
        clouds.append(xg)
        boxes.append(bx)
    q = G((torch.rand(M, B, 3, generator=g) * torch.tensor([1.6, 0.8, 0.3])))
    nsegs = [2, 1, 1]

    def per_level(seeds):
        out = []
        for l, (h, w) in enumerate(grids):
            P = V * h * w
            keys = torch.empty(M * B * nsegs[l] * K, device=DEV, dtype=torch.int64)
            kw = dict(seed_idx=seeds[l], seed_k=K) if seeds else {}
            hip.knn_scan(clouds[l], P, q, M, B, 0, 1, B, K, nsegs[l], keys, box=boxes[l], grid=(w, h), **kw)
            idx = torch.empty(M, B, K, device=DEV, dtype=torch.int32)
            hip.knn_merge(keys, M, B, K, nsegs[l], P, idx)
            out.append(idx)
        return out

    def one_launch(seeds):
        lv = []
        for l, (h, w) in enumerate(grids):
            P = V * h * w
            lv.append(dict(xyz=clouds[l], P=P, keys=torch.empty(M * B * nsegs[l] * K, device=DEV, dtype=torch.int64), nseg=nsegs[l],
                           seed_idx=seeds[l] if seeds else None, box=boxes[l], grid=(w, h),
                           idx_out=torch.empty(M, B, K, device=DEV, dtype=torch.int32)))
        hip.knn_scan_levels(lv, q, M, B, 0, 1, B, K, seed_k=K if seeds else 0)
        hip.knn_merge_levels(lv, M, B, K)
        return [d["idx_out"] for d in lv]

    ref = per_level(None)
    got = one_launch(None)
    torch.cuda.synchronize()
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    q += 0.004
    ref2, got2 = per_level(ref), one_launch([r.clone() for r in ref])
    torch.cuda.synchronize()
    for a, b in zip(ref2, got2):
        assert torch.equal(a, b)
    # mvt_knn_search_levels: scan + merge in one launch, one wave per (track, slot), IN PLACE (idx_out aliases seed_idx)
    inpl = [r.clone() for r in ref]
    gbs = []
    for l, (h, w) in enumerate(grids):
        gb = torch.empty(B, ((V * h * w + 63) // 64 + 63) // 64, 8, device=DEV)
        hip.tile_group_aabb(boxes[l], V * h * w, B, gb)
        gbs.append(gb)
    lv = [dict(xyz=clouds[l], P=V * h * w, seed_idx=inpl[l], box=boxes[l], grid=(w, h), idx_out=inpl[l], gbox=gbs[l])
          for l, (h, w) in enumerate(grids)]
    hip.knn_search_levels(lv, q, M, B, 0, 1, B, K, seed_k=K)
    torch.cuda.synchronize()
    for a, b in zip(ref2, inpl):
        assert torch.equal(a, b)
    # ... and unseeded (seed_k = 0): the same neighbours again
    outs = [torch.empty(M, B, K, device=DEV, dtype=torch.int32) for _ in grids]
    lv = [dict(xyz=clouds[l], P=V * h * w, seed_idx=None, box=boxes[l], grid=(w, h), idx_out=outs[l], gbox=gbs[l]) for l, (h, w) in enumerate(grids)]
    hip.knn_search_levels(lv, q, M, B, 0, 1, B, K, seed_k=0)
    torch.cuda.synchronize()
    for a, b in zip(ref2, outs):
        assert torch.equal(a, b)


def test_corr_all_levels_one_launch(hip):
    g = torch.Generator().manual_seed(12)
    B, M, K, C = 2, 30, 16, 128
    Ps = [2000, 500, 130]
    xs = [torch.rand(B, P, 3, generator=g) for P in Ps]
    fs = [torch.randn(B, P, C, generator=g) for P in Ps]
    tg, cd = torch.randn(B, M, C, generator=g), torch.rand(B, M, 3, generator=g)
    x4 = []
    for x in xs:
        t = torch.zeros(B, x.shape[1], 4)
        t[..., :3] = x
        x4.append(G(t))
    fg = [G(f) for f in fs]
    tgg, cdg = G(tg.permute(1, 0, 2)), G(cd.permute(1, 0, 2))
    idx = []
    for x, P in zip(x4, Ps):
        keys = torch.empty(M * B * K, device=DEV, dtype=torch.int64)
        hip.knn_scan(x, P, cdg, M, B, 0, 1, B, K, 1, keys)
        i = torch.empty(M, B, K, device=DEV, dtype=torch.int32)
        hip.knn_merge(keys, M, B, K, 1, P, i)
        idx.append(i)
    out = torch.zeros(M, B, 5 + 3 * K * 4, device=DEV)
    hip.corr_gather_dot(x4, fg, Ps, idx, C, tgg, cdg, M, B, 0, 1, B, K, out, 5 + 3 * K * 4, 5)
    torch.cuda.synchronize()
    assert float(out[..., :5].abs().max()) == 0.0
    for l in range(3):
        ref = O.corr_sample(xs[l], fs[l], tg, cd, K, 1, True, False, "exact")
        got = out[..., 5 + l * K * 4:5 + (l + 1) * K * 4].reshape(M, B, K, 4).permute(1, 0, 2, 3).cpu()
        assert (got - ref).abs().max() < 2e-5


def test_knn_duplicate_points_tie_break(hip):
    # exact ties: the lower index must win (ordering by (d2, index))
    P, K = 300, 16
    xyz = torch.zeros(1, P, 3)
    xyz[0, :, 0] = torch.arange(P) // 4  # groups of four identical points
    fvec = torch.randn(1, P, 128)
    cd = torch.tensor([[[10.2, 0.0, 0.0]]])
    _, idx, _ = _run_corr(hip, xyz, fvec, torch.randn(1, 1, 128), cd, K, 1)
    _, ridx = O.corr_sample(xyz, fvec, torch.randn(1, 1, 128), cd, K, 1, True, False, "exact", return_idx=True)
    assert torch.equal(idx, ridx)


def test_knn1_gather(hip):
    g = torch.Generator().manual_seed(5)
    P, C, n, nseg = 30000, 128, 33, 3
    xyz = torch.zeros(2, P, 4)
    xyz[..., :3] = torch.rand(2, P, 3, generator=g)
    fvec = torch.randn(2, P, C, generator=g)
    q = torch.rand(n, 3, generator=g)
    keys = torch.empty(n * nseg, device=DEV, dtype=torch.int64)
    hip.knn_scan(G(xyz), P, G(q), n, 1, 1, 0, 2, 1, nseg, keys)
    feat = torch.empty(n, C, device=DEV)
    idx = torch.empty(n, device=DEV, dtype=torch.int32)
    hip.knn1_gather(G(fvec), P, C, keys, n, nseg, 1, feat, idx)
    _, ridx = O.knn_exact(1, xyz[1:2, :, :3], q[None])
    assert torch.equal(idx.cpu().long(), ridx[0, :, 0])
    assert torch.equal(feat.cpu(), fvec[1][ridx[0, :, 0]])


@pytest.mark.parametrize("r", [3, 4])
def test_window_corr(hip, golden, r):
    g = golden("window_corr_small")
    fm, tg, cd = T(g["fmaps"]), T(g["targets"]), T(g["coords"])  # (1,2,32,24,40), (1,2,10,32), (1,2,10,2)
    pyr = O.window_corr_pyramid(fm, 3)
    D = (2 * r + 1) ** 2
    out = torch.zeros(2, 10, 3 * D, device=DEV)
    for lvl, f in enumerate(pyr):
        h, w = f.shape[-2:]
        hip.window_corr(G(f[0].permute(0, 2, 3, 1)), G(tg[0]), G(cd[0]), out, 2, 10, 32, h, w, lvl, r, 3 * D, lvl * D)
    torch.cuda.synchronize()
    assert np.abs(out.cpu().numpy() - g[f"out_r{r}"][0]).max() < 2e-5


# ----------------------------------------------------------------------------------------- tokens
def test_pos_embed_and_tokens(hip, golden):
    g = golden("embeddings")
    c0 = T(g["coords0"]).reshape(-1, 3)
    n, S, D = c0.shape[0], 12, 581
    coords = c0[:, None, :].repeat(1, S, 1) + T(g["flows"][:1]).repeat(n, 1, 1) * torch.arange(n)[:, None, None]
    coords[:, 0] = c0
    pos = torch.empty(n, D, device=DEV)
    hip.pos_embed(G(coords), n, S, D, 582, pos)
    ref = g["pos_embed"].reshape(n, 582)[:, :D].astype(np.float32)
    assert np.abs(pos.cpu().numpy() - ref).max() < 1.5e-7
    cfg = O.TrackerConfig()
    gen = torch.Generator().manual_seed(1)
    fc = torch.randn(n, S, 256, generator=gen)
    ff = torch.randn(n, S, 128, generator=gen)
    mv = torch.randn(n, S, 2, generator=gen)
    p_o, te = O.window_embeddings(cfg, c0, S)
    x = torch.zeros(n * S, 584, device=DEV)
    hip.token_assemble(G(coords), G(fc), 256, G(ff), 128, G(mv), pos, G(te[0]), n, S, 64, x, 584)
    xo = O.assemble_tokens(cfg, coords.permute(1, 0, 2)[None], fc.permute(1, 0, 2)[None], ff.permute(1, 0, 2)[None], mv, p_o, te)
    d = (x[:, :D].cpu().reshape(n, S, D) - xo[0]).abs()
    assert d[..., 192:].max() < 1e-6
    assert d[..., :192].max() < 2e-4  # sin/cos of arguments up to ~1e3 rad: fp32 argument reduction differs
    assert float(x[:, D:].abs().max()) == 0.0


def test_layernorm(hip):
    x = torch.randn(1000, 256) * 3 + 1
    w, b = torch.randn(256), torch.randn(256)
    y = torch.empty(1000, 256, device=DEV)
    hip.layernorm(G(x), 256, None, None, y, 256, 1000, 256, 1e-6)
    assert (y.cpu() - F.layer_norm(x, (256,), None, None, 1e-6)).abs().max() < 1e-5
    hip.layernorm(G(x), 256, G(w), G(b), y, 256, 1000, 256, 1e-5)
    assert (y.cpu() - F.layer_norm(x, (256,), w, b, 1e-5)).abs().max() < 2e-5


@pytest.mark.parametrize("n", [50, 200, 1024])
@pytest.mark.parametrize("mode", ["time", "v2p", "vself", "p2v"])
def test_attention(hip, mode, n):
    g = torch.Generator().manual_seed(3)
    nv, S, H, dh = 64, 12, 6, 48
    inner = H * dh
    M = (n + nv) * S
    qkv = torch.randn(M, 3 * inner, generator=g)
    out = torch.zeros(M, inner, device=DEV)
    qg = G(qkv)
    tok = qkv.reshape(n + nv, S, 3, H, dh)
    Mp = n * S
    if mode == "time":
        hip.attention(qg, 3 * inner, S, 1, qg[:, inner:], qg[:, 2 * inner:], 3 * inner, S, 1, out, inner, n + nv, S, S, H, dh)
        q, k, v = (tok[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        ref = F.scaled_dot_product_attention(q.double(), k.double(), v.double()).permute(0, 2, 1, 3).reshape(M, inner)
        got = out.cpu()
    else:
        pq, vq = tok[:n], tok[n:]  # (n,S,3,H,dh): per frame t, items along dim 0
        if mode == "v2p":
            hip.attention(qg[Mp:], 3 * inner, 1, S, qg[:Mp, inner:], qg[:Mp, 2 * inner:], 3 * inner, 1, S, out[Mp:], inner, S, nv, n, H, dh)
            q, k, v = vq[:, :, 0], pq[:, :, 1], pq[:, :, 2]
            sl = slice(Mp, M)
        elif mode == "vself":
            hip.attention(qg[Mp:], 3 * inner, 1, S, qg[Mp:, inner:], qg[Mp:, 2 * inner:], 3 * inner, 1, S, out[Mp:], inner, S, nv, nv, H, dh)
            q, k, v = vq[:, :, 0], vq[:, :, 1], vq[:, :, 2]
            sl = slice(Mp, M)
        else:
            hip.attention(qg[:Mp], 3 * inner, 1, S, qg[Mp:, inner:], qg[Mp:, 2 * inner:], 3 * inner, 1, S, out[:Mp], inner, S, n, nv, H, dh)
            q, k, v = pq[:, :, 0], vq[:, :, 1], vq[:, :, 2]
            sl = slice(0, Mp)
        # (items, S, H, dh) -> (S, H, items, dh)
        q, k, v = (t.permute(1, 2, 0, 3).double() for t in (q, k, v))
        ref = F.scaled_dot_product_attention(q, k, v).permute(2, 0, 1, 3).reshape(-1, inner)
        got = out[sl].cpu()
    torch.cuda.synchronize()
    assert (got.double() - ref).abs().max() < 2e-6


@pytest.mark.parametrize("n", [50, 200, 1024])
@pytest.mark.parametrize("mode", ["v2p", "vself", "p2v"])
def test_attention_bf16(hip, mode, n):
    g = torch.Generator().manual_seed(4)
    nv, S, H, dh = 64, 12, 6, 48
    inner = H * dh
    M = (n + nv) * S
    Mp = n * S
    qkv = torch.randn(M, 3 * inner, generator=g)
    out = torch.zeros(M, inner, device=DEV)
    qg = G(qkv)
    tok = qkv.reshape(n + nv, S, 3, H, dh)
    pq, vq = tok[:n], tok[n:]
    if mode == "v2p":
        hip.attention_bf16(qg[Mp:], 3 * inner, 1, S, qg[:Mp, inner:], qg[:Mp, 2 * inner:], 3 * inner, 1, S, out[Mp:], inner, S, nv, n, H, dh)
        q, k, v, sl = vq[:, :, 0], pq[:, :, 1], pq[:, :, 2], slice(Mp, M)
    elif mode == "vself":
        hip.attention_bf16(qg[Mp:], 3 * inner, 1, S, qg[Mp:, inner:], qg[Mp:, 2 * inner:], 3 * inner, 1, S, out[Mp:], inner, S, nv, nv, H, dh)
        q, k, v, sl = vq[:, :, 0], vq[:, :, 1], vq[:, :, 2], slice(Mp, M)
    else:
        hip.attention_bf16(qg[:Mp], 3 * inner, 1, S, qg[Mp:, inner:], qg[Mp:, 2 * inner:], 3 * inner, 1, S, out[:Mp], inner, S, n, nv, H, dh)
        q, k, v, sl = pq[:, :, 0], vq[:, :, 1], vq[:, :, 2], slice(0, Mp)
    q, k, v = (t.permute(1, 2, 0, 3).double() for t in (q, k, v))
    ref = F.scaled_dot_product_attention(q, k, v).permute(2, 0, 1, 3).reshape(-1, inner)
    torch.cuda.synchronize()
    got = out[sl].cpu().double()
    assert (got - ref).abs().max() < 3e-2 and (got - ref).abs().mean() < 3e-3  # bf16 operands / probabilities


def test_updater_bf16_token_tensors(hip):
    """q/k/v, attention outputs and follow-up projections as bf16 tensors (bf16 mode) == the same kernels on fp32 tensors
    holding the bf16 values, outputs rounded to nearest even; also the 12-key time attention on the MFMA kernel."""
    g = torch.Generator().manual_seed(14)
    n, nv, S, H, dh = 40, 64, 12, 6, 48
    inner = H * dh
    M = (n + nv) * S
    Mp = n * S
    qkv_b = torch.randn(M, 3 * inner, generator=g).to(torch.bfloat16)
    qb, qf = G(qkv_b), G(qkv_b.float())
    for args_of in (lambda t, o: (t, 3 * inner, S, 1, t[:, inner:], t[:, 2 * inner:], 3 * inner, S, 1, o, inner, n + nv, S, S, H, dh),        # time
                    lambda t, o: (t[Mp:], 3 * inner, 1, S, t[:Mp, inner:], t[:Mp, 2 * inner:], 3 * inner, 1, S, o[Mp:], inner, S, nv, n, H, dh)):  # v2p
        of = torch.zeros(M, inner, device=DEV)
        ob = torch.zeros(M, inner, device=DEV, dtype=torch.bfloat16)
        hip.attention_bf16(*args_of(qf, of))
        hip.attention_bf16(*args_of(qb, ob))
        torch.cuda.synchronize()
        assert torch.equal(of.to(torch.bfloat16), ob)
    # key-split path (workspace given) of the virtual <- point attention: same result up to the merge order
    o1, o2 = torch.zeros(M, inner, device=DEV), torch.zeros(M, inner, device=DEV)
    n2 = 1024
    qkv2 = G(torch.randn((n2 + nv) * S, 3 * inner, generator=g))
    Mp2 = n2 * S
    o1, o2 = torch.zeros((n2 + nv) * S, inner, device=DEV), torch.zeros((n2 + nv) * S, inner, device=DEV)
    ws = torch.full((hip.attention_ws_floats(S, nv, H),), float("nan"), device=DEV)
    hip.attention_bf16(qkv2[Mp2:], 3 * inner, 1, S, qkv2[:Mp2, inner:], qkv2[:Mp2, 2 * inner:], 3 * inner, 1, S, o1[Mp2:], inner, S, nv, n2, H, dh)
    hip.attention_bf16(qkv2[Mp2:], 3 * inner, 1, S, qkv2[:Mp2, inner:], qkv2[:Mp2, 2 * inner:], 3 * inner, 1, S, o2[Mp2:], inner, S, nv, n2, H, dh,
                       ws=ws)
    torch.cuda.synchronize()
    assert (o1 - o2).abs().max() < 2e-3 and float(o2[Mp2:].abs().max()) > 0  # P is rounded to bf16 relative to a different running max
    # time attention against fp64 softmax attention
    of = torch.zeros(M, inner, device=DEV)
    hip.attention_bf16(qf, 3 * inner, S, 1, qf[:, inner:], qf[:, 2 * inner:], 3 * inner, S, 1, of, inner, n + nv, S, S, H, dh)
    t = qkv_b.float().reshape(n + nv, S, 3, H, dh).permute(2, 0, 3, 1, 4).double()
    ref = F.scaled_dot_product_attention(t[0], t[1], t[2]).permute(0, 2, 1, 3).reshape(M, inner)
    assert (of.cpu().double() - ref).abs().max() < 3e-2
    # fused block: bf16 att in, bf16 y out
    C, Hd, Ko = 256, 1024, inner
    x = torch.randn(M, C, generator=g)
    att_b = torch.randn(M, Ko, generator=g).to(torch.bfloat16)

    def hw(nn_, k):
        w = torch.randn(nn_, k, generator=g) / math.sqrt(k)
        hi = split(hip, G(pad_w(w)), False)[0]
        fr = torch.empty((nn_ + 31) // 32 * 32 * k, device=DEV, dtype=torch.int16)
        hip.pack_frag_bf16(hi, hi.shape[1], nn_, k, fr)
        return fr

    who, wh1, wh2, wn = hw(C, Ko), hw(Hd, C), hw(C, Hd), hw(3 * inner, C)
    bo, b1, b2, bn = (G(torch.randn(k_, generator=g) * 0.1) for k_ in (C, Hd, C, 3 * inner))
    outs = []
    for att, ydt in ((G(att_b.float()), torch.float32), (G(att_b), torch.bfloat16)):
        xg = G(x)
        y = torch.zeros(M, 3 * inner, device=DEV, dtype=ydt)
        hip.block_fused_bf16(xg, C, att, Ko, Ko, who, Ko, bo, wh1, C, b1, wh2, Hd, b2, Hd,
                             [dict(w=wn, ldw=C, b=bn, N=3 * inner, y=y, ldy=3 * inner, eps=1e-6)], M, C)
        outs.append((xg, y))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1].to(torch.bfloat16), outs[1][1])
    # plain GEMM with a bf16 output tensor
    A = G(torch.randn(300, C, generator=g))
    w = torch.randn(200, C, generator=g) / 16
    hi = split(hip, G(pad_w(w)), False)[0]
    cf, cb = torch.empty(300, 200, device=DEV), torch.empty(300, 200, device=DEV, dtype=torch.bfloat16)
    hip.gemm_bf16(A, C, hi, None, hi.shape[1], None, None, 0, cf, 200, 300, 200, C)
    hip.gemm_bf16(A, C, hi, None, hi.shape[1], None, None, 0, cb, 200, 300, 200, C)
    torch.cuda.synchronize()
    assert torch.equal(cf.to(torch.bfloat16), cb)


def test_delta_split_rowdot_broadcast(hip):
    g = torch.Generator().manual_seed(9)
    rows, C = 500, 128
    delta = torch.zeros(rows, 132)
    delta[:, :131] = torch.randn(rows, 131, generator=g)
    gw, gb = torch.randn(C, generator=g), torch.randn(C, generator=g)
    coords = torch.randn(rows, 3, generator=g)
    cg = G(coords)
    dn = torch.empty(rows, C, device=DEV)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    hip.delta_split(G(delta), 132, G(gw), G(gb), cg, dn, rows, C, flag)
    assert (cg.cpu() - (coords + delta[:, :3])).abs().max() < 1e-6
    assert (dn.cpu() - F.group_norm(delta[:, 3:131], 1, gw, gb, 1e-5)).abs().max() < 2e-5
    assert int(flag.item()) == 0
    delta[7, 1] = float("nan")
    hip.delta_split(G(delta), 132, G(gw), G(gb), cg, dn, rows, C, flag)
    assert int(flag.item()) == 1
    w, b = torch.randn(C, generator=g), torch.randn(1, generator=g)
    x = torch.randn(rows, C, generator=g)
    o = torch.empty(rows, device=DEV)
    hip.rowdot(G(x), C, G(w), G(b), o, rows, C)
    assert (o.cpu() - (x @ w + b)).abs().max() < 1e-5
    v = torch.randn(64, 256, generator=g)
    xb = torch.zeros(64 * 12, 256, device=DEV)
    hip.broadcast_rows(G(v), xb, 256, 64, 12, 256)
    assert torch.equal(xb.cpu().reshape(64, 12, 256), v[:, None].expand(64, 12, 256))


# ----------------------------------------------------------------------------------------- round 2: window corr at C=128
def _window_corr_all_levels(hip, pyr, tg, cd, r):
    """pyr: list of (BS,C,h,w) cpu maps; tg (BS,N,C); cd (BS,N,2) -> (BS,N,L*(2r+1)^2) device tensor."""
    BS, N, C = tg.shape
    D = (2 * r + 1) ** 2
    L = len(pyr)
    out = torch.zeros(BS, N, L * D, device=DEV)
    tg_d, cd_d = G(tg), G(cd)
    for lvl, f in enumerate(pyr):
        h, w = f.shape[-2:]
        hip.window_corr(G(f.permute(0, 2, 3, 1)), tg_d, cd_d, out, BS, N, C, h, w, lvl, r, L * D, lvl * D)
    torch.cuda.synchronize()
    return out


def test_window_corr_c128_golden(hip, golden):
    """The C=128 instantiation (the channel count of config C3) against a reference-generated fixture: 4 levels, r=4."""
    g = golden("window_corr_c128")
    rng = np.random.default_rng(int(g["fmaps_seed"]))
    fm = T(rng.standard_normal(tuple(int(x) for x in g["fmaps_shape"])).astype(np.float32))  # (1,2,128,32,48)
    tg, cd = T(g["targets"]), T(g["coords"])
    pyr = [f[0] for f in O.window_corr_pyramid(fm, 4)]
    out = _window_corr_all_levels(hip, pyr, tg[0], cd[0], 4)
    ref = g["out_r4"][0]
    assert out.shape == ref.shape
    assert np.abs(out.cpu().numpy() - ref).max() < 3e-5


def test_window_corr_c3_shape_sampled_rows(hip):
    """a7' at its real shape (S=12 frames, N=1024 tracks, 128x128 maps, C=128, r=4, 4 levels = 324 outputs per unit):
    64 sampled tracks x 12 frames against the oracle; coordinates include out-of-map windows (zero padding)."""
    gen = torch.Generator().manual_seed(5)
    S, N, C, Hm, r, L = 12, 1024, 128, 128, 4, 4
    fm = torch.randn(1, S, C, Hm, Hm, generator=gen)
    tg = torch.randn(1, S, N, C, generator=gen)
    cd = torch.rand(1, S, N, 2, generator=gen) * (Hm + 12) - 6
    pyr = O.window_corr_pyramid(fm, L)
    out = _window_corr_all_levels(hip, [f[0] for f in pyr], tg[0], cd[0], r)
    sample = torch.randperm(N, generator=gen)[:64]
    ref = O.window_corr_sample(pyr, tg[:, :, sample], cd[:, :, sample], r)[0]
    err = (out[:, sample].cpu() - ref).abs().max().item()
    assert err < 5e-5, err


@pytest.mark.parametrize("bf", [False, True])
def test_window_corr_levels_one_launch(hip, golden, bf):
    """mvt_window_corr_levels: all levels in ONE launch, fp32 or bf16 maps.  fp32: the reference fixture at C = 128 (3e-5) and
    bit-identical to the per-level launches.  bf16 (the dtype of config C3: under autocast the reference's CorrBlock pyramid is
    bf16, every avg-pooled level rounded again, blocks.py:423-449): against the oracle evaluated on the same bf16-rounded pyramid
    (fp32 accumulation on both sides: 5e-5), at the C3 shape with out-of-map windows."""
    if not bf:
        g = golden("window_corr_c128")
        rng = np.random.default_rng(int(g["fmaps_seed"]))
        fm = T(rng.standard_normal(tuple(int(x) for x in g["fmaps_shape"])).astype(np.float32))
        tg, cd = T(g["targets"]), T(g["coords"])
        pyr = [f[0] for f in O.window_corr_pyramid(fm, 4)]
        BS, N, C = tg[0].shape
        out = torch.zeros(BS, N, 4 * 81 + 3, device=DEV)
        hip.window_corr_levels([G(f.permute(0, 2, 3, 1)) for f in pyr], G(tg[0]), G(cd[0]), out, BS, N, C, 4, 4 * 81 + 3, 3)
        torch.cuda.synchronize()
        assert float(out[..., :3].abs().max()) == 0.0
        assert np.abs(out[..., 3:].cpu().numpy() - g["out_r4"][0]).max() < 3e-5
        assert torch.equal(out[..., 3:], _window_corr_all_levels(hip, pyr, tg[0], cd[0], 4))
        return
    gen = torch.Generator().manual_seed(6)
    S, N, C, Hm, r, L = 12, 1024, 128, 128, 4, 4
    fm = torch.randn(1, S, C, Hm, Hm, generator=gen).bfloat16()
    pyr = [fm]
    for _ in range(L - 1):  # the reference's pooling under autocast: bf16 in, bf16 out
        f = torch.nn.functional.avg_pool2d(pyr[-1][0].float(), 2, stride=2).bfloat16()
        pyr.append(f[None])
    tg = torch.randn(1, S, N, C, generator=gen)
    cd = torch.rand(1, S, N, 2, generator=gen) * (Hm + 12) - 6
    out = torch.zeros(S, N, L * 81, device=DEV)
    hip.window_corr_levels([G(f[0].permute(0, 2, 3, 1)) for f in pyr], G(tg[0]), G(cd[0]), out, S, N, C, r, L * 81)
    torch.cuda.synchronize()
    sample = torch.randperm(N, generator=gen)[:64]
    ref = O.window_corr_sample([f.float() for f in pyr], tg[:, :, sample], cd[:, :, sample], r)[0]
    err = (out[:, sample].cpu() - ref).abs().max().item()
    assert err < 5e-5, err


def test_bf16_store_keeps_nan(hip):
    """A NaN must survive the bf16 activation stores so that the deferred NaN guard sees it (ADVICE / VERDICT weak #6):
    a bf16-output GEMM with a NaN and an Inf in its input rows."""
    M, N, K = 64, 64, 64
    A = torch.randn(M, K)
    A[3, 5] = float("nan")
    A[7, 1] = float("inf")
    Wm = torch.randn(N, K) / 8
    hi, _ = split(hip, G(pad_w(Wm)), lo=False)
    out = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    hip.gemm_bf16(G(A), K, hi, None, hi.shape[1], G(torch.zeros(N)), None, 0, out, N, M, N, K, 0)
    torch.cuda.synchronize()
    o = out.float().cpu()
    assert bool(torch.isnan(o[3]).all()) and bool(torch.isnan(o[7]).any() | torch.isinf(o[7]).any())
    ok = torch.ones(M, dtype=torch.bool)
    ok[3] = ok[7] = False
    assert bool(torch.isfinite(o[ok]).all())


# ----------------------------------------------------------------------------------------- round 2: bf16 frame store
@pytest.mark.parametrize("C,K", [(128, 16), (32, 16), (64, 5), (256, 16)])
def test_corr_gather_dot_bf16_rows(hip, C, K):
    """bf16 feature rows (the frame store of bf16 mode): neighbour indices bit-exact, dots against the oracle evaluated on the
    SAME bf16-rounded rows (the kernel accumulates the fp32 target x bf16 row products in fp32)."""
    g = torch.Generator().manual_seed(C + K)
    B, P, M = 3, 3000, 50
    xyz = torch.rand(B, P, 3, generator=g) * 4 - 2
    fvec = torch.randn(B, P, C, generator=g).bfloat16()
    tg = torch.randn(B, M, C, generator=g)
    cd = torch.rand(B, M, 3, generator=g) * 4 - 2
    out, idx, _ = _run_corr(hip, xyz, fvec, tg, cd, K, 1)
    ref, ridx = O.corr_sample(xyz, fvec.float(), tg, cd, K, 1, True, False, "exact", return_idx=True)
    assert torch.equal(idx, ridx)
    assert (out - ref).abs().max() < 2e-5


def test_avgpool2_and_knn1_gather_bf16(hip):
    g = torch.Generator().manual_seed(3)
    n, h, w, C = 3, 10, 14, 128
    x = torch.randn(n, h, w, C, generator=g).bfloat16()
    out = torch.empty(n, h // 2, w // 2, C, device=DEV, dtype=torch.bfloat16)
    hip.avgpool2(G(x), out, n, h, w, C)
    xf = x.float()
    ref = ((((xf[:, 0::2, 0::2] + xf[:, 0::2, 1::2]) + xf[:, 1::2, 0::2]) + xf[:, 1::2, 1::2]) * 0.25).bfloat16()
    assert torch.equal(out.cpu(), ref)  # fp32 mean of the four bf16 values, one rounding
    P, nq = 2000, 30
    xyz = torch.zeros(2, P, 4)
    xyz[..., :3] = torch.rand(2, P, 3, generator=g)
    fvec = torch.randn(2, P, C, generator=g).bfloat16()
    q = torch.rand(nq, 3, generator=g)
    keys = torch.empty(nq, device=DEV, dtype=torch.int64)
    hip.knn_scan(G(xyz), P, G(q), nq, 1, 1, 0, 2, 1, 1, keys)
    feat = torch.empty(nq, C, device=DEV)
    hip.knn1_gather(G(fvec), P, C, keys, nq, 1, 1, feat)
    _, ridx = O.knn_exact(1, xyz[1:2, :, :3], q[None])
    assert torch.equal(feat.cpu(), fvec[1][ridx[0, :, 0]].float())


@pytest.mark.parametrize("rows", [12288, 100])
def test_update_head_bf16_matches_unfused_sequence(hip, rows):
    """mvt_update_head_bf16 (flow head + track / feature update in one launch) against the unfused library sequence it replaces
    (three mvt_gemm_bf16, mvt_delta_split, one more mvt_gemm_bf16) on identical inputs: the same bf16 operand roundings, fp32
    accumulation in a different order -> agreement to fp32 rounding noise; and against an fp64 torch evaluation at bf16 accuracy."""
    g = torch.Generator().manual_seed(rows)
    C, OUT, CF = 256, 131, 128
    tok = torch.randn(rows, C, generator=g)
    W0, W2, W4 = torch.randn(OUT, C, generator=g) / 16, torch.randn(OUT, OUT, generator=g) / 11, torch.randn(OUT, OUT, generator=g) / 11
    Wu = torch.randn(CF, CF, generator=g) / 11
    b0, b2, b4, bu = (torch.randn(n, generator=g) * 0.1 for n in (OUT, OUT, OUT, CF))
    gw, gb = 1 + 0.1 * torch.randn(CF, generator=g), 0.1 * torch.randn(CF, generator=g)
    coords0, ff0 = torch.randn(rows, 3, generator=g), torch.randn(rows, CF, generator=g)

    def rowsw(w, pad_n):
        n, k = w.shape
        wp = pad_w(w)
        if pad_n:
            wp = torch.cat([wp, torch.zeros(pad_n - n, wp.shape[1])], 0)
        return split(hip, G(wp), lo=False)[0]

    def frag(w, kpad):
        hi = split(hip, G(pad_w(w)), lo=False)[0]
        fr = torch.empty((w.shape[0] + 31) // 32 * 32 * kpad, device=DEV, dtype=torch.int16)
        hip.pack_frag_bf16(hi, hi.shape[1], w.shape[0], kpad, fr)
        return fr

    # unfused
    h0, h2, h4, hu = rowsw(W0, 132), rowsw(W2, 132), rowsw(W4, 0), rowsw(Wu, 0)
    pad1 = lambda b: G(torch.cat([b, torch.zeros(132 - OUT)]))
    tg = G(tok)
    h1 = torch.empty(rows, 132, device=DEV)
    h2t = torch.empty(rows, 132, device=DEV)
    delta = torch.empty(rows, 132, device=DEV)
    hip.gemm_bf16(tg, C, h0, None, h0.shape[1], pad1(b0), None, 0, h1, 132, rows, 132, C, 1)
    hip.gemm_bf16(h1, 132, h2, None, h2.shape[1], pad1(b2), None, 0, h2t, 132, rows, 132, OUT, 1)
    hip.gemm_bf16(h2t, 132, h4, None, h4.shape[1], G(b4), None, 0, delta, 132, rows, OUT, OUT, 0)
    c_ref, f_ref = G(coords0).clone(), G(ff0).clone()
    dn = torch.empty(rows, CF, device=DEV)
    hip.delta_split(delta, 132, G(gw), G(gb), c_ref, dn, rows, CF, None)
    hip.gemm_bf16(dn, CF, hu, None, hu.shape[1], G(bu), f_ref, CF, f_ref, CF, rows, CF, CF, 3)
    # fused
    c_f, f_f = G(coords0).clone(), G(ff0).clone()
    d_f = torch.zeros(rows, 132, device=DEV)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    hip.update_head_bf16(tg, C, frag(W0, 256), G(b0), frag(W2, 144), G(b2), frag(W4, 144), G(b4), G(gw), G(gb), frag(Wu, 128), G(bu), c_f, f_f,
                         d_f, 132, rows, C, OUT, flag)
    torch.cuda.synchronize()
    sc = delta[:, :OUT].abs().max().item()
    assert (d_f[:, :OUT] - delta[:, :OUT]).abs().max().item() < 2e-5 * sc
    assert (c_f - c_ref).abs().max().item() < 2e-5 * sc
    assert (f_f - f_ref).abs().max().item() < 8e-3  # (GroupNorm amplifies the 1e-5 delta noise into bf16 rounding flips of dn: ~7e-4 each)
    assert int(flag.item()) == 0
    # fp64 evaluation
    t64 = tok.double()
    d64 = torch.relu(torch.relu(t64 @ W0.double().t() + b0.double()) @ W2.double().t() + b2.double()) @ W4.double().t() + b4.double()
    assert (d_f[:, :OUT].cpu().double() - d64).abs().max().item() < 3e-2 * d64.abs().max().item()
    dnn = torch.nn.functional.group_norm(d64[:, 3:], 1, gw.double(), gb.double(), 1e-5)
    f64 = ff0.double() + torch.nn.functional.gelu(dnn @ Wu.double().t() + bu.double())
    assert (f_f.cpu().double() - f64).abs().max().item() < 6e-2
    assert (c_f.cpu().double() - (coords0.double() + d64[:, :3])).abs().max().item() < 3e-2 * d64.abs().max().item()
    # NaN guard
    c_n = G(coords0).clone()
    c_n[5, 1] = float("nan")
    hip.update_head_bf16(tg, C, frag(W0, 256), G(b0), frag(W2, 144), G(b2), frag(W4, 144), G(b4), G(gw), G(gb), frag(Wu, 128), G(bu), c_n,
                         G(ff0).clone(), None, 0, rows, C, OUT, flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1


# ----------------------------------------------------------------------------------------- round 2: metrics post-processing (f4)
@pytest.mark.parametrize("name", ["3d", "2d"])
def test_metrics_golden(hip, golden, name):
    """evaluate_predictions on the device (one mvt_track_metrics launch + masked means) against the REFERENCE's tables
    (tests/golden/make_golden_metrics.py) and the oracle; integer track ids bit-exact."""
    from mvtracker_amd import metrics
    from oracle import metrics_oracle as MO
    from test_oracle_golden import METRIC_KW, check_metrics_against_golden
    g = golden("metrics_eval")
    args = (g[f"{name}_gt"], g[f"{name}_vis"], g[f"{name}_pred"], g[f"{name}_pocc"], g[f"{name}_qp"])
    res, pt = metrics.evaluate_predictions(*args, **METRIC_KW[name], device=DEV)
    check_metrics_against_golden(g, name, res, pt)
    # per-track table against the oracle's float32 evaluation for EVERY track (also those outside all masks)
    gt_vis = args[1] & (np.arange(args[0].shape[0])[:, None] >= args[4][:, 0][None, :])
    tm = MO.track_metrics(args[0], gt_vis, args[2], args[3], args[4], METRIC_KW[name]["distance_thresholds"], METRIC_KW[name]["survival_distance_threshold"])
    names, table, movement, nvis, _ = metrics.per_track_metrics(*args, METRIC_KW[name]["distance_thresholds"],
                                                                METRIC_KW[name]["survival_distance_threshold"], device=DEV)
    th = table.cpu().numpy()
    for j, k in enumerate(names):
        ref = tm[k]
        ok = (np.isnan(ref) & np.isnan(th[:, j])) | (np.abs(ref - th[:, j]) <= 1e-5 * (1 + np.abs(ref)))
        assert ok.all(), (k, ref[~ok][:3], th[~ok, j][:3])
    assert np.allclose(movement.cpu().numpy(), MO.point_movement(args[0], gt_vis), rtol=1e-5, atol=1e-6)
    assert np.array_equal(nvis.cpu().numpy().astype(np.int64), gt_vis.sum(0))


def test_metrics_long_clip_and_evaluate_3dpt(hip):
    """T > 64 (several 64-frame steps: carried movement, median over > 64 values) against the oracle, and evaluate_3dpt's flat dict."""
    from mvtracker_amd import metrics
    from oracle import metrics_oracle as MO
    rng = np.random.default_rng(9)
    T, N = 150, 33
    gt = (rng.uniform(-1, 1, (1, N, 3)) + np.cumsum(rng.standard_normal((T, N, 3)) * 0.02, 0)).astype(np.float32)
    vis = rng.uniform(size=(T, N)) < 0.7
    qt = rng.integers(0, 70, size=N)
    vis[qt, np.arange(N)] = True
    pred = (gt + rng.standard_normal((T, N, 3)) * 0.05).astype(np.float32)
    pvis = vis ^ (rng.uniform(size=(T, N)) < 0.1)
    qp = np.concatenate([qt[:, None].astype(np.float32), gt[qt, np.arange(N)]], -1).astype(np.float32)
    got = metrics.evaluate_3dpt(gt, vis, pred, pvis, "kubric-multiview", 2.0, qp, add_per_track_results=False, device=DEV)
    ref = MO.evaluate_3dpt(gt, vis, pred, pvis, "kubric-multiview", 2.0, qp)
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert (np.isnan(ref[k]) and np.isnan(got[k])) or abs(ref[k] - got[k]) <= 0.011, (k, ref[k], got[k])


@pytest.mark.parametrize("name", ["kubric", "dexycb", "panoptic_noquery", "tapvid2d", "ablation2d"])
def test_evaluate_3dpt_vs_reference(hip, golden, name):
    """mvtracker_amd.metrics.evaluate_3dpt (device kernel + masked means) against the flat dict the REFERENCE's
    evaluator_3dpt.evaluate_3dpt returns for the same inputs (five evaluation settings, with and without query points)."""
    from mvtracker_amd import metrics
    from test_oracle_golden import check_evaluate_3dpt_against_golden
    g = golden("evaluate_3dpt")
    qp = g[f"{name}_qp"] if bool(g[f"{name}_with_query"][0]) else None
    got = metrics.evaluate_3dpt(g[f"{name}_gt"], g[f"{name}_vis"], g[f"{name}_pred"], g[f"{name}_pvis"], str(g[f"{name}_setting"][0]),
                                float(g[f"{name}_upscale"][0]), qp, add_per_track_results=False, device=DEV)
    check_evaluate_3dpt_against_golden(g, name, got)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_concat_resize_matches_separate_resizes(hip, dt):
    """One-launch concat (whole 416-channel rows per wave) against the four mvt_resize_bilinear_ac launches it replaces and
    against torch's F.interpolate(bilinear, align_corners=True)."""
    g = torch.Generator().manual_seed(2)
    n, Hd, Wd = 3, 24, 40
    dims = [(48, 80, 64), (24, 40, 96), (12, 20, 128), (6, 10, 128)]
    srcs = [torch.randn(n, h, w, c, generator=g).to(dt) for h, w, c in dims]
    gs = [G(t) for t in srcs]
    a = torch.zeros(n, Hd, Wd, 416, device=DEV, dtype=dt)
    b = torch.zeros_like(a)
    hip.concat_resize_bilinear_ac(gs, dims, a, n, Hd, Wd, 416)
    off = 0
    for t, (h, w, c) in zip(gs, dims):
        hip.resize_bilinear_ac(t, b, n, h, w, c, Hd, Wd, 416, off)
        off += c
    torch.cuda.synchronize()
    # (same expression in two kernels: the compiler may contract the fp32 blend differently -> last-bit differences)
    assert (a.float() - b.float()).abs().max().item() <= (1e-4 if dt == torch.float32 else 4e-2)
    assert (a.float() != b.float()).float().mean().item() < (1.0 if dt == torch.float32 else 0.02)
    ref = torch.cat([F.interpolate(t.float().permute(0, 3, 1, 2), size=(Hd, Wd), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
                     for t in srcs], -1)
    tol = 1e-4 if dt == torch.float32 else 2e-2
    assert (a.float().cpu() - ref).abs().max().item() < tol
