"""Every GEMM, convolution and fused-MLP kernel variant on inputs whose right answer is an integer: no tolerance anywhere.

GPU tests (`-m gpu`) go through the C ABI; the tests without the marker are the CPU-only checks of the dispatch restatement and of
the probes themselves.

The principle.  Operands are small NON-ZERO integers (exact in bf16), sized so that every partial sum stays below 2^24: every fp32
accumulation order, fp32 MFMA, bf16 MFMA, bf16x3 (its `lo` half is exactly zero), any K split and any tile then give the same exact
integer, and a dropped, doubled or misplaced product term moves an element by at least 1.  With bf16 OUTPUT tensors the results
also have to stay at or below 256 (entries in {-1, +1}, K <= 864).  Each test asserts that bound on its own reference before it
looks at the device.

A. The host dispatch restated (gemm_tile, halo_tile, plan_conv and the row-tile variants of csrc/conv_plan.h, the launch forms of
   mvt_block_fused_bf16 / mvt_ln_proj_bf16 of csrc/launch_plan.h; test_conv_plan_host.py and test_launch_plan_host.py tie the
   restatements to the headers on the CPU): `test_cases_reach_every_variant` asserts that the parametrised shapes
   reach every variant the library compiles for these entry points, so a shape that falls back to another variant fails on the CPU.
   (The MVT_ROWS_NW8 / MVT_BLOCK_NMB / MVT_BLOCK_NOSPLIT tuning overrides, which a process reads once from its environment, are
   reached by tests/test_gpu_tuning_switches.py: it runs cases of this file in a child process per value.  The restatements
   below take the switch values as arguments and default to the process's environment.)
B. mvt_gemm, mvt_gemm_bf16 (bf16, bf16x3), mvt_ln_gemm_bf16: every tile at its edges, K on both sides of the 32- and 64-wide
   k-tiles and of the 4-element lda padding, act none / relu, with and without an integer residual, padded and NaN-poisoned ldc /
   ldr / lda.  torch.equal against the fp64 CPU matmul.  (mvt_ln_gemm_bf16 in bf16x3 mode keeps the 1e-6 residue of rstd in the lo
   half of the normalised operand, so there the assertion is D's "rounds to the integer, within 0.25": the residue is at most
   K * 8 * 5e-6 = 0.04 at K = 1024.)
C. mvt_conv2d, mvt_conv2d_bf16 (fp32, bf16x3, bf16; fp32 and bf16 tensors; MVT_IO_SHORT_WG; MVT_CONV_BIG=0), mvt_conv3x3s2_down_bf16:
   every variant of A on both sides of its pixel tile, one batch n > 1 each.  torch.equal against F.conv2d in fp64.
D. mvt_mlp_fused_bf16, mvt_block_fused_bf16 (all four launch forms), mvt_ln_proj_bf16 (both forms), one stage at a time: rows of x
   are +-c with exactly half the entries positive, so LayerNorm in bf16 is exactly +-1; fc1 weights 16 * {+-1} and biases that are
   multiples of 16 make tanh-gelu the identity / zero; fc2 weights +-1.  Every element rounds to the planted integer and lies within
   0.25 of it, asserted of the fp64 emulation (bf16 where the kernel rounds: LayerNorm output, hidden tile, att, bf16 y) first.
E. The probes are themselves tested: a dropped k, a dropped last k-tile, two swapped output columns, a last partial row tile shifted
   by one row, a dropped conv tap at an image border and a skipped hidden chunk of 256 each break the assertion at the smallest and
   the largest shape of each family.
"""
import collections
import functools
import os
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
ACT_NONE, ACT_RELU = 0, 1
C, KO = 256, 288  # the updater's hidden size, the attention width


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ A: the host dispatch, restated


def pick_tile(M, N):
    """conv_plan.h gemm_tile: 0 = 128x128, 1 = 128x96, 2 = 256x64, 3 = 64x128, 4 = 64x64."""
    nb = lambda bm, bn: cdiv(M, bm) * cdiv(N, bn)
    if N % 128 != 0 and N % 96 == 0:
        return 1
    if N <= 64:
        return 2 if nb(256, 64) >= 512 else 4
    if nb(128, 128) >= 512:
        return 0
    if nb(64, 128) >= 512:
        return 3
    return 4


TILE_ROWS = {0: 128, 1: 128, 2: 256, 3: 64, 4: 64}


def halo_tile(Cout):
    """conv_plan.h halo_tile: output channels per workgroup (8 x 16 pixels each)."""
    if Cout % 128 != 0 and Cout % 96 == 0:
        return 96
    return 64 if Cout <= 64 else 128


def env_int(name):
    """A once-per-process tuning variable as the library reads it: atoi of the value, 0 when unset."""
    m = re.match(r"\s*[+-]?\d+", os.environ.get(name, ""))
    return int(m.group()) if m else 0


def env_set(name):
    return name in os.environ


def rows_tile(k, s, Ho=None, nw8=None):
    """conv_plan.h tile_rows: (TM, NW) of the row-tile kernel for (kernel size, stride) -- NW * TM output rows per workgroup.
    nw8 = MVT_ROWS_NW8 (default: this process's): 1 = eight waves / 16 rows where Ho % 16 == 0, 2 = TM 1 / four rows.
    Without Ho (the callers that ask for a case's kernel family, not for a launch) =1 answers for an Ho that is no multiple of 16."""
    nw8 = env_int("MVT_ROWS_NW8") if nw8 is None else nw8
    if k == 3 and s == 1:
        return (2, 8) if (nw8 == 1 and Ho is not None and Ho % 16 == 0) else ((1, 4) if nw8 == 2 else (2, 4))
    return (1, 4) if (k == 3 and s == 2) else (2, 4)


def rows_staged_fits(tm, ks, s, nw, tn):
    """conv_plan.h rows_staged_fits: the per-wave staging tiles of the bf16 epilogue fit the patch LDS (patch_slots)."""
    rows = nw * tm
    pr = rows if ks == 1 else s * (rows - 1) + 3
    pc = 32 if ks == 1 else s * 31 + 3
    rs = 2 * ((pc + 1) // 2) if (ks == 3 and s == 2) else pc
    return nw * 32 * (tn * 32 + 8) <= pr * rs * 40


# one convolution case; io = element types of (input, output): "f" fp32, "b" bf16
Conv = collections.namedtuple("Conv", "prec io Cin Cout k s act ldo_extra short big geos", defaults=(ACT_NONE, 0, False, True, None))


def conv_out(H, W, k, s):
    p = k // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def conv_variant(c, n, H, W, nw8=None):
    """The kernel that mvt_conv2d / mvt_conv2d_bf16 launch for case c on n images of H x W (nw8: see rows_tile)."""
    Ho, Wo = conv_out(H, W, c.k, c.s)
    M, p = n * Ho * Wo, c.k // 2
    stem = c.Cin == 4
    inb, outb = c.io[0] == "b", c.io[1] == "b"
    ldo = c.Cout + c.ldo_extra
    if c.prec == "fp32":
        return ("gemm", "fp32", "stem" if stem else "im2col", pick_tile(M, c.Cout))
    split = c.prec == "bf16x3"
    st_ok = outb and c.Cout % 8 == 0 and ldo % 8 == 0
    if not split and stem and c.k == 7 and c.s == 2 and c.Cout <= 64 and c.act == ACT_NONE:
        return ("stem_rows", 1 if c.Cout <= 32 else 2, st_ok)
    if not split and c.act == ACT_NONE and c.Cin % 32 == 0 and c.k in (1, 3):
        n96 = c.Cout % 64 != 0 and c.Cout % 96 == 0
        if c.k == 3 and c.s == 1 and not c.short and inb and st_ok and c.Cout % 256 == 0 and c.big:
            return ("big",)
        tn = 3 if n96 else 2
        tm, nw = rows_tile(c.k, c.s, Ho, nw8)
        return ("rows", c.k, c.s, tn, inb, st_ok and rows_staged_fits(tm, c.k, c.s, nw, tn))
    if c.k == 3 and c.s == 1 and c.Cin % 32 == 0:
        return ("halo", c.prec, halo_tile(c.Cout))
    return ("gemm", c.prec, "stem" if stem else "im2col", pick_tile(M, c.Cout))


def down_variant(Cout):
    return ("down", 3 if (Cout % 64 != 0 and Cout % 96 == 0) else 2)


def block_forms(M, ws, nmb=None, nosplit=None):
    """mvt_block_fused_bf16: the kernel instantiations <NMB, MODE> one call launches.  nmb = the value MVT_BLOCK_NMB forces
    ("rule": the variable is unset), nosplit = MVT_BLOCK_NOSPLIT is set; default: this process's environment."""
    if nmb is None:
        nmb = env_int("MVT_BLOCK_NMB") if env_set("MVT_BLOCK_NMB") else "rule"
    nosplit = env_set("MVT_BLOCK_NOSPLIT") if nosplit is None else nosplit
    if (nmb if nmb != "rule" else (2 if M >= 4096 else 1)) == 2:
        return [("block", 2, 0)]
    if ws and not nosplit and M <= 2048 and M % 32 == 0:
        return [("block", 1, 1), ("block", 1, 2)]
    return [("block", 1, 0)]


def ln_proj_form(M):
    return ("ln_proj", 2, 3) if M >= 4096 else ("ln_proj", 1, 2)


# ------------------------------------------------------------------ the cases

# (M, N): the smallest shape that reaches each tile, and tile 1 / 4 at a ragged and an exact shape
GEMM_SHAPES = [(8100, 1000), (130917, 40), (130900, 64), (19137, 250), (130, 96), (2000, 864), (33, 131), (64, 64)]
GEMM_TILES = [0, 2, 2, 3, 1, 1, 4, 4]
ALL_K = (32, 36, 64, 70, 131, 256, 581)
COMBOS = [(ACT_NONE, False), (ACT_RELU, True), (ACT_NONE, True), (ACT_RELU, False)]  # (act, residual), cycled over the K list
PRECS = ["fp32", "bf16x3", "bf16"]


def gemm_ks(M):
    return ALL_K if M <= 2000 else ALL_K[:4]  # K stays small at the large-M shapes


GEMM_BF16_OUT = [((130, 96), 256), ((33, 131), 256), ((8100, 1000), 64), ((19137, 250), 70), ((130900, 64), 36)]

LN_CASES = ([((M, N), K) for (M, N) in [(130, 96), (2000, 864), (33, 131), (64, 64)] for K in (128, 256, 1024)] +
            [((8100, 1000), 128), ((8100, 1000), 256), ((130917, 40), 128), ((130900, 64), 128), ((19137, 250), 256)])

# (n, H, W): both sides of the 8 (4: 3x3 / stride 2) x 32 output pixel tiles, stride 2 at odd and even sizes, one batch n > 1
GEOS = [(2, 9, 33), (1, 8, 32), (1, 7, 31), (1, 16, 65), (1, 17, 33)]
GEOS_HALO = GEOS + [(1, 8, 16), (2, 9, 17), (1, 7, 15)]              # 8 x 16 pixel tiles
GEOS_STEM = [(2, 18, 66), (1, 16, 64), (1, 13, 61), (1, 33, 31)]     # output 9 x 33, 8 x 32, 7 x 31, 17 x 16
GEOS_416 = [(1, 9, 33)]


def _row_cases():
    out = []
    for k, s in ((3, 1), (3, 2), (1, 1), (1, 2)):
        # TN 2: fp32 / bf16 input x plain / staged epilogue; Cout 160 = two whole 64-channel tiles and half a tile
        out += [Conv("bf16", "ff", 32, 32, k, s, ldo_extra=1), Conv("bf16", "ff", 64, 160, k, s, ldo_extra=4),
                Conv("bf16", "fb", 96, 64, k, s, ldo_extra=8), Conv("bf16", "fb", 32, 128, k, s, ldo_extra=2),
                Conv("bf16", "bf", 64, 128, k, s), Conv("bf16", "bb", 32, 160, k, s, ldo_extra=8),
                Conv("bf16", "bb", 96, 64, k, s, ldo_extra=1), Conv("bf16", "bb", 64, 256, k, s, short=True),
                Conv("bf16", "bb", 32, 256, k, s, big=False, ldo_extra=8, geos=GEOS[:3])]
        # TN 3 (Cout 96): the quad / pair / single-element stores of the plain epilogue, the staged one where it fits
        out += [Conv("bf16", "ff", 32, 96, k, s, ldo_extra=4), Conv("bf16", "ff", 64, 96, k, s, ldo_extra=2),
                Conv("bf16", "fb", 96, 96, k, s, ldo_extra=8), Conv("bf16", "fb", 32, 96, k, s, ldo_extra=1),
                Conv("bf16", "bf", 64, 96, k, s, ldo_extra=1), Conv("bf16", "bb", 32, 96, k, s), Conv("bf16", "bb", 96, 96, k, s, ldo_extra=4)]
    out.append(Conv("bf16", "ff", 416, 64, 3, 1, geos=GEOS_416))
    return out


CONV_CASES = _row_cases() + [
    # conv3x3_big_bf16: one and two 256-channel blocks
    Conv("bf16", "bb", 32, 256, 3, 1), Conv("bf16", "bb", 64, 512, 3, 1, ldo_extra=8, geos=GEOS[:3]), Conv("bf16", "bb", 416, 256, 3, 1, geos=GEOS_416),
    # the 7x7 stem on the row tiles: TN 1 / 2, staged and plain epilogue
    Conv("bf16", "ff", 4, 32, 7, 2, geos=GEOS_STEM), Conv("bf16", "fb", 4, 32, 7, 2, ldo_extra=8, geos=GEOS_STEM),
    Conv("bf16", "ff", 4, 64, 7, 2, ldo_extra=3, geos=GEOS_STEM), Conv("bf16", "fb", 4, 64, 7, 2, geos=GEOS_STEM),
    Conv("bf16", "fb", 4, 64, 7, 2, ldo_extra=1, geos=GEOS_STEM),
    # the halo kernel (gemm.hip): bf16x3, and bf16 with an activation; 64-, 96- and 128-channel tiles
    Conv("bf16x3", "ff", 32, 32, 3, 1, geos=GEOS_HALO), Conv("bf16x3", "ff", 64, 96, 3, 1, act=ACT_RELU, ldo_extra=3, geos=GEOS_HALO),
    Conv("bf16x3", "ff", 96, 160, 3, 1, geos=GEOS_HALO), Conv("bf16x3", "ff", 32, 256, 3, 1, act=ACT_RELU, geos=GEOS_HALO),
    Conv("bf16", "ff", 64, 64, 3, 1, act=ACT_RELU, ldo_extra=1, geos=GEOS_HALO), Conv("bf16", "bb", 32, 96, 3, 1, act=ACT_RELU, geos=GEOS_HALO),
    Conv("bf16", "bf", 96, 128, 3, 1, act=ACT_RELU, geos=GEOS_HALO), Conv("bf16", "fb", 64, 160, 3, 1, act=ACT_RELU, ldo_extra=5, geos=GEOS_HALO),
    # the im2col / stem loaders of the GEMM kernels at small images (tiles 4 and 1)
    Conv("fp32", "ff", 32, 64, 3, 1), Conv("fp32", "ff", 64, 96, 3, 2, act=ACT_RELU, ldo_extra=3), Conv("fp32", "ff", 96, 128, 1, 1),
    Conv("fp32", "ff", 32, 160, 1, 2, ldo_extra=1), Conv("fp32", "ff", 416, 256, 3, 1, geos=GEOS_416), Conv("fp32", "ff", 64, 32, 3, 2),
    Conv("fp32", "ff", 4, 32, 7, 2, geos=GEOS_STEM), Conv("fp32", "ff", 4, 64, 7, 2, act=ACT_RELU, ldo_extra=2, geos=GEOS_STEM),
    Conv("bf16x3", "ff", 32, 64, 3, 2), Conv("bf16x3", "ff", 64, 96, 1, 1, act=ACT_RELU, ldo_extra=3), Conv("bf16x3", "ff", 96, 128, 1, 2),
    Conv("bf16x3", "ff", 4, 32, 7, 2, geos=GEOS_STEM), Conv("bf16x3", "ff", 4, 64, 7, 2, act=ACT_RELU, geos=GEOS_STEM),
    Conv("bf16", "ff", 32, 64, 3, 2, act=ACT_RELU), Conv("bf16", "bb", 64, 96, 1, 1, act=ACT_RELU, ldo_extra=3),
    Conv("bf16", "bf", 96, 256, 1, 2, act=ACT_RELU), Conv("bf16", "fb", 4, 32, 7, 2, act=ACT_RELU, geos=GEOS_STEM),
    Conv("bf16", "ff", 4, 64, 7, 2, act=ACT_RELU, ldo_extra=1, geos=GEOS_STEM),
]
# ... and at image counts that reach the other three tiles (1x1: K = 32; the stem as the fp32 encoder runs it at full size)
for _prec, _act, _io in (("fp32", ACT_NONE, "ff"), ("bf16x3", ACT_RELU, "ff"), ("bf16", ACT_RELU, "ff")):
    CONV_CASES += [Conv(_prec, _io, 32, 256, 1, 1, act=_act, geos=[(32, 33, 31)]),     # M = 32 736: tile 0
                   Conv(_prec, _io, 32, 64, 1, 1, act=_act, ldo_extra=1, geos=[(128, 33, 31)]),  # M = 130 944: tile 2
                   Conv(_prec, _io, 32, 256, 1, 1, act=_act, geos=[(16, 33, 31)]),     # M = 16 368: tile 3
                   Conv(_prec, _io, 4, 64, 7, 2, act=_act, geos=[(32, 130, 126)])]     # stem, M = 131 040: tile 2

DOWN_CASES = [(32, 64, 8), (64, 96, 0), (96, 160, 8), (32, 96, 8)]  # (Cin, Cout, ldo - Cout)


def conv_geos(c):
    return c.geos if c.geos is not None else GEOS


def conv_id(c):
    return (f"{c.prec}-{c.io}-cin{c.Cin}-cout{c.Cout}-k{c.k}s{c.s}" + ("-relu" if c.act else "") + (f"-ldo{c.ldo_extra}" if c.ldo_extra else "") +
            ("-short" if c.short else "") + ("" if c.big else "-nobig") + (f"-n{c.geos[0][0]}x{c.geos[0][1]}x{c.geos[0][2]}" if c.geos and len(c.geos) == 1 else ""))


# D: rows of the fused kernels.  32 / 64 rows per workgroup, the split path (a workspace, M <= 2048, whole 32-row tiles), 4096
BLOCK_MS = [(31, False), (33, True), (63, False), (65, False), (1000, True), (2080, True), (4095, False),  # <1, 0>
            (32, True), (64, True), (2048, True),                                                          # <1, 1> + <1, 2>
            (4096, True), (4129, False)]                                                                   # <2, 0>
LN_PROJ_MS = [31, 33, 64, 100, 4095, 4096, 4129]
MLP_MS = [1, 127, 128, 129, 1000]


# ------------------------------------------------------------------ integer operands and references (CPU)


def gen_for(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(g, shape, amp):
    """Non-zero integers of magnitude 1..amp, fp32."""
    mag = torch.randint(1, amp + 1, shape, generator=g)
    return (mag * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def balanced_rows(g, M, K, cmax=8):
    """[M][K] rows +-c with exactly K/2 positive entries, c an integer 1..cmax per row; also the signs."""
    assert K % 2 == 0
    if M * K <= (1 << 22):
        order = torch.rand(M, K, generator=g).argsort(dim=1)
        s = torch.where(order < K // 2, 1.0, -1.0)
    else:  # (large: a random half, its negation, one column permutation)
        half = (2 * torch.randint(0, 2, (M, K // 2), generator=g) - 1).float()
        s = torch.cat([half, -half], dim=1)[:, torch.randperm(K, generator=g)]
    c = torch.randint(1, cmax + 1, (M, 1), generator=g).float()
    return s * c, s


def act_ref(y, act):
    return F.relu(y) if act == ACT_RELU else y


def gemm_ref(A, W, b, R, act, mutate=None, bm=64):
    """fp64 act(A W^T + b) + R.  mutate: the index bugs the assertion has to see."""
    A, W = A.double(), W.double()
    K = A.shape[1]
    if mutate == "drop_k":
        A = A.clone()
        A[:, K - 1] = 0
    elif mutate == "drop_last_ktile":
        A = A.clone()
        A[:, 64 * ((K - 1) // 64):] = 0
    y = act_ref(A @ W.t() + b.double(), act)
    if R is not None:
        y = y + R.double()
    if mutate == "swap_cols":
        y = y.clone()
        y[:, [0, 1]] = y[:, [1, 0]]
    elif mutate == "shift_last_rows":
        M = y.shape[0]
        r0 = (M - 1) // bm * bm
        assert M - r0 >= 2 or r0 > 0
        r0 = r0 if M - r0 >= 2 else r0 - bm
        y = torch.cat([y[:r0], y[r0 + 1:], y[r0:r0 + 1]])
    else:
        assert mutate in (None, "drop_k", "drop_last_ktile")
    return y


@functools.lru_cache(maxsize=4)
def gemm_data(M, N, K, amp, act, res):
    g = gen_for("gemm", M, N, K, amp)
    A, W, b = ints(g, (M, K), amp), ints(g, (N, K), amp), ints(g, (N,), 3)
    R = ints(g, (M, N), 3) if res else None
    return A, W, b, R, gemm_ref(A, W, b, R, act)


def conv_operands(c, n, H, W, seed=0):
    """Integer x [n][H][W][Cin], w [Cout][k][k][Cin], bias; +-1 where the output tensor is bf16 or K is large, else up to +-2."""
    return _conv_operands(c.Cin, c.Cout, c.k, c.s, 1 if (c.io[1] == "b" or c.Cin > 96) else 2, n, H, W, seed)


@functools.lru_cache(maxsize=8)
def _conv_operands(Cin, Cout, k, s, amp, n, H, W, seed):
    g = gen_for("conv", Cin, Cout, k, s, n, H, W, seed)
    cin = 3 if Cin == 4 else Cin
    return ints(g, (n, H, W, cin), amp), ints(g, (Cout, k, k, cin), amp), ints(g, (Cout,), 2)


@functools.lru_cache(maxsize=8)
def conv_case_ref(c, n, H, W):
    """(x, w, b, fp64 reference) of case c on n images of H x W; shared by the precisions that run the same operands."""
    x, w, b = conv_operands(c, n, H, W, seed=SEED_416.get(c.io, 0) if c.Cin == 416 else 0)
    return x, w, b, _conv_ref_cached(c.Cin, c.Cout, c.k, c.s, c.act, 1 if (c.io[1] == "b" or c.Cin > 96) else 2, n, H, W,
                                     SEED_416.get(c.io, 0) if c.Cin == 416 else 0)


@functools.lru_cache(maxsize=8)
def _conv_ref_cached(Cin, Cout, k, s, act, amp, n, H, W, seed):
    x, w, b = _conv_operands(Cin, Cout, k, s, amp, n, H, W, seed)
    return conv_ref(x, w, b, k, s, act)


def conv_ref(x, w, b, k, s, act, mutate=None):
    """fp64 F.conv2d with zero padding, NHWC in and out."""
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), b.double(), stride=s, padding=k // 2)
    if mutate == "drop_border_tap":  # the centre tap of the last output row of the last image
        Ho = y.shape[2]
        row = x[-1, min(s * (Ho - 1), x.shape[1] - 1), ::s].double()           # [Wo][Cin]: the pixels under the centre tap
        y = y.clone()
        y[-1, :, Ho - 1, :] -= (row[:y.shape[3]] @ w[:, k // 2, k // 2].double().t()).t()
    else:
        assert mutate is None
    return act_ref(y, act).permute(0, 2, 3, 1).contiguous()


# the one 3 x 3 x 416 case with a bf16 output: K = 3744, so a +-1 sum reaches 256 at 4.2 sigma; the seed is the first whose fp64
# reference stays inside (found on the CPU; the test asserts it)
SEED_416 = {"bb": 7}


def bf(t):
    return t.to(torch.bfloat16).double()


def assert_rounds(got, want, what):
    """Every element rounds to the planted integer and lies within 0.25 of it."""
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got.round() == want) & ((got - want).abs() <= 0.25))  # (a NaN is bad)
    if bool(bad.any()):
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements miss their integer; first at {i}: got {got[tuple(i)].item()} want {want[tuple(i)].item()}")


def assert_exact(got, want, what):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = got != want
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {i}: got {got[tuple(i)].item()} want {want[tuple(i)].item()}")


def breaks(check, got, want):
    try:
        check(got, want, "mutated")
    except AssertionError:
        return True
    return False


# ---- the fused row kernels' planted stages (integers throughout; `emulate_*` = fp64 with the kernel's roundings)


def block_weights(g, H):
    """fc1 16 * {+-1} with biases that are multiples of 16, fc2 {+-1}, integer fc2 bias."""
    W1 = 16.0 * ints(g, (H, C), 1)
    b1 = 16.0 * torch.randint(-2, 3, (H,), generator=g).float()
    return W1, b1, ints(g, (C, H), 1), ints(g, (C,), 3)


def mlp_want(x, s, W1, b1, W2, b2, skip_chunk=None):
    """x + relu(s W1^T + b1) W2^T + b2 in integers (s = the signs of x = its LayerNorm in bf16)."""
    h = F.relu(s.double() @ W1.double().t() + b1.double())
    if skip_chunk is not None:
        h[:, 256 * skip_chunk:256 * (skip_chunk + 1)] = 0
    return x.double() + h @ W2.double().t() + b2.double()


def emulate_mlp(x, W1, b1, W2, b2, eps=1e-6):
    ln = bf(F.layer_norm(x.double(), (C,), None, None, eps).float())
    pre = (ln @ bf(W1).t() + b1.double()).float()
    hid = F.gelu(pre, approximate="tanh")
    assert torch.equal(hid, F.relu(pre)) and torch.equal(bf(hid), hid.double()), "tanh-gelu is not the identity / zero here, or the hidden tile is not exact in bf16"
    assert float(pre.abs().max()) <= 4096
    return x.double() + bf(hid) @ bf(W2).t() + b2.double()


def proj_want(s, Wn, bn, lnw=None, lnb=None):
    a = s.double() if lnw is None else s.double() * lnw.double() + lnb.double()
    return a @ Wn.double().t() + bn.double()


def emulate_proj(x, Wn, bn, lnw, lnb, eps, y_bf16):
    ln = F.layer_norm(x.float(), (C,), lnw, lnb, eps)
    y = bf(ln) @ bf(Wn).t() + bn.double()
    return bf(y.float()) if y_bf16 else y


# the follow-up projections of stage (c): (N, affine, y_bf16); ldy = N + 8, eps 1e-5 with affine parameters (the updater's own)
NEXTS = [(576, True, False), (200, False, False), (864, False, True)]
NEXTS_BF16_AFFINE = [(288, True, True), (576, False, False)]


def next_operands(g, N, affine, y_bf16):
    Wn, bn = ints(g, (N, C), 1), ints(g, (N,), 3)
    lnw = lnb = None
    if affine:
        lnw, lnb = torch.randint(1, 3, (C,), generator=g).float(), torch.randint(4, 7, (C,), generator=g).float()
        if y_bf16:  # keep |y| <= 256: columns in pairs with one lnb and opposite weights, so that sum_k lnb_k Wn[n][k] = 0
            lnb[1::2] = lnb[0::2]
            Wn[:, 1::2] = -Wn[:, 0::2]
    return Wn, bn, lnw, lnb


# ------------------------------------------------------------------ CPU-only: the dispatch restated, the probes themselves


def all_variants():
    v = {("gemm", p, "dense", t) for p in PRECS for t in range(5)}
    v |= {("gemm", p, "im2col", t) for p in PRECS for t in range(5)}
    v |= {("gemm", p, "stem", t) for p in PRECS for t in (2, 4)}
    v |= {("gemm", p, "ln", t) for p in ("bf16x3", "bf16") for t in range(5)}
    v |= {("halo", p, bn) for p in ("bf16x3", "bf16") for bn in (64, 96, 128)}
    for k, s in ((3, 1), (3, 2), (1, 1), (1, 2)):
        v |= {("rows", k, s, tn, inb, st) for tn in (2, 3) for inb in (False, True) for st in (False, True) if not (st and k == 1 and tn == 3)}
    v |= {("big",), ("down", 2), ("down", 3)}
    v |= {("stem_rows", tn, st) for tn in (1, 2) for st in (False, True)}
    v |= {("block", 2, 0), ("block", 1, 0), ("block", 1, 1), ("block", 1, 2), ("ln_proj", 2, 3), ("ln_proj", 1, 2), ("mlp", 256)}
    return v


def reached_variants():
    v = set()
    for (M, N) in GEMM_SHAPES:
        v |= {("gemm", p, "dense", pick_tile(M, N)) for p in PRECS}
    for (M, N), K in LN_CASES:
        v |= {("gemm", p, "ln", pick_tile(M, N)) for p in ("bf16x3", "bf16")}
    for c in CONV_CASES:
        v |= {conv_variant(c, *geo) for geo in conv_geos(c)}
    v |= {down_variant(co) for _, co, _ in DOWN_CASES}
    for M, ws in BLOCK_MS:
        v |= set(block_forms(M, ws))
    v |= {ln_proj_form(M) for M in LN_PROJ_MS}
    v.add(("mlp", 256))
    return v


def test_cases_reach_every_variant():
    assert [pick_tile(M, N) for M, N in GEMM_SHAPES] == GEMM_TILES
    for (M, N), t in zip(GEMM_SHAPES[:3], GEMM_TILES[:3]):  # each the smallest M of its tile: one row tile less falls back
        assert pick_tile(M - (M - 1) % TILE_ROWS[t] - 1, N) != t, (M, N)
    missing = all_variants() - reached_variants()
    assert not missing, sorted(missing, key=str)
    extra = reached_variants() - all_variants()
    assert not extra, sorted(extra, key=str)
    # every variant sees an image count n > 1, and every row-tile / halo variant both sides of its pixel tile
    multi = {conv_variant(c, *geo) for c in CONV_CASES for geo in conv_geos(c) if geo[0] > 1}
    assert {v for v in all_variants() if v[0] in ("rows", "big", "halo", "stem_rows")} <= multi
    assert rows_staged_fits(2, 3, 1, 4, 3) and rows_staged_fits(1, 3, 2, 4, 3) and not rows_staged_fits(2, 1, 1, 4, 3) and rows_staged_fits(2, 1, 2, 4, 2)
    assert block_forms(2048, True) == [("block", 1, 1), ("block", 1, 2)] and block_forms(2080, True) == block_forms(1000, True) == [("block", 1, 0)]


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_balanced_rows_normalise_to_unit_signs(eps):
    """LayerNorm of +-c rows with half the entries positive, rounded to bf16, is exactly +-1 (fp32 and fp64); with w in {1, 2} and
    b in {4, 5, 6} it is exactly +-w + b."""
    g = gen_for("ln", eps)
    for K in (128, 256, 1024):
        x, s = balanced_rows(g, 64, K)
        w, b = torch.randint(1, 3, (K,), generator=g).float(), torch.randint(4, 7, (K,), generator=g).float()
        for t in (x, x.double()):
            assert torch.equal(bf(F.layer_norm(t, (K,), None, None, eps).float()), s.double())
            assert torch.equal(bf(F.layer_norm(t, (K,), w.to(t.dtype), b.to(t.dtype), eps).float()), (s * w + b).double())
        assert bool((x.sum(1) == 0).all()) and bool(((s * w + b) != 0).all())


def test_gelu_is_relu_on_multiples_of_16():
    """tanh-gelu in fp32 maps every multiple of 16 in [-4096, 4096] to relu of itself, as torch computes it and in the kernels'
    form x / (1 + exp2(x (c0 + c1 x^2)))."""
    x = 16.0 * torch.arange(-256, 257).float()
    assert torch.equal(F.gelu(x, approximate="tanh"), F.relu(x))
    a = (x * x * -0.10294324 + -2.3022082) * x
    assert torch.equal(x * (1.0 / (1.0 + torch.exp2(a))), F.relu(x))
    assert torch.equal(bf(F.relu(x)), F.relu(x).double())


@pytest.mark.parametrize("M,N,K,bm", [(33, 131, 131, 64), (64, 64, 32, 64), (130917, 40, 36, 256), (8100, 1000, 70, 128)])
def test_gemm_probe_sees_index_bugs(M, N, K, bm):
    for act, res in COMBOS[:2]:
        A, W, b, R, ref = gemm_data(M, N, K, 2, act, res)
        assert float(ref.abs().max()) < 2 ** 24
        assert not breaks(assert_exact, ref.float(), ref)
        for bug in ("drop_k", "drop_last_ktile", "swap_cols", "shift_last_rows"):
            assert breaks(assert_exact, gemm_ref(A, W, b, R, act, mutate=bug, bm=bm), ref), (bug, act, res)


@pytest.mark.parametrize("c,geo", [(CONV_CASES[0], (1, 7, 31)), (Conv("bf16", "bb", 416, 256, 3, 1), (1, 9, 33)), (Conv("fp32", "ff", 4, 64, 7, 2), (1, 13, 61)),
                                   (Conv("bf16", "bb", 96, 96, 1, 2), (2, 9, 33)), (Conv("bf16", "ff", 64, 160, 3, 2), (1, 16, 65))], ids=str)
def test_conv_probe_sees_a_dropped_border_tap(c, geo):
    x, w, b = conv_operands(c, *geo, seed=SEED_416.get(c.io, 0) if c.Cin == 416 else 0)
    ref = conv_ref(x, w, b, c.k, c.s, c.act)
    assert float(ref.abs().max()) <= (256 if c.io[1] == "b" else 2 ** 24 - 1)
    assert torch.equal(bf(ref.float()), ref) or c.io[1] != "b"
    assert breaks(assert_exact, conv_ref(x, w, b, c.k, c.s, c.act, mutate="drop_border_tap"), ref)
    assert breaks(assert_exact, conv_ref(x, w.roll(1, 0), b.roll(1, 0), c.k, c.s, c.act), ref)  # output channels moved by one


@pytest.mark.parametrize("M,H", [(1, 256), (31, 1024), (4129, 512)])
def test_fused_probe_sees_index_bugs(M, H):
    g = gen_for("fused-probe", M, H)
    x, s = balanced_rows(g, M, C)
    W1, b1, W2, b2 = block_weights(g, H)
    want = mlp_want(x, s, W1, b1, W2, b2)
    assert float(want.abs().max()) < 2 ** 22
    assert_rounds(emulate_mlp(x, W1, b1, W2, b2), want, "emulation")
    assert breaks(assert_rounds, mlp_want(x, s, W1, b1, W2, b2, skip_chunk=H // 256 - 1), want)
    W1d = W1.clone()
    W1d[:, C - 1] = 0
    assert breaks(assert_rounds, mlp_want(x, s, W1d, b1, W2, b2), want)                       # one k of fc1
    W2d = W2.clone()
    W2d[:, 64 * ((H - 1) // 64):] = 0
    assert breaks(assert_rounds, mlp_want(x, s, W1, b1, W2d, b2), want)                       # the last k-tile of fc2
    assert breaks(assert_rounds, want[:, [1, 0] + list(range(2, C))], want)                   # two output columns swapped
    if M > 1:
        r0 = (M - 1) // 32 * 32
        r0 = r0 if M - r0 >= 2 else r0 - 32
        assert breaks(assert_rounds, torch.cat([want[:r0], want[r0 + 1:], want[r0:r0 + 1]]), want)  # the last row tile shifted by one
    for N, affine, yb in NEXTS + NEXTS_BF16_AFFINE:
        Wn, bn, lnw, lnb = next_operands(g, N, affine, yb)
        y = proj_want(s, Wn, bn, lnw, lnb)
        assert float(y.abs().max()) <= (256 if yb else 2 ** 22)
        assert_rounds(emulate_proj(x, Wn, bn, lnw, lnb, 1e-5 if affine else 1e-6, yb), y, "emulated projection")
        Wd = Wn.clone()
        Wd[:, 0] = 0
        assert breaks(assert_rounds, proj_want(s, Wd, bn, lnw, lnb), y)
        assert breaks(assert_rounds, y[:, [1, 0] + list(range(2, N))], y)


# ------------------------------------------------------------------ device staging


def padded(t, ld, rows=None, dtype=torch.float32, fill=NAN, zero_to=None):
    """[rows][ld] on the device: t in the leading columns, zeros up to column zero_to, `fill` everywhere else."""
    out = torch.full((rows or t.shape[0], ld), fill, dtype=dtype)
    if zero_to:
        out[:t.shape[0], :zero_to] = 0
    out[:t.shape[0], :t.shape[1]] = t.to(dtype)
    return out.to(DEV)


def weights_bf16(hip, w, mult=64):
    """[N][K] fp32 integers -> (fp32 zero padded to a multiple of `mult` on the device, its bf16 hi, its bf16 lo)."""
    N, K = w.shape
    wp = torch.zeros(N, cdiv(K, mult) * mult)
    wp[:, :K] = w
    wp = wp.to(DEV)
    hi, lo = torch.empty(wp.shape, device=DEV, dtype=torch.int16), torch.empty(wp.shape, device=DEV, dtype=torch.int16)
    hip.split_bf16(wp, hi, lo, wp.numel())
    return wp, hi, lo


def frag(hip, w):
    """[N][K] values that are exact in bf16 -> the fragment-major bf16 image of mvt_pack_frag_bf16."""
    N, K = w.shape
    hi = w.to(torch.bfloat16).contiguous().view(torch.int16).to(DEV)
    out = torch.empty(cdiv(N, 32) * 32 * K, device=DEV, dtype=torch.int16)
    hip.pack_frag_bf16(hi, K, N, K, out)
    return out


def take(out, rows, cols, what):
    """The [rows][cols] result; every other element of `out` must still be poisoned."""
    torch.cuda.synchronize()
    o = out.double()
    assert bool(torch.isnan(o[:rows, cols:]).all()), f"{what}: columns past {cols} written"
    assert bool(torch.isnan(o[rows:]).all()), f"{what}: rows past {rows} written"
    return o[:rows, :cols].cpu()


# ------------------------------------------------------------------ B: GEMM


def run_gemm(hip, prec, A, W, b, R, act, out_dtype=torch.float32):
    M, K = A.shape
    N = W.shape[0]
    kp4 = cdiv(K, 4) * 4
    lda, ldc, ldr = kp4 + 4, N + 5, N + 3
    Ad = padded(A, lda, zero_to=kp4)  # (columns K .. round_up(K, 4) are K padding and read: zeros; past them: NaN)
    wp, hi, lo = weights_bf16(hip, W)
    Rd = padded(R, ldr) if R is not None else None
    out = torch.full((M + 3, ldc), NAN, device=DEV, dtype=out_dtype)
    if prec == "fp32":
        hip.gemm(Ad, lda, wp, wp.shape[1], b.to(DEV), Rd, ldr, out, ldc, M, N, K, act)
    else:
        hip.gemm_bf16(Ad, lda, hi, lo if prec == "bf16x3" else None, wp.shape[1], b.to(DEV), Rd, ldr, out, ldc, M, N, K, act)
    return take(out, M, N, f"gemm {prec} {M}x{N}x{K}")


@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,N", GEMM_SHAPES)
def test_gemm_exact(hip, M, N, prec):
    for i, K in enumerate(gemm_ks(M)):
        act, res = COMBOS[(i + M) % 4]
        A, W, b, R, ref = gemm_data(M, N, K, 2, act, res)
        assert float(ref.abs().max()) < 2 ** 24
        assert_exact(run_gemm(hip, prec, A, W, b, R, act), ref, f"{prec} M={M} N={N} K={K} act={act} res={res} (tile {pick_tile(M, N)})")


@gpu
@pytest.mark.parametrize("shape,K", GEMM_BF16_OUT, ids=str)
def test_gemm_exact_bf16_output(hip, shape, K):
    M, N = shape
    for act, res in COMBOS[:2]:
        A, W, b, R, ref = gemm_data(M, N, K, 1, act, res)
        assert float(ref.abs().max()) <= 256
        assert_exact(run_gemm(hip, "bf16", A, W, b, R, act, torch.bfloat16), ref, f"bf16 out M={M} N={N} K={K} act={act}")


@functools.lru_cache(maxsize=2)
def ln_data(M, N, K):
    g = gen_for("ln_gemm", M, N, K)
    A, s = balanced_rows(g, M, K)
    W, b, R = ints(g, (N, K), 1), ints(g, (N,), 3), ints(g, (M, N), 3)
    lw, lb = torch.randint(1, 3, (K,), generator=g).float(), torch.randint(4, 7, (K,), generator=g).float()
    return A, s, W, b, R, lw, lb


@gpu
@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("shape,K", LN_CASES, ids=str)
def test_ln_gemm_exact(hip, shape, K, prec):
    M, N = shape
    A, s, W, b, R, lw, lb = ln_data(M, N, K)
    wp, hi, lo = weights_bf16(hip, W)
    lda, ldc, ldr = K + 4, N + 5, N + 3
    Ad, Rd = padded(A, lda), padded(R, ldr)
    for i, (affine, eps) in enumerate([(False, 1e-6), (True, 1e-5)]):
        act, res = COMBOS[(i + M) % 4]
        ref = gemm_ref(s * lw + lb if affine else s, W, b, R if res else None, act)
        assert float(ref.abs().max()) < 2 ** 24
        out = torch.full((M + 3, ldc), NAN, device=DEV)
        hip.ln_gemm_bf16(Ad, lda, lw.to(DEV) if affine else None, lb.to(DEV) if affine else None, eps, hi, lo if prec == "bf16x3" else None,
                         wp.shape[1], b.to(DEV), Rd if res else None, ldr, out, ldc, M, N, K, act)
        what = f"ln_gemm {prec} M={M} N={N} K={K} affine={affine} act={act} res={res} (tile {pick_tile(M, N)})"
        (assert_exact if prec == "bf16" else assert_rounds)(take(out, M, N, what), ref, what)


# ------------------------------------------------------------------ C: convolution


def run_conv(hip, c, n, H, W, x, w, b):
    stem = c.Cin == 4
    Ho, Wo = conv_out(H, W, c.k, c.s)
    if stem:  # [n][H][W][4] fp32 input, weight row = [kh][8][4] with kw < 7, c < 3
        x4 = torch.zeros(n, H, W, 4)
        x4[..., :3] = x
        wt = torch.zeros(c.Cout, 7, 8, 4)
        wt[:, :, :7, :3] = w
        x, w = x4, wt
    dt = lambda ch: torch.bfloat16 if ch == "b" else torch.float32
    xd = x.to(dt(c.io[0])).contiguous().to(DEV)
    wp, hi, lo = weights_bf16(hip, w.reshape(c.Cout, -1))
    ldo = c.Cout + c.ldo_extra
    out = torch.full((n * Ho * Wo + 5, ldo), NAN, device=DEV, dtype=dt(c.io[1]))
    if c.prec == "fp32":
        hip.conv2d(xd, wp, b.to(DEV), out, n, H, W, c.Cin, c.Cout, c.k, c.k, c.s, c.k // 2, ldo, c.act)
    else:
        hip.conv2d_bf16(xd, hi, lo if c.prec == "bf16x3" else None, b.to(DEV), out, n, H, W, c.Cin, c.Cout, c.k, c.k, c.s, c.k // 2, ldo, c.act,
                        short_wg=c.short)
    return take(out, n * Ho * Wo, c.Cout, conv_id(c)).reshape(n, Ho, Wo, c.Cout)


@gpu
@pytest.mark.parametrize("c", CONV_CASES, ids=conv_id)
def test_conv_exact(hip, c, monkeypatch):
    monkeypatch.setenv("MVT_CONV_BIG", "1" if c.big else "0")
    for (n, H, W) in conv_geos(c):
        x, w, b, ref = conv_case_ref(c._replace(geos=None), n, H, W)
        assert float(ref.abs().max()) <= (256 if c.io[1] == "b" else 2 ** 24 - 1)
        assert_exact(run_conv(hip, c, n, H, W, x, w, b), ref, f"{conv_id(c)} n={n} H={H} W={W} -> {conv_variant(c, n, H, W)}")


@gpu
@pytest.mark.parametrize("Cin,Cout,ldo_extra", DOWN_CASES)
def test_conv3x3s2_down_exact(hip, Cin, Cout, ldo_extra):
    """Both outputs of the fused stride-2 ResidualBlock entry: the 3x3 / stride-2 conv and the 1x1 / stride-2 downsample."""
    c3, c1 = Conv("bf16", "bb", Cin, Cout, 3, 2), Conv("bf16", "bb", Cin, Cout, 1, 2)
    ldo = Cout + ldo_extra
    for (n, H, W) in GEOS + [(1, 8, 64)]:
        x, w3, b3 = conv_operands(c3, n, H, W)
        _, wd, bd = conv_operands(c1, n, H, W, seed=1)
        r3, rd = conv_ref(x, w3, b3, 3, 2, ACT_NONE), conv_ref(x, wd, bd, 1, 2, ACT_NONE)
        assert float(r3.abs().max()) <= 256 and float(rd.abs().max()) <= 256 and r3.shape == rd.shape
        Ho, Wo = r3.shape[1:3]
        _, h3, _ = weights_bf16(hip, w3.reshape(Cout, -1))
        _, hd, _ = weights_bf16(hip, wd.reshape(Cout, -1))
        o3 = torch.full((n * Ho * Wo + 5, ldo), NAN, device=DEV, dtype=torch.bfloat16)
        od = o3.clone()
        hip.conv3x3s2_down_bf16(x.to(torch.bfloat16).to(DEV), h3, b3.to(DEV), hd, bd.to(DEV), o3, od, n, H, W, Cin, Cout, ldo)
        what = f"down cin={Cin} cout={Cout} n={n} H={H} W={W}"
        assert_exact(take(o3, n * Ho * Wo, Cout, what).reshape(r3.shape), r3, what + " (3x3)")
        assert_exact(take(od, n * Ho * Wo, Cout, what).reshape(rd.shape), rd, what + " (1x1)")


# ------------------------------------------------------------------ D: the fused row kernels

LDXP = C + 8


def x_rows(x, guard=64):
    return padded(x, LDXP, rows=x.shape[0] + guard)


def make_nexts(hip, g, M, specs, rows=None):
    """(dicts for the binding, [(Wn, bn, lnw, lnb, eps, y, N, yb, (lo, hi))]) for the follow-up projections `specs`."""
    dicts, info = [], []
    for i, (N, affine, yb) in enumerate(specs):
        Wn, bn, lnw, lnb = next_operands(g, N, affine, yb)
        eps = 1e-5 if affine else 1e-6
        y = torch.full((M + 64, N + 8), NAN, device=DEV, dtype=torch.bfloat16 if yb else torch.float32)
        d = dict(w=frag(hip, Wn), ldw=C, b=bn.to(DEV), N=N, y=y, ldy=N + 8, eps=eps)
        if affine:
            d.update(lnw=lnw.to(DEV), lnb=lnb.to(DEV))
        rng = rows[i] if rows else None
        if rng:
            d["rows"] = rng
        dicts.append(d)
        info.append((Wn, bn, lnw, lnb, eps, y, N, yb, rng))
    return dicts, info


def check_nexts(x, s, info, M, what):
    for i, (Wn, bn, lnw, lnb, eps, y, N, yb, rng) in enumerate(info):
        want = proj_want(s, Wn, bn, lnw, lnb)
        assert float(want.abs().max()) <= (256 if yb else 2 ** 22)
        assert_rounds(emulate_proj(x, Wn, bn, lnw, lnb, eps, yb), want, f"{what}: emulated projection {i}")
        lo, hi = (rng[0], rng[1] or M) if rng else (0, M)
        torch.cuda.synchronize()
        yc = y.double().cpu()
        assert bool(torch.isnan(yc[:, N:]).all()), f"{what}: projection {i} wrote its padding columns"
        assert bool(torch.isnan(yc[:lo, :N]).all()) and bool(torch.isnan(yc[hi:, :N]).all()), f"{what}: projection {i} wrote outside rows [{lo}, {hi})"
        assert_rounds(yc[lo:hi, :N], want[lo:hi], f"{what}: projection {i} (N={N}, affine={lnw is not None}, bf16 y={yb})")


def workspace(M, H, ws):
    return torch.full(((H // 256 + 1) * M * C,), NAN, device=DEV) if ws else None


def call_block(hip, xd, att, wo, bo, w1, b1, w2, b2, H, nexts, M, ws):
    hip.block_fused_bf16(xd, LDXP, att, KO + 8, KO, wo, KO, bo, w1, C, b1, w2, H, b2, H, nexts, M, C, ws=ws)


@gpu
@pytest.mark.parametrize("att_bf16", [False, True], ids=["att-fp32", "att-bf16"])
@pytest.mark.parametrize("M,ws", BLOCK_MS)
def test_block_attention_projection_exact(hip, M, ws, att_bf16):
    """(a) x += att Wo^T + bo alone: W2 = 0 and b2 = 0, so the MLP adds exactly nothing."""
    g = gen_for("block-a", M)
    H = 512
    x, att = ints(g, (M, C), 8), ints(g, (M, KO), 3)
    Wo, bo = ints(g, (C, KO), 1), ints(g, (C,), 3)
    W1, b1, _, _ = block_weights(g, H)
    want = x.double() + att.double() @ Wo.double().t() + bo.double()
    assert float(want.abs().max()) < 2 ** 22
    xd = x_rows(x)
    attd = padded(att, KO + 8, dtype=torch.bfloat16 if att_bf16 else torch.float32)
    zero = torch.zeros(C, device=DEV)
    call_block(hip, xd, attd, frag(hip, Wo), bo.to(DEV), frag(hip, W1), b1.to(DEV), frag(hip, torch.zeros(C, H)), zero, H, [], M, workspace(M, H, ws))
    what = f"block (a) M={M} ws={ws} -> {block_forms(M, ws)}"
    assert_rounds(take(xd, M, C, what), want, what)


@gpu
@pytest.mark.parametrize("H", [256, 1024])
@pytest.mark.parametrize("M,ws", BLOCK_MS)
def test_block_mlp_exact(hip, M, ws, H):
    """(b) x += W2 gelu(W1 LayerNorm(x) + b1) + b2 alone (no attention input)."""
    g = gen_for("block-b", M, H)
    x, s = balanced_rows(g, M, C)
    W1, b1, W2, b2 = block_weights(g, H)
    want = mlp_want(x, s, W1, b1, W2, b2)
    assert float(want.abs().max()) < 2 ** 22
    assert_rounds(emulate_mlp(x, W1, b1, W2, b2), want, "fp64 emulation")
    xd = x_rows(x)
    call_block(hip, xd, None, None, None, frag(hip, W1), b1.to(DEV), frag(hip, W2), b2.to(DEV), H, [], M, workspace(M, H, ws))
    what = f"block (b) M={M} H={H} ws={ws} -> {block_forms(M, ws)}"
    assert_rounds(take(xd, M, C, what), want, what)


def row_ranges(M):
    return [(0, 0), (M // 3, M - M // 4), (M - M // 4, 0)] if M >= 8 else None


@gpu
@pytest.mark.parametrize("ranges", [False, True], ids=["all-rows", "row-ranges"])
@pytest.mark.parametrize("M,ws", BLOCK_MS)
def test_block_followup_projections_exact(hip, M, ws, ranges):
    """(c) y_i = LayerNorm(x) Wn_i^T + bn_i alone: W2 = 0 keeps x balanced, so every y is an exact integer; x must come back as
    it went in."""
    g = gen_for("block-c", M)
    H = 256
    x, s = balanced_rows(g, M, C)
    W1, b1, _, _ = block_weights(g, H)
    nexts, info = make_nexts(hip, g, M, NEXTS, row_ranges(M) if ranges else None)
    xd = x_rows(x)
    zero = torch.zeros(C, device=DEV)
    call_block(hip, xd, None, None, None, frag(hip, W1), b1.to(DEV), frag(hip, torch.zeros(C, H)), zero, H, nexts, M, workspace(M, H, ws))
    what = f"block (c) M={M} ws={ws} ranges={ranges} -> {block_forms(M, ws)}"
    assert_exact(take(xd, M, C, what), x, what + ": x")
    check_nexts(x, s, info, M, what)


@gpu
@pytest.mark.parametrize("specs", [NEXTS, NEXTS_BF16_AFFINE], ids=["three", "bf16-affine"])
@pytest.mark.parametrize("ranges", [False, True], ids=["all-rows", "row-ranges"])
@pytest.mark.parametrize("M", LN_PROJ_MS)
def test_ln_proj_exact(hip, M, ranges, specs):
    g = gen_for("ln_proj", M)
    x, s = balanced_rows(g, M, C)
    nexts, info = make_nexts(hip, g, M, specs, row_ranges(M) if ranges else None)
    xd = x_rows(x)
    before = xd.clone()
    hip.ln_proj_bf16(xd, LDXP, nexts, M, C)
    torch.cuda.synchronize()
    assert torch.equal(xd.view(torch.int32), before.view(torch.int32))  # x is only read
    check_nexts(x, s, info, M, f"ln_proj M={M} ranges={ranges} -> {ln_proj_form(M)}")


@gpu
@pytest.mark.parametrize("H", [64, 256, 1024])
@pytest.mark.parametrize("M", MLP_MS)
def test_mlp_fused_exact(hip, M, H):
    g = gen_for("mlp", M, H)
    x, s = balanced_rows(g, M, C)
    W1, b1, W2, b2 = block_weights(g, H)
    want = mlp_want(x, s, W1, b1, W2, b2)
    assert float(want.abs().max()) < 2 ** 22
    assert_rounds(emulate_mlp(x, W1, b1, W2, b2), want, "fp64 emulation")
    xd = x_rows(x)
    ld1, ld2 = C + 8, H + 8
    w1 = padded(W1, ld1, dtype=torch.bfloat16, fill=0.0).view(torch.int16)
    w2 = padded(W2, ld2, dtype=torch.bfloat16, fill=0.0).view(torch.int16)
    hip.mlp_fused_bf16(xd, LDXP, w1, ld1, b1.to(DEV), w2, ld2, b2.to(DEV), M, C, H, 1e-6)
    assert_rounds(take(xd, M, C, f"mlp_fused M={M} H={H}"), want, f"mlp_fused M={M} H={H}")
