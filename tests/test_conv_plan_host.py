"""The launch plans of the GEMM and convolution kernels and of the composite encoder (mvtracker_amd/csrc/conv_plan.h), on the CPU.

The header is the one statement of every rule of that dispatch: the entries of gemm.hip and conv_rows.hip launch what it returns,
mvt_conv2d_stat_slots is its conv_stat_slots and encoder_forward.hip walks its table of the network's convolutions.  It is
HIP-free, so the host compiler alone builds tests/conv_plan_probe.cpp around it (plan_probe.py, shared with
test_launch_plan_host.py); the probe runs ONCE over every case below and the tests compare its answers with

  (a) the dispatch restatements that the exact GPU suites select their cases by -- conv_variant, rows_tile, rows_staged_fits,
      pick_tile, halo_tile, down_variant (test_gpu_matmul_exact.py), conv_variant, tile_rows, stat_slots
      (test_gpu_encoder_norm_exact.py), switched_slots (test_gpu_tuning_switches.py): a threshold edited in the header and not
      in a restatement (or the other way round) fails here, not as a green suite that no longer runs the new side of it;
  (b) the launch table written out below, independently of the header (template tuple, workgroup size, grid, tile rows, slots and
      weight stride of every family, and every refusal): the record of what the entries launched before the rules moved into the
      header.  A wrong grid on these kernels is an out-of-bounds access, not a failed assertion, so this test comes before any GPU run;
  (c) tests/golden/conv_stat_slots.json, the values of mvt_conv2d_stat_slots recorded from the build before the move, for the
      header under every MVT_ROWS_NW8 value and for the built library (a pure host function: the library loads without a GPU).

One answer differs from that record on purpose (table_conv says where): statistics of the stem shape with more than 64 output
channels.  The call ran the im2col GEMM kernel, which writes one slot per 32 output pixels, into a buffer that the caller had sized
by the stem's 8 x 32 tiles: a write past out_partial.  The plan refuses out_partial wherever the family that runs does not write
the slots of conv_stat_slots.

The sweeps take the smallest values on both sides of every threshold, not the workload's shapes.  The full product of all of
them is out of reach (10^10 cases), so they are crossed in groups: the shape dimensions with the precision, tensor types,
activation and statistics (A); the switches, short workgroups and ldo with the shapes that reach the row tiles (B); each
alignment fact against the calls that ask for it (C); three images (D); the image counts that reach the larger GEMM tiles (E).
"""
import collections
import functools
import itertools
import json
import os
import subprocess
import sys

import pytest

import test_gpu_encoder_norm_exact as EN
import test_gpu_matmul_exact as MM
import test_gpu_tuning_switches as TS
from plan_probe import ROOT, run_probe


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ the sweeps

KERNELS = [(1, 1, 1, 0), (1, 1, 2, 0), (3, 3, 1, 1), (3, 3, 2, 1), (7, 7, 2, 3), (3, 3, 1, 0), (5, 5, 1, 2), (1, 3, 1, 0)]  # (KH, KW, stride, pad)
CINS = (4, 32, 64, 96, 416)
COUTS = (1, 31, 32, 33, 64, 96, 128, 192, 256, 288, 512)
SIZES = TS.SLOT_SIZES + [(1, 1), (2, 2), (15, 31), (16, 32), (17, 33), (32, 64)]
IOS = ("ff", "fb", "bf", "bb")
LDO_EXTRA = (0, 1, 4, 8)
NW8 = (0, 1, 2, 3)
ALIGN = ("in16", "out16", "w8", "w16", "lo8", "st16")
GEMM_M = (1, 63, 64, 65, 255, 256, 257, 32767, 32768, 65536, 131072)
GEMM_N = (1, 32, 64, 65, 96, 128, 131, 192, 288, 864, 1024)

Call = collections.namedtuple("Call", "n H W Cin Cout KH KW s p ldo_extra act io short fp32 lo stats part in16 out16 w8 w16 lo8 st16 nw8 big",
                              defaults=(0, 0, "ff", 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1))


@functools.lru_cache(maxsize=None)
def conv_cases():
    """Built on first use: collecting this module costs nothing."""
    out = []
    shapes = [(H, W, Cin, Cout, *k) for k in KERNELS for Cin in CINS for Cout in COUTS for H, W in SIZES]
    # A: shape x precision x tensor types x activation x statistics
    for sh, io, lo, act, (stats, part) in itertools.product(shapes, IOS, (0, 1), (0, 1), itertools.product((0, 1), (0, 1))):
        out.append(Call(1, *sh, io=io, lo=lo, act=act, stats=stats, part=part))
    out += [Call(1, *sh, fp32=1, act=act) for sh in shapes for act in (0, 1)]
    # B: the switches, short workgroups and ldo, where the row tiles, the big tile and the stem are chosen (bf16 mode, no activation)
    few = [(H, W, Cin, Cout, *k) for k in KERNELS[:5] for Cin in (4, 32, 416) for Cout in (32, 33, 64, 96, 256, 288, 512) for H, W in ((16, 32), (17, 33), (32, 64), (5, 7))]
    for sh, io, nw8, big, short, extra, (stats, part) in itertools.product(few, IOS, NW8, (0, 1), (0, 1), LDO_EXTRA, itertools.product((0, 1), (0, 1))):
        out.append(Call(1, *sh, ldo_extra=extra, io=io, short=short, stats=stats, part=part, nw8=nw8, big=big))
    # C: each alignment fact false, alone
    for sh, io, lo, (stats, part), fact, fp32 in itertools.product(few, ("ff", "bb"), (0, 1), itertools.product((0, 1), (0, 1)), ALIGN, (0, 1)):
        if not fp32 or (io == "ff" and not lo and not stats and not part):
            out.append(Call(1, *sh, io=io, lo=lo, stats=stats, part=part, fp32=fp32, **{fact: 0}))
    # D: three images
    for sh, io, lo, part in itertools.product(shapes, ("ff", "bb"), (0, 1), (0, 1)):
        out.append(Call(3, *sh, io=io, lo=lo, part=part))
    out += [Call(3, *sh, fp32=1) for sh in shapes]
    # E: image counts at which the im2col GEMM has 512 workgroups of its larger tiles (1x1: K = 32; the stem at full size)
    for n, sh in ((32, (33, 31, 32, 256, 1, 1, 1, 0)), (128, (33, 31, 32, 64, 1, 1, 1, 0)), (16, (33, 31, 32, 256, 1, 1, 1, 0)), (32, (130, 126, 4, 64, 7, 7, 2, 3))):
        out += [Call(n, *sh, fp32=1), Call(n, *sh, lo=1), Call(n, *sh, act=1)]
    return out


SLOT_CASES = [(H, W, Cin, *k, split, nw8) for nw8 in NW8 for k in KERNELS for Cin in CINS for H, W in SIZES for split in (0, 1)]
GEOS = [(tm, tn, ks, s, nw) for (tm, ks, s, nw) in ((2, 3, 1, 8), (1, 3, 1, 4), (2, 3, 1, 4), (1, 3, 2, 4), (2, 1, 1, 4), (2, 1, 2, 4)) for tn in (2, 3)]
DOWN_CASES = [(n, H, W, Cin, Cout, Cout + extra, same, al) for n in (1, 3) for H, W in SIZES if H > 1 for Cin in (32, 96, 416, 48) for Cout in (32, 64, 96, 160, 288, 33)
              for extra in LDO_EXTRA for same in (0, 1) for al in (0, 1)]
STEM_CASES = [(n, H, W, Cout, Cout + extra, io, al) for n in (1, 3) for H, W in SIZES for Cout in (1, 31, 32, 33, 64, 65) for extra in LDO_EXTRA for io in (0, 1, 2) for al in (0, 1)]
ENC_CASES = [(n, H, W, C, nw8, 1, fold) for n in (1, 3) for H, W in ((64, 64), (128, 96), (512, 512)) for C in (32, 128, 160) for nw8 in NW8 for fold in (0, 1)]


def sw(nw8=0, big=1, fold=1):
    return f"{nw8} {big} {fold}"


def conv_line(c):
    io = ("ff", "bf", "fb", "bb").index(c.io) | (4 if c.short else 0)  # MVT_IO_IN_BF16 = 1, OUT_BF16 = 2, SHORT_WG = 4
    return (f"conv {c.n} {c.H} {c.W} {c.Cin} {c.Cout} {c.KH} {c.KW} {c.s} {c.p} {c.Cout + c.ldo_extra} {c.act} {io} {c.fp32} {c.lo} {c.stats} {c.part} "
            f"{c.in16} {c.out16} {c.w8} {c.w16} {c.lo8} {c.st16} {sw(c.nw8, c.big)}")


def probe_input():
    out = [("gemm", f"gemm {M} {N}") for M in GEMM_M for N in GEMM_N]
    out += [("halo", f"halo {t} {N}") for t in (1, 7, 1000) for N in COUTS]
    out += [("fits", "fits {} {} {} {} {}".format(*g)) for g in GEOS]
    out += [("slots", "slots {} {} {} {} {} {} {} {} {}".format(*c[:8], sw(c[8]))) for c in SLOT_CASES]
    out += [("conv", conv_line(c)) for c in conv_cases()]
    out += [("stem", "stem {} {} {} {} {} {} {}".format(*c)) for c in STEM_CASES]
    out += [("down", "down {} {} {} {} {} {} {} {}".format(*c)) for c in DOWN_CASES]
    out += [("enc", "enc {} {} {} {} {}".format(*c[:4], sw(*c[4:]))) for c in ENC_CASES]
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """{tag: [answer lines]} of ONE run of the probe over every case of this module."""
    cases = probe_input()
    lines = run_probe(tmp_path_factory, "conv_plan_probe.cpp", [line for _, line in cases])
    assert len(lines) == len(cases)
    out = collections.defaultdict(list)
    for (tag, _), line in zip(cases, lines):
        out[tag].append(line)
    return out


def parse_plan(line):
    """-> None (refused) or (family, template tuple, threads, grid, tile rows, slots, ldw)."""
    if line == "refused":
        return None
    f = line.split()
    tm, tn, ks, s, nw, inb, staged, split, gtm, gtn, gwm, gwn, threads, grid, rows, slots, ldw = map(int, f[1:])
    tpl = {"gemm_f32": (gtm, gtn, gwm, gwn), "im2col": (gtm, gtn, gwm, gwn, split), "halo": (gtm, gtn, gwm, gwn, split), "stem_rows": (tn, staged),
           "rows": (tm, tn, ks, s, inb, nw, staged), "big": ()}[f[0]]
    return f[0], tpl, threads, grid, rows, slots, ldw


# ------------------------------------------------------------------ (b) the launch table, written out

# pick_tile's index -> the instantiation <TM, TN, WM, WN> and its tile (rows x columns)
GEMM_TILES = {0: ((2, 2, 2, 2), 128, 128), 1: ((1, 3, 4, 1), 128, 96), 2: ((2, 2, 4, 1), 256, 64), 3: ((1, 2, 2, 2), 64, 128), 4: ((1, 1, 2, 2), 64, 64)}
HALO_TILES = {96: (1, 3, 4, 1), 64: (1, 2, 4, 1), 128: (2, 2, 2, 2)}
# conv_rows_bf16<TM, TN, KS, S, INB, NW, STAGED>: where the staged epilogue is compiled -- NW staging tiles of 32 x (TN * 32 + 8) bf16
# within the patch of 40 bf16 per pixel slot: 18 x 34, 6 x 34, 10 x 34 (3x3), 9 x 66 (3x3 / stride 2), 8 x 32 (1x1) slots
STAGED = {(2, 2, 3, 1, 8): True, (2, 3, 3, 1, 8): False, (1, 2, 3, 1, 4): False, (1, 3, 3, 1, 4): False, (2, 2, 3, 1, 4): True, (2, 3, 3, 1, 4): True,
          (1, 2, 3, 2, 4): True, (1, 3, 3, 2, 4): True, (2, 2, 1, 1, 4): True, (2, 3, 1, 1, 4): False, (2, 2, 1, 2, 4): True, (2, 3, 1, 2, 4): False}
PATCH = {(2, 3, 1, 8): 18 * 34, (1, 3, 1, 4): 6 * 34, (2, 3, 1, 4): 10 * 34, (1, 3, 2, 4): 9 * 66, (2, 1, 1, 4): 8 * 32, (2, 1, 2, 4): 8 * 32}


def table_gemm(M, N):
    nb = lambda bm, bn: cdiv(M, bm) * cdiv(N, bn)
    if N % 128 != 0 and N % 96 == 0:
        t = 1
    elif N <= 64:
        t = 2 if nb(256, 64) >= 512 else 4
    else:
        t = 0 if nb(128, 128) >= 512 else (3 if nb(64, 128) >= 512 else 4)
    tpl, bm, bn = GEMM_TILES[t]
    return t, tpl, nb(bm, bn)


def table_halo(tiles, N):
    bn = 96 if (N % 128 != 0 and N % 96 == 0) else (64 if N <= 64 else 128)
    return bn, HALO_TILES[bn], tiles * cdiv(N, bn)


def table_rows(k, s, Ho, nw8):
    if (k, s) == (3, 1):
        return 16 if (nw8 == 1 and Ho % 16 == 0) else (4 if nw8 == 2 else 8)
    return 4 if k == 3 else 8


def table_slots(H, W, Cin, KH, KW, s, p, split, nw8):
    """mvt_conv2d_stat_slots."""
    Ho, Wo = (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1
    if Ho <= 0 or Wo <= 0:
        return 0
    if not split and Cin % 32 == 0 and KH == KW and ((KH, p) == (3, 1) or (KH, p) == (1, 0)):
        return cdiv(Ho, table_rows(KH, s, Ho, nw8)) * cdiv(Wo, 32)
    if (KH, KW, s, p) == (3, 3, 1, 1) and Cin % 32 == 0:
        return cdiv(Ho, 8) * cdiv(Wo, 16) * 4
    if not split and Cin == 4 and (KH, KW, s, p) == (7, 7, 2, 3):
        return cdiv(Ho, 8) * cdiv(Wo, 32)
    return Ho * Wo // 32 if (Ho * Wo) % 256 == 0 else 0


def table_conv(c):
    """What mvt_conv2d (c.fp32) / mvt_conv2d_bf16 launch for call c: (family, template, threads, grid, tile rows, slots, ldw), None = MVT_ERR_ARG."""
    inb, outb = c.io[0] == "b", c.io[1] == "b"
    ldo = c.Cout + c.ldo_extra
    if not (c.Cin % 32 == 0 or c.Cin == 4) or not c.in16:
        return None
    if (not c.w16) if c.fp32 else (not c.w8 or (c.lo and not c.lo8)):
        return None
    Ho, Wo = (c.H + 2 * c.p - c.KH) // c.s + 1, (c.W + 2 * c.p - c.KW) // c.s + 1
    if Ho <= 0 or Wo <= 0:
        return None
    M = c.n * Ho * Wo
    ldw = cdiv(c.KH * 32 if c.Cin == 4 else c.KH * c.KW * c.Cin, 64) * 64
    if c.fp32:
        _, tpl, blocks = table_gemm(M, c.Cout)
        return "gemm_f32", tpl, 256, blocks, 0, 0, ldw
    shape = (c.KH, c.KW, c.s, c.p)
    halo = shape == (3, 3, 1, 1) and c.Cin % 32 == 0
    rows = not c.lo and c.act == 0 and c.Cin % 32 == 0 and c.KH == c.KW and ((c.KH, c.p) == (3, 1) or (c.KH, c.p) == (1, 0))
    if c.stats and not ((halo or rows) and c.st16):
        return None
    if ((inb or outb) and c.lo) or (inb and c.Cin % 32 != 0):
        return None
    slots = table_slots(c.H, c.W, c.Cin, *shape, c.lo, c.nw8)
    if c.part and not (slots > 0 and (c.lo or c.act == 0)):
        return None
    st_ok = outb and c.Cout % 8 == 0 and ldo % 8 == 0 and bool(c.out16)
    if not c.lo and c.Cin == 4 and shape == (7, 7, 2, 3) and c.Cout <= 64 and c.act == 0:
        return "stem_rows", (1 if c.Cout <= 32 else 2, st_ok), 256, c.n * cdiv(Ho, 8) * cdiv(Wo, 32), 8, slots, ldw
    if rows:
        if c.stats and c.Cin > 512:
            return None
        tr = table_rows(c.KH, c.s, Ho, c.nw8)
        # the big tile writes the slots of its own 8-row tiles: with statistics only where the row tile, which sized them, has 8 rows
        if (c.KH == 3 and c.s == 1 and not c.stats and (not c.part or tr == 8) and not c.short and inb and st_ok and c.Cout % 256 == 0 and c.w16
                and c.big):
            return "big", (), 512, c.n * cdiv(Ho, 8) * cdiv(Wo, 32) * (c.Cout // 256), 8, slots, ldw
        tn = 3 if (c.Cout % 64 != 0 and c.Cout % 96 == 0) else 2
        tm, nw = {16: (2, 8), 8: (2, 4), 4: (1, 4)}[tr]
        staged = st_ok and STAGED[(tm, tn, c.KH, c.s, nw)]
        return "rows", (tm, tn, c.KH, c.s, inb, nw, staged), 64 * nw, c.n * cdiv(Ho, tr) * cdiv(Wo, 32) * cdiv(c.Cout, tn * 32), tr, slots, ldw
    if halo:
        _, tpl, blocks = table_halo(c.n * cdiv(Ho, 8) * cdiv(Wo, 16), c.Cout)
        return "halo", tpl + (c.lo,), 256, blocks, 0, slots, ldw
    if c.part and not c.lo and c.Cin == 4 and shape == (7, 7, 2, 3):
        return None  # the one deliberate difference (module docstring): before the move this launched the GEMM kernel with the stem's slots
    _, tpl, blocks = table_gemm(M, c.Cout)
    return "im2col", tpl + (c.lo,), 256, blocks, 0, slots, ldw


# ------------------------------------------------------------------ the tests


def test_gemm_and_halo_tiles(answers):
    """gemm_tile / halo_tile against the table and MM.pick_tile / MM.halo_tile; every tile is reached on both sides of 512 workgroups."""
    seen = set()
    for (M, N), line in zip(itertools.product(GEMM_M, GEMM_N), answers["gemm"]):
        t, tpl, blocks = table_gemm(M, N)
        assert tuple(map(int, line.split())) == tpl + (blocks,), (M, N, line)
        assert t == MM.pick_tile(M, N) and MM.TILE_ROWS[t] == GEMM_TILES[t][1]
        seen.add(t)
    assert seen == set(GEMM_TILES)
    for (tiles, N), line in zip(itertools.product((1, 7, 1000), COUTS), answers["halo"]):
        bn, tpl, blocks = table_halo(tiles, N)
        assert tuple(map(int, line.split())) == tpl + (blocks,), (tiles, N, line)
        assert bn == MM.halo_tile(N)


def test_staged_epilogue_fits(answers):
    """patch_slots / stage_elems / rows_staged_fits against the written-out record and the suites' rows_staged_fits."""
    for (tm, tn, ks, s, nw), line in zip(GEOS, answers["fits"]):
        patch, stage, fits = map(int, line.split())
        assert (patch, stage, bool(fits)) == (PATCH[(tm, ks, s, nw)], 32 * (tn * 32 + 8), STAGED[(tm, tn, ks, s, nw)]), (tm, tn, ks, s, nw, line)
        assert bool(fits) == MM.rows_staged_fits(tm, ks, s, nw, tn) == EN.rows_staged_fits(tm, ks, s, nw, tn)
    assert MM.rows_staged_fits is EN.rows_staged_fits and MM.rows_tile is EN.rows_tile and MM.conv_out is EN.conv_out and MM.env_int is EN.env_int


def test_stat_slots(answers):
    """conv_stat_slots against the table, the recorded values of the earlier build (c), and the tuning-switch suite's expectation."""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_stat_slots.json")))
    assert [tuple(k) for k in rec["kernels"]] == KERNELS and tuple(rec["cins"]) == CINS and [tuple(s) for s in rec["sizes"]] == SIZES
    recorded = {}
    for nw8 in NW8:
        order = [(H, W, Cin, *k, split, nw8) for k in KERNELS for Cin in CINS for H, W in SIZES for split in (0, 1)]
        recorded.update(zip(order, rec["slots"][str(nw8)]))
    assert len(answers["slots"]) == len(SLOT_CASES)
    zero = 0
    for c, line in zip(SLOT_CASES, answers["slots"]):
        assert int(line) == table_slots(*c) == recorded[c], (c, line)
        zero += int(line) == 0
    assert zero and any(recorded[c] != recorded[c[:8] + (0,)] for c in SLOT_CASES)
    at = {c: int(line) for c, line in zip(SLOT_CASES, answers["slots"])}
    for (H, W), nw8, Cin in itertools.product(TS.SLOT_SIZES, (1, 2), (32, 64, 416)):
        assert at[(H, W, Cin, 3, 3, 1, 1, 0, nw8)] == TS.switched_slots(H, W, 3, 1, nw8)
        assert at[(H, W, Cin, 3, 3, 2, 1, 0, nw8)] == TS.switched_slots(H, W, 3, 2, nw8)
        assert at[(H, W, Cin, 1, 1, 1, 0, 0, nw8)] == TS.switched_slots(H, W, 1, 1, nw8)


SLOTS_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
print(json.dumps([lib.mvt_conv2d_stat_slots(*c) for c in json.loads(sys.stdin.read())]))
"""


@pytest.mark.parametrize("nw8", [0, 1, 2])
def test_library_stat_slots_are_the_recorded_ones(nw8):
    """(c) for the built library: a child process per MVT_ROWS_NW8 value (the library reads it once) loads it and answers the sweep."""
    from mvtracker_amd import hip
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_stat_slots.json")))
    cases = [(H, W, Cin, *k, split) for k in KERNELS for Cin in CINS for H, W in SIZES for split in (0, 1)]
    env = dict(os.environ, MVT_ROWS_NW8=str(nw8))
    p = subprocess.run([sys.executable, "-c", SLOTS_CHILD, hip.LIB_PATH], input=json.dumps(cases), env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert json.loads(p.stdout) == rec["slots"][str(nw8)]
    if MM.env_int("MVT_ROWS_NW8") == nw8:
        assert [hip.conv2d_stat_slots(*c[:7], split=bool(c[7])) for c in cases] == rec["slots"][str(nw8)]


def mm_variant(c, plan):
    """The plan in the words of MM.conv_variant."""
    family, tpl = plan[:2]
    prec = "fp32" if c.fp32 else ("bf16x3" if c.lo else "bf16")
    tile = {v[0]: t for t, v in GEMM_TILES.items()}
    if family in ("gemm_f32", "im2col"):
        return ("gemm", prec, "stem" if c.Cin == 4 else "im2col", tile[tpl[:4]])
    if family == "halo":
        return ("halo", prec, {v: k for k, v in HALO_TILES.items()}[tpl[:4]])
    if family == "stem_rows":
        return ("stem_rows", tpl[0], bool(tpl[1]))
    if family == "big":
        return ("big",)
    tm, tn, ks, s, inb, nw, staged = tpl
    assert (tm, nw) == MM.rows_tile(ks, s, MM.conv_out(c.H, c.W, ks, s)[0], c.nw8)
    return ("rows", ks, s, tn, bool(inb), bool(staged))


def en_variant(plan):
    """The plan in the words of EN.conv_variant."""
    family, tpl = plan[:2]
    if family == "stem_rows":
        return ("stem", tpl[0], bool(tpl[1]))
    if family == "rows":
        return ("rows", tpl[2], tpl[3], tpl[1], bool(tpl[6]))
    return (family,)


def test_conv_plans(answers):
    """plan_conv against the table (b) over every sweep, and against the suites' restatements (a) wherever a call lies in their domain."""
    assert len(answers["conv"]) == len(conv_cases())
    seen, refused, mm_seen, en_seen, big_checked = set(), 0, set(), set(), 0
    for c, line in zip(conv_cases(), answers["conv"]):
        got = parse_plan(line)
        want = table_conv(c)
        if want is not None:
            want = (want[0], tuple(int(x) for x in want[1])) + want[2:]
        assert got == want, (c, line, want)
        if got is None:
            refused += 1
            continue
        family, tpl, threads, grid, rows, slots, ldw = got
        seen.add((family, tpl))
        assert 0 < grid < 2 ** 31
        if family == "big" and c.part:  # the big tile never runs where its own slots are not the caller's
            Ho, Wo = MM.conv_out(c.H, c.W, 3, 1)
            assert slots == cdiv(Ho, 8) * cdiv(Wo, 32) == table_slots(c.H, c.W, c.Cin, 3, 3, 1, 1, 0, c.nw8)
            big_checked += 1
        std = c.KH == c.KW and c.p == c.KH // 2 and all(getattr(c, a) for a in ALIGN)
        if std and not c.stats and not c.part:  # test_gpu_matmul_exact.py: no statistics
            m = MM.Conv("fp32" if c.fp32 else ("bf16x3" if c.lo else "bf16"), c.io, c.Cin, c.Cout, c.KH, c.s, c.act, c.ldo_extra, bool(c.short), bool(c.big))
            assert mm_variant(c, got) == MM.conv_variant(m, c.n, c.H, c.W, c.nw8), (c, line)
            mm_seen.add(mm_variant(c, got)[:2])
        en_domain = (c.KH in (1, 3) and c.Cin != 4) or ((c.KH, c.s, c.Cin) == (7, 2, 4) and (c.lo or c.Cout <= 64))
        if std and en_domain and c.part and not c.act and not c.short and not c.fp32 and (not c.stats or (c.KH, c.s) == (3, 1)):
            e = EN.Conv("bf16x3" if c.lo else "bf16", c.io, c.Cin, c.Cout, c.KH, c.s, c.ldo_extra, bool(c.stats), bool(c.big))
            Ho = EN.conv_out(c.H, c.W, c.KH, c.s)[0]
            assert en_variant(got) == EN.conv_variant(e, Ho, c.nw8), (c, line)
            assert slots == EN.stat_slots(e, c.H, c.W, c.nw8), (c, line)
            if family in ("rows", "big", "stem_rows"):
                assert rows == EN.tile_rows(e, Ho, c.nw8), (c, line)
            en_seen.add(en_variant(got)[0])
    families = {f for f, _ in seen}
    assert families == {"gemm_f32", "im2col", "halo", "stem_rows", "rows", "big"} and refused and big_checked
    # every instantiation the launchers name: 5 GEMM tiles (fp32; bf16 and bf16x3), 3 halo tiles x 2, 4 stems, the row tiles
    assert {t for f, t in seen if f == "gemm_f32"} == {v[0] for v in GEMM_TILES.values()}
    assert {t for f, t in seen if f == "im2col"} == {v[0] + (s,) for v in GEMM_TILES.values() for s in (0, 1)}
    assert {t for f, t in seen if f == "halo"} == {v + (s,) for v in HALO_TILES.values() for s in (0, 1)}
    assert {t for f, t in seen if f == "stem_rows"} == {(tn, st) for tn in (1, 2) for st in (0, 1)}
    want_rows = {(tm, tn, ks, s, inb, nw, st) for (tm, tn, ks, s, nw), fits in STAGED.items() for inb in (0, 1) for st in ((0, 1) if fits else (0,))}
    assert {t for f, t in seen if f == "rows"} == want_rows
    assert mm_seen >= {("gemm", "fp32"), ("gemm", "bf16"), ("gemm", "bf16x3"), ("halo", "bf16"), ("halo", "bf16x3"), ("stem_rows", 1), ("stem_rows", 2),
                       ("rows", 1), ("rows", 3), ("big",)}
    assert en_seen == {"halo", "im2col", "stem", "rows", "big"}


def test_stem_and_down_plans(answers):
    """plan_stem (both stem sources) and plan_down against the table and MM.down_variant / EN.down_tile."""
    ok = refused = 0
    for (n, H, W, Cout, ldo, io, al), line in zip(STEM_CASES, answers["stem"]):
        got = parse_plan(line)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        if Cout > 64 or (io & 1):
            assert got is None, line
            refused += 1
            continue
        staged = int(bool(io & 2) and Cout % 8 == 0 and ldo % 8 == 0 and bool(al))
        assert got == ("stem_rows", (1 if Cout <= 32 else 2, staged), 256, n * cdiv(Ho, 8) * cdiv(Wo, 32), 8, cdiv(Ho, 8) * cdiv(Wo, 32), 256), (line,)
        ok += 1
    assert ok and refused
    ok = refused = 0
    for (n, H, W, Cin, Cout, ldo, same, al), line in zip(DOWN_CASES, answers["down"]):
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        if Cin % 32 or Cout % 32 or ldo % 8 or not same or not al:
            assert line == "refused", (n, H, W, Cin, Cout, ldo, same, al, line)
            refused += 1
            continue
        tn = 3 if (Cout % 64 != 0 and Cout % 96 == 0) else 2
        want = (tn, 256, n * cdiv(Ho, 4) * cdiv(Wo, 32) * cdiv(Cout, tn * 32), 4, cdiv(Ho, 4) * cdiv(Wo, 32), cdiv(9 * Cin, 64) * 64, cdiv(Cin, 64) * 64)
        assert tuple(map(int, line.split())) == want, (n, H, W, Cin, Cout, ldo, line)
        assert ("down", tn) == MM.down_variant(Cout) and tn == EN.down_tile(Cout)
        ok += 1
    assert ok and refused


def network(H, W, C, fold):
    """BasicEncoder's convolutions as encoder_forward.hip launches them: [(index, H, W, Cin, Cout, k, stride, statistics, halves)]."""
    out = [(0, H, W, 4, 64, 7, 2, 1, 1)]
    h, w, cin = H // 2, W // 2, 64
    for l, cout in enumerate((64, 96, 128, 128)):
        b0, s = 1 + 5 * l, 2 if l else 1
        out.append((b0, h, w, cin, cout, 3, s, 1, 2 if (l and fold) else 1))
        if l and not fold:
            out.append((b0 + 2, h, w, cin, cout, 1, s, 1, 1))
        h, w = (h - 1) // s + 1, (w - 1) // s + 1
        out += [(b0 + i, h, w, cout, cout, 3, 1, 1, 1) for i in (1, 3, 4)]
        cin = cout
    return out + [(21, H // 4, W // 4, 416, 2 * C, 3, 1, 1, 1), (22, H // 4, W // 4, 2 * C, C, 1, 1, 0, 1)]


def test_encoder_partials_fit(answers):
    """The composite encoder's own list of convolutions is the network, and under every MVT_ROWS_NW8 value, folded or not, every
    launch's n * slots * Cout * 2 floats (twice that for a folded launch) stay within the partials buffer: what partials_fit enforces."""
    for (n, H, W, C, nw8, _, fold), line in zip(ENC_CASES, answers["enc"]):
        f = line.split()
        part_floats, st_ch, fit = int(f[0]), int(f[1]), int(f[2])
        convs = [tuple(map(int, x.split(":"))) for x in f[3:]]
        assert len(convs) == 23
        assert st_ch == max(2 * C, 256) and part_floats == n * cdiv(H // 2, 8) * cdiv(W // 2, 32) * st_ch * 2 and fit == 1
        launched = set()
        for ci, h, w, cin, cout, k, s, stats, halves in network(H, W, C, fold):
            th, tw, tcin, tcout, tk, ts, tstats, with_down, folded, slots = convs[ci]
            assert (th, tw, tcin, tcout, tk, ts, tstats, with_down, folded) == (h, w, cin, cout, k, s, stats, int(halves == 2), 0), (ci, convs[ci])
            assert slots == table_slots(h, w, cin, k, k, s, k // 2, 0, nw8)
            if stats:
                assert slots > 0 and halves * n * slots * cout * 2 <= part_floats, (n, H, W, C, nw8, fold, ci)
            if halves == 2:
                assert convs[ci + 2][6:9] == (1, 0, 1) and convs[ci + 2][:6] == (h, w, cin, cout, 1, s)
                launched.add(ci + 2)
            launched.add(ci)
        assert set(range(23)) - launched == {3} and convs[3][6] == 0  # (layer 1 has no downsample branch)
