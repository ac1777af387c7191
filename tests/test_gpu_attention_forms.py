"""The bf16 attention paths, one kernel form at a time: planted-key probes and bars that follow an emulation of the rounding.

GPU tests (`-m gpu`) go through the C ABI; the tests without the marker are the CPU-only checks of the probes themselves.

A. Planted keys.  k = unit-direction rows of norm sqrt(48), q_i = BETA * k_pi(i): the score of the planted key is 6.9 BETA, every
   other score has sigma = BETA, so the softmax is the V row of key pi(i) up to a residual far below 1/2.  V rows are small integers
   (exact in bf16) that spell out the key index, the column and the (group, head): the assertion is "every output element rounds
   to the planted integer", and it is asserted of the fp64 reference first (a too-small BETA fails there, not on the kernel).
   (The rows of k are normalised: with plain randn rows the shortest of 8192 keys has |k|^2 near 20 and its planted score no
   longer clears the largest of its 8191 competitors.)
B. Random data (plain, and peaked with the keys sorted so that the running maximum moves on every key block / on none):
   err_gpu <= c * err_emulation for max and mean, where the emulation is the specified rounding (q * scale, k, v and the
   numerator's P to bf16, everything else fp64) on the same inputs and both errors are distances from fp64 attention.
   c = twice the largest ratio measured on the MI355X ("Attention forms against the rounding emulation"); the CPU-only
   test below checks that a dropped last key and two swapped V rows fail that bar at nk = 1024 and nk = 8192.
C. Every output / workspace tensor is NaN-poisoned before a launch, padding columns and guard rows must stay poisoned; the fp32
   kernel's four forms at both sides of their thresholds; argument refusals launch nothing.

MVT_ATTN_FRAME_CTX is not reached here: its keys are not an input but LayerNorm + projection of the context block's rows inside the
kernel, so no key tensor can be planted.  Planted weights can: tests/test_gpu_updater_wiring_exact.py drives it through the
composite updater call with planted projections, at full and ragged 64-token tiles; the bit-identity with the two-launch form is in
test_updater_fused_attention_matches_separate_launches (n = 1024).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

DEV = "cuda:0"
S, H, DH = 12, 6, 48
INNER = H * DH
NSPLIT = 4
BETA = 8.0
NAN = float("nan")

# err_gpu <= C * err_emulation: twice the largest ratio measured on the MI355X over every case below (1.107 with fp32
# tensors -- KS 4, nk = 513, max error; 1.422 with bf16 tensors / in the block kernels -- partials, nk = 512, max error)
C_FP32 = 2.2
C_BF16 = 2.8


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ the host dispatch of mvt_attention_bf16, restated


def form_of(groups, nq, nk, ws):
    nchunk = groups * H * cdiv(nq, 64)
    if nk >= 512 and nchunk < 256 and ws and cdiv(nk, 32) % NSPLIT == 0:
        return "split"
    return "ks4" if nk >= 512 and nchunk < 1024 else "ks1"


def key_edges(nk, form):
    """Key indices on both sides of every boundary the kernel cuts the keys at: 32-key blocks, the [g0, g1) block range of a
    split workgroup, the [kb0, kb1) range of a wave (attention_mfma's own arithmetic), plus the first and the last key."""
    nkb = cdiv(nk, 32)
    blocks = set(range(nkb + 1))
    splits, KS = (NSPLIT if form == "split" else 1), (1 if form == "ks1" else 4)
    gper = cdiv(nkb, splits)
    for by in range(splits):
        g0 = by * gper
        g1 = min(g0 + gper, nkb)
        per = cdiv(gper, KS)
        for wave in range(KS):
            kb0 = g0 if KS == 1 else g0 + wave * per
            kb1 = g1 if KS == 1 else min(kb0 + per, g1)
            blocks.update(b for b in (g0, g1, kb0, kb1) if 0 <= b <= nkb)
    keys = {0, nk - 1}
    for b in blocks:
        keys.update(x for x in (32 * b - 1, 32 * b) if 0 <= x < nk)
    return sorted(keys)


# ------------------------------------------------------------------ references (torch, fp64; any device)


def sdpa64(q, k, v):
    """q [G][nq][H][DH], k / v [G][nk][H][DH] -> fp64 softmax(q k^T / sqrt(DH)) v as [G][nq][H][DH]."""
    q, k, v = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    return F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3)


def bf(t):
    return t.to(torch.bfloat16).double()


def emulate(q, k, v, out_bf16=False, mutate=None):
    """The specified rounding and nothing else: q * scale (an fp32 product) -> bf16, k, v -> bf16, P = exp(s - max) -> bf16 in the
    numerator, the denominator from the unrounded P; fp64 accumulation.  mutate: the index bugs the bar has to see."""
    scale = torch.tensor(float(DH), dtype=torch.float32).sqrt().reciprocal().to(q.device)
    qs = (q.float() * scale).to(torch.bfloat16).double().permute(0, 2, 1, 3)
    kb, vb = bf(k).permute(0, 2, 1, 3), bf(v).permute(0, 2, 1, 3)
    s = qs @ kb.transpose(-1, -2)
    nk = k.shape[1]
    if mutate == "drop_last_key":
        s[..., nk - 1] = -math.inf
    elif mutate == "drop_last_block":
        s[..., 32 * ((nk - 1) // 32):] = -math.inf
    elif mutate == "swap_last_v":
        vb = vb.clone()
        vb[:, :, [nk - 2, nk - 1]] = vb[:, :, [nk - 1, nk - 2]]
    else:
        assert mutate is None
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (bf(p) @ vb) / p.sum(-1, keepdim=True)
    return (bf(o) if out_bf16 else o).permute(0, 2, 1, 3)


def errs(a, ref):
    d = (a.double() - ref).abs()
    return d.max().item(), d.mean().item()


# ------------------------------------------------------------------ inputs


def v_code(nk):
    """[nk][DH] integers 0..7: base-8 digits of the key index in d < 5, (j * (d + 1)) mod 7 elsewhere."""
    j = torch.arange(nk)[:, None]
    d = torch.arange(DH)[None]
    return torch.where(d < 5, (j >> (3 * d.clamp(max=4))) & 7, (j * (d + 1)) % 7).float()


def gh_offset(G):
    """[G][H] multiples of 8 up to 48: differs between neighbouring groups and between any two heads of a group."""
    return 8.0 * ((torch.arange(G)[:, None] * H + torch.arange(H)[None]) % 7)


@functools.lru_cache(maxsize=3)
def planted(G, nq, nk, must=(), shared_keys=False, seed=0):
    """(q, k, v, want): q [G][nq][H][DH] etc. on the CPU in fp32; want = the V row of the planted key of every query.
    The planted keys cover every key index when there are at least nk queries, and otherwise all of `must`.
    shared_keys: every group has the same k rows (the V rows still differ by group): a query that also sees the keys of a
    neighbouring group then splits its weight between two different V rows and decodes to neither."""
    gen = torch.Generator().manual_seed(1000 * nk + nq + seed)
    k = torch.randn(1 if shared_keys else G, nk, H, DH, generator=gen)
    k = (k * (math.sqrt(DH) / k.norm(dim=-1, keepdim=True))).expand(G, nk, H, DH).contiguous()
    total = G * H * nq
    if total >= nk:
        pi = torch.randperm(nk, generator=gen)[torch.arange(total) % nk]
    else:
        m = torch.tensor(sorted(must), dtype=torch.long)
        assert 0 < m.numel() <= total
        rest = torch.ones(nk, dtype=torch.bool)
        rest[m] = False
        rest = rest.nonzero()[:, 0]
        fill = rest[torch.randperm(rest.numel(), generator=gen)[:total - m.numel()]]
        pi = torch.cat([m, fill])[torch.randperm(total, generator=gen)]
        assert set(m.tolist()) <= set(pi.tolist())
    if total >= nk:
        assert pi.unique().numel() == nk
    idx = pi.reshape(G, H, nq, 1).expand(G, H, nq, DH)
    q = (BETA * k.permute(0, 2, 1, 3).gather(2, idx)).permute(0, 2, 1, 3).contiguous()
    v = (v_code(nk)[None, :, None, :] + gh_offset(G)[:, None, :, None]).contiguous()
    want = v.permute(0, 2, 1, 3).gather(2, idx).permute(0, 2, 1, 3).contiguous()
    return q, k, v, want.double()


def random_qkv(G, nq, nk, flavour, seed=0):
    """randn q / k / v as in test_attention_bf16; "asc" / "desc": q * 4 and the keys of every group sorted by the score of the
    group's probe (query 0, head 0), so that probe's running maximum moves on every key block / never after the first."""
    gen = torch.Generator().manual_seed(7000 + 10 * nk + nq + seed)
    q, k, v = torch.randn(G, nq, H, DH, generator=gen), torch.randn(G, nk, H, DH, generator=gen), torch.randn(G, nk, H, DH, generator=gen)
    if flavour != "plain":
        q = q * 4
        order = torch.einsum("gd,gkd->gk", q[:, 0, 0], k[:, :, 0]).argsort(dim=1, descending=flavour == "desc")
        k = torch.gather(k, 1, order[:, :, None, None].expand_as(k))
        v = torch.gather(v, 1, order[:, :, None, None].expand_as(v))
    return q, k, v


FLAVOURS = ["plain", "asc", "desc"]


def assert_decodes(got, want, what):
    """Every element rounds to the planted integer."""
    bad = (got.double().round() != want.double().to(got.device)).reshape(-1, got.shape[-1]).any(dim=1)
    n = int(bad.sum())
    if n:
        i = int(bad.nonzero()[0])
        g = got.reshape(-1, got.shape[-1])[i].double().round().tolist()
        w = want.reshape(-1, want.shape[-1])[i].tolist()
        raise AssertionError(f"{what}: {n} of {bad.numel()} rows decode to another V row; first: flat row {i}, got {g[:8]} .. want {w[:8]} ..")


# ------------------------------------------------------------------ staging for mvt_attention[_bf16]: the updater's own layout
# (row of item i of group g = i * G + g: group stride 1 row, item stride G rows), k | v side by side in one matrix, padded leading
# dimensions, NaN everywhere a kernel has no business


def rows_of(t):  # [G][n][H][DH] -> [n * G][INNER]
    return t.permute(1, 0, 2, 3).reshape(-1, INNER)


def unrows(m, G, n):
    return m.reshape(n, G, H, DH).permute(1, 0, 2, 3)


LDQ, LDKV, LDO = INNER + 8, 2 * INNER + 8, INNER + 8


def stage(q, k, v, dtype, out_dtype=None):
    G, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    qd = torch.full((nq * G, LDQ), NAN, dtype=dtype)
    qd[:, :INNER] = rows_of(q).to(dtype)
    kv = torch.full((nk * G, LDKV), NAN, dtype=dtype)
    kv[:, :INNER] = rows_of(k).to(dtype)
    kv[:, INNER:2 * INNER] = rows_of(v).to(dtype)
    guard = (cdiv(nq, 64) * 64 - nq + 1) * G  # where the padding queries of the last 64-query chunk would land
    o = torch.full((nq * G + guard, LDO), NAN, dtype=out_dtype or dtype, device=DEV)
    return qd.to(DEV), kv.to(DEV), o


def take_out(o, G, nq):
    """The [G][nq][H][DH] result; everything else of `o` must still be poisoned."""
    torch.cuda.synchronize()
    oc = o.double()
    body = oc[:nq * G, :INNER]
    assert bool(torch.isfinite(body).all()), "non-finite attention output"
    assert bool(torch.isnan(oc[:nq * G, INNER:]).all()), "padding columns of the output written"
    assert bool(torch.isnan(oc[nq * G:]).all()), "rows past the last query written"
    return unrows(body, G, nq)


def run_mfma(hip, q, k, v, dtype, with_ws, expect_form):
    G, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    assert form_of(G, nq, nk, with_ws) == expect_form, (form_of(G, nq, nk, with_ws), expect_form)
    qd, kv, o = stage(q, k, v, dtype)
    ws = torch.full((hip.attention_ws_floats(G, nq, H),), NAN, device=DEV) if with_ws else None
    hip.attention_bf16(qd, LDQ, 1, G, kv, kv[:, INNER:], LDKV, 1, G, o, LDO, G, nq, nk, H, DH, ws=ws)
    return take_out(o, G, nq)


# (nq, nk) per form, G = S groups
KS1 = [(64, 50), (64, 64), (64, 511), (50, 64), (200, 64), (1000, 33), (960, 600)]
KS4 = [(64, 512), (64, 513), (64, 640), (64, 1000), (64, 8192), (130, 999)]
SPLIT = [(64, 512), (64, 640), (64, 1024), (64, 8191), (64, 8192)]
SPLIT_FALLBACK = [(64, 513)]  # a workspace is given but ceil(nk / 32) % 4 != 0: the KS 4 form answers
MFMA_CASES = ([("ks1", False, s) for s in KS1] + [("ks4", False, s) for s in KS4] + [("split", True, s) for s in SPLIT] +
              [("ks4", True, s) for s in SPLIT_FALLBACK])
BF16_IO_CASES = [("ks1", False, (1000, 33)), ("ks4", False, (130, 999)), ("split", True, (64, 8191))]
case_id = lambda c: f"{c[0]}{'-ws' if c[1] else ''}-nq{c[2][0]}-nk{c[2][1]}"


def planted_for(form, nq, nk, G=S, **kw):
    return planted(G, nq, nk, must=tuple(key_edges(nk, form)), **kw)


def ratio_check(tag, got, q, k, v, out_bf16, c):
    """err(got) <= c * err(emulation), max and mean, both against fp64 attention of the same inputs (device tensors)."""
    ref = sdpa64(q, k, v)
    e_max, e_mean = errs(emulate(q, k, v, out_bf16=out_bf16), ref)
    g_max, g_mean = errs(got.to(ref.device), ref)
    print(f"RATIO {tag}: gpu {g_max:.3e} / {g_mean:.3e}  emulation {e_max:.3e} / {e_mean:.3e}  ratio {g_max / e_max:.3f} / {g_mean / e_mean:.3f}")
    assert g_max <= c * e_max and g_mean <= c * e_mean, (tag, g_max, g_mean, e_max, e_mean, c)


# ------------------------------------------------------------------ CPU-only: the probes themselves


ALL_PLANTED_SHAPES = sorted({(f, S, nq, nk) for f, _, (nq, nk) in MFMA_CASES + BF16_IO_CASES} |
                            {("ks1", S, nq, nk) for nq in (63, 64, 65) for nk in (64, 65)} |
                            {("split", S, 64, nk) for nk in (512, 640, 1024, 8192)} |          # partials
                            {("ks1", S, n, 64) for n in (16, 37, 64, 400, 1024)})              # frame attention in the block kernels


@pytest.mark.parametrize("form,G,nq,nk", ALL_PLANTED_SHAPES, ids=lambda x: str(x))
def test_planted_reference_decodes(form, G, nq, nk):
    """fp64 attention of the planted inputs is the planted V row, for every shape of the GPU tests; the planted keys cover
    every key (or every boundary key the form has)."""
    q, k, v, want = planted_for(form, nq, nk, G=G)
    assert_decodes(sdpa64(q, k, v), want, "fp64 reference")
    assert_decodes(sdpa64(bf(q), bf(k), bf(v)), want, "fp64 reference on the bf16-rounded inputs")
    assert float(v.max()) <= 55 and bool((v == bf(v)).all())


@pytest.mark.parametrize("Sx,tracks", [(7, 19), (8, 9), (12, 11), (16, 5), (32, 3)])
def test_planted_reference_decodes_time(Sx, tracks):
    q, k, v, want = planted(tracks, Sx, Sx, shared_keys=True)
    assert_decodes(sdpa64(bf(q), bf(k), bf(v)), want, "fp64 reference")


def test_key_edges_follow_the_kernel_partition():
    # nk = 640 split: 20 blocks, 5 per workgroup, 2 per wave -> wave 3 of every workgroup owns no block
    assert {159, 160, 319, 320, 479, 480} <= set(key_edges(640, "split"))
    # nk = 513, KS 4: 17 blocks, 5 per wave, the last wave holds the one-key block
    assert {0, 159, 160, 511, 512} <= set(key_edges(513, "ks4"))
    assert form_of(S, 64, 640, True) == "split" and form_of(S, 64, 513, True) == "ks4" and form_of(S, 960, 600, False) == "ks1"


@pytest.mark.parametrize("nk", [1024, 8192])
@pytest.mark.parametrize("c,out_bf16", [(C_FP32, False), (C_BF16, True)], ids=["fp32io", "bf16io"])
def test_bar_sees_a_dropped_key_and_swapped_rows(nk, c, out_bf16):
    """The bar of section B is only worth something if an index bug fails it at the sizes where the fixed 3e-2 / 3e-3 bar is
    blind: emulate the bug (same rounding), 72 chunks x 64 queries of randn data, and require err > c * err_clean in max or mean."""
    q, k, v = random_qkv(S, 64, nk, "plain")
    if out_bf16:
        q, k, v = bf(q), bf(k), bf(v)
    ref = sdpa64(q, k, v)
    c_max, c_mean = errs(emulate(q, k, v, out_bf16=out_bf16), ref)
    print(f"nk={nk} clean {c_max:.3e} / {c_mean:.3e}")
    assert c_max < 3e-2 and c_mean < 3e-3  # the emulation itself is inside today's fixed bar
    for bug in ("drop_last_key", "swap_last_v", "drop_last_block"):
        b_max, b_mean = errs(emulate(q, k, v, out_bf16=out_bf16, mutate=bug), ref)
        print(f"nk={nk} {bug} {b_max:.3e} / {b_mean:.3e}  = {b_max / c_max:.1f} x / {b_mean / c_mean:.1f} x clean")
        assert b_max > c * c_max or b_mean > c * c_mean, (bug, b_max, b_mean, c_max, c_mean, c)


# ------------------------------------------------------------------ A + B: mvt_attention_bf16, form by form


@gpu
@pytest.mark.parametrize("case", MFMA_CASES, ids=case_id)
def test_mfma_planted_keys(hip, case):
    form, with_ws, (nq, nk) = case
    q, k, v, want = planted_for(form, nq, nk)
    assert_decodes(sdpa64(q.to(DEV), k.to(DEV), v.to(DEV)), want, "fp64 reference")
    assert_decodes(run_mfma(hip, q, k, v, torch.float32, with_ws, form), want, case_id(case))


@gpu
@pytest.mark.parametrize("case", BF16_IO_CASES, ids=case_id)
def test_mfma_planted_keys_bf16_tensors(hip, case):
    form, with_ws, (nq, nk) = case
    q, k, v, want = planted_for(form, nq, nk)
    assert_decodes(sdpa64(bf(q).to(DEV), bf(k).to(DEV), bf(v).to(DEV)), want, "fp64 reference")
    assert_decodes(run_mfma(hip, q, k, v, torch.bfloat16, with_ws, form), want, case_id(case))


@gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("case", MFMA_CASES, ids=case_id)
def test_mfma_random_follows_emulation(hip, case, flavour):
    form, with_ws, (nq, nk) = case
    q, k, v = random_qkv(S, nq, nk, flavour)
    got = run_mfma(hip, q, k, v, torch.float32, with_ws, form)
    ratio_check(f"fp32io {case_id(case)} {flavour}", got, q.to(DEV), k.to(DEV), v.to(DEV), False, C_FP32)


@gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("case", BF16_IO_CASES, ids=case_id)
def test_mfma_random_follows_emulation_bf16_tensors(hip, case, flavour):
    form, with_ws, (nq, nk) = case
    q, k, v = (t.to(torch.bfloat16).float() for t in random_qkv(S, nq, nk, flavour))
    got = run_mfma(hip, q, k, v, torch.bfloat16, with_ws, form)
    ratio_check(f"bf16io {case_id(case)} {flavour}", got, q.to(DEV), k.to(DEV), v.to(DEV), True, C_BF16)


SEGMENTS = [("split", 130, 999), ("ks4", 64, 513), ("ks1", 50, 64), ("ks1", 200, 33)]  # one table, all three forms, ragged


def run_segmented(hip, parts, dtype):
    """parts: [(q, k, v)] per segment; one segmented launch sequence with a workspace; returns the per-segment results."""
    G = S
    nqs, nks = [p[0].shape[1] for p in parts], [p[1].shape[1] for p in parts]
    for (form, nq, nk) in SEGMENTS:
        assert form_of(G, nq, nk, True) == form
    qd = torch.full((sum(nqs) * G, LDQ), NAN, dtype=dtype)
    kv = torch.full((sum(nks) * G, LDKV), NAN, dtype=dtype)
    q0, k0, r, c = [], [], 0, 0
    for (q, k, v) in parts:
        q0.append(r)
        k0.append(c)
        qd[r:r + q.shape[1] * G, :INNER] = rows_of(q).to(dtype)
        kv[c:c + k.shape[1] * G, :INNER] = rows_of(k).to(dtype)
        kv[c:c + k.shape[1] * G, INNER:2 * INNER] = rows_of(v).to(dtype)
        r += q.shape[1] * G
        c += k.shape[1] * G
    qd, kv = qd.to(DEV), kv.to(DEV)
    o = torch.full((r + 64 * G, LDO), NAN, dtype=dtype, device=DEV)
    ws = torch.full((hip.attention_segmented_ws_floats(G, nqs, H),), NAN, device=DEV)
    hip.attention_bf16_segmented(qd, LDQ, 1, G, kv, kv[:, INNER:], LDKV, 1, G, o, LDO, G, H, DH, q0, nqs, k0, nks, ws=ws)
    torch.cuda.synchronize()
    oc = o.double()
    assert bool(torch.isfinite(oc[:r, :INNER]).all()) and bool(torch.isnan(oc[:r, INNER:]).all()) and bool(torch.isnan(oc[r:]).all())
    return [unrows(oc[a:a + n * G, :INNER], G, n) for a, n in zip(q0, nqs)]


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32io", "bf16io"])
def test_segmented_planted_keys_and_emulation(hip, dtype):
    b16 = dtype == torch.bfloat16
    parts, wants = [], []
    for form, nq, nk in SEGMENTS:
        q, k, v, want = planted(S, nq, nk, must=tuple(key_edges(nk, form)), seed=5)
        parts.append((q, k, v))
        wants.append(want)
    for got, want, seg in zip(run_segmented(hip, parts, dtype), wants, SEGMENTS):
        assert_decodes(got, want, f"segment {seg}")
    for flavour in FLAVOURS:
        parts = [tuple(t.to(dtype).float() for t in random_qkv(S, nq, nk, flavour, seed=5)) for _, nq, nk in SEGMENTS]
        for got, (q, k, v), seg in zip(run_segmented(hip, parts, dtype), parts, SEGMENTS):
            ratio_check(f"{'bf16io' if b16 else 'fp32io'} segmented {seg} {flavour}", got, q.to(DEV), k.to(DEV), v.to(DEV), b16,
                        C_BF16 if b16 else C_FP32)


# ------------------------------------------------------------------ the attention inside the block kernels
# x = 0, bo = 0, W2 = 0, b2 = 0, no follow-up projection, Wo a 0/1 selection of 256 of the 288 attention columns: every product is
# exact, so x on return IS the selected attention columns as the kernel hands them to the Wo GEMM (rounded to bf16).  Two runs
# (columns 0..255, columns 32..287) give all 288.

CX, HID = 256, 256


def frag(hip, w):
    """[N][K] values that are exact in bf16 -> the fragment-major bf16 image of mvt_pack_frag_bf16."""
    N, K = w.shape
    hi = w.to(torch.bfloat16).contiguous().view(torch.int16).to(DEV)
    out = torch.empty(cdiv(N, 32) * 32 * K, device=DEV, dtype=torch.int16)
    hip.pack_frag_bf16(hi, K, N, K, out)
    return out


def block_attention(hip, kind, Sx, M, n_keys, q=None, ldq=0, k=None, v=None, ldkv=0, split=False, partials=None):
    """All 288 attention columns of the M rows as the block kernel computed them ([M][288] fp64 on the device)."""
    gen = torch.Generator().manual_seed(M)
    w1, b1 = frag(hip, (torch.randn(HID, CX, generator=gen) / 16).to(torch.bfloat16).float()), torch.randn(HID, generator=gen).to(DEV)
    w2, zc = torch.zeros(CX * HID, device=DEV, dtype=torch.int16), torch.zeros(CX, device=DEV)
    ldx, guard = CX + 8, 64
    cols = []
    for first in (0, INNER - CX):
        sel = torch.zeros(CX, INNER)
        sel[torch.arange(CX), first + torch.arange(CX)] = 1.0
        x = torch.full((M + guard, ldx), NAN, device=DEV)
        x[:M, :CX] = 0.0
        ws = torch.full(((HID // 256 + 1) * M * CX,), NAN, device=DEV) if split else None
        hip.attn_block_fused_bf16(x, ldx, kind, Sx, q, ldq, k, v, ldkv, n_keys, frag(hip, sel), zc, w1, b1, w2, zc, HID, [], M, CX, ws=ws,
                                  partials=partials, n_splits=NSPLIT if partials is not None else 0)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(x[:M, :CX]).all()), "non-finite block output"
        assert bool(torch.isnan(x[:M, CX:]).all()) and bool(torch.isnan(x[M:]).all()), "the block kernel wrote outside its rows / columns"
        cols.append(x[:M, :CX].double())
    assert torch.equal(cols[0][:, INNER - CX:], cols[1][:, :2 * CX - INNER]), "the two selections disagree on the columns they share"
    return torch.cat([cols[0], cols[1][:, 2 * CX - INNER:]], dim=1)


def padded_bf16(m, ld):
    out = torch.full((m.shape[0], ld), NAN, dtype=torch.bfloat16)
    out[:, :m.shape[1]] = m.to(torch.bfloat16)
    return out.to(DEV)


def run_time_block(hip, q, k, v):
    """q / k / v [tracks][S][H][DH]: rows track-major, q | k | v side by side as the updater keeps them."""
    G, Sx = q.shape[0], q.shape[1]
    M, ld3 = G * Sx, 3 * INNER + 8
    qkv = padded_bf16(torch.cat([t.reshape(M, INNER) for t in (q, k, v)], dim=1), ld3)
    out = block_attention(hip, hip.ATTN_TIME, Sx, M, Sx, qkv, ld3, qkv[:, INNER:], qkv[:, 2 * INNER:], ld3)
    return out.reshape(G, Sx, H, DH)


def run_frame_block(hip, q, k, v):
    """q [S][n][H][DH], k / v [S][n_keys][H][DH]: the tokens of frame t against the context tokens of frame t."""
    Sx, n, nkeys = q.shape[0], q.shape[1], k.shape[1]
    M = n * Sx
    qd = padded_bf16(rows_of(q), LDQ)
    kv = padded_bf16(torch.cat([rows_of(k), rows_of(v)], dim=1), LDKV)
    out = block_attention(hip, hip.ATTN_FRAME, Sx, M, nkeys, qd, LDQ, kv, kv[:, INNER:], LDKV, split=M < 4096)
    return unrows(out, Sx, n)


def run_partials_block(hip, q, k, v):
    """Virtual <- point: the key-split partials of mvt_attention_bf16 combined in the prologue of the consuming block."""
    Sx, nk = q.shape[0], k.shape[1]
    assert q.shape[1] == 64 and form_of(Sx, 64, nk, True) == "split"
    qd, kv, o = stage(q, k, v, torch.bfloat16)
    ws = torch.full((hip.attention_ws_floats(Sx, 64, H),), NAN, device=DEV)
    hip.attention_bf16(qd, LDQ, 1, Sx, kv, kv[:, INNER:], LDKV, 1, Sx, o, LDO, Sx, 64, nk, H, DH, ws=ws, partials_only=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o.float()).all()), "PARTIALS_ONLY wrote the output tensor"
    assert bool(torch.isfinite(ws[:NSPLIT * Sx * H * 17 * 256]).all()), "a partial record was left unwritten"
    out = block_attention(hip, hip.ATTN_PARTIALS, Sx, 64 * Sx, 64, split=True, partials=ws)
    return unrows(out, Sx, 64)


# tracks: a ragged last tile in the 32-row form (M / tile <= 256 tiles) and, the larger count, in the 64-row form
TIME_SHAPES = [(7, 19), (7, 1201), (8, 9), (8, 1100), (12, 11), (12, 703), (16, 5), (16, 601), (32, 3), (32, 301)]


@gpu
@pytest.mark.parametrize("Sx,tracks", TIME_SHAPES)
def test_block_time_attention_planted_keys(hip, Sx, tracks):
    """Block-diagonal time attention: every track has the SAME keys and its own V rows, so a query that sees a key of another
    track of its tile, or misses one of its own, decodes to no V row at all."""
    q, k, v, want = planted(tracks, Sx, Sx, shared_keys=True)
    assert_decodes(sdpa64(bf(q), bf(k), bf(v)), want, "fp64 reference")
    assert_decodes(run_time_block(hip, q, k, v), want, f"time attention S={Sx} tracks={tracks}")


@gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("Sx,tracks", TIME_SHAPES)
def test_block_time_attention_follows_emulation(hip, Sx, tracks, flavour):
    q, k, v = (t.to(torch.bfloat16).float() for t in random_qkv(tracks, Sx, Sx, flavour))
    got = run_time_block(hip, q, k, v)
    ratio_check(f"block time S={Sx} tracks={tracks} {flavour}", got, q.to(DEV), k.to(DEV), v.to(DEV), True, C_BF16)


# (frames, tokens): point <- virtual at S = 12 from 4096 rows (n = 400: 32-token tiles, ragged; n = 1024: 64-token tiles), the
# virtual-self shape on the split path (64 x 12 rows), and the ragged token counts 16 / 37 at frame counts that reach 4096 rows
# (below 4096 rows the entry only takes whole 32-token tiles: test_refusals)
FRAME_SHAPES = [(12, 400), (12, 1024), (12, 64), (256, 16), (112, 37)]


@gpu
@pytest.mark.parametrize("Sx,n", FRAME_SHAPES)
def test_block_frame_attention_planted_keys(hip, Sx, n):
    q, k, v, want = planted(Sx, n, 64)
    assert_decodes(sdpa64(bf(q), bf(k), bf(v)), want, "fp64 reference")
    assert_decodes(run_frame_block(hip, q, k, v), want, f"frame attention S={Sx} n={n}")


@gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("Sx,n", FRAME_SHAPES)
def test_block_frame_attention_follows_emulation(hip, Sx, n, flavour):
    q, k, v = (t.to(torch.bfloat16).float() for t in random_qkv(Sx, n, 64, flavour))
    got = run_frame_block(hip, q, k, v)
    ratio_check(f"block frame S={Sx} n={n} {flavour}", got, q.to(DEV), k.to(DEV), v.to(DEV), True, C_BF16)


@gpu
@pytest.mark.parametrize("nk", [512, 640, 1024, 8192])
def test_block_partials_planted_keys(hip, nk):
    q, k, v, want = planted_for("split", 64, nk)
    assert_decodes(sdpa64(bf(q), bf(k), bf(v)), want, "fp64 reference")
    assert_decodes(run_partials_block(hip, q, k, v), want, f"partials nk={nk}")


@gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("nk", [512, 640, 1024, 8192])
def test_block_partials_follow_emulation(hip, nk, flavour):
    q, k, v = (t.to(torch.bfloat16).float() for t in random_qkv(S, 64, nk, flavour))
    got = run_partials_block(hip, q, k, v)
    ratio_check(f"block partials nk={nk} {flavour}", got, q.to(DEV), k.to(DEV), v.to(DEV), True, C_BF16)


# ------------------------------------------------------------------ C: the fp32 kernel's four forms, refusals


@gpu
@pytest.mark.parametrize("nk", [64, 65])
@pytest.mark.parametrize("nq", [63, 64, 65])
def test_fp32_attention_forms(hip, nq, nk):
    """mvt_attention: ukeys KS 8 (nq >= 64, nk > 64), ukeys KS 1 (nq >= 64, nk <= 64), qlane (nq < 64, nk <= 64), klane: planted
    keys decode, and randn data (test_attention's distribution) within its 2e-6 of fp64.  On the planted data the outputs are
    integers up to 55 (one fp32 ulp there is 3.8e-6), so the same bar is taken relative to the largest V value."""
    def run(q, k, v):
        qd, kv, o = stage(q, k, v, torch.float32)
        hip.attention(qd, LDQ, 1, S, kv, kv[:, INNER:], LDKV, 1, S, o, LDO, S, nq, nk, H, DH)
        return take_out(o, S, nq)

    q, k, v, want = planted(S, nq, nk)
    ref = sdpa64(q, k, v)
    assert_decodes(ref, want, "fp64 reference")
    got = run(q, k, v)
    assert_decodes(got, want, f"fp32 attention nq={nq} nk={nk}")
    e, vmax = (got.cpu() - ref).abs().max().item(), float(v.max())
    q, k, v = random_qkv(S, nq, nk, "plain")
    e_r = (run(q, k, v).cpu() - sdpa64(q, k, v)).abs().max().item()
    print(f"fp32 attention nq={nq} nk={nk}: planted max err {e:.3e} (V up to {vmax:.0f}), randn max err {e_r:.3e}")
    assert e_r < 2e-6
    assert e < 2e-6 * vmax


@gpu
def test_refusals(hip):
    """Rejected arguments return an error and launch nothing (the poisoned output and workspace stay poisoned)."""
    def attempt(nq, nk, dtype=torch.float32, ldq=LDQ, dh=DH, ws=True, partials_only=False):
        q, k, v = random_qkv(S, nq, nk, "plain")
        qd, kv, o = stage(q, k, v, dtype)
        w = torch.full((hip.attention_ws_floats(S, nq, H),), NAN, device=DEV) if ws else None
        with pytest.raises(hip.HipError, match="arguments rejected"):
            hip.attention_bf16(qd, ldq, 1, S, kv, kv[:, INNER:], LDKV, 1, S, o, LDO, S, nq, nk, H, dh, ws=w, partials_only=partials_only)
        torch.cuda.synchronize()
        assert bool(torch.isnan(o.float()).all()) and (w is None or bool(torch.isnan(w).all()))

    attempt(64, 1024, ws=False, partials_only=True)   # no workspace
    attempt(64, 513, partials_only=True)              # 17 key blocks: not 4 x whole blocks
    attempt(64, 500, partials_only=True)              # < 512 keys
    attempt(300, 1024, partials_only=True)            # 360 chunks >= 256
    attempt(64, 64, dh=32)                            # the MFMA entry is dh == 48 only
    attempt(64, 64, dtype=torch.bfloat16, ldq=INNER + 4)  # bf16 rows must be 16-byte aligned
    # in-kernel frame attention below 4096 rows is the split path: whole 32-token tiles only
    for n in (16, 37):
        q, k, v = (t.to(torch.bfloat16).float() for t in random_qkv(S, n, 64, "plain"))
        with pytest.raises(hip.HipError, match="arguments rejected"):
            run_frame_block(hip, q, k, v)
