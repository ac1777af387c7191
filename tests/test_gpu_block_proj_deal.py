"""The follow-up projections of the updater's block kernels, dealt as one work list over the 8 waves, against the sequential loop
(one projection after another) in the same process: the per-call switch MVT_PROJ_SEQ=1 selects the loop.  Every output element is
the same MFMA chain over K = 256 in both, so every comparison is torch.equal -- x, every y (rows outside a projection's row range
keep a planted sentinel), and for the composite call coords, ffeats and delta.  (The list is dealt in tiles with two or more
projections on the staged bf16 path and at most two LayerNorm images; the other cases check that the fall-backs stay what they were.)

Forms reached (block_fused_bf16<NMB, MODE, ATT>): <1,0,0> / <2,0,0> (block_fused_bf16 at M = 160 / 4 160), <1,2,0> / <2,3,0>
(ln_proj_bf16 at M = 64 / 4 160), <2,3,4> (input_proj_bf16), <1,0,1> / <2,0,1> (time attention inside, small / large M),
<2,0,6> and <1,0,2> (the composite call at 680 / 400 tracks)."""
import math
import os

import pytest
import torch

gpu = pytest.mark.gpu
pytestmark = gpu

DEV = "cuda:0"
C, H, KO = 256, 1024, 288
SENTINEL = -1536.0  # exact in bf16, far outside the outputs


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


def gen(seed):
    return torch.Generator().manual_seed(seed)


def frag(hip, n, k, seed):
    """Random bf16 weights [n][k], fragment-major."""
    w = (torch.randn(n, k, generator=gen(seed)) / math.sqrt(k)).to(torch.bfloat16).to(DEV)
    out = torch.zeros((n + 31) // 32 * 32 * k, device=DEV, dtype=torch.bfloat16)
    hip.pack_frag_bf16(w.view(torch.int16), k, n, k, out.view(torch.int16))
    return out


def vec(n, seed, scale=0.1, shift=0.0):
    return (torch.randn(n, generator=gen(seed)) * scale + shift).to(DEV)


# a projection: (N, LayerNorm image, row range); image None = plain eps 1e-6, an int = affine parameters of that seed, eps 1e-5
def spec_sets(M, cut):
    A, B, ALL = (0, cut), (cut, M), (0, 0)
    return {
        "one_864": [(864, None, ALL)],
        "576_288": [(576, None, ALL), (288, None, ALL)],
        "triple": [(576, 1, A), (288, None, A), (288, None, B)],
        "triple_affine_last": [(288, None, A), (288, None, B), (576, 1, A)],
        "three_images": [(576, 1, A), (288, None, A), (288, 2, B)],
        "n131": [(131, None, ALL), (288, None, A)],
    }


SPEC_NAMES = ["one_864", "576_288", "triple", "triple_affine_last", "three_images", "n131"]


class Nexts:
    """The projections of one case: weights made once, y buffers (sentinel-filled) made per run."""

    def __init__(self, hip, specs, M):
        self.specs, self.M = specs, M
        self.fixed = []
        for i, (N, img, rows) in enumerate(specs):
            d = dict(w=frag(hip, N, C, 100 + i), ldw=C, b=vec(N, 200 + i), N=N, ldy=(N + 7) // 8 * 8 if N % 8 == 0 else (N + 3) // 4 * 4,
                     eps=1e-6 if img is None else 1e-5, rows=rows)
            if img is not None:
                d["lnw"], d["lnb"] = vec(C, 300 + img, 0.2, 1.0), vec(C, 400 + img, 0.2)
            self.fixed.append(d)

    def fresh(self):
        return [dict(d, y=torch.full((self.M, d["ldy"]), SENTINEL, device=DEV, dtype=torch.bfloat16)) for d in self.fixed]

    def check_sentinels(self, nexts):
        for d in nexts:
            lo, hi = d["rows"] if d["rows"] != (0, 0) else (0, self.M)
            y = d["y"].float()
            assert bool((y[:lo] == SENTINEL).all()) and bool((y[hi:] == SENTINEL).all()), "a row outside the range was written"
            assert bool((y[:, d["N"]:] == SENTINEL).all()), "a pad column was written"
            assert bool(torch.isfinite(y[lo:hi, :d["N"]]).all())
            assert not bool((y[lo:hi, :d["N"]] == SENTINEL).all(dim=1).any()), "a row inside the range was left out"


def both_ways(run):
    """run() -> list of tensors, once through the sequential loop and once through the dealt pass; equal bit for bit."""
    os.environ["MVT_PROJ_SEQ"] = "1"
    try:
        seq = run()
        torch.cuda.synchronize()
    finally:
        del os.environ["MVT_PROJ_SEQ"]
    new = run()
    torch.cuda.synchronize()
    assert len(seq) == len(new)
    for i, (a, b) in enumerate(zip(seq, new)):
        assert a.shape == b.shape and torch.equal(a, b), f"output {i} differs: {(a.float() - b.float()).abs().max().item()}"
    return new


class Block:
    """Weights of one block (output projection + MLP), made once per module."""

    def __init__(self, hip):
        self.wo, self.w1, self.w2 = frag(hip, C, KO, 1), frag(hip, H, C, 2), frag(hip, C, H, 3)
        self.bo, self.b1, self.b2 = vec(C, 4), vec(H, 5), vec(C, 6)


@pytest.fixture(scope="module")
def blk(hip):
    return Block(hip)


@pytest.mark.parametrize("M", [160, 4160])
@pytest.mark.parametrize("name", SPEC_NAMES)
def test_block_fused(hip, blk, name, M):
    nx = Nexts(hip, spec_sets(M, 100)[name], M)
    x0 = torch.randn(M, C, generator=gen(7)).to(DEV)
    att = torch.randn(M, KO, generator=gen(8)).to(torch.bfloat16).to(DEV)

    def run():
        x, nexts = x0.clone(), nx.fresh()
        hip.block_fused_bf16(x, C, att, KO, KO, blk.wo, KO, blk.bo, blk.w1, C, blk.b1, blk.w2, H, blk.b2, H, nexts, M, C)
        torch.cuda.synchronize()
        nx.check_sentinels(nexts)
        return [x] + [d["y"] for d in nexts]

    out = both_ways(run)
    assert not torch.equal(out[0], x0)


@pytest.mark.parametrize("M", [64, 4160])
@pytest.mark.parametrize("name", SPEC_NAMES)
def test_ln_proj(hip, name, M):
    nx = Nexts(hip, spec_sets(M, 40)[name], M)
    x0 = torch.randn(M, C, generator=gen(9)).to(DEV)

    def run():
        x, nexts = x0.clone(), nx.fresh()
        hip.ln_proj_bf16(x, C, nexts, M, C)
        torch.cuda.synchronize()
        nx.check_sentinels(nexts)
        assert torch.equal(x, x0)  # read only
        return [d["y"] for d in nexts]

    both_ways(run)


def test_input_proj(hip):
    S, Mp, TD, LDT = 12, 96, 581, 584
    M = Mp + 64 * S
    nx = Nexts(hip, [(864, None, (0, 0))], M)
    tok = torch.randn(Mp, LDT, generator=gen(10)).to(DEV)
    tok[:, TD:] = 0
    win, bin_ = frag(hip, C, 592, 11), vec(C, 12)
    virt = torch.randn(64, C, generator=gen(13)).to(DEV)

    def run():
        x, nexts = torch.full((M, C), SENTINEL, device=DEV), nx.fresh()
        hip.input_proj_bf16(tok, LDT, TD, Mp, win, bin_, virt, S, x, C, nexts, M, C)
        torch.cuda.synchronize()
        nx.check_sentinels(nexts)
        assert not bool((x == SENTINEL).any())
        return [x] + [d["y"] for d in nexts]

    both_ways(run)


# (S, point tracks): 75 / 85 tracks run the 32-row tiles of the small-M form, 525 tracks the 64-row tiles (60 rows = 5 whole tracks
# at S = 12; 461 = 92 * 5 + 1: tile 92 holds one point track and four virtual ones)
@pytest.mark.parametrize("S,n", [(12, 11), (8, 21), (16, 21), (12, 461)])
def test_time_block_writes_into_its_own_qkv(hip, blk, S, n):
    """The product's triple: v2p k|v and p2v q of the point rows, v2p q of the virtual rows; k|v and the virtual q go into the qkv
    buffer that the tile's attention reads first."""
    Mp, M = n * S, (n + 64) * S
    qkv0 = (torch.randn(M, 864, generator=gen(14)) * 0.5).to(torch.bfloat16).to(DEV)
    x0 = torch.randn(M, C, generator=gen(15)).to(DEV)
    nx = Nexts(hip, [(576, 1, (0, Mp)), (288, None, (0, Mp)), (288, None, (Mp, M))], M)

    def run():
        x, qkv, nexts = x0.clone(), qkv0.clone(), nx.fresh()
        qp = nexts[1]["y"]
        nexts[0].update(y=qkv[:, 288:], ldy=864)
        nexts[2].update(y=qkv, ldy=864)
        hip.attn_block_fused_bf16(x, C, hip.ATTN_TIME, S, qkv, 864, qkv[:, 288:], qkv[:, 576:], 864, S, blk.wo, blk.bo, blk.w1, blk.b1, blk.w2,
                                  blk.b2, H, nexts, M, C)
        torch.cuda.synchronize()
        assert torch.equal(qkv[:Mp, :288], qkv0[:Mp, :288]) and torch.equal(qkv[Mp:, 288:], qkv0[Mp:, 288:]), "outside the ranges"
        assert not torch.equal(qkv[:Mp, 288:], qkv0[:Mp, 288:]) and not torch.equal(qkv[Mp:, :288], qkv0[Mp:, :288])
        assert bool((qp[Mp:].float() == SENTINEL).all()) and not bool((qp[:Mp].float() == SENTINEL).all(dim=1).any())
        return [x, qkv, qp]

    both_ways(run)


@pytest.fixture(scope="module")
def model():
    from mvtracker_amd import synth
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV)
    m.precision = "bf16"
    return m


# 680 tracks: the 64-row point<-virtual block finishes the virtual-self block (deferred pass 2); 400: the small-M forms
@pytest.mark.parametrize("n", [680, 400])
def test_composite_updater(hip, model, n):
    m = model
    S, Cf, E = m.S, m.latent_dim, m.flow_embed_dim
    Fc = m.corr_n_levels * m.corr_neighbors * m.corr_width
    D = m.updateformer_input_dim
    assert m.fuse_attention == 55
    pk = m._pack(torch.device(DEV))
    w = pk["updater_struct"]
    assert w.input_frag.w
    g = gen(n)
    coords0 = (torch.randn(n, S, 3, generator=g) * 2).to(DEV)
    fcorr = torch.randn(n, S, Fc, generator=g).to(DEV)
    ffeats0 = torch.randn(n, S, Cf, generator=g).to(DEV)
    mask_vis = torch.rand(n, S, 2, generator=g).to(DEV)
    pos = torch.randn(n, D, generator=g).to(DEV)
    ldd = (m.out_dim + 3) // 4 * 4
    ws = torch.empty(hip.updateformer_workspace_bytes(n, S), device=DEV, dtype=torch.uint8)

    def run():
        ws.fill_(255)
        coords, ffeats = coords0.clone(), ffeats0.clone()
        delta = torch.zeros(n * S, ldd, device=DEV)
        flag = torch.zeros(1, device=DEV, dtype=torch.int32)
        hip.updateformer_forward_tokens(w, coords, fcorr, Fc, ffeats, Cf, mask_vis, pos, pk["time_embed"], E, n, delta, ldd, ws, coords, ffeats, flag)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(delta[:, :m.out_dim]).all()) and int(flag.item()) == 0
        return [coords, ffeats, delta[:, :m.out_dim].clone()]

    out = both_ways(run)
    assert not torch.equal(out[0], coords0)
