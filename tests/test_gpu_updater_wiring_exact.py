"""The composite updater's wiring, exactly: planted weights make every answer an integer that says which row went where.

mvt_updateformer_forward and its _tokens / _grouped variants have no kernels of their own; what they decide is which rows attend
to which keys, which row range every epilogue projects into which q|k|v buffer, which layer's weights a block gets and where the
virtual rows and the query sets start.  Every kernel underneath has an exact suite; this file is the one for the composition.

Construction.  A token row is +-C (C = 16) with 128 entries of each sign: 128 bits, bit b as the column pair [e, -e], e = C (1 - 2b).
Its fp32 LayerNorm is +-(1 - eps / 8), +-1 after the bf16 rounding that every projection applies, so every projection sees the
sign pattern exactly.  A row is a set of bit fields (make_plan): an own-key code, wanted-key codes, identity bits (track /
virtual token, frame, query set) and blank fields.  An attention stage is planted as "copy bits of the key row I want into one of
my blank fields": Wk reads the key-code field, Wq the wanted-code field times BETA = 8, both repeating a 16-bit codeword of the
extended Hamming code [16, 11, 4] three times over the 48 head dimensions (planted score 55.4, every other <= 27.7); Wv / bv turn
the copied bits into 0 / 1, Wo writes [-2C b, +2C b] onto the blank pair [+C, -C], which keeps the row balanced.  Key codes are
shared across what must stay separate (time: the code is the frame, V carries track and frame; space: the code is the point /
virtual token, V carries token, frame and set), so a query that sees a neighbouring track's, frame's or set's keys splits its
weight over two V rows and decodes to neither.  The context LayerNorms carry a different weight in {1, 2} and an integer bias per
(layer, block), compensated in the planted k|v weights: a swapped norm decodes to nothing.  An MLP stage is fc1 = -+16 on one
column (tanh-GELU of 0, +-16 is relu exactly), fc2 = -+C / 8: "copy a bit, xor a (layer, block) pattern", its hidden units spread
over all four 256-chunks.  Stages not under test have zero to_q / to_kv / to_out / fc2: exact identities whose launches, epilogue
projections and buffer traffic still run.  The flow head is a selection: delta[:, :3] and the +-pairs of delta[:, 3:] are 65 chosen
bits of the final point rows, so delta is +-C everywhere (and balanced past column 3, which makes the fused head exact as well).

The expected integers come from `simulate`, an integer restatement of the planted copies; the fp64 oracle must reproduce them
to 1e-6 with every active softmax putting <= 1e-8 off its planted key before any kernel is asked (`test_reference_decodes`).
`wiring` is a plain torch restatement of updater_run's buffers and row ranges; `test_probes` plants 14 wiring faults in it and each
must break the decode on the cases' own inputs.

Not observable by this construction: LayerNorm eps 1e-5 against 1e-6 (both give +-1 in bf16).  The tuning variables read once per
process (MVT_TIME_NMB1, MVT_FRAME_NMB1, MVT_BLOCK_NMB) are set by tests/test_gpu_tuning_switches.py, which runs cases of this file
in a child process per value; `forms` takes the two it depends on as arguments and defaults to the environment.  Per-head targets exist only in the virtual<-point stage (two wanted
codes, heads alternate): its 128 targets cover every point index up to n = 128 and otherwise both sides of every 32-key block
(which contains every key-split and tile edge); rotated target sets reach every index up to n = 384.

GPU tests (`-m gpu`) drive the product's entries; the tests without the marker are the CPU checks of the construction.
"""
import collections
import functools
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import hip_mock
from oracle import mvt_oracle as O

gpu = pytest.mark.gpu

DEV = "cuda:0"
HID, HEADS, DH, NV, MLP, OUT, TOK_D = 256, 6, 48, 64, 1024, 131, 581
INNER = HEADS * DH
FC0 = 3 * 64 + 3  # the correlation block of a token row: columns [195, 451), exactly 256 wide
C = 16.0  # (the fp64 reference keeps the 1 - eps / (2 C^2) of a context LayerNorm, eps = 1e-5: every copy through one adds eps / (2 C) to
#            the written columns, 3.1e-7 at C = 16 -- two of them in a chain stay below the 1e-6 asked of the reference; C = 2 gives 2.5e-6)
BETA = 8.0
NBITS = 128
NAN = float("nan")
BLOCKS = ("time", "v2p", "vself", "p2v")  # launch order within a layer
PREFIX = {"time": ("time_blocks", "attn"), "v2p": ("space_virtual2point_blocks", "cross_attn"),
          "vself": ("space_virtual_blocks", "attn"), "p2v": ("space_point2virtual_blocks", "cross_attn")}
U = "updateformer."


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ codes, columns


@functools.lru_cache(None)
def codebook():
    """[2048][16] bits of RM(2, 4) = extended Hamming [16, 11, 4]; the first 32 words are RM(1, 4) (pairwise distance >= 8)."""
    pts = torch.arange(16)
    xs = [(pts >> i) & 1 for i in range(4)]
    gens = xs + [torch.ones(16, dtype=torch.long)] + [xs[i] * xs[j] for i in range(4) for j in range(i + 1, 4)]
    msg = (torch.arange(2048)[:, None] >> torch.arange(11)[None]) & 1
    return (msg @ torch.stack(gens)) % 2


_g = torch.Generator().manual_seed(5)
COLS = torch.randperm(HID, generator=_g)   # bit k lives in columns COLS[2k] (e) and COLS[2k + 1] (-e)
TOKP = torch.randperm(HID, generator=_g)   # row column c is token column FC0 + TOKP[c]


def ecol(k):
    return int(COLS[2 * k])


def ocol(k):
    return int(COLS[2 * k + 1])


def to_rows(bits):
    """[R][128] bits -> [R][256] fp64 rows of +-C."""
    s = C * (1 - 2 * bits.double())
    x = torch.empty(bits.shape[0], HID, dtype=torch.float64)
    x[:, COLS[0::2]] = s
    x[:, COLS[1::2]] = -s
    return x


# ------------------------------------------------------------------ configurations

Attn = collections.namedtuple("Attn", "layer block want key heads")  # want: 6 field names; heads: 6 lists of (src, dst)
Mlp = collections.namedtuple("Mlp", "layer block pairs")             # pairs: (src, dst, xor); src -1: the constant
Plan = collections.namedtuple("Plan", "name S fields ops readout")
ONE, ZERO = -2, -1  # constant sources of an attention copy


def layout(spec, alias=()):
    """Sequential bit fields; alias: (name, [bits]) for fields that reuse bits which are blank on the rows that write them."""
    f, o = {}, 0
    for name, w in spec:
        f[name] = list(range(o, o + w))
        o += w
    for name, bits in alias:
        f[name] = [b if isinstance(b, int) else o + int(b[1:]) for b in bits]  # "+3": the 4th free bit after the spec
    assert max(max(v) for v in f.values()) < NBITS, max(max(v) for v in f.values())
    return f


def spread(copies, hs=range(HEADS)):
    hs, out = list(hs), [[] for _ in range(HEADS)]
    for i, c in enumerate(copies):
        out[hs[i % len(hs)]].append(c)
    assert all(len(o) <= DH for o in out)
    return out


def tag(layer):
    return [ONE, ONE if layer else ZERO]


def copy(src, dst):
    assert len(src) == len(dst), (len(src), len(dst))
    return list(zip(src, dst))


def id_fields(S):
    return [("TRK", 10), ("FRM", 5 if S > 16 else 4), ("SET", 2)]


def make_plan(name, S):
    base, _, L = name.partition("@")
    L = int(L or 0)
    idw = sum(w for _, w in id_fields(S))
    T4 = [("KF", 16), ("WT", 16), ("KP", 16), ("WV", 16)]
    ops = []
    if base == "time_pt":
        f = layout([("KF", 16), ("WT", 16)] + id_fields(S) + [("B1", idw + 2)])
        ident = f["TRK"] + f["FRM"] + f["SET"]
        ops = [Attn(L, "time", ["WT"] * 6, "KF", spread(copy(ident + tag(L), f["B1"])))]
        show = f["B1"] + ident
    elif base == "time_virt_p2v":
        f = layout(T4 + id_fields(S) + [("B1", 12), ("B2", 14)])
        ops = [Attn(L, "time", ["WT"] * 6, "KF", spread(copy(f["TRK"] + tag(L), f["B1"]))),
               Attn(L, "p2v", ["WV"] * 6, "KP", spread(copy(f["B1"] + tag(L), f["B2"])))]
        show = f["B2"] + f["B1"]
    elif base == "p2v":
        f = layout([("KP", 16), ("WV", 16)] + id_fields(S) + [("B2", idw + 2)])
        ident = f["TRK"] + f["FRM"] + f["SET"]
        ops = [Attn(L, "p2v", ["WV"] * 6, "KP", spread(copy(ident + tag(L), f["B2"])))]
        show = f["B2"] + ident
    elif base == "v2p_p2v":
        spec = [("KP", 16), ("WV", 16), ("WP0", 16), ("WP1", 16)] + id_fields(S) + [("B10", idw), ("B11", idw)]
        f = layout(spec, alias=[("B2", list(range(32, 64)) + ["+%d" % i for i in range(2 * idw + 2 - 32)])])
        ident = f["TRK"] + f["FRM"] + f["SET"]
        h0, h1 = spread(copy(ident, f["B10"]), (0, 2, 4)), spread(copy(ident, f["B11"]), (1, 3, 5))
        ops = [Attn(L, "v2p", ["WP0", "WP1"] * 3, "KP", [a + b for a, b in zip(h0, h1)]),
               Attn(L, "p2v", ["WV"] * 6, "KP", spread(copy(f["B10"] + f["B11"] + tag(L), f["B2"])))]
        show = f["B2"]
    elif base == "v2p_vself_p2v":
        spec = [("KP", 16), ("WV", 16), ("WP0", 16)] + id_fields(S) + [("B1", idw + 2), ("B3", idw + 4)]
        f = layout(spec, alias=[("B2", list(range(32, 48)) + ["+%d" % i for i in range(idw + 6 - 16)])])
        ident = f["TRK"] + f["FRM"] + f["SET"]
        ops = [Attn(L, "v2p", ["WP0"] * 6, "KP", spread(copy(ident + tag(L), f["B1"]))),
               Attn(L, "vself", ["WV"] * 6, "KP", spread(copy(f["B1"] + tag(L), f["B3"]))),
               Attn(L, "p2v", ["WV"] * 6, "KP", spread(copy(f["B3"] + tag(L), f["B2"])))]
        show = f["B2"]
    elif base == "l0p2v_l1time":
        f = layout(T4 + id_fields(S) + [("B2", 8), ("B1", 8 + dict(id_fields(S))["FRM"] + 2)])
        ops = [Attn(0, "p2v", ["WV"] * 6, "KP", spread(copy(f["TRK"][:6] + tag(0), f["B2"]))),
               Attn(1, "time", ["WT"] * 6, "KF", spread(copy(f["B2"] + f["FRM"] + tag(1), f["B1"])))]
        show = f["B1"] + f["B2"]
    elif base == "l0vself_l1time_l1p2v":
        f = layout(T4 + id_fields(S) + [("B3", 8), ("B1", 10), ("B2", 12)])
        ops = [Attn(0, "vself", ["WV"] * 6, "KP", spread(copy(f["TRK"][:6] + tag(0), f["B3"]))),
               Attn(1, "time", ["WT"] * 6, "KF", spread(copy(f["B3"] + tag(1), f["B1"]))),
               Attn(1, "p2v", ["WV"] * 6, "KP", spread(copy(f["B1"] + tag(1), f["B2"])))]
        show = f["B2"] + f["B1"]
    elif base.startswith("mlp_"):
        blk = base[4:]
        f = layout([("KP", 16), ("WV", 16)] + id_fields(S) + [("B1", 11), ("B2", 13), ("B4", 11)])
        pat = 5 + 3 * (4 * L + BLOCKS.index(blk))
        xor = [(pat >> i) & 1 for i in range(10)]
        if blk == "p2v":  # the attention part of the same block writes what its MLP reads
            ops = [Attn(L, "p2v", ["WV"] * 6, "KP", spread(copy(f["TRK"] + [ZERO] + tag(L), f["B2"]))),
                   Mlp(L, "p2v", [(s, d, x) for s, d, x in zip(f["B2"][:10], f["B4"], xor)] + [(-1, f["B4"][10], 0)])]
        else:
            ops = [Mlp(L, blk, [(s, d, x) for s, d, x in zip(f["TRK"], f["B1"], xor)] + [(-1, f["B1"][10], 0)]),
                   Attn(L, "p2v", ["WV"] * 6, "KP", spread(copy(f["B1"] + tag(L), f["B2"])))]
        show = f["B4"] + f["B2"] + f["B1"]
    else:
        raise KeyError(name)
    ops.sort(key=lambda o: (o.layer, BLOCKS.index(o.block), isinstance(o, Mlp)))
    show = list(dict.fromkeys(show))
    readout = (show + [b for b in range(NBITS) if b not in show])[:65]
    return Plan(name, S, f, ops, readout)


SPACE = [f"{b}@{L}" for b in ("time_virt_p2v", "p2v", "v2p_p2v", "v2p_vself_p2v") for L in (0, 1)]
TIME = ["time_pt@0", "time_pt@1", "time_virt_p2v@0", "time_virt_p2v@1"]
CHAINS = ["time_pt@0", "time_pt@1"] + SPACE + ["l0p2v_l1time", "l0vself_l1time_l1p2v"]
MLPS = [f"mlp_{b}@{L}" for L in (0, 1) for b in BLOCKS]
CONFIGS = CHAINS + MLPS

# ------------------------------------------------------------------ planted rows

Case = collections.namedtuple("Case", "plan group_n S pbits vbits tau mu pi nu pset pj pt_")  # pset: position of the row's set


def v2p_targets(nmin, rot=0):
    """128 point indices every query set has: all of them up to 128 tracks, otherwise both sides of every 32-key block.
    rot = 1, 2, 3: the indices from 0, 128, 256 on instead (up to 384 tracks the three reach every point index)."""
    if nmin <= 128 or rot:
        return [(i + 128 * max(rot - 1, 0)) % nmin for i in range(128)]
    e = {0, nmin - 1}
    for b in range(cdiv(nmin, 32) + 1):
        e.update(x for x in (32 * b - 1, 32 * b) if 0 <= x < nmin)
    e = sorted(e)
    i = 0
    while len(e) < 128:
        x = (97 * i + 13) % nmin
        if x not in e:
            e.append(x)
        i += 1
    return e[:128]


def put(bits, field, value):
    for i, b in enumerate(field):
        bits[:, b] = (value >> i) & 1


@functools.lru_cache(maxsize=64)
def make_case(name, group_n, S, nmin=None, set_ids=None, rot=0):
    """nmin / set_ids: one set of a grouped case on its own -- the virtual tokens of the whole case (their wanted points are
    indices that its smallest set has) and the set's own identity bits."""
    plan = make_plan(name, S)
    f, cb = plan.fields, codebook()
    n, nmin = sum(group_n), nmin or min(group_n)
    assert nmin <= min(group_n)
    pset = torch.repeat_interleave(torch.arange(len(group_n)), torch.tensor(group_n) * S)
    sid = torch.tensor(set_ids or range(len(group_n)))[pset]
    pj = torch.cat([torch.arange(k).repeat_interleave(S) for k in group_n])
    pt_ = torch.arange(S).repeat(n)
    tau = (pt_ + 1 + pj) % S
    mu = (5 * pj + 7 * pt_ + 3 + 13 * sid) % NV
    m = torch.arange(NV)
    tg = torch.tensor(v2p_targets(nmin, rot))
    pi = torch.stack([tg[0::2], tg[1::2]])
    nu = (29 * m + 11) % NV
    pb, vb = torch.zeros(n * S, NBITS, dtype=torch.long), torch.zeros(NV, NBITS, dtype=torch.long)
    for name_, pv, vv in (("KF", cb[pt_], cb[0].expand(NV, 16)), ("WT", cb[tau], cb[0].expand(NV, 16)), ("KP", cb[pj], cb[m]),
                          ("WV", cb[mu], cb[nu]), ("WP0", None, cb[pi[0]]), ("WP1", None, cb[pi[1]])):
        if name_ in f:
            if pv is not None:
                pb[:, f[name_]] = pv
            vb[:, f[name_]] = vv
    put(pb, f["TRK"], pj)
    put(pb, f["FRM"], pt_)
    put(pb, f["SET"], sid)
    put(vb, f["TRK"], m)
    return Case(plan, group_n, S, pb, vb, tau, mu, pi, nu, pset, pj, pt_)


def simulate(case):
    """The planted copies in integers: final bits of all rows (points, then the virtual rows set by set), in device order."""
    plan, S, G = case.plan, case.S, len(case.group_n)
    Mp = case.pbits.shape[0]
    bits = torch.cat([case.pbits, case.vbits.repeat_interleave(S, 0).repeat(G, 1)], 0)
    R = bits.shape[0]
    virt = torch.arange(R) >= Mp
    vr = torch.arange(R - Mp)
    set_ = torch.cat([case.pset, vr // (NV * S)])
    item = torch.cat([case.pj, (vr // S) % NV])
    frame = torch.cat([case.pt_, vr % S])
    poff = torch.tensor([0] + list(case.group_n)).cumsum(0)[:-1] * S
    rows_of = {"time": torch.arange(R), "v2p": torch.arange(Mp, R), "vself": torch.arange(Mp, R), "p2v": torch.arange(Mp)}
    for op in plan.ops:
        q = rows_of[op.block]
        new = bits.clone()
        if isinstance(op, Mlp):
            for s, d, x in op.pairs:
                assert not bits[q, d].any()
                new[q, d] = (1 if s < 0 else bits[q, s]) ^ x
            bits = new
            continue
        for h in range(HEADS):
            if op.block == "time":
                tgt = torch.where(virt, torch.arange(R), torch.arange(R) - frame + torch.cat([case.tau, frame[Mp:]]))
            elif op.block == "v2p":
                tgt = poff[set_[q]] + case.pi[int(op.want[h][2])][item[q]] * S + frame[q]
            elif op.block == "vself":
                tgt = Mp + (set_[q] * NV + case.nu[item[q]]) * S + frame[q]
            else:
                tgt = Mp + (set_[q] * NV + case.mu) * S + frame[q]
            assert torch.equal(bits[tgt][:, plan.fields[op.key]], bits[q][:, plan.fields[op.want[h]]]), (plan.name, op.block, h)
            for s, d in op.heads[h]:
                assert not bits[q, d].any(), (plan.name, op.block, d)
                new[q, d] = (s == ONE) * 1 if s < 0 else bits[tgt, s]
                if op.block == "time" and s >= 0:  # the virtual rows see all their frames: the copy must not depend on it
                    assert torch.equal(bits[Mp:, s], bits[Mp + (vr // S) * S, s])
        bits = new
    return bits


def readout_columns(bits_r):
    """[R][65] read-out bits -> the planted delta [R][131]: 3 coordinates, then +-pairs (bits 3 .. 64, bits 3 and 4 once more)."""
    e = C * (1 - 2 * bits_r.double())
    pairs = torch.cat([e[:, 3:], e[:, 3:5]], 1)
    return torch.cat([e[:, :3], torch.stack([pairs, -pairs], 2).reshape(e.shape[0], -1)], 1)


def expected_delta(case):
    Mp = case.pbits.shape[0]
    return readout_columns(simulate(case)[:Mp][:, case.plan.readout])


# ------------------------------------------------------------------ planted weights


def ctx_norm(layer, block):
    i = 2 * layer + (block == "p2v")
    col = torch.arange(HID)
    return (1 + ((col * (2 * i + 3) + i) // 3) % 2).double(), (3 + (col * (i + 2) + i) % 3).double()


HEAD_GW = (1 + torch.arange(128) % 2).double()
# (gw s + gb is never 0: the fp32 GroupNorm gives +-(1 - 1.25e-6), which rounds to +-1 in bf16 only next to a non-zero integer)
HEAD_GB = torch.where(torch.arange(128) % 2 == 0, torch.tensor([-3, -2, 0, 2, 3])[(torch.arange(128) // 2) % 5],
                      torch.tensor([-3, -1, 0, 1, 3])[(torch.arange(128) // 2) % 5]).double()
_gh = torch.Generator().manual_seed(11)
HEAD_WU = 16.0 * (2 * torch.randint(0, 2, (128, 128), generator=_gh) - 1).double()
HEAD_BU = 16.0 * torch.randint(-40, 8, (128,), generator=_gh).double()


@functools.lru_cache(maxsize=64)
def plant(name, S):
    """fp64 state-dict entries of the planted updater (everything but the virtual tokens, which are rows)."""
    plan = make_plan(name, S)
    W = {}

    def lin(nm, n, k):
        W[nm + ".weight"], W[nm + ".bias"] = torch.zeros(n, k, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        return W[nm + ".weight"], W[nm + ".bias"]

    w, _ = lin(U + "input_transform", HID, TOK_D)
    w[torch.arange(HID), FC0 + TOKP] = 1
    w0, _ = lin(U + "flow_head.0", OUT, HID)
    w2, _ = lin(U + "flow_head.2", OUT, OUT)
    w4, _ = lin(U + "flow_head.4", OUT, OUT)
    w2 += torch.eye(OUT, dtype=torch.float64)
    for i, b in enumerate(plan.readout):
        w0[2 * i, ecol(b)], w0[2 * i + 1, ecol(b)] = 1, -1
    for i in range(3):
        w4[i, 2 * i], w4[i, 2 * i + 1] = 1, -1
    for p in range(64):  # pair p: bit 3 + p (p < 62), then bits 3 and 4 again
        i = 3 + p if p < 62 else 3 + p - 62
        w4[3 + 2 * p, 2 * i], w4[3 + 2 * p, 2 * i + 1] = 1, -1
        w4[4 + 2 * p, 2 * i], w4[4 + 2 * p, 2 * i + 1] = -1, 1
    for layer in range(2):
        for blk in BLOCKS:
            p = f"{U}{PREFIX[blk][0]}.{layer}"
            a = f"{p}.{PREFIX[blk][1]}"
            lin(a + ".to_q", INNER, HID), lin(a + ".to_kv", 2 * INNER, HID), lin(a + ".to_out", HID, INNER)
            lin(p + ".mlp.fc1", MLP, HID), lin(p + ".mlp.fc2", HID, MLP)
            if "cross" in a:
                W[p + ".norm_context.weight"], W[p + ".norm_context.bias"] = ctx_norm(layer, blk)
    for op in plan.ops:
        p = f"{U}{PREFIX[op.block][0]}.{op.layer}"
        if isinstance(op, Mlp):
            w1, b1, w2_ = W[p + ".mlp.fc1.weight"], W[p + ".mlp.fc1.bias"], W[p + ".mlp.fc2.weight"]
            for k, (s, d, x) in enumerate(op.pairs):
                u = 256 * (k % 4) + 17 * (k // 4) + 3  # every 256-chunk of the hidden layer carries bits
                if s < 0:
                    b1[u] = 16.0
                else:
                    w1[u, ecol(s)] = 16.0 if x else -16.0
                w2_[ecol(d), u], w2_[ocol(d), u] = -2 * C / 16, 2 * C / 16
            continue
        a = f"{p}.{PREFIX[op.block][1]}"
        g, b = ctx_norm(op.layer, op.block) if "cross" in a else (torch.ones(HID, dtype=torch.float64), torch.zeros(HID, dtype=torch.float64))
        wq, wkv, bkv, wo = W[a + ".to_q.weight"], W[a + ".to_kv.weight"], W[a + ".to_kv.bias"], W[a + ".to_out.weight"]
        for h in range(HEADS):
            wf, kf = plan.fields[op.want[h]], plan.fields[op.key]
            for r in range(3):
                for i in range(16):
                    d = h * DH + r * 16 + i
                    wq[d, ecol(wf[i])] = BETA
                    c = ecol(kf[i])
                    wkv[d, c] = 1 / g[c]
                    bkv[d] = -b[c] / g[c]
            for dd, (s, dst) in enumerate(op.heads[h]):
                d = h * DH + dd
                if s < 0:
                    bkv[INNER + d] = float(s == ONE)
                else:
                    c = ecol(s)
                    wkv[INNER + d, c] = -0.5 / g[c]
                    bkv[INNER + d] = 0.5 + 0.5 * b[c] / g[c]
                wo[ecol(dst), d], wo[ocol(dst), d] = -2 * C, 2 * C
    # the track / feature update behind the flow head (fused head): integer GroupNorm affine, +-16 feature update
    W["ffeats_norm.weight"], W["ffeats_norm.bias"] = HEAD_GW, HEAD_GB
    W["ffeats_updater.0.weight"], W["ffeats_updater.0.bias"] = HEAD_WU, HEAD_BU
    return W


def weights_of(case):
    W = dict(plant(case.plan.name, case.S))
    W[U + "virual_tracks"] = to_rows(case.vbits).reshape(1, NV, 1, HID)
    return W


def tokens_of(case):
    """[Mp][581] fp64 token rows: the planted row in the correlation block, everything else zero."""
    x = torch.zeros(case.pbits.shape[0], TOK_D, dtype=torch.float64)
    x[:, FC0 + TOKP] = to_rows(case.pbits)
    return x


# ------------------------------------------------------------------ the fp64 reference, with every softmax watched


class _WatchedF:
    """torch.nn.functional with a scaled_dot_product_attention that records, per call, the weight not on the planted keys (the
    keys whose score ties with the best one: the frames of a virtual track are identical until a stage writes them)."""

    def __init__(self):
        self.off = []

    def __getattr__(self, k):
        return getattr(F, k)

    def scaled_dot_product_attention(self, q, k, v):
        s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
        p = torch.softmax(s, -1)
        self.off.append(float((1 - (p * (s >= s.amax(-1, keepdim=True) - 1e-6)).sum(-1)).max()))
        return p @ v


def oracle_cfg(S):
    return O.TrackerConfig(sliding_window_len=S, space_depth=2, time_depth=2)


@functools.lru_cache(maxsize=8)
def oracle_delta(name, group_n, S, rot=0):
    """oracle.update_former in fp64 on the planted model, set by set (the sets are independent) -> delta [Mp][131], and the
    largest off-target softmax weight of the active stages."""
    case = make_case(name, group_n, S, rot=rot)
    W, x = weights_of(case), tokens_of(case)
    active = {4 * op.layer + BLOCKS.index(op.block) for op in case.plan.ops if isinstance(op, Attn)}
    outs, off, r0 = [], 0.0, 0
    watch, old = _WatchedF(), O.F
    O.F = watch
    try:
        with torch.no_grad():
            for k in group_n:
                del watch.off[:]
                outs.append(O.update_former(W, x[r0:r0 + k * S].reshape(1, k, S, TOK_D), oracle_cfg(S)).reshape(k * S, OUT))
                assert len(watch.off) == 8
                off = max([off] + [watch.off[i] for i in active])
                r0 += k * S
    finally:
        O.F = old
    return torch.cat(outs, 0), off


def check_decodes(delta, want, what=""):
    """Every element rounds to the planted integer and lies within 2^-6 of it."""
    delta = delta.detach().double().cpu()
    assert delta.shape == want.shape, (delta.shape, want.shape)
    assert bool(torch.isfinite(delta).all()), f"{what}: {int((~torch.isfinite(delta)).sum())} non-finite elements"
    bad = ((delta - want).abs() > 2.0 ** -6).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} elements do not decode, first (row, column) {bad[0].tolist()}: "
                              f"{delta[tuple(bad[0])].item()} for {want[tuple(bad[0])].item()}")
    assert torch.equal(delta.round(), want)


# ------------------------------------------------------------------ the form selection of updater_run / mvt_attn_block_fused_bf16, restated


def env_is_zero(name):
    """`getenv(name) && atoi(getenv(name)) == 0`: how the library reads MVT_TIME_NMB1 / MVT_FRAME_NMB1."""
    v = os.environ.get(name)
    m = None if v is None else re.match(r"\s*[+-]?\d+", v)
    return v is not None and (int(m.group()) if m else 0) == 0


def forms(n, S, mask, G=1, time_small=None, frame_small=None):
    """time_small / frame_small: the 32-row time tiles / 32-token frame tiles are allowed (False = MVT_TIME_NMB1=0 /
    MVT_FRAME_NMB1=0; default: this process's environment)."""
    time_small = not env_is_zero("MVT_TIME_NMB1") if time_small is None else time_small
    frame_small = not env_is_zero("MVT_FRAME_NMB1") if frame_small is None else frame_small
    Mp, Mv = n * S, G * NV * S
    M = Mp + Mv
    grouped = G > 1
    fuse_time, fuse_p2v, fuse_vs = bool(mask & 1) and S <= 32, bool(mask & 2) and not grouped, bool(mask & 4) and not grouped
    small = frame_small and Mp >= 4096 and cdiv(n, 32) * S <= 256
    fold = bool(mask & 32) and fuse_p2v and fuse_vs and Mp >= 4096 and not small and 8 * cdiv(n, 64) >= cdiv(3 * INNER, 32)
    parts = bool(mask & 16) and not grouped and n >= 512 and cdiv(n, 32) % 4 == 0
    f = {"time": "sep" if not fuse_time else ("tile32" if time_small and cdiv(M, (32 // S) * S) <= 256 else "tile64"),
         "v2p": "partials" if parts else ("segmented" if grouped else "plain"),
         "vself": "deferred" if fold else ("frame_split" if fuse_vs else ("segmented" if grouped else "sep")),
         "p2v": "ctx" if fold else (("frame32" if small else "frame64") if fuse_p2v and Mp >= 4096 else ("segmented" if grouped else "sep"))}
    if fold and n % 64:
        f["p2v"] = "ctx_ragged"
    return f


N_S12 = (5, 37, 341, 342, 448, 449, 511, 512, 513, 672, 673, 704, 740)  # (704 = 11 full 64-token tiles of the context form)
N_MLP = (5, 37, 342, 513, 673, 704, 740)
# the MLPs of the two blocks whose kernel MVT_FRAME_NMB1 switches, at the other ends of the range of n that it moves ([342, 672]) and
# at whole 64-token tiles inside it (test_gpu_tuning_switches.py runs them under MVT_FRAME_NMB1=0)
N_MLP_FRAME = (341, 448, 512, 672)
MLPS_FRAME = [f"mlp_{b}@{L}" for L in (0, 1) for b in ("p2v", "vself")]
MASKS = (0, 1, 2, 4, 16, 23, 39, 55)
GROUPS = ((1, 37, 300, 5), (342, 400))


def test_cases_reach_every_form():
    """Both sides of every threshold of the table take the form the table says, and every form is taken by some case."""
    at = lambda n, mask, S=12: forms(n, S, mask)
    assert at(341, 55)["p2v"] == "sep" and at(342, 55)["p2v"] == "frame32"
    assert at(448, 55)["time"] == "tile32" and at(449, 55)["time"] == "tile64"
    assert [at(n, 55)["v2p"] for n in (511, 512, 513)] == ["plain", "partials", "plain"]
    assert at(672, 55) == {"time": "tile64", "v2p": "plain", "vself": "frame_split", "p2v": "frame32"}  # (21 key blocks: no partials)
    assert at(673, 55)["p2v"] == "ctx_ragged" and at(673, 55)["vself"] == "deferred" and 673 % 64 == 33
    assert at(673, 23)["p2v"] == "frame64" and at(673, 39)["v2p"] == "plain"
    assert at(740, 55) == {"time": "tile64", "v2p": "partials", "vself": "deferred", "p2v": "ctx_ragged"} and 740 % 32 == 4 and 740 % 64 == 36
    assert forms(511, 8, 55)["p2v"] == "sep" and forms(512, 8, 55)["p2v"] == "frame32" and forms(512, 8, 55)["v2p"] == "partials"
    assert forms(21, 32, 55)["time"] == "tile32" and forms(21, 7, 1)["time"] == "tile32"
    seen = {k: set() for k in BLOCKS}
    for n in N_S12:
        for m in MASKS:
            for k, v in forms(n, 12, m).items():
                seen[k].add(v)
    for gn in GROUPS:
        for k, v in forms(sum(gn), 12, 55, len(gn)).items():
            seen[k].add(v)
    assert seen["time"] == {"sep", "tile32", "tile64"}
    assert seen["v2p"] == {"plain", "partials", "segmented"}
    assert seen["vself"] == {"sep", "frame_split", "deferred", "segmented"}
    assert at(704, 55)["p2v"] == "ctx" and at(704, 55)["v2p"] == "plain"
    assert seen["p2v"] == {"sep", "frame32", "frame64", "ctx", "ctx_ragged", "segmented"}


# ------------------------------------------------------------------ CPU: the reference decodes


REF_CASES = ([(c, g, 12) for c in CONFIGS for g in ((5,), (37,), (1, 37, 5))] + [(c, (513,), 12) for c in CHAINS]
             + [(c, (21,), S) for c in TIME for S in (7, 16, 32)] + [(c, (40,), 8) for c in CHAINS])


@pytest.mark.parametrize("name,group_n,S", REF_CASES)
def test_reference_decodes(name, group_n, S):
    """The fp64 oracle on the planted model is within 1e-6 of the simulated integers, and no active softmax leaks more than 1e-8."""
    case = make_case(name, group_n, S)
    d, off = oracle_delta(name, group_n, S)
    want = expected_delta(case)
    assert (d - want).abs().max().item() <= 1e-6, (d - want).abs().max().item()
    assert off <= 1e-8, off
    check_decodes(d, want, "oracle")
    x = to_rows(simulate(case))
    assert bool((x.sum(1) == 0).all()) and bool((x.abs() == C).all())  # every final row is still balanced


@pytest.mark.parametrize("rot", [1, 2, 3])
def test_reference_decodes_rotated_targets(rot):
    """The virtual<-point targets rotated by 128: with rot = 1, 2, 3 every point index up to 384 tracks is some token's planted key."""
    n = 300
    assert sorted(set(sum((v2p_targets(n, r) for r in (1, 2, 3)), []))) == list(range(n))
    d, off = oracle_delta("v2p_p2v@0", (n,), 12, rot)
    want = expected_delta(make_case("v2p_p2v@0", (n,), 12, rot=rot))
    assert (d - want).abs().max().item() <= 1e-6 and off <= 1e-8, ((d - want).abs().max().item(), off)


def test_rows_are_exact_under_layernorm():
    """LayerNorm of a balanced +-C row is the sign pattern after bf16 rounding, at both eps, also with a 1e-6 relative residue."""
    case = make_case("v2p_vself_p2v@0", (37,), 12)
    x = to_rows(simulate(case)).float()
    for eps in (1e-6, 1e-5):
        for r in (x, x * (1 + 1e-6 * torch.randn(x.shape, generator=torch.Generator().manual_seed(1)))):
            assert torch.equal(F.layer_norm(r, (HID,), None, None, eps).to(torch.bfloat16).float(), torch.sign(x))
    h = torch.tensor([16.0, -16.0, 0.0])
    assert torch.equal(F.gelu(h, approximate="tanh"), torch.relu(h)) and torch.equal(F.gelu(h), torch.relu(h))


# ------------------------------------------------------------------ CPU: the wiring restated, and the faults it must not survive

FAULTS = ("time_next_track", "virtual_token_mod", "v2p_next_frame", "last_point_key_dropped", "segment_plus_one_track",
          "vself_other_set", "p2v_kv_before_vself", "ctx_norms_swapped", "layer1_uses_layer0_to_out", "no_buffer_swap",
          "next_projection_virtual_rows_only", "qp_one_row_short", "virtual_mlp_chunk_skipped", "residual_dropped")


def wiring(W, x, group_n, S, fault=None):
    """updater_run restated in fp64 torch: the same buffers (tok, qkv, qkv_nx, qp), row ranges and order of projections."""
    G, n = len(group_n), sum(group_n)
    Mp, Mv = n * S, G * NV * S
    M = Mp + Mv
    ln = lambda a, w=None, b=None, eps=1e-6: F.layer_norm(a, (HID,), w, b, eps)
    lin = lambda nm, a: a @ W[nm + ".weight"].t() + W[nm + ".bias"]
    name = lambda blk, i: (f"{U}{PREFIX[blk][0]}.{i}", f"{U}{PREFIX[blk][0]}.{i}.{PREFIX[blk][1]}")
    qkv_of = lambda a_, t: torch.cat([lin(a_ + ".to_q", t), lin(a_ + ".to_kv", t)], 1)
    vr = torch.arange(Mv)
    vtok = W[U + "virual_tracks"].reshape(NV, HID)[(vr % NV) if fault == "virtual_token_mod" else (vr // S) % NV]
    tok = torch.cat([lin(U + "input_transform", x), vtok], 0)
    off = torch.tensor([0] + list(group_n)).cumsum(0)
    set_ = torch.cat([torch.repeat_interleave(torch.arange(G), torch.tensor(group_n) * S), vr // (NV * S)])
    track = torch.cat([torch.arange(n).repeat_interleave(S), n + vr // S])
    frame = torch.cat([torch.arange(S).repeat(n), vr % S])
    P, V = slice(0, Mp), slice(Mp, M)

    def attend(q, k, v, mask):
        out = []
        for h in range(HEADS):
            hs = slice(h * DH, (h + 1) * DH)
            s = (q[:, hs] @ k[:, hs].t() / math.sqrt(DH)).masked_fill(~mask, -math.inf)
            out.append(torch.softmax(s, 1) @ v[:, hs])
        return torch.cat(out, 1)

    def block(blk, i, xr, att, virtual=False):
        p, a_ = name(blk, i)
        wo = name(blk, 0)[1] if (fault == "layer1_uses_layer0_to_out" and i == 1) else a_
        xr = xr + lin(wo + ".to_out", att)
        hdn = F.gelu(lin(p + ".mlp.fc1", ln(xr)), approximate="tanh")
        if virtual and fault == "virtual_mlp_chunk_skipped":
            hdn[:, 256:512] = 0
        mlp = lin(p + ".mlp.fc2", hdn)
        return mlp if fault == "residual_dropped" else xr + mlp

    def ctx(blk, i):
        if fault == "ctx_norms_swapped":
            blk = {"v2p": "p2v", "p2v": "v2p"}[blk]
        p = name(blk, i)[0]
        return W[p + ".norm_context.weight"], W[p + ".norm_context.bias"], 1e-5

    same = lambda a_, b_: a_[:, None] == b_[None, :]
    qkv, qkv_nx, qp = torch.zeros(M, 3 * INNER, dtype=x.dtype), torch.zeros(M, 3 * INNER, dtype=x.dtype), torch.zeros(Mp, INNER, dtype=x.dtype)
    qkv[:] = qkv_of(name("time", 0)[1], ln(tok))
    I = INNER
    for i in range(2):
        last = i == 1
        # time attention over the frames of every track, then the block over all rows and its three row-ranged projections
        m = same(track, track)
        if fault == "time_next_track":
            m = m | same(track + 1, track)
        tok = block("time", i, tok, attend(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], m))
        qkv[P, I:] = lin(name("v2p", i)[1] + ".to_kv", ln(tok[P], *ctx("v2p", i)))
        hi = Mp - 1 if fault == "qp_one_row_short" else Mp
        qp[:hi] = lin(name("p2v", i)[1] + ".to_q", ln(tok[:hi]))
        qkv[V, :I] = lin(name("v2p", i)[1] + ".to_q", ln(tok[V]))
        # virtual <- point, per frame and per query set
        kf = (frame[P] + S - 1) % S if fault == "v2p_next_frame" else frame[P]
        m = same(frame[V], kf) & same(set_[V], set_[P])
        if fault == "last_point_key_dropped":
            m = m & ~torch.isin(track[P], off[1:] - 1)[None, :]
        if fault == "segment_plus_one_track":
            m = m | (same(frame[V], kf) & (track[P][None, :] == off[1:][set_[V]][:, None]))
        tok[V] = block("v2p", i, tok[V], attend(qkv[V, :I], qkv[P, I:2 * I], qkv[P, 2 * I:], m), True)
        qkv[V] = qkv_of(name("vself", i)[1], ln(tok[V]))
        # virtual self
        ks = (set_[V] + 1) % G if fault == "vself_other_set" else set_[V]
        m = same(frame[V], frame[V]) & same(set_[V], ks)
        if fault == "p2v_kv_before_vself":
            stale = lin(name("p2v", i)[1] + ".to_kv", ln(tok[V], *ctx("p2v", i)))
        tok[V] = block("vself", i, tok[V], attend(qkv[V, :I], qkv[V, I:2 * I], qkv[V, 2 * I:], m), True)
        qkv[V, I:] = stale if fault == "p2v_kv_before_vself" else lin(name("p2v", i)[1] + ".to_kv", ln(tok[V], *ctx("p2v", i)))
        if not last:
            qkv_nx[V] = qkv_of(name("time", i + 1)[1], ln(tok[V]))
        # point <- virtual
        m = same(frame[P], frame[V]) & same(set_[P], set_[V])
        tok[P] = block("p2v", i, tok[P], attend(qp, qkv[V, I:2 * I], qkv[V, 2 * I:], m))
        if not last and fault != "next_projection_virtual_rows_only":
            qkv_nx[P] = qkv_of(name("time", i + 1)[1], ln(tok[P]))
        if fault != "no_buffer_swap":
            qkv, qkv_nx = qkv_nx, qkv
    y = F.relu(lin(U + "flow_head.0", tok[P]))
    return lin(U + "flow_head.4", F.relu(lin(U + "flow_head.2", y)))


def decodes(delta, want):
    return bool(torch.isfinite(delta).all()) and (delta - want).abs().max().item() <= 2.0 ** -6


PROBE_GROUPS = ((37,), (3, 5, 2))


@pytest.mark.parametrize("group_n", PROBE_GROUPS)
@pytest.mark.parametrize("name", CONFIGS)
def test_restated_wiring_decodes(name, group_n):
    case = make_case(name, group_n, 12)
    check_decodes(wiring(weights_of(case), tokens_of(case), group_n, 12), expected_delta(case), "restated wiring")


# the configuration and shape on which each planted fault has to show
PROBE_CASE = {"time_next_track": ("time_pt@0", (37,)), "virtual_token_mod": ("time_virt_p2v@0", (37,)),
              "v2p_next_frame": ("v2p_p2v@1", (37,)), "last_point_key_dropped": ("v2p_p2v@0", (37,)),
              "segment_plus_one_track": ("v2p_p2v@0", (3, 5, 2)), "vself_other_set": ("v2p_vself_p2v@1", (3, 5, 2)),
              "p2v_kv_before_vself": ("v2p_vself_p2v@0", (37,)), "ctx_norms_swapped": ("p2v@1", (37,)),
              "layer1_uses_layer0_to_out": ("l0p2v_l1time", (37,)), "no_buffer_swap": ("time_pt@1", (37,)),
              "next_projection_virtual_rows_only": ("l0p2v_l1time", (37,)), "qp_one_row_short": ("p2v@0", (37,)),
              "virtual_mlp_chunk_skipped": ("mlp_vself@1", (37,)), "residual_dropped": ("mlp_time@0", (37,))}


@pytest.mark.parametrize("fault", FAULTS)
def test_probes(fault):
    """Each planted wiring fault breaks the decode assertion on the cases' own inputs (and the same call without it passes)."""
    name, group_n = PROBE_CASE[fault]
    case = make_case(name, group_n, 12)
    W, x, want = weights_of(case), tokens_of(case), expected_delta(case)
    assert decodes(wiring(W, x, group_n, 12), want)
    assert not decodes(wiring(W, x, group_n, 12, fault), want), fault


def test_probe_faults_show_in_other_configurations_too():
    """The faults are not tied to one configuration: the stale k|v, the swapped buffers and the short qp show wherever their
    stage is active; the v2p faults also in the three-stage chain."""
    for fault, name in (("no_buffer_swap", "l0vself_l1time_l1p2v"), ("qp_one_row_short", "v2p_p2v@1"),
                        ("last_point_key_dropped", "v2p_vself_p2v@1"), ("ctx_norms_swapped", "v2p_p2v@0"),
                        ("virtual_mlp_chunk_skipped", "mlp_v2p@0"), ("residual_dropped", "mlp_p2v@1")):
        case = make_case(name, (37,), 12)
        assert not decodes(wiring(weights_of(case), tokens_of(case), (37,), 12, fault), expected_delta(case)), (fault, name)


# ------------------------------------------------------------------ models


def new_model(S):
    from mvtracker_amd.tracker import MVTracker
    return MVTracker(hidden_size=256, sliding_window_len=S, space_depth=2, time_depth=2).eval()


def load(model, case, mutate=None):
    W = weights_of(case)
    if mutate:
        mutate(W)
    sd = {k: torch.zeros_like(v) for k, v in model.state_dict().items()}
    for k, v in W.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
        sd[k] = v.float()
    model.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("name", ["time_pt@1", "v2p_vself_p2v@0", "l0vself_l1time_l1p2v", "mlp_v2p@1", "mlp_p2v@0"])
def test_mock_host_sequence_decodes(name, monkeypatch):
    """The host's fused launch sequence on the torch stand-ins of the kernels (tests/hip_mock.py) decodes the planted model."""
    hip_mock.install(monkeypatch)
    case = make_case(name, (37,), 12)
    m = new_model(12)
    load(m, case)
    m.precision = "bf16"
    with torch.no_grad():
        d = m.update_former(tokens_of(case).float().reshape(1, 37, 12, TOK_D))
    check_decodes(d.reshape(-1, OUT), expected_delta(case), "mock")


# ------------------------------------------------------------------ GPU


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


@functools.lru_cache(maxsize=None)
def gpu_model(S):
    m = new_model(S).to(DEV)
    m.precision = "bf16"
    return m


LDD = 136


class Run:
    """One planted case on the device: the product's packed struct, driven through the C entries with poisoned buffers."""

    def __init__(self, hip, case, mutate=None):
        self.hip, self.case = hip, case
        self.S, self.group_n, self.n = case.S, case.group_n, sum(case.group_n)
        self.m = gpu_model(case.S)
        self.m.fuse_attention, self.m.fuse_input = 55, True
        load(self.m, case, mutate)
        self.pk = self.m._pack(torch.device(DEV))
        self.w = self.pk["updater_struct"]
        self.frag = (self.w.input_frag.w, self.w.input_frag.b, self.w.input_frag.N, self.w.input_frag.K)
        assert self.frag[0]
        self.Mp = self.n * self.S
        rows = to_rows(case.pbits).float()
        x = torch.zeros(self.Mp, 584)
        x[:, FC0 + TOKP] = rows
        self.x = x.to(DEV)
        self.fcorr = rows[:, torch.argsort(TOKP)].contiguous().to(DEV)  # token column FC0 + c holds row column argsort(TOKP)[c]
        self.want = expected_delta(case)
        G = len(self.group_n)
        nbytes = hip.updateformer_workspace_bytes(self.n, self.S) if G == 1 else hip.updateformer_grouped_workspace_bytes(self.n, self.S, G)
        self.ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)

    def __call__(self, mask, entry="x", fuse_input=True, head=None):
        hip, w, S, n = self.hip, self.w, self.S, self.n
        w.fuse_attention = mask
        w.input_frag.w, w.input_frag.b, w.input_frag.N, w.input_frag.K = self.frag if fuse_input else (None, None, 0, 0)
        self.ws.fill_(255)  # every fp32 and every bf16 of the workspace is a NaN: an unwritten region decodes to nothing
        delta = torch.full((self.Mp + 1, LDD), NAN, device=DEV)
        upd = head or ()
        grouped = len(self.group_n) > 1
        if entry == "x":
            if grouped:
                hip.updateformer_forward_grouped(w, self.x, 584, list(self.group_n), delta, LDD, self.ws, *upd)
            else:
                hip.updateformer_forward(w, self.x, 584, n, delta, LDD, self.ws, *upd)
        else:
            z = lambda *s: torch.zeros(*s, device=DEV)
            coords = torch.arange(n, device=DEV, dtype=torch.float32)[:, None, None].expand(n, S, 3).contiguous()  # constant per track
            args = (coords, self.fcorr, 256, z(self.Mp, 128), 128, z(n, S, 2), z(n, TOK_D), z(S, TOK_D), 64)
            if grouped:
                hip.updateformer_forward_tokens_grouped(w, *args, list(self.group_n), delta, LDD, self.ws, *upd)
            else:
                hip.updateformer_forward_tokens(w, *args, n, delta, LDD, self.ws, *upd)
        torch.cuda.synchronize()
        w.fuse_attention = 55
        w.input_frag.w, w.input_frag.b, w.input_frag.N, w.input_frag.K = self.frag
        assert bool(torch.isnan(delta[:, OUT:]).all()) and bool(torch.isnan(delta[self.Mp]).all()), "padding / guard row written"
        return delta[:self.Mp, :OUT]

    def check(self, mask, **kw):
        d = self(mask, **kw)
        check_decodes(d, self.want, f"{self.case.plan.name} n={self.group_n} S={self.S} fuse_attention={mask} {kw} {forms(self.n, self.S, mask, len(self.group_n))}")
        return d


@gpu
@pytest.mark.parametrize("name,n", [(c, n) for c in CHAINS for n in N_S12] + [(c, n) for c in MLPS for n in N_MLP]
                         + [(c, n) for c in MLPS_FRAME for n in N_MLP_FRAME])
def test_composite_decodes(hip, name, n):
    """Every fuse mask, the fused-input path on and off and the _tokens entry decode to the planted integers; delta's padding
    columns and guard row stay NaN, the workspace is NaN before every call.
    (The MLP configurations run at the sizes where the block kernels change form.)"""
    run = Run(hip, make_case(name, (n,), 12))
    for mask in MASKS:
        run.check(mask)
    for mask in (0, 55):
        run.check(mask, fuse_input=False)
        run.check(mask, entry="tokens")


@gpu
@pytest.mark.parametrize("n", [341, 342, 384])
@pytest.mark.parametrize("name", ["v2p_p2v@0", "v2p_p2v@1"])
def test_v2p_reaches_every_point_index(hip, name, n):
    """Up to 384 tracks every point index is the planted key of some virtual token and head: the target sets that start at 0, 128 and 256."""
    assert sorted(set(sum((v2p_targets(n, r) for r in (1, 2, 3)), []))) == list(range(n))
    for rot in (1, 2, 3):
        run = Run(hip, make_case(name, (n,), 12, rot=rot))
        for mask in (0, 16, 55):
            run.check(mask)


def _swap_ctx_norms(W):
    a, b = (f"{U}{PREFIX[k][0]}.1.norm_context." for k in ("v2p", "p2v"))
    for t in ("weight", "bias"):
        W[a + t], W[b + t] = W[b + t], W[a + t]


def _layer0_to_out(W):
    for k in BLOCKS:
        W[f"{U}{PREFIX[k][0]}.1.{PREFIX[k][1]}.to_out.weight"] = W[f"{U}{PREFIX[k][0]}.0.{PREFIX[k][1]}.to_out.weight"]


def _layer0_vself_to_q(W):
    W[f"{U}space_virtual_blocks.1.attn.to_q.weight"] = W[f"{U}space_virtual_blocks.0.attn.to_q.weight"]


@gpu
@pytest.mark.parametrize("mutate", [_swap_ctx_norms, _layer0_to_out, _layer0_vself_to_q])
@pytest.mark.parametrize("n", [37, 740])
def test_device_answer_follows_the_planted_weights(hip, n, mutate):
    """The device's decode is not vacuous: with the two context norms of layer 1 swapped, layer 0's to_out in layer 1 or layer 0's
    virtual-self to_q in layer 1, the same inputs no longer decode under any mask (wrong answers, no faults: all buffers as before)."""
    case = make_case("v2p_vself_p2v@1", (n,), 12)
    run = Run(hip, case, mutate)
    for mask in (0, 55):
        assert not decodes(run(mask).double().cpu(), run.want), mask


@gpu
@pytest.mark.parametrize("name,S,n", [(c, 8, n) for c in CHAINS for n in (511, 512)] + [(c, S, 21) for c in TIME for S in (7, 16, 32)])
def test_other_window_lengths_decode(hip, name, S, n):
    """S = 8 at 4096 point rows exactly (and one track less); the time configurations alone at S = 7, 16, 32."""
    run = Run(hip, make_case(name, (n,), S))
    for mask in MASKS:
        run.check(mask)
    run.check(55, entry="tokens")


@gpu
@pytest.mark.parametrize("group_n", GROUPS)
@pytest.mark.parametrize("name", CHAINS + ["mlp_v2p@0", "mlp_vself@1"])
def test_grouped_decodes(hip, name, group_n):
    """G > 1: key codes are shared between the sets and V carries the set, so a leak across a set boundary does not decode; every
    set's rows are bit-equal to the same set run alone."""
    run = Run(hip, make_case(name, group_n, 12))
    outs = [run.check(mask) for mask in (0, 1, 55)] + [run.check(55, entry="tokens"), run.check(55, fuse_input=False)]
    d = outs[2].clone()
    assert all(torch.equal(o, d) for o in outs)
    r0 = 0
    for g, k in enumerate(group_n):  # the same set alone: the whole case's virtual tokens, the set's own identity bits
        alone = Run(hip, make_case(name, (k,), 12, nmin=min(group_n), set_ids=(g,))).check(55)
        assert torch.equal(alone, d[r0:r0 + k * 12]), g
        r0 += k * 12
    mdl = gpu_model(12)
    load(mdl, run.case)
    xs = [t.reshape(1, k, 12, TOK_D) for t, k in zip(torch.split(run.x[:, :TOK_D], [k * 12 for k in group_n]), group_n)]
    got = mdl.update_former_grouped(xs)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([g.reshape(-1, OUT) for g in got], 0), d)


@gpu
@pytest.mark.parametrize("n", [37, 342])
@pytest.mark.parametrize("name", CHAINS + ["mlp_time@0", "mlp_v2p@1", "mlp_vself@0", "mlp_p2v@1"])
def test_host_paths_decode(hip, name, n, monkeypatch):
    """The same planted model through the product entry (composite), the host's fused launch sequence (MVT_COMPOSITE=0) and the
    fp32 unfused sequence: the same integers."""
    case = make_case(name, (n,), 12)
    m = gpu_model(12)
    load(m, case)
    x = tokens_of(case).float().reshape(1, n, 12, TOK_D).to(DEV)
    want = expected_delta(case)
    try:
        m.fuse_attention, m.fuse_input = 55, True
        assert "updater_struct" in m._pack(torch.device(DEV))
        check_decodes(m.update_former(x).reshape(-1, OUT), want, "update_former")
        monkeypatch.setenv("MVT_COMPOSITE", "0")
        assert "updater_struct" not in m._pack(torch.device(DEV))
        check_decodes(m.update_former(x).reshape(-1, OUT), want, "MVT_COMPOSITE=0")
        m.precision = "fp32"
        check_decodes(m.update_former(x).reshape(-1, OUT), want, "fp32")
    finally:
        m.precision = "bf16"


# ------------------------------------------------------------------ the fused head, exactly

HEAD_ROWS = (1, 63, 64, 65, 100, 4097)


@functools.lru_cache(maxsize=None)
def head_case(rows):
    """Integer inputs and the exact results of mvt_update_head_bf16.  tok: 128 signal columns +-1, one column m, three coordinate
    columns and 2 x 62 junk columns that W0 reads with opposite signs (a skipped K step breaks the cancellation).
    delta = 2 x through W0 (b0 = 16 keeps the relus open, except on the rows whose coordinate is pushed below -16), W2 = 2 Q and
    W4 = Q^T (b4 = -32): delta[:, 3:] = 2 m +- 2, balanced."""
    g = torch.Generator().manual_seed(rows)
    perm = torch.randperm(HID, generator=g)
    sig, mcol, dcols, ju, jv = perm[:128], perm[128], perm[129:132], perm[132:194], perm[194:256]
    s = torch.stack([torch.randperm(128, generator=g) for _ in range(rows)]) % 2 * 2 - 1
    tok = torch.zeros(rows, HID, dtype=torch.float64)
    tok[:, sig] = s.double()
    tok[:, mcol] = torch.randint(-3, 4, (rows,), generator=g).double()
    tok[:, dcols] = torch.randint(-5, 6, (rows, 3), generator=g).double()
    tok[::7, dcols[1]] = -20.0  # relu closes: the coordinate update saturates at 2 * 0 - 32
    junk = torch.randint(-3, 4, (rows, 62), generator=g).double()
    tok[:, ju], tok[:, jv] = junk, junk
    W0 = torch.zeros(OUT, HID, dtype=torch.float64)
    R = torch.randint(-2, 3, (OUT, 62), generator=g).double()
    W0[:, ju], W0[:, jv] = R, -R
    W0[torch.arange(3), dcols] = 1
    W0[3 + torch.arange(128), sig] = 1
    W0[3:, mcol] = 1
    Q = torch.eye(OUT, dtype=torch.float64)[torch.randperm(OUT, generator=g)]
    W2, W4 = 2 * Q, Q.t().contiguous()
    b0, b2, b4 = torch.full((OUT,), 16.0, dtype=torch.float64), torch.zeros(OUT, dtype=torch.float64), torch.full((OUT,), -32.0, dtype=torch.float64)
    coords0 = torch.randint(-50, 51, (rows, 3), generator=g).double()
    ff0 = torch.randint(-9, 10, (rows, 128), generator=g).double()
    delta = F.relu(F.relu(tok @ W0.t() + b0) @ W2.t() + b2) @ W4.t() + b4
    want = head_results(delta, coords0, ff0)
    return dict(tok=tok, W0=W0, W2=W2, W4=W4, b0=b0, b2=b2, b4=b4, coords0=coords0, ff0=ff0, delta=delta, coords=want[0], ffeats=want[1])


def head_results(delta, coords0, ff0):
    """The fp64 formula of the track / feature update on an integral, balanced delta; asserted integral first."""
    assert torch.equal(delta, delta.round()) and delta.abs().max().item() <= 256
    d = delta[:, 3:]
    mean = d.mean(1, keepdim=True)
    c = (d - mean).abs()
    assert c[0, 0].item() >= 2 and bool((c == c[0, 0]).all())  # balanced m +- c: GroupNorm gives +-(1 - eps / (2 c^2)), +-1 in bf16
    dn = HEAD_GW * torch.sign(d - mean) + HEAD_GB  # GroupNorm(1, 128): +-1 in bf16, times {1, 2} plus an integer
    assert (F.group_norm(d, 1, HEAD_GW, HEAD_GB, 1e-5) - dn).abs().max().item() < 1e-5
    pre = dn @ HEAD_WU.t() + HEAD_BU
    assert bool((pre % 16 == 0).all()) and torch.equal(F.gelu(pre), F.relu(pre))  # erf-GELU is relu on multiples of 16
    ff = ff0 + F.relu(pre)
    assert ff.abs().max().item() < 2 ** 24
    return coords0 + delta[:, :3], ff


@pytest.mark.parametrize("rows", HEAD_ROWS[:-1])
def test_head_case_is_integral(rows):
    c = head_case(rows)
    assert torch.equal(c["ffeats"], c["ffeats"].round()) and bool((c["delta"][::7, 1] == -32).all())
    assert bool((c["ffeats"] != c["ff0"]).any())


def frag_bf16(hip, w, kpad):
    n, k = w.shape
    wp = torch.zeros(n, (max(k, kpad) + 63) // 64 * 64, device=DEV)
    wp[:, :k] = w.float().to(DEV)
    hi = wp.to(torch.bfloat16).view(torch.int16)
    fr = torch.empty((n + 31) // 32 * 32 * kpad, device=DEV, dtype=torch.int16)
    hip.pack_frag_bf16(hi, hi.shape[1], n, kpad, fr)
    return fr


@gpu
@pytest.mark.parametrize("rows", HEAD_ROWS)
def test_update_head_exact(hip, rows):
    """mvt_update_head_bf16 on integer inputs: coords, ffeats and the optional delta copy equal the fp64 formula bit for bit; the
    NaN flag answers to every coordinate column and to the last row, not to a feature column; delta=None is accepted."""
    c = head_case(rows)
    Gd = lambda t: t.float().contiguous().to(DEV)
    wts = (frag_bf16(hip, c["W0"], 256), Gd(c["b0"]), frag_bf16(hip, c["W2"], 144), Gd(c["b2"]), frag_bf16(hip, c["W4"], 144), Gd(c["b4"]),
           Gd(HEAD_GW), Gd(HEAD_GB), frag_bf16(hip, HEAD_WU, 128), Gd(HEAD_BU))
    tok = Gd(c["tok"])

    def run(coords, ff, with_delta=True):
        delta = torch.full((rows + 1, LDD), NAN, device=DEV) if with_delta else None
        flag = torch.zeros(1, device=DEV, dtype=torch.int32)
        hip.update_head_bf16(tok, HID, *wts, coords, ff, delta, LDD if with_delta else 0, rows, HID, OUT, flag)
        torch.cuda.synchronize()
        return delta, int(flag.item())

    for with_delta in (True, False):
        co, ff = Gd(c["coords0"]), Gd(c["ff0"])
        delta, flag = run(co, ff, with_delta)
        assert flag == 0
        assert torch.equal(co.cpu().double(), c["coords"]) and torch.equal(ff.cpu().double(), c["ffeats"])
        if with_delta:
            assert torch.equal(delta[:rows, :OUT].cpu().double(), c["delta"])
            assert bool(torch.isnan(delta[:, OUT:]).all()) and bool(torch.isnan(delta[rows]).all())
    for r, col in {(0, 0), (rows // 2, 1), (rows - 1, 2), (rows - 1, 0)}:
        co = Gd(c["coords0"])
        co[r, col] = NAN
        assert run(co, Gd(c["ff0"]), False)[1] == 1, (r, col)
    ff = Gd(c["ff0"])
    ff[rows - 1, 5] = NAN
    assert run(Gd(c["coords0"]), ff, False)[1] == 0


@gpu
@pytest.mark.parametrize("n,mask", [(5, 0), (37, 55), (342, 55), (449, 1), (512, 55), (513, 23), (672, 55), (673, 55), (740, 55), (740, 39)])
def test_update_head_through_composite(hip, n, mask):
    """One case per form of the table with the track / feature update inside the composite call: delta decodes, coords and ffeats
    equal the fp64 formula on the planted delta bit for bit."""
    case = make_case("v2p_vself_p2v@1", (n,), 12)
    run = Run(hip, case)
    g = torch.Generator().manual_seed(n)
    coords0 = torch.randint(-50, 51, (n * 12, 3), generator=g).double()
    ff0 = torch.randint(-9, 10, (n * 12, 128), generator=g).double()
    want_c, want_f = head_results(run.want, coords0, ff0)
    for entry in ("x", "tokens"):
        co, ff = coords0.float().to(DEV), ff0.float().to(DEV)
        flag = torch.zeros(1, device=DEV, dtype=torch.int32)
        d = run.check(mask, entry=entry, head=(co, ff, flag))
        assert torch.equal(d.cpu().double(), run.want)
        assert int(flag.item()) == 0
        assert torch.equal(co.cpu().double(), want_c) and torch.equal(ff.cpu().double(), want_f)
