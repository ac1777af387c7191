"""The update transformer of MVTracker (reference cotracker2/blocks.py:455-494) sequenced three ways: the composite library call
(bf16 mode, shipped geometry), the fused block kernels (bf16 mode, hidden 256) and one launch per operator (every mode).

``UpdaterMixin`` reads these model attributes: precision, fuse_mlp, fuse_blocks, fuse_head, mfma_attention, bf16_tokens, S,
hidden, num_heads, dim_head, nv, depth, out_dim, updateformer_input_dim; and calls _pack (weights), _workspace and
_scratch_buffer (frame store).  Every internal call of the updater goes through ``self._update_former``, so a replacement set
on the instance (the benchmark's timing wrapper) is honoured.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip
from .weights import _round_up


class UpdaterMixin:
    def _lin(self, pk, name, A, lda, M, out, ldc, act=hip.ACT_NONE, R=None, ldr=0):
        r = pk[name]
        if r.bf16:
            hip.gemm_bf16(A, lda, r.w, r.lo, r.w.shape[1], r.b, R, ldr, out, ldc, M, r.n, r.k, act)
        else:
            hip.gemm(A, lda, r.w, r.w.shape[1], r.b, R, ldr, out, ldc, M, r.n, r.k, act)

    def _ln_lin(self, pk, name, x, rows, out, ldc, scratch, ln_w=None, ln_b=None, eps=1e-6, act=hip.ACT_NONE):
        """out = act(LayerNorm(x) @ W^T + b).  (mvt_ln_gemm_bf16, LayerNorm inside the GEMM's A loader, measured slower than
        the separate 7 us LayerNorm pass + GEMM -- every column tile recomputes the row statistics -- and is not used here.)"""
        h = self.hidden
        hip.layernorm(x, h, ln_w, ln_b, scratch, h, rows, h, eps)
        self._lin(pk, name, scratch, h, rows, out, ldc, act)

    def _mlp_residual(self, pk, p, tok, rows, xn, hbuf):
        h = self.hidden
        w1, w2 = pk[p + ".mlp.fc1"], pk[p + ".mlp.fc2"]
        if self.precision == "bf16" and h == 256 and self.fuse_mlp and rows >= 4096:  # LN + fc1 + GELU + fc2 + residual in one kernel
            hip.mlp_fused_bf16(tok, h, w1.w, w1.w.shape[1], w1.b, w2.w, w2.w.shape[1], w2.b, rows, h, 4 * h, 1e-6)
            return
        self._ln_lin(pk, p + ".mlp.fc1", tok, rows, hbuf, 4 * h, xn, act=hip.ACT_GELU_TANH)
        self._lin(pk, p + ".mlp.fc2", hbuf, 4 * h, rows, tok, h, R=tok, ldr=h)

    def _space_attention(self, q, ldq, k, v, ldkv, o, ldo, nq, nk, seg, pattern, bf16=False, ws=None):
        """One per-frame space attention (query / key row of item j in frame t: j*S + t).  ``seg`` None: one query set (nq, nk).
        ``seg`` = track counts n_g of G independent query sets: point rows of set g are its tracks [off_g, off_g + n_g), virtual
        rows (g*nv + j)*S + t; ``pattern`` names the form -- "v2p" (virtual <- point), "vs" (virtual self), "p2v" (point <- virtual)
        -- and every set attends within itself only."""
        S, H, dh, nv = self.S, self.num_heads, self.dim_head, self.nv
        if seg is None:
            if bf16:
                hip.attention_bf16(q, ldq, 1, S, k, v, ldkv, 1, S, o, ldo, S, nq, nk, H, dh, **({"ws": ws} if ws is not None else {}))
            else:
                hip.attention(q, ldq, 1, S, k, v, ldkv, 1, S, o, ldo, S, nq, nk, H, dh)
            return
        pts = [(int(o_) * S, int(n_)) for o_, n_ in zip(np.cumsum([0] + list(seg[:-1])), seg)]
        virt = [(g * nv * S, nv) for g in range(len(seg))]
        qs, ks = {"v2p": (virt, pts), "vs": (virt, virt), "p2v": (pts, virt)}[pattern]
        q0, nqs = zip(*qs)
        k0, nks = zip(*ks)
        if bf16:
            hip.attention_bf16_segmented(q, ldq, 1, S, k, v, ldkv, 1, S, o, ldo, S, H, dh, q0, nqs, k0, nks, ws=ws)
        else:
            hip.attention_segmented(q, ldq, 1, S, k, v, ldkv, 1, S, o, ldo, S, H, dh, q0, nqs, k0, nks)

    def _composite_call(self, plain, grouped, n, seg, pk, head, delta, ldd, upd):
        """One composite updater call with its workspace: entry ``plain`` on n tracks, or entry ``grouped`` on the query sets
        ``seg``.  The entries are given by NAME and looked up in ``hip`` now: the benchmark and the tests replace attributes of that
        module.  ``head``: the arguments between the weights and the track count; ``upd``: (coords, ffeats, nan_flag)."""
        dev = head[0].device
        if seg is None:
            ws = self._workspace(hip.updateformer_workspace_bytes(n, self.S), dev)
            return getattr(hip, plain)(pk["updater_struct"], *head, n, delta, ldd, ws, *upd)
        ws = self._workspace(hip.updateformer_grouped_workspace_bytes(n, self.S, len(seg)), dev)
        return getattr(hip, grouped)(pk["updater_struct"], *head, seg, delta, ldd, ws, *upd)

    def _input_tokens(self, pk, x, ldx, n, seg, tok):
        """Prologue of the sequenced paths: tok = [input_transform(x) for the n * S point rows | the virtual tokens broadcast over
        S, once per query set]."""
        S, h, Mp = self.S, self.hidden, n * self.S
        self._lin(pk, "updateformer.input_transform", x, ldx, Mp, tok, h)
        if seg is None:
            hip.broadcast_rows(pk["virtual"], tok[Mp:], h, self.nv, S, h)
        else:
            hip.broadcast_rows_repeat(pk["virtual"], tok[Mp:], h, self.nv, S, h, len(seg))

    def _flow_head(self, pk, pt, Mp, delta, ldd):
        """Epilogue of the sequenced paths: delta = flow_head(point tokens), three GEMMs through the cached zero-padded scratch."""
        u, ldh = "updateformer.", _round_up(self.out_dim, 4)
        h1, h2 = self._scratch_buffer("flow", pt.device, (Mp, ldh))
        self._lin(pk, u + "flow_head.0", pt, self.hidden, Mp, h1, ldh, hip.ACT_RELU)
        self._lin(pk, u + "flow_head.2", h1, ldh, Mp, h2, ldh, hip.ACT_RELU)
        self._lin(pk, u + "flow_head.4", h2, ldh, Mp, delta, ldd)

    def _update_former(self, pk, x, ldx, n, delta, ldd, coords=None, ffeats=None, nan_flag=None, seg=None):
        """delta = updater(x).  With ``coords`` / ``ffeats`` (composite path only) the track / feature update of mvtracker.py:392-399
        is applied inside the same library call and True is returned.  ``seg``: the track counts of independent query sets laid
        out back to back in x (``forward_grouped``), each with its own 64 virtual tracks."""
        if "updater_struct" in pk:  # the whole transformer as ONE library call (mvt_updateformer_forward[_grouped])
            fused = coords is not None and self.fuse_head
            upd = (coords if fused else None, ffeats if fused else None, nan_flag if fused else None)
            self._composite_call("updateformer_forward", "updateformer_forward_grouped", n, seg, pk, (x, ldx), delta, ldd, upd)
            return fused
        if self.precision == "bf16" and self.hidden == 256 and self.num_heads * self.dim_head == 288 and self.fuse_blocks:
            return self._update_former_fused(pk, x, ldx, n, delta, ldd, seg=seg)
        S, h, H, dh = self.S, self.hidden, self.num_heads, self.dim_head
        nv = self.nv * (1 if seg is None else len(seg))  # virtual tracks of all query sets
        inner = H * dh
        dev = x.device
        Mp, Mv = n * S, nv * S
        M = Mp + Mv
        tok = torch.empty(M, h, device=dev)
        xn = torch.empty(M, h, device=dev)
        qkv = torch.empty(M, 3 * inner, device=dev)
        att = torch.empty(M, inner, device=dev)
        hbuf = torch.empty(M, 4 * h, device=dev)
        u = "updateformer."
        self._input_tokens(pk, x, ldx, n, seg, tok)
        pt, vt = tok[:Mp], tok[Mp:]
        for i in range(self.depth):
            # time attention over the S frames of every (point or virtual) track
            p = f"{u}time_blocks.{i}"
            self._ln_lin(pk, p + ".attn.qkv", tok, M, qkv, 3 * inner, xn)
            hip.attention(qkv, 3 * inner, S, 1, qkv[:, inner:], qkv[:, 2 * inner:], 3 * inner, S, 1, att, inner, n + nv, S, S, H, dh)
            self._lin(pk, p + ".attn.to_out", att, inner, M, tok, h, R=tok, ldr=h)
            self._mlp_residual(pk, p, tok, M, xn, hbuf)
            # virtual <- point cross attention, per frame (row of item j in frame t is j*S + t)
            p = f"{u}space_virtual2point_blocks.{i}"
            ctx = pk[p + ".norm_context"]
            self._ln_lin(pk, p + ".cross_attn.to_q", vt, Mv, qkv[Mp:], 3 * inner, xn[Mp:])
            self._ln_lin(pk, p + ".cross_attn.to_kv", pt, Mp, qkv[:Mp, inner:], 3 * inner, xn[:Mp], ctx.w, ctx.b, eps=1e-5)
            self._space_attention(qkv[Mp:], 3 * inner, qkv[:Mp, inner:], qkv[:Mp, 2 * inner:], 3 * inner, att[Mp:], inner, nv, n, seg, "v2p")
            self._lin(pk, p + ".cross_attn.to_out", att[Mp:], inner, Mv, vt, h, R=vt, ldr=h)
            self._mlp_residual(pk, p, vt, Mv, xn[Mp:], hbuf[Mp:])
            # virtual self attention, per frame
            p = f"{u}space_virtual_blocks.{i}"
            self._ln_lin(pk, p + ".attn.qkv", vt, Mv, qkv[Mp:], 3 * inner, xn[Mp:])
            self._space_attention(qkv[Mp:], 3 * inner, qkv[Mp:, inner:], qkv[Mp:, 2 * inner:], 3 * inner, att[Mp:], inner, nv, nv, seg, "vs")
            self._lin(pk, p + ".attn.to_out", att[Mp:], inner, Mv, vt, h, R=vt, ldr=h)
            self._mlp_residual(pk, p, vt, Mv, xn[Mp:], hbuf[Mp:])
            # point <- virtual cross attention, per frame
            p = f"{u}space_point2virtual_blocks.{i}"
            ctx = pk[p + ".norm_context"]
            self._ln_lin(pk, p + ".cross_attn.to_q", pt, Mp, qkv[:Mp], 3 * inner, xn[:Mp])
            self._ln_lin(pk, p + ".cross_attn.to_kv", vt, Mv, qkv[Mp:, inner:], 3 * inner, xn[Mp:], ctx.w, ctx.b, eps=1e-5)
            self._space_attention(qkv[:Mp], 3 * inner, qkv[Mp:, inner:], qkv[Mp:, 2 * inner:], 3 * inner, att[:Mp], inner, n, nv, seg, "p2v")
            self._lin(pk, p + ".cross_attn.to_out", att[:Mp], inner, Mp, pt, h, R=pt, ldr=h)
            self._mlp_residual(pk, p, pt, Mp, xn[:Mp], hbuf[:Mp])
        self._flow_head(pk, pt, Mp, delta, ldd)

    # ---- fused path (precision "bf16", hidden 256): per layer 4 attention launches + 5 fused block launches
    def _fused_block(self, pk, p, attn_key, x, rows, att, nexts, ws=None):
        """x += att @ Wo^T + bo; x += MLP(LN(x)); then the follow-up projections of LN(x) listed in ``nexts``."""
        h = self.hidden
        wo, w1, w2 = pk[f"{p}.{attn_key}.to_out"], pk[p + ".mlp.fc1"], pk[p + ".mlp.fc2"]
        inner = self.num_heads * self.dim_head
        hip.block_fused_bf16(x, h, att, inner, inner, wo.frag, inner, wo.b, w1.frag, h, w1.b, w2.frag, 4 * h, w2.b, 4 * h, nexts, rows, h, ws=ws)

    def _next(self, pk, name, y, ldy, ln=None, eps=1e-6, rows=(0, 0)):
        r = pk[name]
        d = dict(w=r.frag, ldw=r.k, b=r.b, N=r.n, y=y, ldy=ldy, eps=eps, rows=rows)
        if ln is not None:
            d.update(lnw=ln.w, lnb=ln.b)
        return d

    def _update_former_fused(self, pk, x, ldx, n, delta, ldd, seg=None):
        S, h, H, dh = self.S, self.hidden, self.num_heads, self.dim_head
        G = 1 if seg is None else len(seg)
        nv = self.nv * G  # virtual tracks of all query sets
        inner = H * dh
        dev = x.device
        Mp, Mv = n * S, nv * S
        M = Mp + Mv
        space_mfma = self.mfma_attention and dh == 48
        tok = torch.empty(M, h, device=dev)
        xn = torch.empty(M, h, device=dev)
        # q|k|v of the time / virtual-self attention; cross attention: q in [:, :inner], k|v in [:, inner:].  Two buffers,
        # swapped every layer: the next layer's time q|k|v is projected (by the block epilogues) while this layer's
        # cross-attention k|v are still being read.
        # (bf16 tensors in bf16 mode: they only ever feed bf16 MFMA operands, and the block / attention kernels are bound
        #  by exactly this traffic)
        tdt = torch.bfloat16 if (self.bf16_tokens and space_mfma) else torch.float32
        qkv = torch.empty(M, 3 * inner, device=dev, dtype=tdt)
        qkv_nx = torch.empty(M, 3 * inner, device=dev, dtype=tdt)
        qp = torch.empty(Mp, inner, device=dev, dtype=tdt)       # point <- virtual queries (computed right after the time block)
        att = torch.empty(M, inner, device=dev, dtype=tdt)
        ws = torch.empty(5 * Mv * h, device=dev) if 4 * h == 1024 else None  # split path of the virtual-track blocks
        # key-split virtual <- point attention (one region per query set)
        aws = torch.empty(G * hip.attention_ws_floats(S, self.nv, H), device=dev) if space_mfma else None
        u = "updateformer."
        time_attn = hip.attention_bf16 if space_mfma else hip.attention  # 12 keys pad to one 32-key MFMA block: still 1.4x the VALU kernel
        self._input_tokens(pk, x, ldx, n, seg, tok)
        pt, vt = tok[:Mp], tok[Mp:]
        if h == 256:  # LayerNorm + projection in one launch (the split path's second pass without a workspace)
            hip.ln_proj_bf16(tok, h, [self._next(pk, f"{u}time_blocks.0.attn.qkv", qkv, 3 * inner)], M, h)
        else:
            self._ln_lin(pk, f"{u}time_blocks.0.attn.qkv", tok, M, qkv, 3 * inner, xn)
        for i in range(self.depth):
            tb, v2p = f"{u}time_blocks.{i}", f"{u}space_virtual2point_blocks.{i}"
            vs, p2v = f"{u}space_virtual_blocks.{i}", f"{u}space_point2virtual_blocks.{i}"
            last = i + 1 == self.depth
            nxt_qkv = f"{u}time_blocks.{i + 1}.attn.qkv"
            # time attention, then the rest of the time block; its epilogue already projects what the space blocks need
            time_attn(qkv, 3 * inner, S, 1, qkv[:, inner:], qkv[:, 2 * inner:], 3 * inner, S, 1, att, inner, n + nv, S, S, H, dh)
            # (one launch over point and virtual rows: same weights, the follow-up projections differ by row range)
            self._fused_block(pk, tb, "attn", tok, M, att,
                              [self._next(pk, v2p + ".cross_attn.to_kv", qkv[:, inner:], 3 * inner, pk[v2p + ".norm_context"], 1e-5,
                                          rows=(0, Mp)),
                               self._next(pk, p2v + ".cross_attn.to_q", qp, inner, rows=(0, Mp)),
                               self._next(pk, v2p + ".cross_attn.to_q", qkv, 3 * inner, rows=(Mp, M))])
            # virtual <- point
            self._space_attention(qkv[Mp:], 3 * inner, qkv[:Mp, inner:], qkv[:Mp, 2 * inner:], 3 * inner, att[Mp:], inner, nv, n, seg,
                                  "v2p", bf16=space_mfma, ws=aws)
            self._fused_block(pk, v2p, "cross_attn", vt, Mv, att[Mp:], [self._next(pk, vs + ".attn.qkv", qkv[Mp:], 3 * inner)], ws=ws)
            # virtual self attention
            self._space_attention(qkv[Mp:], 3 * inner, qkv[Mp:, inner:], qkv[Mp:, 2 * inner:], 3 * inner, att[Mp:], inner, nv, nv, seg, "vs",
                                  bf16=space_mfma)
            nx = [self._next(pk, p2v + ".cross_attn.to_kv", qkv[Mp:, inner:], 3 * inner, pk[p2v + ".norm_context"], 1e-5)]
            if not last:  # the virtual rows are final for this layer: project the next layer's time q|k|v right here
                nx.append(self._next(pk, nxt_qkv, qkv_nx[Mp:], 3 * inner))
            self._fused_block(pk, vs, "attn", vt, Mv, att[Mp:], nx, ws=ws)
            # point <- virtual
            self._space_attention(qp, inner, qkv[Mp:, inner:], qkv[Mp:, 2 * inner:], 3 * inner, att[:Mp], inner, n, nv, seg, "p2v",
                                  bf16=space_mfma)
            self._fused_block(pk, p2v, "cross_attn", pt, Mp, att[:Mp], [] if last else [self._next(pk, nxt_qkv, qkv_nx[:Mp], 3 * inner)])
            qkv, qkv_nx = qkv_nx, qkv
        self._flow_head(pk, pt, Mp, delta, ldd)

    def _update_former_padded(self, xs, seg=None):
        """The token sets xs[g] (1,N_g,S,D) back to back through ``_update_former`` in zero-padded staging tensors (row strides
        rounded up to 4 floats, as the window loop's) -> deltas (sum N_g, S, 3+C).  ``seg`` None: one set, the plain kernels."""
        D = self.updateformer_input_dim
        for x in xs:
            assert x.shape[2] == self.S and x.shape[3] == D and (seg is None or (x.shape[0] == 1 and x.shape[1] > 0))
        S, n = self.S, sum(int(x.shape[1]) for x in xs)
        dev = xs[0].device
        pk = self._pack(dev)
        ldx = _round_up(D, 4)
        xp = torch.zeros(n * S, ldx, device=dev)
        xp[:, :D] = torch.cat([x.reshape(-1, D) for x in xs], 0) if seg is not None else xs[0].reshape(n * S, D)
        ldd = _round_up(self.out_dim, 4)
        delta = torch.zeros(n * S, ldd, device=dev)
        self._update_former(pk, xp, ldx, n, delta, ldd, seg=seg)
        return delta[:, :self.out_dim].reshape(n, S, self.out_dim)

    @hip.guarded
    def update_former(self, x):
        """EfficientUpdateFormer.forward on tokens x (1,N,S,D) -> (1,N,S,3+C) (test / parity entry)."""
        return self._update_former_padded([x])[None]

    def update_former_grouped(self, xs):
        """``update_former`` on G independent token sets xs[g] (1,N_g,S,D) in one launch sequence (test / parity entry): the sets
        share every row-wise kernel and attend only within themselves.  Returns the list of (1,N_g,S,3+C) deltas."""
        with hip.device_guard(xs[0]):
            seg = [int(x.shape[1]) for x in xs]
            return [o[None] for o in torch.split(self._update_former_padded(xs, seg), seg, 0)]
