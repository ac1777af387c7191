"""Packed weights of MVTracker: the state-dict tree, the per-precision matrix layouts and the composite entries' host structs.

``_pack`` turns the state dict into ``pk``: a dict of ``Packed`` records by layer name (convolutions, linears and norms alike)
plus a few named entries -- "updater_struct" / "encoder_struct" / "encoder_struct_shared" (host structs of device pointers for
the composite library calls, present only where those cover the configuration), "virtual", "time_embed", "pos_omega".

``WeightsMixin`` reads these model attributes: precision, fuse_attention, fuse_input, composite_encoder, bf16_tokens,
bf16_activations, fuse_blocks, mfma_attention, fuse_norm, depth, hidden, num_heads, dim_head, nv, S, latent_dim,
updateformer_input_dim, out_dim, _time_embed_host; it owns _packed, _packed_sig, _plist, _plist_epoch.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import nn

from . import hip

_param_epoch = [0]  # bumped whenever a Parameter OBJECT is (re)registered anywhere in a tracker's module tree


class _Node(nn.Module):
    """Anonymous container used to reproduce the reference's dotted state_dict keys."""

    def register_parameter(self, name, param):
        # (assigning a new nn.Parameter, load_state_dict(assign=True), ... all end here: the cached parameter list of
        #  MVTracker._signature must be rebuilt, or a stale packed weight set would be used silently)
        _param_epoch[0] += 1
        super().register_parameter(name, param)


def _insert(root: nn.Module, dotted: str, tensor: torch.Tensor) -> None:
    *path, leaf = dotted.split(".")
    m = root
    for p in path:
        if p not in m._modules:
            m.add_module(p, _Node())
        m = m._modules[p]
    m.register_parameter(leaf, nn.Parameter(tensor, requires_grad=False))


def _round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


class Packed(NamedTuple):
    """One layer of ``pk``.  ``w``: the [N][round_up(K, 64)] zero-padded matrix -- fp32 in fp32 mode, otherwise the bf16 hi part as
    int16 -- or a norm's / the visibility head's weight vector; ``lo``: the bf16x3 lo part; ``b``: bias; ``n``, ``k``: a linear's
    logical shape; ``frag``: its fragment-major bf16 copy for the block kernels.  Unused fields are None."""
    w: torch.Tensor
    lo: Optional[torch.Tensor] = None
    b: Optional[torch.Tensor] = None
    n: Optional[int] = None
    k: Optional[int] = None
    frag: Optional[torch.Tensor] = None

    @property
    def bf16(self) -> bool:
        return self.w.dtype == torch.int16  # a bf16 layout (bf16 or bf16x3 mode): the bf16 MFMA kernels take the matrix


class WeightsMixin:
    def _signature(self, dev):
        assert self.precision in ("fp32", "bf16x3", "bf16"), self.precision
        # (everything _pack reads: the switches that decide which structs / layouts are built, then the parameter versions)
        flags = (str(dev), self.precision, self.fuse_attention, self.fuse_input, self.composite_encoder, self._composite_updater_ok(),
                 self._composite_encoder_ok(), self.bf16_tokens, self.bf16_activations, self.fuse_blocks, self.mfma_attention, self.fuse_norm,
                 self.depth, self.hidden)
        # (the Parameter objects are fixed at construction -- load_state_dict / .to() change their data in place -- so the module
        #  tree is walked once: nn.Module.parameters() costs ~0.8 ms per walk, and this runs several times per call)
        #  again only after a Parameter object has been registered somewhere: _Node.register_parameter / MVTracker.register_parameter)
        if self._plist is None or self._plist_epoch != _param_epoch[0]:
            self._plist = list(self.parameters())
            self._plist_epoch = _param_epoch[0]
        return flags + tuple(p._version for p in self._plist) + tuple(p.data_ptr() for p in self._plist)

    def _pack(self, dev) -> dict:
        sig = self._signature(dev)
        if self._packed is not None and self._packed_sig == sig:
            return self._packed
        sd = {k: v.detach().to(device=dev, dtype=torch.float32) for k, v in self.state_dict().items()}
        pk: dict = {}

        prec = self.precision

        def matrix(w2d):
            """[N][K] fp32 -> zero-padded [N][round_up(K,64)] in the layout of the selected precision: (fp32 tensor, None), or
            (bf16 hi, bf16 lo | None) as int16 tensors."""
            n, k = w2d.shape
            wp = torch.zeros(n, _round_up(k, 64), device=dev)
            wp[:, :k] = w2d
            if prec == "fp32":
                return wp, None
            hi = torch.empty(wp.shape, device=dev, dtype=torch.int16)
            lo = torch.empty(wp.shape, device=dev, dtype=torch.int16) if prec == "bf16x3" else None
            hip.split_bf16(wp, hi, lo, wp.numel())
            return hi, lo

        def vec(name):
            return Packed(sd[name + ".weight"].contiguous(), b=sd[name + ".bias"].contiguous())

        def conv(name, w2d):
            hi, lo = matrix(w2d)
            pk[name] = Packed(hi, lo, sd[name + ".bias"].contiguous())

        def lin(name, w=None, b=None):
            w = sd[name + ".weight"] if w is None else w
            b = sd[name + ".bias"] if b is None else b
            n, k = w.shape
            hi, lo = matrix(w)
            fr = None
            if prec == "bf16" and name.startswith("updateformer.") and k % 16 == 0 and "flow_head" not in name:
                fr = torch.empty(_round_up(n, 32) * k, device=dev, dtype=torch.int16)  # fragment-major copy for the fused block kernel
                hip.pack_frag_bf16(hi, hi.shape[1], n, k, fr)
            pk[name] = Packed(hi, lo, b.contiguous(), n, k, fr)

        w = sd["fnet.conv1.weight"]  # (64,3,7,7) -> [64][7][32] with element kw*4+c
        st = torch.zeros(64, 7, 8, 4, device=dev)
        st[:, :, :7, :3] = w.permute(0, 2, 3, 1)
        conv("fnet.conv1", st.reshape(64, 7 * 32))
        for k in sd:
            if k.startswith("fnet.") and k.endswith(".weight") and k != "fnet.conv1.weight":
                conv(k[:-7], sd[k].permute(0, 2, 3, 1).reshape(sd[k].shape[0], -1))
        u = "updateformer."
        for name in ("input_transform", "flow_head.0", "flow_head.2", "flow_head.4"):
            lin(u + name)
        for i in range(self.depth):
            for blk in ("time_blocks", "space_virtual_blocks"):
                p = f"{u}{blk}.{i}"
                lin(p + ".attn.qkv", torch.cat([sd[p + ".attn.to_q.weight"], sd[p + ".attn.to_kv.weight"]], 0),
                    torch.cat([sd[p + ".attn.to_q.bias"], sd[p + ".attn.to_kv.bias"]], 0))
                lin(p + ".attn.to_out")
                lin(p + ".mlp.fc1")
                lin(p + ".mlp.fc2")
            for blk in ("space_point2virtual_blocks", "space_virtual2point_blocks"):
                p = f"{u}{blk}.{i}"
                pk[p + ".norm_context"] = vec(p + ".norm_context")
                for nme in (".cross_attn.to_q", ".cross_attn.to_kv", ".cross_attn.to_out", ".mlp.fc1", ".mlp.fc2"):
                    lin(p + nme)
        pk["virtual"] = sd[u + "virual_tracks"].reshape(self.nv, self.hidden).contiguous()
        if self._composite_updater_ok():
            pk["updater_struct"] = self._updater_struct(pk, sd, matrix)
        if self._composite_encoder_ok():
            pk["encoder_struct"], pk["encoder_struct_shared"] = self._encoder_structs(pk)
        pk["ffeats_norm"] = vec("ffeats_norm")
        lin("ffeats_updater.0")
        pk["vis"] = Packed(sd["vis_predictor.0.weight"].reshape(-1).contiguous(), b=sd["vis_predictor.0.bias"].contiguous())
        pk["time_embed"] = self._time_embed_host.to(dev)
        a3 = _round_up(self.updateformer_input_dim, 6) // 3  # embeddings.py:95-97 with embed_dim = dim_padded / 3
        om = np.arange(a3 // 2, dtype=np.float64)
        om /= a3 / 2.0
        pk["pos_omega"] = torch.from_numpy(1.0 / 10000 ** om).to(dev)
        self._packed, self._packed_sig = pk, sig
        return pk

    def _composite_updater_ok(self):
        """mvt_updateformer_forward covers the shipped geometry in bf16 mode with bf16 q/k/v tensors."""
        return (self.precision == "bf16" and self.hidden == 256 and self.num_heads == 6 and self.dim_head == 48 and self.nv == 64
                and self.latent_dim == 128 and self.fuse_blocks and self.mfma_attention and self.bf16_tokens
                and self.depth <= hip.UPDATER_MAX_DEPTH and hip.COMPOSITE and os.environ.get("MVT_COMPOSITE", "1") != "0")

    def _composite_encoder_ok(self):
        """mvt_encoder_forward covers bf16 mode with bf16 activations and the fused InstanceNorm path."""
        return (self.precision == "bf16" and self.bf16_activations and self.fuse_norm and self.latent_dim % 32 == 0 and hip.COMPOSITE
                and self.composite_encoder)

    def _encoder_structs(self, pk):
        """mvt_encoder_weights (host structs of device pointers into ``pk``, which keeps the tensors alive) for mvt_encoder_forward:
        one for calls that own the GPU, one with the same weights for calls that share it with the refinement windows
        (MVT_IO_SHORT_WG)."""
        ew, ews = hip.EncoderWeights(), hip.EncoderWeights()
        ew.latent_dim = self.latent_dim
        ews.latent_dim, ews.short_workgroups = self.latent_dim, 1
        names = ["fnet.conv1"]
        for li in range(1, 5):
            names += [f"fnet.layer{li}.0.conv1", f"fnet.layer{li}.0.conv2", f"fnet.layer{li}.0.downsample.0" if li > 1 else f"fnet.layer{li}.0.conv1",
                      f"fnet.layer{li}.1.conv1", f"fnet.layer{li}.1.conv2"]
        names += ["fnet.conv2", "fnet.conv3"]
        for i, nm in enumerate(names):  # (layer 1 has no downsample conv: slot 3 repeats a valid pointer and is never used)
            ew.conv[i].w, ew.conv[i].b = pk[nm].w.data_ptr(), pk[nm].b.data_ptr()
            ews.conv[i].w, ews.conv[i].b = ew.conv[i].w, ew.conv[i].b
        return ew, ews

    def _updater_struct(self, pk, sd, matrix):
        """mvt_updater_weights (host struct of device pointers into ``pk``) for mvt_updateformer_forward."""
        u = "updateformer."
        h = self.hidden
        w = hip.UpdaterWeights()
        w.depth, w.hidden, w.heads, w.dim_head, w.n_virtual, w.S = self.depth, h, self.num_heads, self.dim_head, self.nv, self.S
        w.token_dim, w.out_dim = self.updateformer_input_dim, self.out_dim
        w.fuse_attention = self.fuse_attention
        w.virtual_tokens = pk["virtual"].data_ptr()
        keep = w.tensors = []  # tensors referenced by the struct only: they live as long as it does

        def rows(name, pad_n=False):
            wt, b = sd[name + ".weight"], sd[name + ".bias"]
            n, k = wt.shape
            if pad_n and n % 4:  # zero rows + zero bias: the GEMM itself writes the pad columns of the hidden activations as zeros
                n4 = _round_up(n, 4)
                wt = torch.cat([wt, torch.zeros(n4 - n, k, device=wt.device)], 0)
                b = torch.cat([b, torch.zeros(n4 - n, device=b.device)], 0)
            hi = matrix(wt)[0]
            b = b.contiguous()
            keep.extend([hi, b])
            return hip.lin_rows(hi, b, wt.shape[0], k)

        w.input_transform = rows(u + "input_transform")
        w.flow0, w.flow2, w.flow4 = rows(u + "flow_head.0", True), rows(u + "flow_head.2", True), rows(u + "flow_head.4")

        def frag_of(name, kpad):  # fragment-major bf16 of a [N][K] linear, K zero-padded to kpad (a multiple of 16)
            wt, b = sd[name + ".weight"], sd[name + ".bias"].contiguous()
            n, k = wt.shape
            if kpad > _round_up(k, 64):  # (the row-major image must be at least kpad wide: token widths well below 592)
                wt = torch.cat([wt, torch.zeros(n, kpad - k, device=wt.device)], 1)
            hi = matrix(wt)[0]  # [n][round_up(k, 64)], zero padded
            fr = torch.empty(_round_up(n, 32) * kpad, device=wt.device, dtype=torch.int16)
            hip.pack_frag_bf16(hi, hi.shape[1], n, kpad, fr)
            keep.extend([fr, b])
            return hip.lin_frag(fr, b, n, kpad)

        w.flow0_frag, w.flow2_frag, w.flow4_frag = frag_of(u + "flow_head.0", h), frag_of(u + "flow_head.2", 144), frag_of(u + "flow_head.4", 144)
        w.ffeats_updater = frag_of("ffeats_updater.0", self.latent_dim)
        if self.fuse_input and self.updateformer_input_dim <= 592:
            w.input_frag = frag_of(u + "input_transform", 592)
        gw, gb = sd["ffeats_norm.weight"].contiguous(), sd["ffeats_norm.bias"].contiguous()
        keep.extend([gw, gb])
        w.ffeats_norm_w, w.ffeats_norm_b = gw.data_ptr(), gb.data_ptr()

        def frag(name):
            r = pk[name]
            return hip.lin_frag(r.frag, r.b, r.n, r.k)

        for i in range(self.depth):
            for arr, blk, attn, cross in ((w.time_blk, "time_blocks", "attn", False), (w.vself, "space_virtual_blocks", "attn", False),
                                          (w.v2p, "space_virtual2point_blocks", "cross_attn", True),
                                          (w.p2v, "space_point2virtual_blocks", "cross_attn", True)):
                p = f"{u}{blk}.{i}"
                b = arr[i]
                if cross:
                    b.q, b.kv = frag(f"{p}.{attn}.to_q"), frag(f"{p}.{attn}.to_kv")
                    b.ctx_ln_w, b.ctx_ln_b = pk[p + ".norm_context"].w.data_ptr(), pk[p + ".norm_context"].b.data_ptr()
                else:
                    b.qkv = frag(f"{p}.{attn}.qkv")
                b.out, b.fc1, b.fc2 = frag(f"{p}.{attn}.to_out"), frag(p + ".mlp.fc1"), frag(p + ".mlp.fc2")
        return w
