"""The feature encoder of MVTracker (reference spatracker/blocks.py:214-284): the CNN as one composite library call where that
covers the configuration, otherwise sequenced layer by layer here; chunked over images, alternating between two streams.

``EncoderMixin`` reads these model attributes: precision, fuse_norm, fold_downsample, bf16_activations, bf16_store,
stem_reads_clip, encoder_streams, latent_dim, stride, _shared_gpu; and calls _pack (weights), _workspace, _helper_stream,
_handover (frame store).  Every internal call of the encoder goes through ``self._encode``, so a replacement set on the instance
(the benchmark's timing wrapper) is honoured.
"""
from __future__ import annotations

import contextlib

import torch

from . import hip


class _Shifted:
    """View of a tensor whose row ``i`` is ``base[i - shift]`` (slice access only)."""

    def __init__(self, base, shift):
        self.base, self.shift = base, shift

    def __getitem__(self, sl):
        return self.base[sl.start - self.shift:sl.stop - self.shift]


class _ClipImages:
    """Images img0 .. (frame-major numbering t * V + v) of the planar clip rgbs (V,T,3,H,W), fp32 or uint8 in [0, 255], by reference."""

    def __init__(self, rgbs, V, T, img0):
        self.rgbs, self.V, self.T, self.img0 = rgbs, V, T, img0


class EncoderMixin:
    def _conv(self, pk, name, x, n, H, W, cin, cout, k, stride, pad, out=None, ldo=None, in_stats=None, stats=False):
        """Convolution; ``stats=True`` also returns the InstanceNorm (mean, rstd) of the output (taken from the conv epilogue
        on the bf16 kernels), ``in_stats`` makes the kernel read its input as relu(IN(x)) (bf16 3x3 stride-1 only)."""
        r = pk[name]
        Ho = (H + 2 * pad - k) // stride + 1
        Wo = (W + 2 * pad - k) // stride + 1
        if out is None:
            out = torch.empty(n, Ho, Wo, cout, device=x.device, dtype=self._act_dtype(pk))
            ldo = cout
        st = None
        if r.bf16:
            slots = hip.conv2d_stat_slots(H, W, cin, k, k, stride, pad, r.lo is not None) if (stats and self.fuse_norm) else 0
            part = torch.empty(n * slots * cout * 2, device=x.device) if slots else None
            hip.conv2d_bf16(x, r.w, r.lo, r.b, out, n, H, W, cin, cout, k, k, stride, pad, ldo, in_stats=in_stats, out_partial=part,
                            short_wg=self._shared_gpu)
            if slots:
                st = torch.empty(n, cout, 2, device=x.device)
                hip.instnorm_finish_slots(part, slots, st, n, Ho * Wo, cout)
        else:
            assert in_stats is None
            hip.conv2d(x, r.w, r.b, out, n, H, W, cin, cout, k, k, stride, pad, ldo)
        if stats and st is None:
            st = self._inorm(out, n, Ho * Wo, cout, apply=False)
        return (out, Ho, Wo, st) if stats else (out, Ho, Wo)

    def store_dtype(self):
        """Element type of the frame store's feature rows: bf16 in bf16 mode -- under autocast the reference's fmaps / pc_fvec are
        bf16 tensors (model_utils.py:467-476) -- which halves the store, the correlation kernel's gather traffic and the
        multi-GPU all-gather; fp32 in the fp32 / bf16x3 modes."""
        return torch.bfloat16 if (self.precision == "bf16" and self.bf16_store) else torch.float32

    def _act_dtype(self, pk):
        """Element type of the encoder's intermediate activations: bf16 in bf16 mode (HBM-bound layers, bf16 MFMA operands)."""
        return torch.bfloat16 if (self.bf16_activations and self.precision == "bf16") else torch.float32

    def _inorm(self, x, n, HW, C, skip=None, skip_stats=None, apply=True, st=None, skip_relu=False):
        if st is None:
            partial = torch.empty(n * hip.IN_SLABS * C * 2, device=x.device, dtype=torch.float64)
            st = torch.empty(n, C, 2, device=x.device)
            hip.instnorm_stats(x, C, partial, st, n, HW, C)
        if apply:
            hip.instnorm_apply(x, st, skip, skip_stats, x, n, HW, C, skip_relu=skip_relu)
        return st

    def _res_block(self, pk, p, x, n, H, W, cin, cout, stride, x_stats=None):
        """ResidualBlock (blocks.py:84-128).  ``x_stats``: x is a raw conv output whose InstanceNorm + ReLU was never
        materialised (the stem): conv1 normalises while it loads and the skip connection is normalised in the final pass."""
        fuse_in = self.fuse_norm and pk[p + ".conv2"].bf16 and cout % 32 == 0
        assert x_stats is None or (stride == 1 and (p + ".downsample.0") not in pk)
        d = dst = None
        fold = (fuse_in and stride == 2 and (p + ".downsample.0") in pk and x.dtype == torch.bfloat16 and pk[p + ".conv1"].lo is None
                and self.fold_downsample)
        if fold:
            # conv1 (3x3 / stride 2) and downsample[0] (1x1 / stride 2) read the same x: one launch (mvt_conv3x3s2_down_bf16)
            Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            y = torch.empty(n, Ho, Wo, cout, device=x.device, dtype=torch.bfloat16)
            d = torch.empty(n, Ho, Wo, cout, device=x.device, dtype=torch.bfloat16)
            slots = hip.conv2d_stat_slots(H, W, cin, 3, 3, 2, 1, False)
            part = torch.empty(2, n * slots * cout * 2, device=x.device)
            c1, cd = pk[p + ".conv1"], pk[p + ".downsample.0"]
            hip.conv3x3s2_down_bf16(x, c1.w, c1.b, cd.w, cd.b, y, d, n, H, W, cin, cout, cout, part[0], part[1])
            st1, dst = torch.empty(n, cout, 2, device=x.device), torch.empty(n, cout, 2, device=x.device)
            hip.instnorm_finish_slots(part[0], slots, st1, n, Ho * Wo, cout)
            hip.instnorm_finish_slots(part[1], slots, dst, n, Ho * Wo, cout)
        else:
            y, Ho, Wo, st1 = self._conv(pk, p + ".conv1", x, n, H, W, cin, cout, 3, stride, 1, stats=True, in_stats=x_stats)
        if not fuse_in:  # otherwise conv2 normalises while it loads its patch
            self._inorm(y, n, Ho * Wo, cout, st=st1)
        y2, _, _, st2 = self._conv(pk, p + ".conv2", y, n, Ho, Wo, cout, cout, 3, 1, 1, in_stats=st1 if fuse_in else None,
                                   stats=True)
        if (p + ".downsample.0") in pk:
            if d is None:
                d, _, _, dst = self._conv(pk, p + ".downsample.0", x, n, H, W, cin, cout, 1, stride, 0, stats=True)
            self._inorm(y2, n, Ho * Wo, cout, skip=d, skip_stats=dst, st=st2)
        else:
            self._inorm(y2, n, Ho * Wo, cout, skip=x, skip_stats=x_stats, skip_relu=x_stats is not None, st=st2)
        return y2, Ho, Wo

    def _encode(self, pk, x4, n, H, W, out_rows):
        """x4 (n,H,W,4) normalised RGB -- or a ``_ClipImages`` reference to n images of the planar clip, which the composite
        encoder's stem reads directly -- -> writes (n, H/4, W/4, C) into ``out_rows``."""
        C = self.latent_dim
        composite = "encoder_struct" in pk and out_rows.is_contiguous()
        est = "encoder_struct_shared" if self._shared_gpu else "encoder_struct"
        if isinstance(x4, _ClipImages):
            src = x4
            if composite and self.stem_reads_clip:  # mvt_encoder_forward_rgb: no (n,H,W,4) staging tensor, one launch less
                ws = self._workspace(hip.encoder_workspace_bytes(n, H, W, C), src.rgbs.device)
                return hip.encoder_forward_rgb(pk[est], src.rgbs, src.V, src.T, src.img0, n, H, W, out_rows, C, ws)
            x4 = torch.empty(n, H, W, 4, device=src.rgbs.device)
            hip.rgb_images_to_nhwc4(src.rgbs, x4, src.V, src.T, H, W, src.img0, n)
        if composite:  # the whole CNN as ONE library call (mvt_encoder_forward)
            ws = self._workspace(hip.encoder_workspace_bytes(n, H, W, C), x4.device)
            return hip.encoder_forward(pk[est], x4, n, H, W, out_rows, C, ws)
        hs, ws = H // self.stride, W // self.stride
        x, h, w, st = self._conv(pk, "fnet.conv1", x4, n, H, W, 4, 64, 7, 2, 3, stats=True)
        lazy_stem = self.fuse_norm and self.precision == "bf16"  # relu(IN(stem)) is applied by its two consumers instead
        if not lazy_stem:
            self._inorm(x, n, h * w, 64, st=st)
        cat = torch.empty(n, hs, ws, 416, device=x4.device, dtype=self._act_dtype(pk))
        cin = 64
        stages, dims = [], []
        for li, (cout, stride) in enumerate(((64, 1), (96, 2), (128, 2), (128, 2)), start=1):
            x, h, w = self._res_block(pk, f"fnet.layer{li}.0", x, n, h, w, cin, cout, stride, x_stats=st if (li == 1 and lazy_stem) else None)
            x, h, w = self._res_block(pk, f"fnet.layer{li}.1", x, n, h, w, cout, cout, 1)
            stages.append(x)
            dims.append((h, w, cout))
            cin = cout
        # the four resized stage outputs side by side (blocks.py:266-276), one launch writing whole 416-channel rows
        hip.concat_resize_bilinear_ac(stages, dims, cat, n, hs, ws, 416)
        y, _, _, st = self._conv(pk, "fnet.conv2", cat, n, hs, ws, 416, 2 * C, 3, 1, 1, stats=True)
        if self.fuse_norm and self.precision == "bf16" and (2 * C) % 32 == 0:
            # the 1x1 output conv normalises while it loads (row-tile kernel): no separate InstanceNorm pass
            self._conv(pk, "fnet.conv3", y, n, hs, ws, 2 * C, C, 1, 1, 0, out=out_rows, ldo=C, in_stats=st)
        else:
            self._inorm(y, n, hs * ws, 2 * C, st=st)
            self._conv(pk, "fnet.conv3", y, n, hs, ws, 2 * C, C, 1, 1, 0, out=out_rows, ldo=C)

    @hip.guarded
    def encode_images(self, rgbs, i0, i1, out, images_per_chunk=16, after_first_chunk=None):
        """Encode images [i0, i1) of rgbs (V,T,3,H,W) in [0,255] -- images numbered frame-major, t * V + v, the order of the
        frame store -- into ``out`` (>= i1 images, H/4, W/4, C): image i lands in out[i]."""
        V, T, _, H, W = rgbs.shape
        dev = rgbs.device
        pk = self._pack(dev)
        starts = list(range(i0, i1, images_per_chunk))
        # MVT_ENC_STREAMS=2: the chunks of one call alternate between the caller's stream and a helper stream, so that the small
        # layers of one chunk (layer 3 / 4 and the 1x1 convolutions fill a fraction of the chip) run beside the big layers of the other
        two = self.encoder_streams == 2 and dev.type == "cuda" and len(starts) > 1
        cur = torch.cuda.current_stream(dev) if two else None
        helper = self._helper_stream(dev) if two else None
        if two:
            helper.wait_stream(cur)  # hand-over H1: the helper stream reads the clip / writes store rows the caller's stream owns
            self._handover(dev)
        joins = []
        for ci, a in enumerate(starts):
            n = min(images_per_chunk, i1 - a)
            on_helper = two and ci % 2 == 1
            ctx = torch.cuda.stream(helper) if on_helper else contextlib.nullcontext()
            with ctx:
                # (images a .. a+n-1 of the clip by reference: the composite encoder's stem reads the planar frames itself)
                self._encode(pk, _ClipImages(rgbs, V, T, a), n, H, W, out[a:a + n])
                if on_helper:
                    ev = torch.cuda.Event()
                    ev.record(helper)
                    joins.append(ev)
            if after_first_chunk is not None:  # (host-side hook: the GPU has work queued now, see MVTracker.forward)
                after_first_chunk()
                after_first_chunk = None
        for ev in joins:
            cur.wait_event(ev)  # hand-over H2: the helper's chunks (store rows) back to the caller's stream
        if joins:
            self._handover(dev)
        if after_first_chunk is not None:
            after_first_chunk()

    def encode_frames(self, rgbs, t0=0, t1=None, images_per_chunk=16, out=None, out_t0=0, after_first_chunk=None):
        """rgbs (V,T,3,H,W) in [0,255] -> level-0 features (T,V,H/4,W/4,C); frames outside [t0,t1) are left zero
        (or untouched when the result goes into ``out``, whose first row is frame ``out_t0``)."""
        V, T, _, H, W = rgbs.shape
        t1 = T if t1 is None else t1
        hs, ws = H // self.stride, W // self.stride
        F0 = out if out is not None else torch.zeros(T, V, hs, ws, self.latent_dim, device=rgbs.device, dtype=self.store_dtype())
        flat = F0.view(-1, hs, ws, self.latent_dim)
        # (whole frames per chunk, as before: the chunk boundaries do not change any result, only the launch shapes)
        self.encode_images(rgbs, t0 * V, t1 * V, _Shifted(flat, out_t0 * V), images_per_chunk=max(1, images_per_chunk // V) * V,
                           after_first_chunk=after_first_chunk)
        return F0
