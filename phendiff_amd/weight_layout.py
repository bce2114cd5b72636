"""Kernel-layout weights of the layers the three trainable model families share (pixel UNet, SD UNet, VAE encoder), written once.

Every convolution or linear layer that trains exists in three forms: the forward packed weights (``pd_conv`` / ``pd_linear``'s
``w_packed``), the input-gradient ("dgrad") packed weights (transposed, taps flipped) and the ``pd_pack_weight`` jobs that
refresh both IN PLACE from the fp32 master parameters after an optimizer step.

* :class:`WeightSet` builds the first two: one entry (a ``SimpleNamespace`` whose attributes the launch plans read) per ResNet
  block, ``_Attention`` block, ``_Sampler`` and padded convolution -- the forward entry, or the dgrad entry of a set built with
  ``dgrad=True``.
* :class:`Repacker` builds the third for the same layers, from a forward entry and a dgrad entry, and runs them.

The family classes (``unet._PackedWeights`` / ``unet_train.TrainWeights`` / ``unet_train._Repacker`` and their SD and VAE
counterparts) walk ``named_modules()`` over these builders and add what is their own.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import torch

from . import _lib as L
from .packing import dgrad_weight, pack_conv_weight, upsample_phase_weights_stacked

# elements of one packed fragment pair: 32 output rows x 32 input channels of one tap ([2][64][8], packing.pack_conv_weight)
FRAGMENT = 2 * 64 * 8


def pad32(n: int) -> int:
    return ((n + 31) // 32) * 32


def tile_elems(cin_pad: int, ksize: int) -> int:
    """Elements of one 32-output-row tile of a packed ``ksize`` x ``ksize`` weight over ``cin_pad`` input channels."""
    return (cin_pad // 32) * ksize * ksize * FRAGMENT


def contiguous_after(a: torch.Tensor, b: torch.Tensor) -> bool:
    return b.data_ptr() == a.data_ptr() + a.numel() * a.element_size()


def require_adjacent(message: str, *groups):
    """Each group of parameters is read as ONE fused matrix / vector (q | k | v): its members must follow each other in memory."""
    for g in groups:
        if not all(contiguous_after(a.data, b.data) for a, b in zip(g[:-1], g[1:])):
            raise ValueError(message)


def require_alias(pairs):
    """fp32 vectors the kernels read directly (norm affines, plain biases) are the master parameters themselves."""
    for a, b in pairs:
        if a.data_ptr() != b.data_ptr():
            raise RuntimeError("kernel-side fp32 vectors must alias the master parameters (build the packed weights "
                               "after the parameters were moved into the flat training buffer)")


class WeightSet:
    """Base of the kernel-layout weight sets: forward layouts, or (``dgrad=True``) those of the input-gradient convolution,
    W'[ci][co][ky][kx] = W[co][ci][K-1-ky][K-1-kx]."""

    def __init__(self, device, tdt, dgrad: bool = False):
        self.device, self.tdt, self._dgrad = device, tdt, dgrad

    def f32(self, t):
        return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def pack(self, w, cout_pad=None):
        """Packed on the device the plans run on; a Linear weight [out][in] is a 1x1 convolution."""
        w = w.detach().to(device=self.device, dtype=torch.float32)
        w = w if w.ndim == 4 else w[:, :, None, None]
        return pack_conv_weight(dgrad_weight(w) if self._dgrad else w, self.tdt, cout_pad)

    def padded(self, conv, cout_pad, cin_pad):
        """A convolution zero-padded to (``cout_pad``, ``cin_pad``) channels.  A dgrad set returns the packed weight alone, a
        forward set (packed weight, bias).  With ``cout_pad == cout`` the bias is the parameter itself, which follows the master
        buffer like every other plain bias; otherwise it is a padded copy, which the family's re-packer refreshes."""
        co, ci, k, _ = conv.weight.shape
        w = torch.zeros((cout_pad, cin_pad, k, k), dtype=torch.float32, device=self.device)
        w[:co, :ci] = self.f32(conv.weight)
        if self._dgrad:
            return self.pack(w)
        b = self.f32(conv.bias)
        if cout_pad != co:
            b = torch.zeros(cout_pad, dtype=torch.float32, device=self.device)
            b[:co] = self.f32(conv.bias)
        return self.pack(w), b

    def im2col_conv_in(self, conv):
        """A 3x3 convolution over <= 3 NCHW planes as a 1x1 convolution over 32 virtual channels k = ci*9 + ky*3 + kx
        (``pd_conv`` im2col3 mode)."""
        co, ci = conv.weight.shape[:2]
        if ci > 3:
            raise NotImplementedError("the im2col conv_in of the HIP path takes <= 3 input channels (pixel-space models)")
        wv = torch.zeros((co, 32, 1, 1), dtype=torch.float32, device=self.device)
        wv[:, :ci * 9, 0, 0] = self.f32(conv.weight).reshape(-1, ci * 9)
        return self.pack(wv)

    def resnet(self, r):
        if self._dgrad:
            e = SimpleNamespace(w1d=self.pack(r.conv1.weight), w2d=self.pack(r.conv2.weight))
            if r.conv_shortcut is not None:
                e.wsd = self.pack(r.conv_shortcut.weight)
            return e
        f32 = self.f32
        e = SimpleNamespace(cin=r.in_channels, cout=r.out_channels, eps=r.norm1.eps, fused_shortcut=r.conv_shortcut is not None)
        e.g1, e.be1, e.g2, e.be2 = f32(r.norm1.weight), f32(r.norm1.bias), f32(r.norm2.weight), f32(r.norm2.bias)
        e.w1, e.b1, e.w2, e.b2 = self.pack(r.conv1.weight), f32(r.conv1.bias), self.pack(r.conv2.weight), f32(r.conv2.bias)
        if e.fused_shortcut:
            # conv_shortcut is folded into conv2 (pd_conv tail): per 32-row tile the tail's fragments follow conv2's
            ws = self.pack(r.conv_shortcut.weight)
            ct = e.w2.shape[0]
            e.w2 = torch.cat([e.w2.reshape(ct, -1, 64, 8), ws.reshape(ct, -1, 64, 8)], 1).contiguous()
            e.b2 = e.b2 + f32(r.conv_shortcut.bias)
        return e

    def attention(self, a):
        wqkv = torch.cat([a.to_q.weight, a.to_k.weight, a.to_v.weight], 0)
        if self._dgrad:
            return SimpleNamespace(wqkvd=self.pack(wqkv), wod=self.pack(a.to_out[0].weight))
        f32 = self.f32
        e = SimpleNamespace(heads=a.heads, g=f32(a.group_norm.weight), be=f32(a.group_norm.bias), eps=a.group_norm.eps)
        e.wqkv, e.bqkv = self.pack(wqkv), f32(torch.cat([a.to_q.bias, a.to_k.bias, a.to_v.bias], 0))
        e.wo, e.bo = self.pack(a.to_out[0].weight), f32(a.to_out[0].bias)
        return e

    def sampler(self, s, phases: bool = False, keep_src: bool = True):
        """``phases``: an Upsample2D also gets the four 2x2 sub-pixel phase kernels (``pd_conv`` phase 1..4, 4 / 9 of the FLOPs
        of the 3x3 convolution over the nearest-upsampled tensor; a dgrad set: ``phase_in``), a TUPLE of packed tensors;
        ``keep_src``: the forward entry keeps the four fp32 kernels stacked (``w4_src``), which the re-pack refreshes and reads.
        The VAE passes False: its upsamplers are the decoder's, which never trains, and ``Repacker.sampler`` re-packs the
        phases of every entry that has a ``w4_src``."""
        e = SimpleNamespace(wd=self.pack(s.conv.weight)) if self._dgrad else \
            SimpleNamespace(w=self.pack(s.conv.weight), b=self.f32(s.conv.bias), padding=s.padding)
        if phases:
            k4 = upsample_phase_weights_stacked(s.conv.weight.detach().to(device=self.device, dtype=torch.float32))
            if keep_src and not self._dgrad:
                e.w4_src = k4
            setattr(e, "wd4" if self._dgrad else "w4", tuple(self.pack(k4[p]) for p in range(4)))
        return e

    def time_mlp_and_conv_out(self, m):
        """Forward sets of the UNets: the time MLP transposed, ``conv_norm_out`` and the padded ``conv_out``."""
        f32, te = self.f32, m.time_embedding
        self.w1T, self.b1 = f32(te.linear_1.weight.t()), f32(te.linear_1.bias)
        self.w2T, self.b2 = f32(te.linear_2.weight.t()), f32(te.linear_2.bias)
        self.gn_out = (f32(m.conv_norm_out.weight), f32(m.conv_norm_out.bias), m.conv_norm_out.eps)
        self.conv_out_pad = pad32(m.conv_out.weight.shape[0])
        self.conv_out_w, self.conv_out_b = self.padded(m.conv_out, self.conv_out_pad, m.conv_out.weight.shape[1])

    def stack_time_emb_proj(self, resnets):
        """Every ResNet block's ``time_emb_proj`` as ONE [tdim][proj_dim] matrix (``pd_temb``); sets each entry's ``temb_off``."""
        off = 0
        for r, e in resnets:
            e.temb_off = off
            off += r.time_emb_proj.weight.shape[0]
        self.proj_dim = off
        self.wpT = self.f32(torch.cat([r.time_emb_proj.weight.detach() for r, _ in resnets], 0).t())
        self.bp = self.f32(torch.cat([r.time_emb_proj.bias.detach() for r, _ in resnets], 0))


def fuse_pack_jobs(jobs):
    """A weight is re-packed twice after every optimizer step -- the forward layout and the input-gradient layout (transposed, taps
    flipped) -- from the same fp32 master tensor.  Pairs whose 32 x 32 blocks coincide become ONE job with ``dst2`` (ABI 7): the master
    weights are read once (the re-pack of the SD-2.1 UNet: 6.9 -> 3.5 GB of reads per step).  Jobs without a partner stay as they are."""
    fwd = {}
    for a in jobs:
        if not a.dgrad and not a.dst2:
            fwd.setdefault((a.src, a.ksize, a.cout, a.cin, a.cout_pad, a.cin_pad, a.src_in), []).append(a)
    out, used = [], set()
    for a in jobs:
        if a.dgrad:
            cands = fwd.get((a.src, a.ksize, a.cin, a.cout, a.cin_pad, a.cout_pad, a.src_in), [])
            partner = next((f for f in cands if id(f) not in used), None)
            if partner is not None:
                used.add(id(partner))
                partner.dst2, partner.dst2_ct_stride = a.dst, a.dst_ct_stride
                continue
        out.append(a)
    return out


def run_pack_jobs(lib, jobs, stream, cache, device):
    """All ``pd_pack_weight`` jobs of an optimizer step as ONE ``pd_pack_weight_batch`` launch: the descriptors are uploaded
    once (``cache``: a dict owned by the re-packer) next to the block-range table the kernel searches."""
    if not jobs:
        return
    st = cache.get("batch")
    if st is None:
        jobs = fuse_pack_jobs(jobs)
        for a in jobs:     # what pd_pack_weight would refuse
            if a.cout_pad % 32 or a.cin_pad % 32 or a.cout_pad < a.cout or a.cin_pad < a.cin or a.dtype != jobs[0].dtype:
                raise L.PhenDiffHipError("pd_pack_weight_batch: inconsistent job descriptors")
        dev = torch.device(device)
        st = []
        # one launch per kernel size: the workgroup's LDS tile is sized by the launch's largest kernel (37 KB for 3x3 against 4 KB for the
        # Linear / 1x1 blocks, which are most of the latent-diffusion UNet's blocks and would run at a quarter of the occupancy beside them)
        for ks in sorted({a.ksize for a in jobs}):
            sel = [a for a in jobs if a.ksize == ks]
            raw = (L.PackWeightArgs * len(sel))(*sel)
            table = torch.frombuffer(bytearray(bytes(raw)), dtype=torch.uint8).to(dev)
            starts, tot = [0], 0
            for a in sel:
                tot += (a.cout_pad // 32) * (a.cin_pad // 32)
                starts.append(tot)
            starts_t = torch.tensor(starts, dtype=torch.int32, device=dev)
            args = L.PackWeightBatchArgs(dtype=sel[0].dtype, n=len(sel), jobs=table.data_ptr(), starts=starts_t.data_ptr(), total_blocks=tot,
                                         max_ksize=ks)
            st.append((args, table, starts_t))
        cache["batch"] = st
    for args, _, _ in st:
        L.check(lib.pd_pack_weight_batch(C.byref(args), stream), "pd_pack_weight_batch")


class Repacker:
    """After an optimizer step: fp32 master parameters -> every kernel-layout copy the plans read, IN PLACE.  ``pre``: torch-side
    preparations the pack jobs read (run first); ``jobs``: the ``pd_pack_weight`` descriptors, with (source tensor, destination
    tensor) of each in ``job_tensors`` (the descriptors hold raw pointers: these keep the tensors alive); ``small``: the few fp32
    copies that are not a packed weight (run last).  Parameters the kernels read as plain fp32 vectors alias the flat master
    buffer and need nothing."""

    def __init__(self, code, device):
        self.lib = L.lib()
        self.code, self.jobs_device = code, device
        self.jobs, self.job_tensors, self.pre, self.small = [], [], [], []
        self._batch = {}

    def job(self, dst, src, cout, cin, k, *, dgrad=0, cout_pad=None, cin_pad=None, ct_stride=None, dst_off=0):
        """Pack ``src`` (OIHW, ``cout`` x ``cin`` in the orientation of the PACKED weight) into ``dst``; ``ct_stride`` / ``dst_off``
        (elements): the 32-row tiles of ``dst`` are interleaved with another weight's."""
        cp, ip = cout_pad or pad32(cout), cin_pad or pad32(cin)
        self.jobs.append(L.PackWeightArgs(dtype=self.code, cout=cout, cin=cin, cout_pad=cp, cin_pad=ip, ksize=k,
                                          src_in=(cout if dgrad else cin), dgrad=dgrad, src=src.data_ptr(),
                                          dst=dst.data_ptr() + dst_off * dst.element_size(), dst_ct_stride=ct_stride or tile_elems(ip, k)))
        self.job_tensors.append((src, dst))

    def pair(self, dst, dstd, weight, cout, cin, k=1, *, cout_pad=None, cin_pad=None):
        """The forward layout and the input-gradient layout of one weight."""
        self.job(dst, weight, cout, cin, k, cout_pad=cout_pad, cin_pad=cin_pad)
        self.job(dstd, weight, cin, cout, k, dgrad=1, cout_pad=cin_pad, cin_pad=cout_pad)

    def resnet(self, r, e, t):
        cin, cout = r.in_channels, r.out_channels
        stride = e.w2[0].numel()          # (conv2's tile, and the shortcut's behind it when it is fused)
        self.job(e.w1, r.conv1.weight, cout, cin, 3)
        self.job(e.w2, r.conv2.weight, cout, cout, 3, ct_stride=stride)
        self.job(t.w1d, r.conv1.weight, cin, cout, 3, dgrad=1)
        self.job(t.w2d, r.conv2.weight, cout, cout, 3, dgrad=1)
        if r.conv_shortcut is not None:
            self.job(e.w2, r.conv_shortcut.weight, cout, cin, 1, ct_stride=stride, dst_off=tile_elems(cout, 3))
            self.job(t.wsd, r.conv_shortcut.weight, cin, cout, 1, dgrad=1)
            b2, bs, dst = r.conv2.bias, r.conv_shortcut.bias, e.b2
            self.small.append(lambda: torch.add(b2.data, bs.data, out=dst))

    def attention(self, a, e, t, order: str):
        """``order``: name of the family's parameter-order function (for the error message)."""
        ch = a.to_q.weight.shape[0]
        require_adjacent(f"to_q/to_k/to_v parameters must be adjacent (use {order})",
                         (a.to_q.weight, a.to_k.weight, a.to_v.weight), (a.to_q.bias, a.to_k.bias, a.to_v.bias))
        self.job(e.wqkv, a.to_q.weight, 3 * ch, ch, 1)
        self.job(e.wo, a.to_out[0].weight, ch, ch, 1)
        self.job(t.wqkvd, a.to_q.weight, ch, 3 * ch, 1, dgrad=1)
        self.job(t.wod, a.to_out[0].weight, ch, ch, 1, dgrad=1)
        qb, dst = a.to_q.bias, e.bqkv
        self.small.append(lambda: dst.copy_(torch.as_strided(qb.data, (3 * ch,), (1,))))

    def sampler(self, s, e, t):
        ch, wt = s.conv.weight.shape[0], s.conv.weight
        self.pair(e.w, t.wd, wt, ch, ch, 3)
        src4 = getattr(e, "w4_src", None)
        if src4 is not None:      # the sub-pixel phase kernels: pre-summed taps first (one contraction), then packed like any weight
            self.pre.append(lambda: upsample_phase_weights_stacked(wt.data, out=src4))
            for p in range(4):
                self.pair(e.w4[p], t.wd4[p], src4[p], ch, ch, 2)

    def time_mlp_and_conv_out(self, m, w, first_proj):
        """The fp32 copies of a UNet's forward set that are not the parameters themselves (``WeightSet.time_mlp_and_conv_out`` /
        ``stack_time_emb_proj``); ``first_proj``: the first ResNet block's ``time_emb_proj`` -- the others follow it in memory."""
        te, pd_, tdim, co = m.time_embedding, w.proj_dim, m.time_embed_dim, m.conv_out.weight.shape[0]
        self.small += [
            lambda: w.w1T.copy_(te.linear_1.weight.data.t()),
            lambda: w.w2T.copy_(te.linear_2.weight.data.t()),
            lambda: w.wpT.copy_(torch.as_strided(first_proj.weight.data, (pd_, tdim), (tdim, 1)).t()),
            lambda: w.bp.copy_(torch.as_strided(first_proj.bias.data, (pd_,), (1,))),
            lambda: w.conv_out_b[:co].copy_(m.conv_out.bias.data),
        ]

    def run(self, stream):
        with torch.no_grad():
            for f in self.pre:
                f()
        run_pack_jobs(self.lib, self.jobs, stream, self._batch, self.jobs_device)
        with torch.no_grad():
            for f in self.small:
                f()
