"""Training the autoencoder's encoder on MI355X: ``--components_to_train autoencoder`` (``args_parser.py:34-41``).  When the
VAE is not frozen (``train.py:189-199``) the reference encodes inside the step (``utils_training.py:237-256``), so the diffusion
loss flows back through ``quant_conv`` and the encoder; nothing sends a gradient to the decoder or ``post_quant_conv``.

``VaeEncodeTrainPlan`` = the forward of :class:`phendiff_amd.vae.VaeEncodePlan` (GroupNorm statistics, attention log-sum-exp and
activations kept) + the backward of its block tape on the emitters of :class:`phendiff_amd.unet_train.UNetTrainPlan` -- the
same launches the pixel-space UNet's backward uses (ResNet blocks without a time embedding, the pad-0 stride-2 downsampler, the
im2col ``conv_in``, one wide attention head), plus the two 32-lane output layers ``encoder.conv_out`` (2 x latent channels inside
32) and ``quant_conv`` (2 x latent -> 2 x latent inside 32 / 32), whose pad lanes carry exact zeros.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from .unet import _Attention, _Sampler
from .unet_train import UNetTrainPlan
from .weight_layout import Repacker, WeightSet, require_alias
from .vae import AutoencoderKL, VaeEncodePlan, _VaePlan, _VaeResnet, _VaeWeights

VAE_PREFIX = "vae."


def vae_training_param_order(vae: AutoencoderKL) -> List[Tuple[str, torch.nn.Parameter]]:
    """(name, parameter) pairs of the VAE in the order of the flat training buffers: each attention's to_q / to_k / to_v weights
    (then biases) adjacent -- the fused [3C][C] projection one gradient launch writes --, then everything else in
    ``named_parameters()`` order."""
    named = dict(vae.named_parameters())
    out, seen = [], set()
    for n, mod in vae.named_modules():
        if isinstance(mod, _Attention):
            for suffix in ("weight", "bias"):
                for which in ("to_q", "to_k", "to_v"):
                    k = f"{n}.{which}.{suffix}"
                    out.append((k, named[k]))
                    seen.add(k)
    out += [(n, p) for n, p in named.items() if n not in seen]
    return out


def vae_never_graded(vae: AutoencoderKL) -> frozenset:
    """Parameters the diffusion loss never reaches (``decoder.*``, ``post_quant_conv.*``): their ``.grad`` stays None in the
    reference, so ``torch.optim.AdamW`` skips them -- no update, no weight decay."""
    return frozenset(n for n, _ in vae.named_parameters() if not (n.startswith("encoder.") or n.startswith("quant_conv.")))


class VaeTrainWeights(WeightSet):
    """Input-gradient weights of the encoder and ``quant_conv`` in ``pd_conv``'s packed layout (transposed, taps flipped)."""

    def __init__(self, vae: AutoencoderKL, device, tdt):
        super().__init__(device, tdt, dgrad=True)
        self.resnets, self.attns, self.samplers = {}, {}, {}
        for name, mod in vae.encoder.named_modules(prefix="encoder"):
            if isinstance(mod, _VaeResnet):
                self.resnets[name] = self.resnet(mod)
            elif isinstance(mod, _Attention):
                self.attns[name] = self.attention(mod)
            elif isinstance(mod, _Sampler):
                self.samplers[name] = self.sampler(mod)
        co = vae.encoder.conv_out
        self.enc_out_d = self.padded(co, 32, co.weight.shape[1])      # 32 (2 x latent real) output-gradient lanes -> block_out_channels[-1]
        self.quant_d = self.padded(vae.quant_conv, 32, 32)


class VaeEncodeTrainPlan(UNetTrainPlan, VaeEncodePlan):
    """Forward (with saved statistics) + backward launch plan of ``quant_conv(encoder(x))`` for a fixed (B, H, W).

    ``params`` / ``grads``: VAE ``state_dict`` name -> fp32 device tensor laid out as :func:`vae_training_param_order` prescribes.
    ``backward`` ACCUMULATES into ``grads``; ``decoder.*`` / ``post_quant_conv.*`` never receive a gradient."""

    def __init__(self, vae: AutoencoderKL, w: _VaeWeights, tw: VaeTrainWeights, B, H, W, device,
                 params: Optional[Dict[str, torch.Tensor]] = None, grads: Optional[Dict[str, torch.Tensor]] = None, frozen=()):
        self.train = True
        _VaePlan.__init__(self, vae, w, B, H, W, device)
        nlev = len(vae.config.block_out_channels)
        self.h, self.wd = H >> (nlev - 1), W >> (nlev - 1)
        # d loss / d quant_conv output, NHWC, 32 lanes ([d mean | d logvar | zeros]): what pd_latent_chain_bwd writes
        self.dmom = torch.zeros((B, self.h, self.wd, 32), dtype=self.tdt, device=device)
        self.bufs.append(self.dmom)
        self._dout_args = SimpleNamespace(x=None)
        self._init_train(tw, params, grads, False, frozen)

    param_order_name = "vae_training_param_order"

    def _fused_param_groups(self):
        return [("to_q/to_k/to_v parameters must be adjacent", [f"{n}.{x}.{suffix}" for x in ("to_q", "to_k", "to_v")])
                for n, mod in self.m.encoder.named_modules(prefix="encoder") if isinstance(mod, _Attention) for suffix in ("weight", "bias")]

    # ---- forward -----------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, moments: torch.Tensor, stream):
        """fp32 NCHW images (B, C, H, W) -> fp32 NCHW moments (B, 2 latent, H/8, W/8); keeps what ``backward`` needs."""
        self.run(x.data_ptr(), moments.data_ptr(), stream)
        for args in self._sample_ptr_args:
            args.x = x.data_ptr()
        self.keepalive = (x, moments)

    # ---- backward ----------------------------------------------------------------------------------------------------
    def _bwd_record(self, rec):
        c, tw = self.m.config, self.tw
        lat2 = 2 * c.latent_channels
        if rec.kind == "vae_out":
            dmom = self.dmom
            # quant_conv: 2 latent -> 2 latent inside 32 / 32 lanes.  The pad lanes of its input (conv_out's zero weights and bias)
            # and of its output gradient (pd_latent_chain_bwd) hold exact zeros; only the valid slice reaches the parameter
            self._bias_grad(dmom, "quant_conv.bias", valid=lat2)
            self._wgrad(rec.z, None, None, 0, dmom, "quant_conv.weight", ksize=1, pad=0, cout_valid=lat2, cin_valid=lat2)
            dz = self._dgrad(dmom, tw.quant_d, 32, ksize=1, tag="dz_quant")
            # encoder.conv_out: block_out_channels[-1] -> 2 latent inside 32 lanes, over SiLU(GroupNorm(x))
            self._bias_grad(dz, "encoder.conv_out.bias", valid=lat2)
            self._wgrad(rec.x, None, rec.gn, 1, dz, "encoder.conv_out.weight", cout_valid=lat2)
            dx = self._dgrad(dz, tw.enc_out_d, rec.x.shape[3], tag="dz_out")
            self._gn_bwd(rec.gn, dx, 1, wname="encoder.conv_norm_out")
        elif rec.kind == "vae_conv_in":
            if self.param_grads:
                self._im2col_wgrad(self._g(rec.out)[0], "encoder.conv_in")
        else:
            super()._bwd_record(rec)

    def backward(self, d_moments_nhwc: torch.Tensor, stream, after_op=None):
        """Accumulate d loss / d (encoder, quant_conv parameters) given d loss / d moments: NHWC in the compute dtype, 32 lanes,
        lanes >= 2 x latent zero (``self.dmom`` is that buffer: ``pd_latent_chain_bwd`` may write it in place)."""
        if d_moments_nhwc.data_ptr() != self.dmom.data_ptr():
            if tuple(d_moments_nhwc.shape) != tuple(self.dmom.shape):
                raise ValueError(f"d_moments_nhwc: expected {tuple(self.dmom.shape)}, got {tuple(d_moments_nhwc.shape)}")
            self.dmom.copy_(d_moments_nhwc)
        super().backward(self.dmom, stream, after_op=after_op)


class _VaeRepacker(Repacker):
    """The re-pack of the encoder's and ``quant_conv``'s kernel-layout copies, which the encode plans (inference and training)
    and the backward read.  The decoder never changes."""

    def __init__(self, vae: AutoencoderKL, w: _VaeWeights, tw: VaeTrainWeights):
        super().__init__(w.code, vae.quant_conv.weight.device)
        enc, q = vae.encoder, vae.quant_conv
        c0, ci = enc.conv_in.weight.shape[:2]
        co, cc = enc.conv_out.weight.shape[:2]
        qo, qi = q.weight.shape[:2]
        self.job(w.enc_in_w, enc.conv_in.weight, c0, ci * 9, 1, cin_pad=32)
        for name, mod in enc.named_modules(prefix="encoder"):
            if isinstance(mod, _VaeResnet):
                self.resnet(mod, w.resnets[name], tw.resnets[name])
            elif isinstance(mod, _Attention):
                self.attention(mod, w.attns[name], tw.attns[name], "vae_training_param_order")
            elif isinstance(mod, _Sampler):
                self.sampler(mod, w.samplers[name], tw.samplers[name])
        self.pair(w.enc_out_w, tw.enc_out_d, enc.conv_out.weight, co, cc, 3, cout_pad=32)
        self.pair(w.quant_w, tw.quant_d, q.weight, qo, qi, 1, cout_pad=32, cin_pad=32)
        self.small += [lambda: w.enc_out_b[:co].copy_(enc.conv_out.bias.data), lambda: w.quant_b[:qo].copy_(q.bias.data)]
        require_alias([(w.enc_in_b, enc.conv_in.bias), (w.enc_gn[0], enc.conv_norm_out.weight)])


def latent_chain_bwd(g_noisy, g_out, moments, eps, sa, sb, pred_type: str, scale: float, out, code, stream):
    """One ``pd_latent_chain_bwd`` launch: d loss / d noisy latents (+ d loss / d model_out for the target term) -> d loss / d
    moments, NHWC in the compute dtype (``out``: (B, h, w, Cpad), pad lanes zero)."""
    B, C2, h, w = moments.shape
    for t in (g_noisy, g_out, moments, eps, sa, sb, out):
        if t is not None and not t.is_cuda:
            raise L.PhenDiffHipError("phendiff_amd runs on MI355X only (no CPU fallback)")
    a = L.LatentChainBwdArgs(dtype=code, B=B, C=C2 // 2, HW=h * w, Cpad=out.shape[-1], pred_type=L.PD_PRED[pred_type], scale=float(scale),
                             g_noisy=g_noisy.data_ptr(), g_out=L.ptr(g_out), moments=moments.data_ptr(), eps=L.ptr(eps),
                             sa=sa.data_ptr(), sb=sb.data_ptr(), out=out.data_ptr())
    L.check(L.lib().pd_latent_chain_bwd(C.byref(a), stream), "pd_latent_chain_bwd")
    return out
