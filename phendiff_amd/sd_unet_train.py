"""Training step of the SD-2.1 ``UNet2DConditionModel`` + ``CustomEmbedding`` on MI355X (BASELINE
configs[3]): what ``_SD_prediction_wrapper`` + ``_diffusion_and_backward`` (``utils_training.py:459-496,371-456``) ask autograd
to do, as a static plan of HIP launches on the engine of :mod:`phendiff_amd.unet_train`.

``SDUNetTrainPlan`` = the forward of :class:`phendiff_amd.sd_unet.SDUNetPlan` (statistics / log-sum-exp kept) + the backward of
its block tape.  ResnetBlock2D / sampling convs / conv_out / the time-embedding path reuse the pixel-space UNet's emitters; a
``Transformer2DModel`` block adds, in reverse order of its forward: every ``nn.Linear`` as a 1x1 convolution (input gradient =
``pd_conv`` with the transposed weights, weight gradient = ``pd_conv_wgrad``), ``pd_geglu_bwd``, ``pd_layernorm_bwd`` (which also
folds the skip-connection gradient in), ``pd_attn_d64_bwd`` for the self attention and the 77-token cross attention, and the
gradient of the class token (``pd_token_embedding_grad``) -- the only trainable part of ``encoder_hidden_states``.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from .sd_unet import (CustomEmbedding, SDUNet2DConditionModel, SDUNetPlan, _SDPackedWeights, _Transformer2D,
                      class_emb_to_encoder_hidden_states)
from .unet import _Resnet, _Sampler
from .unet_train import UNetTrainer, UNetTrainPlan, _FusedSums
from .weight_layout import Repacker, WeightSet, pad32, require_adjacent, require_alias


EMB_NAME = "class_embedding.inner_module.weight"


def sd_training_param_order(m: SDUNet2DConditionModel) -> List[Tuple[str, torch.nn.Parameter]]:
    """(name, parameter) pairs in the order of the flat training buffers: all ``time_emb_proj`` weights (then biases) stacked
    -- the one [proj_dim][tdim] matrix ``pd_temb`` sees --, each transformer's attn1 to_q/to_k/to_v and attn2 to_k/to_v weights
    adjacent (the fused projections), then everything else."""
    named = dict(m.named_parameters())
    out, seen = [], set()

    def take(n):
        out.append((n, named[n]))
        seen.add(n)

    res = [n for n, mod in m.named_modules() if isinstance(mod, _Resnet)]
    for suffix in ("weight", "bias"):
        for n in res:
            take(f"{n}.time_emb_proj.{suffix}")
    for n, mod in m.named_modules():
        if isinstance(mod, _Transformer2D):
            b = f"{n}.transformer_blocks.0"
            for which in ("to_q", "to_k", "to_v"):
                take(f"{b}.attn1.{which}.weight")
            for which in ("to_k", "to_v"):
                take(f"{b}.attn2.{which}.weight")
    for n in named:
        if n not in seen:
            take(n)
    return out


class SDTrainWeights(WeightSet):
    """Input-gradient weights in ``pd_conv``'s packed layout (W'[ci][co][ky][kx] = W[co][ci][K-1-ky][K-1-kx])."""

    def __init__(self, m: SDUNet2DConditionModel, device, tdt):
        # fp16 (round 5): `--mixed_precision fp16` fine-tuning (args_parser.py:381-390) under training.LossScaler, set up by SDUNetTrainer
        super().__init__(device, tdt, dgrad=True)
        pk = self.pack
        self.resnets, self.transformers, self.samplers = {}, {}, {}
        for name, mod in m.named_modules():
            if isinstance(mod, _Resnet):
                self.resnets[name] = self.resnet(mod)
            elif isinstance(mod, _Transformer2D):
                blk = mod.transformer_blocks[0]
                a1, a2 = blk.attn1, blk.attn2
                self.transformers[name] = SimpleNamespace(
                    w_in_d=pk(mod.proj_in.weight), w_out_d=pk(mod.proj_out.weight),
                    wqkv1_d=pk(torch.cat([a1.to_q.weight, a1.to_k.weight, a1.to_v.weight], 0)),
                    wo1_d=pk(a1.to_out[0].weight), wq2_d=pk(a2.to_q.weight),
                    wkv2_d=pk(torch.cat([a2.to_k.weight, a2.to_v.weight], 0)), wo2_d=pk(a2.to_out[0].weight),
                    wff1_d=pk(blk.ff.net[0].proj.weight), wff2_d=pk(blk.ff.net[2].weight))
            elif isinstance(mod, _Sampler):
                self.samplers[name] = self.sampler(mod, phases=".upsamplers." in name)
        co, cc = m.conv_out.weight.shape[:2]
        self.conv_out_d = self.padded(m.conv_out, pad32(co), cc)
        # conv_in's input gradient (the latent gradient of the gradient-guided transfer): block_out_channels[0] -> 4 channels (pad 32)
        self.conv_in_d = self.padded(m.conv_in, m.conv_in.weight.shape[0], 32)


class SDUNetTrainPlan(UNetTrainPlan, SDUNetPlan):
    """Forward (with saved statistics) + backward launch plan of the SD UNet for a fixed (B, H, W, context tokens).
    ``params`` / ``grads``: state_dict-name -> fp32 device tensor, laid out as :func:`sd_training_param_order` prescribes, plus
    ``EMB_NAME`` -> the ``CustomEmbedding`` table (optional).  ``backward`` ACCUMULATES into ``grads``."""

    def __init__(self, m: SDUNet2DConditionModel, w: _SDPackedWeights, tw: SDTrainWeights, B, H, W, tokens, device,
                 params: Optional[Dict[str, torch.Tensor]] = None, grads: Optional[Dict[str, torch.Tensor]] = None, frozen=(),
                 input_grad: bool = False):
        """``input_grad``: also produce d loss / d latents (fp32 NCHW, ``self.dsample``) -- the gradient-guided transfer's
        ``torch.autograd.grad(losses_seq, images)`` through the UNet (utils_Img2Img.py:718-745, latent-diffusion branch)."""
        m.require_attention_backward("SDUNetTrainPlan")
        self.train = True
        SDUNetPlan.__init__(self, m, w, B, H, W, tokens, device)
        self._init_train(tw, params, grads, input_grad, frozen)

    # ---- layout checks -----------------------------------------------------------------------------------------------
    param_order_name = "sd_training_param_order"

    def _fused_param_groups(self):
        groups = self._time_emb_proj_groups()
        for n, mod in self.m.named_modules():
            if isinstance(mod, _Transformer2D):
                b = f"{n}.transformer_blocks.0"
                for attn, which in ((".attn1", ("to_q", "to_k", "to_v")), (".attn2", ("to_k", "to_v"))):
                    groups.append(("attn1 to_q/to_k/to_v and attn2 to_k/to_v weights must be adjacent", [f"{b}{attn}.{x}.weight" for x in which]))
        return groups

    def _zero_bias_len(self):
        return 8 * max(self.m.config.block_out_channels) + 64

    # ---- forward -----------------------------------------------------------------------------------------------------
    def forward(self, sample: torch.Tensor, timesteps: torch.Tensor, ehs: torch.Tensor, out: torch.Tensor, stream,
                labels: Optional[torch.Tensor] = None):
        """One training forward: fp32 NCHW latents + (B,) timesteps + (B, tokens, D) context -> fp32 NCHW prediction.
        ``labels``: the class ids whose embedding is token 0 of ``ehs`` (None on an unconditional step)."""
        self.ehs.view(self.B, self.tokens, -1).copy_(ehs)
        a = self.temb_args
        a.rows = self.B
        a.timesteps, a.labels, a.class_emb = timesteps.data_ptr(), None, None
        a.emb, a.proj = self.t_emb.data_ptr(), self.temb_table.data_ptr()
        a.feat, a.z1 = self.t_feat.data_ptr(), self.t_z1.data_ptr()
        L.check(self.lib.pd_temb(C.byref(a), stream), "pd_temb")
        a.feat, a.z1 = None, None
        self.run(sample.data_ptr(), self.temb_table.data_ptr(), out.data_ptr(), stream)
        self._labels = None
        if self._token_grad_args is not None:
            self._token_grad_args.labels = L.ptr(labels)
        self.keepalive = (sample, timesteps, ehs, out, labels)

    # ---- backward emitters -------------------------------------------------------------------------------------------
    def _build_backward(self):
        self._dehs = [torch.empty_like(self.ehs), False]
        self.bufs.append(self._dehs[0])
        self._token_grad_args = None
        super()._build_backward()
        if self._want_ehs_grad():
            dehs, dt = self._dehs[0], self.grads[EMB_NAME]
            a = L.TokenEmbeddingGradArgs(dtype=self.code, rows=self.B, dim=dt.shape[1], num_classes=dt.shape[0],
                                         row_stride=self.tokens * dt.shape[1], labels=None, d=dehs.data_ptr(), dtable=dt.data_ptr())
            self._token_grad_args = a
            self._emit(self.lib.pd_token_embedding_grad, a, "token_embedding_grad")
            self._mark_ready(EMB_NAME)

    def _bwd_record(self, rec):
        if rec.kind == "transformer":
            self._transformer_bwd(rec)
        elif rec.kind == "sd_conv_in":
            if self.input_grad:
                dout = self._g(rec.out)[0]
                self._conv(dout, None, self.tw.conv_in_d, self._zero_bias, self.m.config.in_channels, out_mode=L.PD_OUT_NCHW_F32,
                           cout_pad=32, y=self.dsample, stats=False, what="dgrad3x3")
            if not self.param_grads:
                return
            dout = self._g(rec.out)[0]
            self._bias_grad(dout, "conv_in.bias")
            self._wgrad(rec.x, None, None, 0, dout, "conv_in.weight", cin_valid=self.m.config.in_channels)
        else:
            super()._bwd_record(rec)

    def _ln_bwd(self, x, ln, pname, dy, res, tag, bias_name=None):
        """LayerNorm backward (+ the gradient arriving over the skip connection).  ``bias_name``: the bias of the Linear layer whose output gradient the
        returned dx is -- its gradient (the column sums of dx) comes out of the same launch (round 6, ``pd_layernorm_bwd_args.dxsum``) instead of a
        ``pd_channel_sum`` pass over dx; returns (dx, whether that happened)."""
        gamma, _, eps = ln
        B, h, w, ch = x.shape
        rows = B * h * w
        dx = self._tmp((B, h, w, ch), tag)
        partial = None
        affine = (pname + ".weight", pname + ".bias")
        dgam, dbet = self._grad(affine), self._grad(affine[::-1])       # both, or neither when both are frozen (one launch writes the two)
        fuse = bias_name is not None and dgam is not None and ch <= 1536 and bias_name not in self.frozen
        dxsum = self._grad(bias_name) if fuse else None
        if dgam is not None:
            partial = self._tmp((self.lib.pd_layernorm_bwd_blocks(rows) * (3 if fuse else 2) * ch,), "lnpart3" if fuse else "lnpart", torch.float32)
        a = L.LayerNormBwdArgs(dtype=self.code, rows=rows, C=ch, eps=eps, x=x.data_ptr(), dy=dy.data_ptr(), gamma=gamma.data_ptr(),
                               res=L.ptr(res), dx=dx.data_ptr(), dgamma=L.ptr(dgam), dbeta=L.ptr(dbet), partial=L.ptr(partial), dxsum=L.ptr(dxsum))
        self._emit(self.lib.pd_layernorm_bwd, a, "layernorm_bwd", 0.0, (3 + (res is not None)) * x.numel() * self._esz())
        if dgam is not None:
            self._mark_ready(affine + ((bias_name,) if fuse else ()))
        return dx, fuse

    def _attn_bwd64(self, q, qs, k, v, kvs, o, do, lse, heads, nq, nkv, dq, dqs, dk, dv, dkvs):
        delta = self._tmp((self.B, heads, nq), "delta64", torch.float32)
        a = L.AttnD64BwdArgs(dtype=self.code, B=self.B, heads=heads, Nq=nq, Nkv=nkv, q=q, q_stride=qs, k=k, v=v, kv_stride=kvs,
                             o=o.data_ptr(), dout=do.data_ptr(), o_stride=heads * 64, lse=lse.data_ptr(), delta=delta.data_ptr(),
                             dq=dq, dq_stride=dqs, dk=dk, dv=dv, dkv_stride=dkvs)
        self._emit(self.lib.pd_attn_d64_bwd, a, "attn_d64_bwd", 10.0 * self.B * heads * nq * nkv * 64,
                (4.0 * nq + 4.0 * nkv) * self.B * heads * 64 * self._esz())

    def _transformer_bwd(self, rec):
        e, te, n = rec.e, self.tw.transformers[rec.name], rec.name
        blk = n + ".transformer_blocks.0"
        B, h, w, ch = rec.x.shape
        N, esz, T = h * w, self._esz(), self.tokens
        lin_w = lambda x, dy, wname, gn=None: self._wgrad(x, None, gn, 0, dy, wname, ksize=1, pad=0)
        dout = self._g(rec.out)[0]
        # proj_out (+ residual x: folded into the GroupNorm backward at the end)
        self._bias_grad(dout, n + ".proj_out.bias")
        lin_w(rec.h3, dout, n + ".proj_out.weight")
        dh3 = self._dgrad(dout, te.w_out_d, ch, ksize=1, tag="t_dh3")
        # feed-forward: h3 = ff2(geglu(ff1(LN3(h2)))) + h2
        self._bias_grad(dh3, blk + ".ff.net.2.bias")
        lin_w(rec.gg, dh3, blk + ".ff.net.2.weight")
        dgg = self._dgrad(dh3, te.wff2_d, 4 * ch, ksize=1, tag="t_dgg")
        dff = self._tmp((B, h, w, 8 * ch), "t_dff")
        ga = L.GegluBwdArgs(dtype=self.code, rows=B * N, inner=4 * ch, x=rec.ff.data_ptr(), dy=dgg.data_ptr(), dx=dff.data_ptr())
        if self.param_grads and (4 * ch) % 256 == 0 and (blk + ".ff.net.0.proj.bias") not in self.frozen:
            # the gate's backward also leaves the per-split column sums of dff (the widest gradient of the block): the bias gradient folds
            # those (B x splits x 8 ch floats) instead of reading dff back
            gs = max(1, min(64, N // 64))
            gws = torch.empty((B * gs * 8 * ch,), dtype=torch.float32, device=self.device)      # this block's own (its fold may run on the second stream)
            self.bufs.append(gws)
            ga.sums, ga.sum_splits, ga.B = gws.data_ptr(), gs, B
            self._fused_sums[id(dff)] = _FusedSums(gws, gs, True)
        self._emit(self.lib.pd_geglu_bwd, ga, "geglu_bwd", 0.0, 5.0 * dgg.numel() * esz)
        self._bias_grad(dff, blk + ".ff.net.0.proj.bias")
        self._fused_sums.pop(id(dff), None)               # (dff is a scratch buffer other blocks reuse)
        lin_w(rec.y3, dff, blk + ".ff.net.0.proj.weight")
        dy3 = self._dgrad(dff, te.wff1_d, ch, ksize=1, tag="t_dy")
        dh2, fb = self._ln_bwd(rec.h2, e.ln3, blk + ".norm3", dy3, dh3, "t_dh2", bias_name=blk + ".attn2.to_out.0.bias")
        # cross attention: h2 = to_out(attn(to_q(LN2(h1)), to_k(ehs), to_v(ehs))) + h1
        if not fb:
            self._bias_grad(dh2, blk + ".attn2.to_out.0.bias")
        lin_w(rec.a2, dh2, blk + ".attn2.to_out.0.weight")
        da2 = self._dgrad(dh2, te.wo2_d, ch, ksize=1, tag="t_da")
        dq2 = self._tmp((B, h, w, ch), "t_dq2")
        dkv = self._tmp((B, 1, T, 2 * ch), "t_dkv")
        kvp = rec.kv.data_ptr()
        self._attn_bwd64(rec.q2.data_ptr(), ch, kvp, kvp + ch * esz, 2 * ch, rec.a2, da2, rec.lse2, e.heads, N, T,
                         dq2.data_ptr(), ch, dkv.data_ptr(), dkv.data_ptr() + ch * esz, 2 * ch)
        lin_w(rec.y2, dq2, blk + ".attn2.to_q.weight")
        lin_w(self.ehs, dkv, (blk + ".attn2.to_k.weight", blk + ".attn2.to_v.weight"))       # fused [2C][D] gradient
        if self._want_ehs_grad():
            self._dgrad(dkv, te.wkv2_d, self.ehs.shape[3], ksize=1, into=self._dehs)
        dy2 = self._dgrad(dq2, te.wq2_d, ch, ksize=1, tag="t_dy")
        dh1, fb = self._ln_bwd(rec.h1, e.ln2, blk + ".norm2", dy2, dh2, "t_dh1", bias_name=blk + ".attn1.to_out.0.bias")
        # self attention: h1 = to_out(attn(qkv(LN1(h0)))) + h0
        if not fb:
            self._bias_grad(dh1, blk + ".attn1.to_out.0.bias")
        lin_w(rec.a1, dh1, blk + ".attn1.to_out.0.weight")
        da1 = self._dgrad(dh1, te.wo1_d, ch, ksize=1, tag="t_da")
        dqkv = self._tmp((B, h, w, 3 * ch), "t_dqkv")
        p, dp = rec.qkv.data_ptr(), dqkv.data_ptr()
        self._attn_bwd64(p, 3 * ch, p + ch * esz, p + 2 * ch * esz, 3 * ch, rec.a1, da1, rec.lse1, e.heads, N, N,
                         dp, 3 * ch, dp + ch * esz, dp + 2 * ch * esz, 3 * ch)
        lin_w(rec.y1, dqkv, tuple(f"{blk}.attn1.{x}.weight" for x in ("to_q", "to_k", "to_v")))
        dy1 = self._dgrad(dqkv, te.wqkv1_d, ch, ksize=1, tag="t_dy")
        dh0, fb = self._ln_bwd(rec.h0, e.ln1, blk + ".norm1", dy1, dh1, "t_dh0", bias_name=n + ".proj_in.bias")
        # proj_in over GroupNorm(x) (no SiLU)
        if not fb:
            self._bias_grad(dh0, n + ".proj_in.bias")
        lin_w(rec.x, dh0, n + ".proj_in.weight", gn=rec.gn)
        dz = self._dgrad(dh0, te.w_in_d, ch, ksize=1, tag="t_dz")
        self._gn_bwd(rec.gn, dz, 0, res=dout, wname=n + ".norm")

    def _want_ehs_grad(self):
        return self.param_grads and EMB_NAME in self.grads and EMB_NAME not in self.frozen


def sd_training_layout(model, class_embedding, vae=None, train_class_embedding: bool = True, trainable=None):
    """(order, flags, never_graded, vae_trains) of an :class:`SDUNetTrainer`'s flat buffers -- pure host logic.

    ``order``: (name, parameter) pairs.  With a training autoencoder the order follows the reference's ``params_to_optimize``
    (train.py:268-272), which walks the pipeline's components in the order of its constructor (vae, unet, class_embedding;
    custom_pipeline_stable_diffusion_img2img.py:62-68): the VAE's parameters (names prefixed ``vae.``) come first, then the UNet's,
    the class table stays the tail.  ``flags``: what ``requires_grad`` / ``trainable`` say.  ``never_graded``: trainable names the
    loss never reaches (``vae.decoder.*``, ``vae.post_quant_conv.*``): ``torch.optim.AdamW`` skips them (``grad is None``).
    A VAE none of whose parameters trains (``pipeline.vae.requires_grad_(False)``, train.py:189-191) stays out of the buffers."""
    from .training import resolve_trainable
    from .vae_train import VAE_PREFIX, vae_never_graded, vae_training_param_order
    uorder = sd_training_param_order(model)
    emb = [(EMB_NAME, class_embedding.inner_module.weight)] if train_class_embedding else []
    vorder = [(VAE_PREFIX + n, p) for n, p in vae_training_param_order(vae)] if vae is not None else []
    if trainable is not None:
        flags = resolve_trainable(vorder + uorder + emb, None, trainable)
        vflags, rest = flags[:len(vorder)], flags[len(vorder):]
    else:
        vflags = resolve_trainable(vorder, vae) if vorder else []
        rest = resolve_trainable(uorder, model) + (resolve_trainable(emb, class_embedding) if emb else [])
    if not any(vflags):
        return uorder + emb, rest, frozenset(), False
    skip = {VAE_PREFIX + n for n in vae_never_graded(vae)}
    never = frozenset(n for (n, _), f in zip(vorder, vflags) if f and n in skip)
    if not any(f and n not in skip for (n, _), f in zip(vorder, vflags)):
        raise ValueError("SDUNetTrainer: the trainable autoencoder parameters (decoder / post_quant_conv) never receive a gradient")
    return vorder + uorder + emb, vflags + rest, never, True


def sd_checkpoint_modules(model, class_embedding, vae, names):
    """accelerate's numbering of the prepared models (train.py:318-326): unet 0, vae 1, class embedding 2, as
    [(file index, module, flat-name prefix)] in the order of the optimizer's parameter list (vae, unet, class embedding)."""
    from .vae_train import VAE_PREFIX
    mods = []
    if vae is not None and any(n.startswith(VAE_PREFIX) for n in names):
        mods.append((1, vae, VAE_PREFIX))
    mods.append((0, model, ""))
    if EMB_NAME in names:
        mods.append((2, class_embedding, "class_embedding."))
    return mods


def check_training_images(vae, images):
    """Argument guards of :meth:`SDUNetTrainer.step_images`."""
    if vae is None:
        raise ValueError("step_images needs the autoencoder: build the trainer with SDUNetTrainer(..., vae=pipeline.vae)")
    c = vae.config
    if images.ndim != 4 or images.shape[1] != c.in_channels:
        raise ValueError(f"step_images: expected images (B, {c.in_channels}, H, W), got {tuple(images.shape)}")
    s = 1 << (len(c.block_out_channels) - 1)
    if images.shape[2] % s or images.shape[3] % s:
        raise ValueError(f"step_images: image size {tuple(images.shape[2:])} must be a multiple of {s}")
    if not images.is_cuda:
        raise L.PhenDiffHipError("phendiff_amd trains on MI355X only (no CPU fallback): move the images to 'cuda'")


class _SDRepacker(Repacker):
    """The SD UNet's re-pack: the ``_SDPackedWeights`` and ``SDTrainWeights`` tensors."""

    def __init__(self, m: SDUNet2DConditionModel, w: _SDPackedWeights, tw: SDTrainWeights):
        super().__init__(w.code, m.conv_in.weight.device)
        self.w = w
        pair = self.pair
        c0, ci = m.conv_in.weight.shape[:2]
        co, cc = m.conv_out.weight.shape[:2]
        pair(w.conv_in_w, tw.conv_in_d, m.conv_in.weight, c0, ci, 3, cin_pad=32)
        res, blk0 = [], None
        for name, mod in m.named_modules():
            if isinstance(mod, _Resnet):
                self.resnet(mod, w.resnets[name], tw.resnets[name])
                res.append(mod)
            elif isinstance(mod, _Transformer2D):
                e, t = w.transformers[name], tw.transformers[name]
                blk = mod.transformer_blocks[0]
                blk0 = blk0 or (e, blk)
                a1, a2 = blk.attn1, blk.attn2
                ch, D = e.ch, a2.to_k.weight.shape[1]
                require_adjacent("fused projection weights must be adjacent (use sd_training_param_order)",
                                 (a1.to_q.weight, a1.to_k.weight, a1.to_v.weight), (a2.to_k.weight, a2.to_v.weight))
                pair(e.w_in, t.w_in_d, mod.proj_in.weight, ch, ch)
                pair(e.w_out, t.w_out_d, mod.proj_out.weight, ch, ch)
                pair(e.wqkv1, t.wqkv1_d, a1.to_q.weight, 3 * ch, ch)
                pair(e.wo1, t.wo1_d, a1.to_out[0].weight, ch, ch)
                pair(e.wq2, t.wq2_d, a2.to_q.weight, ch, ch)
                pair(e.wkv2, t.wkv2_d, a2.to_k.weight, 2 * ch, D)
                pair(e.wo2, t.wo2_d, a2.to_out[0].weight, ch, ch)
                pair(e.wff1, t.wff1_d, blk.ff.net[0].proj.weight, 8 * ch, ch)
                wf = blk.ff.net[0].proj.weight                       # inference copy: value / gate tiles interleaved
                tile = e.wff1_glu[0].numel()
                self.job(e.wff1_glu, wf.data[:4 * ch], 4 * ch, ch, 1, ct_stride=2 * tile)
                self.job(e.wff1_glu, wf.data[4 * ch:], 4 * ch, ch, 1, ct_stride=2 * tile, dst_off=tile)
                pair(e.wff2, t.wff2_d, blk.ff.net[2].weight, ch, 4 * ch)
            elif isinstance(mod, _Sampler):      # (the inference plans' sub-pixel phase kernels follow the weights too)
                self.sampler(mod, w.samplers[name], tw.samplers[name])
        pair(w.conv_out_w, tw.conv_out_d, m.conv_out.weight, co, cc, 3, cout_pad=w.conv_out_pad)
        self.time_mlp_and_conv_out(m, w, res[0].time_emb_proj)
        require_alias([(w.b1, m.time_embedding.linear_1.bias), (w.conv_in_b, m.conv_in.bias), (w.gn_out[0], m.conv_norm_out.weight),
                       (blk0[0].ln1[0], blk0[1].norm1.weight)])

    def run(self, stream):
        super().run(stream)
        self.w.version = getattr(self.w, "version", 0) + 1      # inference plans drop what they cached of the old weights (cross-attention k / v)


class SDUNetTrainer(UNetTrainer):
    """One optimisation step of ``perform_training_epoch`` for ``model_type == "StableDiffusion"``
    (``utils_training.py:244-454``; components_to_train = denoiser [+ class_embedding], ``train.py:189-199``): latents + noise +
    timesteps -> ``_SD_prediction_wrapper`` forward -> loss -> backward (+ overlapped RCCL gradient all-reduce) -> clip + AdamW
    + EMA -> re-pack.  Call ``step(noisy_latents, timesteps, clean_latents, noise, class_labels, unconditional=False)``."""

    def __init__(self, model: SDUNet2DConditionModel, class_embedding: CustomEmbedding, scheduler, lr: float, *, device=None,
                 train_class_embedding: bool = True, use_ema: bool = True, max_grad_norm: Optional[float] = 1.0, group=None,
                 trainable=None, vae=None, _vae_chunk: Optional[int] = None, **adamw):
        """``trainable``: as for :class:`UNetTrainer` (names carry ``EMB_NAME`` for the class table, the ``vae.`` prefix for the
        autoencoder); default: the ``requires_grad`` flags of the UNet's parameters decide for the UNet (``components_to_train`` /
        ``--attention_fine_tuning``, train.py:189-220), ``train_class_embedding`` and the table's own flag for the ``CustomEmbedding``.
        ``vae``: the pipeline's :class:`phendiff_amd.vae.AutoencoderKL` (``components_to_train autoencoder``): it trains when at
        least one of its parameters does (:func:`sd_training_layout`); :meth:`step_images` then encodes inside the step and sends
        the loss gradient back through ``quant_conv`` and the encoder.  ``_vae_chunk``: tests force the encoder's chunk size."""
        model.require_attention_backward("SDUNetTrainer (SD fine-tuning)")
        self.model, self.class_embedding, self.scheduler, self.vae = model, class_embedding, scheduler, vae
        order, flags, never, self._vae_trains = sd_training_layout(model, class_embedding, vae, train_class_embedding, trainable)
        if self._vae_trains and torch.device(vae.device) != torch.device(device or model.device):
            raise L.PhenDiffHipError("SDUNetTrainer: the autoencoder must live on the UNet's device")
        # parameters the loss never reaches get what torch.optim.AdamW gives `grad is None`: no update, no decay, no moments -- the
        # optimizer treats them as frozen (their EMA shadow is the parameter itself), and so do the all-reduce buckets
        self.trainable_flags, self.never_graded, self._vae_chunk = list(flags), never, _vae_chunk
        flags = [f and n not in never for (n, _), f in zip(order, flags)]
        tail = (class_embedding.inner_module.weight.numel(), (EMB_NAME,)) if train_class_embedding and flags[-1] else None
        self._uncond = False
        self._init_state(order, flags, tail, lr, device, use_ema, max_grad_norm, group, adamw)
        if self._vae_trains:
            if vae.compute_dtype != model.compute_dtype:
                raise ValueError("SDUNetTrainer: the autoencoder and the UNet must share one compute_dtype")
            from .vae_train import VAE_PREFIX
            k = len(VAE_PREFIX)
            self._vparams = {n[k:]: t for n, t in self.params.items() if n.startswith(VAE_PREFIX)}
            self._vgrads = {n[k:]: t for n, t in self.grads.items() if n.startswith(VAE_PREFIX)}
            self._vfrozen = frozenset(n[k:] for n in self.frozen if n.startswith(VAE_PREFIX))
            vae.invalidate()
        self._vplans, self._vtw, self._vrepack, self._bound_vw = {}, None, None, None

    def checkpoint_modules(self):
        """accelerate's numbering of the prepared models (train.py:318-326): unet 0, vae 1 (only when it trains: a frozen one is not
        the trainer's), class embedding 2 -- flat names carry the ``vae.`` / ``class_embedding.`` prefixes."""
        return sd_checkpoint_modules(self.model, self.class_embedding, self.vae, self.params)

    def _optimizer_step(self, lr):
        # an unconditional step leaves the CustomEmbedding without a gradient: torch's AdamW skips it (EMA still steps)
        self.opt.step(lr, tail_active=not self._uncond)

    def _make_packed(self):
        return _SDPackedWeights(self.model, self.device)

    def _make_train_weights(self):
        return SDTrainWeights(self.model, self.device, self.model._weights.tdt)

    def _make_repacker(self):
        return _SDRepacker(self.model, self.model._weights, self._tw)

    def _make_plan(self, key):
        m = self.model
        return SDUNetTrainPlan(m, m._weights, self._tw, *key, self.device, self.params, self.grads, frozen=self.frozen,
                               input_grad=self._vae_trains)      # d loss / d noisy latents feeds the encoder's backward

    def plan_for(self, B, H, W, tokens=77):
        self._bind_weights()
        key = (B, H, W, tokens)
        p = self._plans.get(key)
        if p is None:
            p = self._make_plan(key)
            self._plans[key] = p
        return p

    def encoder_hidden_states(self, class_labels, unconditional: bool):
        """``_SD_prediction_wrapper`` (utils_training.py:470-484): zeros(B, 77, D) on an unconditional step, else the class
        embedding as token 0 followed by 76 zero tokens."""
        table = self.class_embedding.inner_module.weight
        if unconditional:
            return torch.zeros((class_labels.shape[0], 77, table.shape[1]), dtype=torch.float32, device=self.device)
        return class_emb_to_encoder_hidden_states(table.data[class_labels.to(device=self.device, dtype=torch.int64)])

    def forward_backward(self, noisy, timesteps, clean, noise, class_labels=None, class_emb=None, after_op=None, unconditional=None):
        if unconditional is None:
            unconditional = self._uncond
        B, _, H, W = noisy.shape
        plan = self.plan_for(B, H, W)
        st = torch.cuda.current_stream(self.device).cuda_stream
        x = noisy.contiguous().float()
        ts = timesteps.to(device=self.device, dtype=torch.float32).contiguous()
        labels = class_labels.to(device=self.device, dtype=torch.int64).contiguous()
        ehs = self.encoder_hidden_states(labels, unconditional)
        out = torch.empty_like(x)
        plan.forward(x, ts, ehs, out, st, labels=None if unconditional else labels)
        loss, dout = self.loss_fn(out, clean, noise, timesteps, grad_scale=self.opt.scaler.scale if self.opt.scaler is not None else 1.0)
        plan.backward(dout, st, after_op=after_op)
        return loss, out

    def step(self, noisy, timesteps, clean, noise, class_labels, unconditional: bool = False, lr: Optional[float] = None,
             group=None, overlap: bool = True, bucket_bytes: int = 64 << 20):
        """3.46 GB of fp32 gradients per step: 64 MB buckets (xGMI rings are per-link bound: few, large messages)."""
        if self._vae_trains:
            raise ValueError("SDUNetTrainer: the autoencoder trains -- the step starts from images (step_images), not from latents")
        self._uncond = bool(unconditional)
        return super().step(noisy, timesteps, clean, noise, class_labels=class_labels, class_emb=None, lr=lr, group=group,
                            overlap=overlap, bucket_bytes=bucket_bytes)

    def step_clean(self, clean, class_labels, **step_kwargs):
        """:meth:`step` from the clean LATENTS alone: the attached sampler draws (noise, timesteps, noisy) on the device."""
        noise, timesteps, noisy = self._require_sampler("step_clean").sample(clean)
        return self.step(noisy, timesteps, clean, noise, class_labels, **step_kwargs)

    # ---- components_to_train autoencoder: the step starts from images --------------------------------------------------------
    def _bind_vae_weights(self):
        """The VAE's kernel-layout weights the trainer's encoder plans, gradient-layout set and re-packer are bound to: rebuilt
        when the model dropped them (``vae.to()`` / ``load_state_dict`` -> ``invalidate``)."""
        from .vae import _VaeWeights
        from .vae_train import VaeTrainWeights
        vae = self.vae
        if vae._weights is not None and vae._weights is self._bound_vw:
            return
        for n, p in vae.named_parameters():
            if p.data_ptr() != self._vparams[n].data_ptr():
                raise L.PhenDiffHipError(f"parameter vae.{n} no longer aliases the trainer's flat buffer (the autoencoder was converted "
                                         "or moved after the trainer was built): build a new trainer")
        if vae._weights is None:
            vae._weights = _VaeWeights(vae, self.device)
        self._vtw = VaeTrainWeights(vae, self.device, vae._weights.tdt)
        self._vrepack, self._vplans, self._bound_vw = None, {}, vae._weights

    def vae_plan_for(self, B, H, W, slot=0):
        """The encoder's training plan of chunk ``slot`` (every chunk of a step keeps its own activations until its backward)."""
        from .vae_train import VaeEncodeTrainPlan
        self._bind_vae_weights()
        key = (B, H, W, slot)
        p = self._vplans.get(key)
        if p is None:
            p = VaeEncodeTrainPlan(self.vae, self.vae._weights, self._vtw, B, H, W, self.device, self._vparams, self._vgrads,
                                   frozen=self._vfrozen)
            self._vplans[key] = p
        return p

    def refresh_weights(self):
        super().refresh_weights()
        if self._vae_trains and not (self.vae._weights is None and self._bound_vw is None):
            from .vae_train import _VaeRepacker
            self._bind_vae_weights()
            if self._vrepack is None:
                self._vrepack = _VaeRepacker(self.vae, self.vae._weights, self._vtw)
            self._vrepack.run(torch.cuda.current_stream(self.device).cuda_stream)

    def _coefficients(self, timesteps):
        """sqrt(alpha_bar_t), sqrt(1 - alpha_bar_t) per sample: the host-computed fp32 tables ``DDIMScheduler.add_noise`` gathers from."""
        idx = timesteps.detach().to(device=self.device, dtype=torch.long)
        if self.loss_fn.tables[0].device != idx.device:
            self.loss_fn.tables = tuple(t.to(idx.device) for t in self.loss_fn.tables)
        return self.loss_fn.tables[1][idx].contiguous(), self.loss_fn.tables[2][idx].contiguous()

    def images_forward_backward(self, images, timesteps, noise, class_labels, posterior_noise=None, unconditional=None):
        """Loss of one image batch and the gradients of every trained component (accumulated into the flat gradient buffer):
        encode (train plan) -> ``pd_latent_sample`` -> ``pd_add_noise`` -> UNet forward -> ``pd_diffusion_loss`` -> UNet backward
        with the input gradient -> ``pd_latent_chain_bwd`` -> encoder backward.  Returns (loss, latents)."""
        from .vae import DiagonalGaussianDistribution
        from .vae_train import latent_chain_bwd
        if unconditional is None:
            unconditional = self._uncond
        vae, c = self.vae, self.vae.config
        B, _, H, W = images.shape
        st = torch.cuda.current_stream(self.device).cuda_stream
        x = images.contiguous().float()
        nlev = len(c.block_out_channels)
        h, w, lat = H >> (nlev - 1), W >> (nlev - 1), c.latent_channels
        sf = float(c.scaling_factor)
        chunk = self._vae_chunk or vae._max_batch(H, W, "enc")      # pd_conv's 2 GiB source-offset limit holds for training too
        moments = torch.empty((B, 2 * lat, h, w), dtype=torch.float32, device=self.device)
        chunks = [(b0, min(chunk, B - b0)) for b0 in range(0, B, chunk)]
        vplans = []
        for slot, (b0, nb) in enumerate(chunks):
            vp = self.vae_plan_for(nb, H, W, slot)
            vp.forward(x[b0:b0 + nb], moments[b0:b0 + nb], st)
            vplans.append(vp)
        if posterior_noise is None:
            posterior_noise = torch.randn((B, lat, h, w), dtype=torch.float32, device=self.device)      # randn_tensor on the device
        pn = posterior_noise.to(device=self.device, dtype=torch.float32).contiguous()
        latents = DiagonalGaussianDistribution(moments).sample(noise=pn, scale=sf)
        nz = noise.to(device=self.device, dtype=torch.float32).contiguous()
        sa, sb = self._coefficients(timesteps)
        noisy = torch.empty_like(latents)
        a = L.AddNoiseArgs(numel=latents.numel(), per_sample=latents[0].numel(), velocity=0, x=latents.data_ptr(), noise=nz.data_ptr(),
                           sa=sa.data_ptr(), sb=sb.data_ptr(), out=noisy.data_ptr())
        L.check(L.lib().pd_add_noise(C.byref(a), st), "pd_add_noise")
        plan = self.plan_for(B, h, w)
        ts = timesteps.to(device=self.device, dtype=torch.float32).contiguous()
        labels = class_labels.to(device=self.device, dtype=torch.int64).contiguous()
        ehs = self.encoder_hidden_states(labels, unconditional)
        out = torch.empty_like(noisy)
        plan.forward(noisy, ts, ehs, out, st, labels=None if unconditional else labels)
        loss, dout = self.loss_fn(out, latents, nz, timesteps, grad_scale=self.opt.scaler.scale if self.opt.scaler is not None else 1.0)
        plan.backward(dout, st)
        pt = self.scheduler.config.prediction_type
        for vp, (b0, nb) in zip(vplans, chunks):
            sl = slice(b0, b0 + nb)
            latent_chain_bwd(plan.dsample[sl], dout[sl], moments[sl], pn[sl], sa[sl], sb[sl], pt, sf, vp.dmom, vp.code, st)
            vp.backward(vp.dmom, st)      # weight gradients accumulate across the chunks
        self._keep_images = (x, moments, pn, nz, latents, noisy, out, dout, sa, sb, ts, labels, ehs)
        return loss, latents

    def step_images(self, images, timesteps=None, noise=None, class_labels=None, posterior_noise=None, unconditional: bool = False,
                    lr: Optional[float] = None, group=None, overlap: bool = True, bucket_bytes: int = 64 << 20):
        """One optimisation step from IMAGES (``utils_training.py:237-256``: the batch is encoded inside the step): with a training
        autoencoder, :meth:`images_forward_backward`, then the bucketed gradient all-reduce over the trainable runs of the flat buffer
        (VAE segments included; never-graded ones, like frozen ones, are not exchanged), the joint clip over all trained parameters,
        AdamW + EMA and the in-place re-pack of the UNet's and the encoder's kernel-layout weights.  With a frozen autoencoder
        (``pipeline.vae.requires_grad_(False)``): encode -> sample -> add_noise -> :meth:`step`, i.e. today's step.
        ``noise`` / ``posterior_noise``: (B, latent, H/8, W/8); the posterior noise is drawn on the device when None.
        With an attached sampler (``attach_sampler``) ``timesteps``, ``noise`` and ``posterior_noise`` may be None: the sampler draws the
        posterior noise first (``randn``), then noise and timesteps, each consuming one of its steps."""
        check_training_images(self.vae, images)
        vae, sampler = self.vae, self.sampler
        if sampler is not None and (timesteps is None or noise is None):
            nlev = len(vae.config.block_out_channels)
            shape = (images.shape[0], vae.config.latent_channels, images.shape[2] >> (nlev - 1), images.shape[3] >> (nlev - 1))
            if posterior_noise is None:
                posterior_noise = sampler.randn(shape)
            if not self._vae_trains:
                latents = vae.encode(images).latent_dist.sample(noise=posterior_noise, scale=float(vae.config.scaling_factor))
                nz, timesteps, noisy = sampler.sample(latents, timesteps=timesteps)
                if noise is not None:       # the caller's noise with drawn timesteps
                    nz = noise.to(device=latents.device, dtype=torch.float32)
                    noisy = self.scheduler.add_noise(latents, nz, timesteps)
                return self.step(noisy, timesteps, latents, nz, class_labels, unconditional=unconditional, lr=lr, group=group,
                                 overlap=overlap, bucket_bytes=bucket_bytes)
            nz, ts = sampler.sample_noise(shape)
            noise = nz if noise is None else noise
            timesteps = ts if timesteps is None else timesteps
        if not self._vae_trains:
            sf = float(vae.config.scaling_factor)
            latents = vae.encode(images).latent_dist.sample(noise=posterior_noise, scale=sf)
            nz = noise.to(device=latents.device, dtype=torch.float32)
            noisy = self.scheduler.add_noise(latents, nz, timesteps)
            return self.step(noisy, timesteps, latents, nz, class_labels, unconditional=unconditional, lr=lr, group=group,
                             overlap=overlap, bucket_bytes=bucket_bytes)
        import torch.distributed as dist
        self._uncond = bool(unconditional)
        loss, _ = self.images_forward_backward(images, timesteps, noise, class_labels, posterior_noise)
        world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
        if world > 1 or self.force_collectives:
            # the buckets are exchanged once both backward plans have run (the overlapped schedule of `step` follows ONE plan's launches)
            from .training import allreduce_mean_ranges_
            allreduce_mean_ranges_(self.opt.grad, self.opt.trainable_ranges(), group, bucket_bytes=bucket_bytes)
        self._optimizer_step(lr)
        self.refresh_weights()
        return loss
