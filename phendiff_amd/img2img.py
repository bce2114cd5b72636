"""DDIB class transfer: DDIM inversion under the original class -> denoising under the target class.

Mirrors ``src/utils_Img2Img.py``: ``_inversion`` (``:763-800``), ``_ddib`` (``:566-612``), the binary
class swap and batch sharding of ``perform_class_transfer_experiment`` (``:307-317,341-345``).

Two execution modes, same arithmetic:
  * eager  -- this module: ``inversion`` / ``ddib`` walk the reference's Python loops over the drop-in objects;
  * graph  -- ``trajectories.py``: :class:`~phendiff_amd.trajectories.DDIBGraph` captures the whole 2*S-step trajectory (time/class
    embedding table, 2*S UNet evaluations, 2*S fused scheduler updates, post-processing) into ONE hipGraph and replays it per batch.
``tiled_inversion`` / ``tiled_ddib`` / ``tiled_inverted_regeneration`` run the same trajectories on a canvas larger than the size the model
was trained at (``tiling.py``: overlapping tiles through the UNet, blended into one model output per step); captured:
:class:`~phendiff_amd.trajectories.TiledDDIBGraph`.
The gradient-guided transfer (``:651-760``) has the same two modes: ``custom_guided_generation`` here, ``GuidedTransferGraph`` /
``SDGuidedTransferGraph`` there; what both need to build a step's ``pd_lp_guidance`` arguments (:class:`_LpGuidance`) lives here.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import List, Optional

import torch

from . import _lib as L
from .pipeline import ConditionalDDIMPipeline, require_pil_channels
from .schedulers import (MULTISTEP_NOT_GUIDED, MULTISTEP_NOT_LATENT, MULTISTEP_NOT_TILED, THRESHOLDING_NOT_GUIDED, THRESHOLDING_NOT_LATENT,
                         DDIMInverseScheduler, check_guidance_rescale, inverse_scheduler, quantile_rank, refuse_multistep,
                         refuse_thresholding)


@torch.no_grad()
def inversion(pipe, input_images: torch.Tensor, class_labels: torch.Tensor, num_inference_steps: int,
              proc_idx: Optional[int] = None, variant: str = "0.18.2") -> torch.Tensor:
    """``_inversion`` (utils_Img2Img.py:763-800)."""
    from .sd_pipeline import CustomStableDiffusionImg2ImgPipeline
    if isinstance(pipe, CustomStableDiffusionImg2ImgPipeline):
        refuse_multistep(pipe.scheduler, "inversion with a latent-diffusion pipeline", MULTISTEP_NOT_LATENT)
    gauss = input_images.clone().detach()
    inv = inverse_scheduler(pipe.scheduler, variant)      # (the eager counterpart of trajectories._schedules)
    inv.set_timesteps(num_inference_steps)
    for t in inv.timesteps:
        model_output = pipe.unet(gauss, t, class_labels).sample
        gauss = inv.step(model_output, t, gauss).prev_sample
    return gauss


@torch.no_grad()
def encode_to_latents(pipe, images: torch.Tensor, generator=None) -> torch.Tensor:
    """``_encode_to_latents`` (utils_Img2Img.py:827-836): ``vae.encode(x).latent_dist.sample() * scaling_factor`` (the scale
    is folded into the sampling kernel)."""
    return pipe.vae.encode(images).latent_dist.sample(generator, scale=float(pipe.vae.config.scaling_factor))


@torch.no_grad()
def decode_to_images(pipe, latents: torch.Tensor) -> torch.Tensor:
    """``_decode_to_images`` (utils_Img2Img.py:839-847)."""
    return pipe.vae.decode(latents / pipe.vae.config.scaling_factor, return_dict=False)[0]


@torch.no_grad()
def LDM_preprocess(pipe, images: torch.Tensor, class_labels_seq=None, generator=None):
    """``_LDM_preprocess`` (utils_Img2Img.py:803-824): images -> scaled latents, each label tensor -> (B, 77, D) embedding."""
    from .sd_pipeline import hack_class_embedding
    latents = encode_to_latents(pipe, images, generator)
    if class_labels_seq is None:
        return latents, None
    embeds = [hack_class_embedding(pipe._encode_class(class_labels=cl, device=latents.device, do_classifier_free_guidance=False))
              for cl in class_labels_seq]
    return latents, embeds


@torch.no_grad()
def ddib(pipe, clean_images, orig_class_labels, target_class_labels, num_inference_steps: int,
         process_idx: Optional[int] = None, variant: str = "0.18.2", output_type: str = "numpy", generator=None):
    """``_ddib`` (utils_Img2Img.py:566-612), both pipeline branches.  ``generator`` seeds the VAE posterior draw of the
    latent-diffusion branch (the reference draws it unseeded)."""
    from .sd_pipeline import CustomStableDiffusionImg2ImgPipeline
    if isinstance(pipe, CustomStableDiffusionImg2ImgPipeline):
        refuse_thresholding(pipe.scheduler, "ddib with a latent-diffusion pipeline", THRESHOLDING_NOT_LATENT)      # (before the VAE encodes)
        refuse_multistep(pipe.scheduler, "ddib with a latent-diffusion pipeline", MULTISTEP_NOT_LATENT)
        clean_images, [orig_class_cond] = LDM_preprocess(pipe, clean_images, [orig_class_labels], generator)
    elif isinstance(pipe, ConditionalDDIMPipeline):
        require_pil_channels(clean_images.shape[1], output_type)      # (before the inversion: half of the trajectory)
        orig_class_cond = orig_class_labels
    else:
        raise NotImplementedError(type(pipe))
    inverted_gauss = inversion(pipe, clean_images, orig_class_cond, num_inference_steps, process_idx, variant)
    if isinstance(pipe, ConditionalDDIMPipeline):
        return pipe(class_labels=target_class_labels, w=0, num_inference_steps=num_inference_steps,
                    start_image=inverted_gauss, add_forward_noise_to_image=False, frac_diffusion_skipped=0,
                    output_type=output_type).images
    return pipe(image=inverted_gauss, class_labels=target_class_labels, strength=1, add_forward_noise_to_image=False,
                num_inference_steps=num_inference_steps, guidance_scale=0,     # guidance_scale <= 1.0 disables guidance
                output_type={"numpy": "np"}.get(output_type, output_type))


@torch.no_grad()
def inverted_regeneration(pipe, clean_images, orig_class_labels, num_inference_steps: int, **kw):
    """``"inverted_regeneration"`` (utils_Img2Img.py:374-384): DDIB with the original class as target."""
    return ddib(pipe, clean_images, orig_class_labels, orig_class_labels, num_inference_steps, **kw)


# ---- tiled trajectories: a field of view larger than the training size -------------------------------------------------------------------
class TiledTransferOutput(SimpleNamespace):
    """What a tiled transfer returns: ``.images`` (NHWC float in [0, 1]), ``.images_u8`` (its ``uint8`` quantisation), ``.inverted`` (the
    canvas at the end of the inversion) and ``.sample`` (the canvas at the end of the transfer, in the model's range: what
    ``ImagePreprocessor.restore`` takes) -- the last two NCHW on the device."""


def _check_tiled_request(pipe, canvas_shape, who: str):
    """What a tiled trajectory refuses before it packs a weight, builds a plan or launches anything."""
    from .sd_pipeline import CustomStableDiffusionImg2ImgPipeline
    if isinstance(pipe, CustomStableDiffusionImg2ImgPipeline):
        raise NotImplementedError(f"{who}: tiled trajectories run in image space (ConditionalDDIMPipeline); the latent tier is not tiled")
    if not isinstance(pipe, ConditionalDDIMPipeline):
        raise NotImplementedError(f"{who}: {type(pipe).__name__} (a ConditionalDDIMPipeline is needed; the gradient-guided transfer is not tiled)")
    if len(canvas_shape) != 4:
        raise ValueError(f"{who}: expected (B, C, H, W) images, got {tuple(canvas_shape)}")
    refuse_multistep(pipe.scheduler, who, MULTISTEP_NOT_TILED)
    c, u = pipe.scheduler.config, pipe.unet.config
    if u.in_channels != u.out_channels or canvas_shape[1] != u.in_channels:
        raise ValueError(f"{who}: {canvas_shape[1]}-channel images for a model with in_channels = {u.in_channels}, out_channels = "
                         f"{u.out_channels} (the blended model output updates the canvas: all three must agree)")
    if getattr(c, "thresholding", False):      # the quantile of a step is taken over the whole image, not per tile
        n = int(canvas_shape[1]) * int(canvas_shape[2]) * int(canvas_shape[3])
        try:
            quantile_rank(n, float(c.dynamic_thresholding_ratio))
        except ValueError as e:
            raise ValueError(f"{who}: thresholding=True takes the quantile of a step over the whole {tuple(canvas_shape[1:])} canvas: {e}") from None


def tile_conditioning(cond: torch.Tensor, tiles_per_image: int) -> torch.Tensor:
    """A batch's class conditioning (labels, label values or embedding rows) per tile: a tile carries its image's class."""
    return cond.repeat_interleave(tiles_per_image, dim=0)


class _TiledForward:
    """One evaluation of the UNet over a canvas, for the eager loop and the captured one: ``pd_tile_gather`` of all ``T = B * nty * ntx``
    tiles into ``tiles_in``, the launch plan over chunks of ``tile_batch`` tiles (default ``min(T, unet.max_batch(th, tw))``; a short last
    chunk runs on a second plan of its own size, so no slot is ever padded), ``pd_tile_blend`` of ``tiles_out`` into the model output.
    ``bind(canvas, model_out)`` fixes the two canvas-sized tensors; ``evaluate(temb_ptr, st)`` launches, ``temb_ptr``: the [T][proj_dim]
    projection table of the step (tile order: image, then ky, then kx)."""

    def __init__(self, unet, grid, batch_size: int, tile_batch, device, private_plan: bool = False):
        self.lib, self.grid, self.B = L.lib(), grid, batch_size
        self.T = T = batch_size * grid.tiles_per_image
        most = unet.max_batch(grid.th, grid.tw)
        tb = min(T, most) if tile_batch is None else int(tile_batch)
        if not 1 <= tb <= most:
            raise ValueError(f"tile_batch {tile_batch}: one launch plan holds 1 to {most} tiles of {grid.th}x{grid.tw}")
        self.tile_batch = tb = min(tb, T)
        self.chunks = [(first, min(tb, T - first)) for first in range(0, T, tb)]
        make = unet.new_plan if private_plan else unet.plan_for
        self.plans = {n: make(n, grid.th, grid.tw, device) for n in sorted({n for _, n in self.chunks}, reverse=True)}
        self.plan = self.plans[tb]
        ch = unet.config.in_channels
        self.tiles_in = torch.empty((T, ch, grid.th, grid.tw), dtype=torch.float32, device=device)
        self.tiles_out = torch.empty_like(self.tiles_in)
        self.tile_bytes, self.row_bytes = 4 * ch * grid.th * grid.tw, 4 * self.plan.w.proj_dim
        self.gather_args = self.blend_args = None

    def bind(self, canvas: torch.Tensor, model_out: torch.Tensor):
        self.gather_args = self.grid.gather_args(canvas, self.tiles_in)
        self.blend_args = self.grid.blend_args(self.tiles_out, model_out)
        self._bound = (canvas, model_out)
        return self

    def evaluate(self, temb_ptr: int, st: int):
        L.check(self.lib.pd_tile_gather(C.byref(self.gather_args), st), "pd_tile_gather")
        src, dst = self.tiles_in.data_ptr(), self.tiles_out.data_ptr()
        for first, count in self.chunks:
            self.plans[count].run(src + first * self.tile_bytes, temb_ptr + first * self.row_bytes, dst + first * self.tile_bytes, st)
        L.check(self.lib.pd_tile_blend(C.byref(self.blend_args), st), "pd_tile_blend")


class _TiledEager:
    """The eager tiled loop: the canvas ``x`` (updated in place), the blended ``model_out`` and :class:`_TiledForward` between them."""

    def __init__(self, pipe, images: torch.Tensor, tile, overlap, tile_batch, who: str):
        from .tiling import TileGrid
        _check_tiled_request(pipe, images.shape, who)
        self.pipe, unet = pipe, pipe.unet
        B, _, H, W = images.shape
        self.grid = TileGrid(H, W, tile, default_overlap(tile) if overlap is None else overlap)
        if not images.is_cuda:
            raise L.PhenDiffHipError("phendiff_amd runs on MI355X only (no CPU fallback): move the inputs to 'cuda'")
        self.x = images.detach().to(torch.float32).contiguous().clone()
        self.model_out = torch.empty_like(self.x)
        self.dev = self.x.device
        self.fwd = _TiledForward(unet, self.grid, B, tile_batch, self.dev).bind(self.x, self.model_out)
        T = self.fwd.T
        self.ts = torch.empty((T,), dtype=torch.float32, device=self.dev)
        self.temb = torch.empty((T, self.fwd.plan.w.proj_dim), dtype=torch.float32, device=self.dev)
        self.label_dtype = torch.int64 if unet.config.class_embed_type is None else torch.float32

    def steps(self, sched, timesteps, class_labels: torch.Tensor):
        """Per timestep: the tiled UNet evaluation under ``class_labels`` (one entry per image), then the scheduler's own update of the
        canvas -- ``pd_ddim_step``, or the launches of ``threshold_step`` where the scheduler thresholds (quantile over the whole image)."""
        fwd, x, out = self.fwd, self.x, self.model_out
        st = torch.cuda.current_stream(self.dev).cuda_stream
        labels = tile_conditioning(class_labels.to(device=self.dev, dtype=self.label_dtype), self.grid.tiles_per_image).contiguous()
        for t in timesteps:
            self.ts.fill_(float(t))
            fwd.plan.temb_rows(self.ts, labels, None, st, rows=fwd.T, out=self.temb)
            fwd.evaluate(self.temb.data_ptr(), st)
            if getattr(sched.config, "thresholding", False):
                sched.threshold_step(t, x, out, x, st).enqueue(st)
            else:
                L.check(fwd.lib.pd_ddim_step(C.byref(sched.ddim_step_args(t, x, out, x)), st), "pd_ddim_step")

    def invert(self, class_labels, num_inference_steps: int, variant: str):
        inv = DDIMInverseScheduler.from_config(self.pipe.scheduler.config, variant=variant)
        inv.set_timesteps(num_inference_steps)
        self.steps(inv, inv.timesteps, class_labels)

    def generate(self, class_labels, num_inference_steps: int):
        fwd = self.pipe.scheduler
        fwd.set_timesteps(num_inference_steps)
        self.steps(fwd, fwd.timesteps, class_labels)      # (frac_diffusion_skipped = 0: every timestep, pipeline :250-258)

    def postproc(self):
        """``(x / 2 + .5).clamp(0, 1)`` NCHW -> NHWC, float and uint8, in one ``pd_postproc``."""
        B, Cc, H, W = self.x.shape
        f32 = torch.empty((B, H, W, Cc), dtype=torch.float32, device=self.dev)
        u8 = torch.empty((B, H, W, Cc), dtype=torch.uint8, device=self.dev)
        a = L.PostprocArgs(B=B, C=Cc, H=H, W=W, x=self.x.data_ptr(), out_f32=f32.data_ptr(), out_u8=u8.data_ptr())
        L.check(self.fwd.lib.pd_postproc(C.byref(a), torch.cuda.current_stream(self.dev).cuda_stream), "pd_postproc")
        return f32, u8


def default_overlap(tile):
    """An eighth of the tile on each axis (256 -> 32), what the tiled functions take when no overlap is given."""
    return tuple(int(t) // 8 for t in tile) if isinstance(tile, (tuple, list)) else int(tile) // 8


@torch.no_grad()
def tiled_inversion(pipe, input_images: torch.Tensor, class_labels: torch.Tensor, num_inference_steps: int, tile, overlap=None,
                    tile_batch: Optional[int] = None, variant: str = "0.18.2") -> torch.Tensor:
    """:func:`inversion` of a canvas larger than the training size (``ConditionalDDIMPipeline`` only): at every step the UNet evaluates
    the overlapping ``tile`` x ``tile`` tiles of the canvas (:class:`~phendiff_amd.tiling.TileGrid`; ``overlap`` defaults to an eighth of
    the tile), their outputs are blended into one canvas-sized model output and the inverse scheduler steps on the canvas.  ``tile_batch``:
    tiles per launch-plan call (default: all of them, up to ``unet.max_batch``); the result does not depend on it.  On a canvas of one
    tile this is :func:`inversion`, bit for bit."""
    run = _TiledEager(pipe, input_images, tile, overlap, tile_batch, "tiled_inversion")
    run.invert(class_labels, num_inference_steps, variant)
    return run.x


@torch.no_grad()
def tiled_ddib(pipe, clean_images: torch.Tensor, orig_class_labels: torch.Tensor, target_class_labels: torch.Tensor,
               num_inference_steps: int, tile, overlap=None, tile_batch: Optional[int] = None, variant: str = "0.18.2",
               output_type: str = "numpy") -> TiledTransferOutput:
    """:func:`ddib` of a canvas larger than the training size, tiled as in :func:`tiled_inversion`: inversion under the original class,
    denoising under the target class.  With ``thresholding=True`` the forward scheduler takes its quantile over the whole image (a canvas
    above ``quantile_rank``'s 16 000 000 elements is refused before anything is launched).  ``output_type``: "numpy" (host arrays, as
    :func:`ddib` returns them) or "pt" (device tensors); ``.inverted`` stays on the device either way."""
    if output_type not in ("numpy", "pt"):
        raise ValueError(f'output_type must be "numpy" or "pt", got {output_type!r}')
    run = _TiledEager(pipe, clean_images, tile, overlap, tile_batch, "tiled_ddib")
    run.invert(orig_class_labels, num_inference_steps, variant)
    inverted = run.x.clone()
    run.generate(target_class_labels, num_inference_steps)
    images, images_u8 = run.postproc()
    if output_type == "numpy":
        images, images_u8 = images.cpu().numpy(), images_u8.cpu().numpy()
    return TiledTransferOutput(images=images, images_u8=images_u8, inverted=inverted, sample=run.x)


@torch.no_grad()
def tiled_inverted_regeneration(pipe, clean_images, orig_class_labels, num_inference_steps: int, tile, **kw) -> TiledTransferOutput:
    """:func:`inverted_regeneration` of a canvas: :func:`tiled_ddib` with the original class as target."""
    return tiled_ddib(pipe, clean_images, orig_class_labels, orig_class_labels, num_inference_steps, tile, **kw)


@torch.no_grad()
def classifier_free_guidance_forward_start(pipe, clean_images, target_class_labels, guidance_scale: float,
                                           frac_diffusion_skipped: float, num_inference_steps: int, generator=None,
                                           output_type: str = "numpy", guidance_rescale: float = 0.0):
    """``_classifier_free_guidance_forward_start`` (utils_Img2Img.py:615-648), both pipeline branches: noise
    the image up to ``(1 - frac_diffusion_skipped)`` of the trajectory, then denoise under the target class with
    classifier-free guidance.  ``guidance_rescale``: the pipelines' argument (0 = off)."""
    from .sd_pipeline import CustomStableDiffusionImg2ImgPipeline
    check_guidance_rescale(guidance_rescale, "classifier_free_guidance_forward_start")
    if isinstance(pipe, CustomStableDiffusionImg2ImgPipeline):       # :638-645: strength = frac_diffusion_skipped
        refuse_multistep(pipe.scheduler, "classifier_free_guidance_forward_start with a latent-diffusion pipeline", MULTISTEP_NOT_LATENT)
        return pipe(image=clean_images, class_labels=target_class_labels, strength=frac_diffusion_skipped,
                    num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, generator=generator,
                    output_type={"numpy": "np"}.get(output_type, output_type), guidance_rescale=guidance_rescale)
    return pipe(class_labels=target_class_labels, w=guidance_scale, num_inference_steps=num_inference_steps,
                start_image=clean_images, frac_diffusion_skipped=frac_diffusion_skipped, generator=generator,
                output_type=output_type, guidance_rescale=guidance_rescale).images


# fp16 engine: the factor the Lp loss gradient carries through the UNet backward (`custom_guided_generation`).  |d loss / d x0| of an
# Lp norm is <= 1 per element and ~ numel^-1/2 typically (2e-3 at 256 x 256 x 3): times 2^12 it sits mid-range of fp16 with 2^4 of
# head-room for what the backward adds; a step that overflows anyway halves it.
GUIDANCE_GRAD_SCALE = 4096.0
# ... and is not halved below this, per step here or per trajectory in the captured form (`trajectories._GuidedSteps`)
GUIDANCE_MIN_GRAD_SCALE = 2.0 ** -10


def _check_lp_exponent(p):
    if isinstance(p, str) or not (1.0 <= float(p) < 1e6):
        raise NotImplementedError("Lp guidance: finite p >= 1 only (the reference config uses p = 2)")


class _LpGuidance:
    """What ``pd_lp_guidance`` works with, for the eager loop and the captured one: the two gradients it writes (``d_out`` w.r.t. the
    model output, ``d_direct`` w.r.t. the sample directly), its per-image partial sums, and the arguments of a step."""

    def __init__(self, sched, like: torch.Tensor, model_out: torch.Tensor, target: torch.Tensor, p: float):
        self.sched, self.p, self.model_out, self.target = sched, float(p), model_out, target
        self.d_out, self.d_direct = torch.empty_like(like), torch.empty_like(like)
        self.splits = max(1, min(64, like[0].numel() // 4096))
        self.partial = torch.empty(like.shape[0] * self.splits, dtype=torch.float64, device=like.device)
        self.sizes = dict(numel=like.numel(), per_sample=like[0].numel())      # (the fields `GuidedStepArgs` shares, with step_fields)

    def args(self, t, sample: torch.Tensor, losses: torch.Tensor) -> L.LpGuidanceArgs:
        fields = self.sched.step_fields(t)      # x0 is DDIMScheduler.step's: its prediction type, clamp and level; not the update's half
        del fields["sqrt_ap"], fields["dir_coef"]
        return L.LpGuidanceArgs(p=self.p, sample=sample.data_ptr(), model_out=self.model_out.data_ptr(),
                                target=self.target.data_ptr(), partial=self.partial.data_ptr(), splits=self.splits,
                                d_model_out=self.d_out.data_ptr(), d_sample_direct=self.d_direct.data_ptr(), losses=losses.data_ptr(),
                                **fields, **self.sizes)


@torch.no_grad()
def custom_guided_generation(pipe, input_images: torch.Tensor, target_class_labels: torch.Tensor, p: float,
                             guidance_loss_scale: float, num_inference_steps: int, return_losses: bool = False):
    """``_custom_guided_generation`` (utils_Img2Img.py:699-760), both pipeline branches (latent diffusion: ``input_images`` are latents,
    ``target_class_labels`` the (B, 77, D) class embeddings, :663-671).  Per step: UNet forward
    (statistics kept), ``x0 = scheduler.step(...).pred_original_sample``, per-image ``Lp_loss(x0, input_images, p)``
    (``:245-270``), its gradient w.r.t. the image THROUGH the UNet (what ``torch.autograd.grad(losses_seq, images)`` returns:
    ``pd_lp_guidance`` -> input-gradient-only UNet backward), ``images -= guidance_loss_scale * grad``, then the scheduler
    step with the model output computed before the push.  No autograd graph exists: the backward is the HIP plan.

    fp16 engine (the reference runs this method under ``mixed_precision: fp16``, general_config.yaml:46 -- there autocast keeps the
    gradient in fp32 where it can; here every activation gradient is fp16): the Lp loss gradient enters the backward times a static
    power-of-two scale (:data:`GUIDANCE_GRAD_SCALE`, the role accelerate's GradScaler plays in training) and the image gradient is
    un-scaled before the ``guidance_loss_scale`` push; a step whose gradient is not finite halves the scale and is redone (one host
    read per step; the scale reached is kept for the following steps)."""
    from .sd_pipeline import CustomStableDiffusionImg2ImgPipeline
    ldm = isinstance(pipe, CustomStableDiffusionImg2ImgPipeline)
    if not ldm and not isinstance(pipe, ConditionalDDIMPipeline):
        raise NotImplementedError(type(pipe))
    refuse_thresholding(pipe.scheduler, "custom_guided_generation", THRESHOLDING_NOT_GUIDED)
    refuse_multistep(pipe.scheduler, "custom_guided_generation", MULTISTEP_NOT_GUIDED)
    if not input_images.is_cuda:
        raise L.PhenDiffHipError("phendiff_amd runs on MI355X only (no CPU fallback): move the inputs to 'cuda'")
    _check_lp_exponent(p)
    lib = L.lib()
    unet, sched = pipe.unet, pipe.scheduler
    dev = input_images.device
    B, _, H, W = input_images.shape
    st = torch.cuda.current_stream(dev).cuda_stream
    target = input_images.detach().contiguous().float()
    images = target.clone()
    if ldm:
        # latent-diffusion branch (:718-726): `target_class_labels` IS the (B, 77, D) class embedding `_LDM_preprocess` made, handed to
        # `pipe.unet(images, t, target_class_embeds)` as encoder_hidden_states; `images` are latents
        ehs = target_class_labels.to(device=dev, dtype=torch.float32).contiguous()
        if ehs.ndim != 3 or ehs.shape[0] != B:
            raise ValueError(f"latent-diffusion branch: target_class_labels must be the (B, tokens, D) class embeddings, got {tuple(ehs.shape)}")
        plan = unet.input_grad_plan(B, H, W, ehs.shape[1], dev)
        run_forward = lambda ts: plan.forward(images, ts, ehs, model_out, st)
    else:
        labels = target_class_labels.to(device=dev, dtype=torch.int64).contiguous()
        plan = unet.input_grad_plan(B, H, W, dev)
        run_forward = lambda ts: plan.forward(images, ts, labels, None, model_out, st)
    model_out, pushed = torch.empty_like(images), torch.empty_like(images)
    lp = _LpGuidance(sched, images, model_out, target, p)
    d_out, d_direct = lp.d_out, lp.d_direct
    fp16 = getattr(unet, "compute_dtype", None) == "fp16"
    gscale = float(GUIDANCE_GRAD_SCALE) if fp16 else 1.0
    d_scaled = torch.empty_like(images) if fp16 else None
    losses = torch.empty(B, dtype=torch.float32, device=dev)
    all_losses = []
    sched.set_timesteps(num_inference_steps)
    for t in sched.timesteps:
        ts = torch.full((B,), float(t), dtype=torch.float32, device=dev)
        a = lp.args(t, images, losses)
        while True:
            run_forward(ts)
            L.check(lib.pd_lp_guidance(C.byref(a), st), "pd_lp_guidance")
            if not fp16:
                plan.backward(d_out, st)
                break
            torch.mul(d_out, gscale, out=d_scaled)
            plan.backward(d_scaled, st)
            if bool(torch.isfinite(plan.dsample).all()):       # (the one host read of an fp16 step)
                plan.dsample.mul_(1.0 / gscale)
                break
            gscale *= 0.5                                       # overflow somewhere in the fp16 chain: halve and redo the step
            if gscale < GUIDANCE_MIN_GRAD_SCALE:
                raise FloatingPointError("gradient-guided transfer (fp16): the UNet input gradient is not finite at any scale")
        g = L.GuidanceApplyArgs(numel=images.numel(), scale=float(guidance_loss_scale), x=images.data_ptr(),
                                g_direct=d_direct.data_ptr(), g_unet=plan.dsample.data_ptr(), out=pushed.data_ptr())
        L.check(lib.pd_guidance_apply(C.byref(g), st), "pd_guidance_apply")
        images = sched.step(model_out, t, pushed).prev_sample
        if return_losses:
            all_losses.append(losses.clone())
    return (images, all_losses) if return_losses else images


@torch.no_grad()
def linear_interp_custom_guidance_inverted_start(pipe, clean_images, orig_class_labels, target_class_labels, p: float,
                                                 guidance_loss_scale: float, num_inference_steps: int,
                                                 variant: str = "0.18.2", output_type: str = "numpy", generator=None):
    """``_linear_interp_custom_guidance_inverted_start`` (utils_Img2Img.py:651-696), both pipeline branches (``generator`` seeds the
    VAE posterior draw of the latent-diffusion branch; the reference draws it unseeded): inversion under the original class,
    then gradient-guided generation under the target class (``p`` / ``guidance_loss_scale``: the method's config keys,
    defaults 2 / 0.001).  ``output_type``: "pt" = the [-1, 1] tensor the reference hands to ``tensor_to_PIL``; "numpy" =
    NHWC float in [0, 1]; "pil"."""
    from .sd_pipeline import CustomStableDiffusionImg2ImgPipeline
    ldm = isinstance(pipe, CustomStableDiffusionImg2ImgPipeline)
    target_cond = target_class_labels
    refuse_thresholding(pipe.scheduler, "the gradient-guided transfer", THRESHOLDING_NOT_GUIDED)      # (before the inversion half)
    refuse_multistep(pipe.scheduler, "the gradient-guided transfer", MULTISTEP_NOT_GUIDED)
    if not ldm:
        require_pil_channels(clean_images.shape[1], output_type)
    if ldm:      # :663-671: images -> latents, both label tensors -> 77-token class embeddings
        clean_images, (orig_class_labels, target_cond) = LDM_preprocess(pipe, clean_images, [orig_class_labels, target_class_labels], generator)
    inverted = inversion(pipe, clean_images, orig_class_labels, num_inference_steps, None, variant)
    image = custom_guided_generation(pipe, inverted, target_cond, p, guidance_loss_scale, num_inference_steps)
    if ldm:      # :689-695: decode, then min-max renormalisation back to [-1, 1]
        image = decode_to_images(pipe, image)
        image = image - image.min()
        image = image / image.max()
        image = image * 2 - 1
    if output_type == "pt":
        return image
    arr = (image / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).cpu().numpy()
    return pipe.numpy_to_pil(arr) if output_type == "pil" else arr


@torch.no_grad()
def tensor_to_PIL(tensor: torch.Tensor, channel="mean"):
    """``tensor_to_PIL`` (utils_Img2Img.py:96-150): (N, 3, H, W) images in [-1, 1] -> RGB PIL images through ``pd_postproc``
    (``uint8 = round(255 * clamp(x/2 + 1/2, 0, 1))`` on the device); (N, 4, h, w) latents -> global min-max normalisation, then
    one channel or the channel mean as a greyscale image (visualisation only).  One image is returned bare, like the reference."""
    from PIL import Image
    assert tensor.ndim == 4, "Expecting a tensor of shape (N, C, H, W)"
    assert channel in ["mean"] + list(range(tensor.shape[1])), \
        f"Expecting a channel in {list(range(tensor.shape[1]))} or 'mean', got {channel}"
    if tensor.shape[1] == 4:
        img = tensor.detach().float().clone()
        img -= img.min()
        img /= img.max()
        img = img.clamp(0, 1)
        img = img[:, channel:channel + 1] if isinstance(channel, int) else img.mean(dim=1, keepdim=True)
        arr = (img.cpu().permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")
    else:
        assert float(tensor.min()) >= -1 and float(tensor.max()) <= 1, "Expecting values in [-1, 1]"
        x = tensor.detach().contiguous().float()
        if not x.is_cuda:
            raise L.PhenDiffHipError("phendiff_amd runs on MI355X only (no CPU fallback): move the tensor to 'cuda'")
        B, Cc, H, W = x.shape
        out = torch.empty((B, H, W, Cc), dtype=torch.uint8, device=x.device)
        a = L.PostprocArgs(B=B, C=Cc, H=H, W=W, x=x.data_ptr(), out_f32=None, out_u8=out.data_ptr())
        L.check(L.lib().pd_postproc(C.byref(a), torch.cuda.current_stream(x.device).cuda_stream), "pd_postproc")
        arr = out.cpu().numpy()
    if arr.shape[-1] == 1:
        pil = [Image.fromarray(im.squeeze(-1), mode="L") for im in arr]
    else:
        pil = [Image.fromarray(im) for im in arr]
    return pil[0] if len(pil) == 1 else pil


def swap_binary_labels(orig_class_labels: torch.Tensor) -> torch.Tensor:
    """``target = 1 - orig`` (utils_Img2Img.py:343-344): strictly binary datasets."""
    return 1 - orig_class_labels


def shard_batches(num_batches: int, rank: int, world_size: int, even_batches: bool = True) -> List[int]:
    """Batch indices rank ``rank`` processes -- accelerate ``BatchSamplerShard`` semantics as reached through
    ``accelerator.prepare(dataloader)`` (utils_Img2Img.py:316): rank r takes batches r, r+G, r+2G, ...; with
    ``even_batches`` (accelerate's default) the tail is completed by wrapping around to the first batches so
    that every rank runs the same number of iterations.  No collective on the data path."""
    if world_size <= 0 or not 0 <= rank < world_size:
        raise ValueError("bad rank / world_size")
    mine = list(range(rank, num_batches, world_size))
    if even_batches and num_batches > 0:
        # accelerate completes the last round with the samples of the first batches, in order: the k-th filler
        # batch is batch k (mod num_batches) and goes to the rank whose turn it is
        idx, k = num_batches, 0
        while idx % world_size != 0:
            if idx % world_size == rank:
                mine.append(k % num_batches)
            idx += 1
            k += 1
    return mine
