"""DDIB class transfer: DDIM inversion under the original class -> denoising under the target class.

Mirrors ``src/utils_Img2Img.py``: ``_inversion`` (``:763-800``), ``_ddib`` (``:566-612``), the binary
class swap and batch sharding of ``perform_class_transfer_experiment`` (``:307-317,341-345``).

Two execution modes, same arithmetic:
  * eager  -- this module: ``inversion`` / ``ddib`` walk the reference's Python loops over the drop-in objects;
  * graph  -- ``trajectories.py``: :class:`~phendiff_amd.trajectories.DDIBGraph` captures the whole 2*S-step trajectory (time/class
    embedding table, 2*S UNet evaluations, 2*S fused scheduler updates, post-processing) into ONE hipGraph and replays it per batch.
The gradient-guided transfer (``:651-760``) has the same two modes: ``custom_guided_generation`` here, ``GuidedTransferGraph`` /
``SDGuidedTransferGraph`` there; what both need to build a step's ``pd_lp_guidance`` arguments (:class:`_LpGuidance`) lives here.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch

from . import _lib as L
from .pipeline import ConditionalDDIMPipeline, require_pil_channels
from .schedulers import THRESHOLDING_NOT_GUIDED, THRESHOLDING_NOT_LATENT, DDIMInverseScheduler, refuse_thresholding


@torch.no_grad()
def inversion(pipe, input_images: torch.Tensor, class_labels: torch.Tensor, num_inference_steps: int,
              proc_idx: Optional[int] = None, variant: str = "0.18.2") -> torch.Tensor:
    """``_inversion`` (utils_Img2Img.py:763-800)."""
    gauss = input_images.clone().detach()
    inv = DDIMInverseScheduler.from_config(pipe.scheduler.config, variant=variant)
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


@torch.no_grad()
def classifier_free_guidance_forward_start(pipe, clean_images, target_class_labels, guidance_scale: float,
                                           frac_diffusion_skipped: float, num_inference_steps: int, generator=None,
                                           output_type: str = "numpy"):
    """``_classifier_free_guidance_forward_start`` (utils_Img2Img.py:615-648), both pipeline branches: noise
    the image up to ``(1 - frac_diffusion_skipped)`` of the trajectory, then denoise under the target class with
    classifier-free guidance."""
    from .sd_pipeline import CustomStableDiffusionImg2ImgPipeline
    if isinstance(pipe, CustomStableDiffusionImg2ImgPipeline):       # :638-645: strength = frac_diffusion_skipped
        return pipe(image=clean_images, class_labels=target_class_labels, strength=frac_diffusion_skipped,
                    num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, generator=generator,
                    output_type={"numpy": "np"}.get(output_type, output_type))
    return pipe(class_labels=target_class_labels, w=guidance_scale, num_inference_steps=num_inference_steps,
                start_image=clean_images, frac_diffusion_skipped=frac_diffusion_skipped, generator=generator,
                output_type=output_type).images


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
        c = sched.config
        # (the fields `GuidedStepArgs` shares)
        self.common = dict(numel=like.numel(), per_sample=like[0].numel(), pred_type=L.PD_PRED[c.prediction_type],
                           clip=int(bool(c.clip_sample)), clip_range=float(c.clip_sample_range))

    def args(self, t, sample: torch.Tensor, losses: torch.Tensor) -> L.LpGuidanceArgs:
        sa, sb, _, _, _ = self.sched.step_coefficients(t)
        return L.LpGuidanceArgs(sqrt_a=sa, sqrt_b=sb, p=self.p, sample=sample.data_ptr(), model_out=self.model_out.data_ptr(),
                                target=self.target.data_ptr(), partial=self.partial.data_ptr(), splits=self.splits,
                                d_model_out=self.d_out.data_ptr(), d_sample_direct=self.d_direct.data_ptr(), losses=losses.data_ptr(),
                                **self.common)


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
