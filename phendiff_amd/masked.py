"""Masked class transfer: a transfer that keeps what has nothing to do with the phenotype -- the DiffEdit recipe (Couairon et al., arXiv
2210.11427; diffusers' ``StableDiffusionDiffEditPipeline``) on the pixel tier (``ConditionalDDIMPipeline``).

  1. **Where do the two classes disagree?**  :func:`class_contrast_mask`: noise the image to a middle level, evaluate the UNet under the
     target and under the source class, average ``|eps_target - eps_source|`` over channels and ``num_maps`` noise draws
     (``pd_class_contrast``, one launch per draw), then saturate at ``threshold_ratio`` times the per-sample mean, rescale to [0, 1] and
     binarise at 0.5 (``pd_contrast_mask``).
  2. **Transfer only there.**  :func:`masked_ddib` (eager) / :class:`MaskedDDIBGraph` (captured): DDIB whose inversion keeps its states;
     after every denoising step the state the inversion had at the same level is put back outside the mask (``pd_mask_blend``: a
     selection).  At the last step that state is the input image itself, so outside the mask the result IS the input, bit for bit.

The mean of a map is taken PER SAMPLE (diffusers takes ``.mean()`` over the whole batch; equal at B = 1): a sample's mask is a function of
that sample alone, like everything else here.

``refine=dict(...)`` (the parameters of :class:`~phendiff_amd.mask_ops.MaskRefine`: ``close``, ``open``, ``fill_holes``, ``min_area``,
``dilate``, ``connectivity``) cleans the mask up on the device before it is used: a per-pixel contrast mask is a thresholded noise
difference, with specks on the background, pin-holes inside cells and ragged outlines.  ``.mask`` is then the refined mask, ``.raw_mask``
what the refinement read and ``.refine_stats`` its stats; with ``refine=None`` the launches are exactly those without it.

Out of scope: the latent tier, the tiled and the gradient-guided transfers, classifier-free guidance during the masked generation, soft
(fractional) masks and feathered blends.  Refused before anything is packed or launched: ``DPMSolverMultistep*`` schedulers
(:data:`~phendiff_amd.schedulers.MULTISTEP_NOT_MASKED`), the latent-diffusion pipeline, batches beyond ``unet.max_batch`` (no sliced form), a
mask of the wrong shape, dtype or device, ``num_maps < 1``, ``threshold_ratio <= 0``, ``refine`` parameters ``MaskRefine.check_params``
refuses.
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import torch

from . import _lib as L
from .mask_ops import MaskRefine
from .noise import DeviceNoise
from .pipeline import ConditionalDDIMPipeline, numpy_to_pil, require_pil_channels
from .schedulers import MULTISTEP_NOT_MASKED, randn_tensor, refuse_multistep
from .trajectories import _check_shape, _PixelTrajectory, _sample_hw, _schedules

CONTRAST_MASK_CHUNK = L.CONSTANTS["PD_CONTRAST_MASK_CHUNK"]      # the pixels one workgroup reduces: a sample has ceil(H W / this) partials


class MaskedTransferOutput(SimpleNamespace):
    """What :func:`masked_ddib` returns: ``.images`` (as :func:`~phendiff_amd.img2img.ddib` returns them), ``.mask`` ((B, 1, H, W) uint8),
    ``.inverted`` (the end of the inversion) and ``.sample`` (the final state, fp32 NCHW in the model's range) -- the last three on the
    device; ``.map`` / ``.stats`` where the mask was computed here (else None)."""


# ---- host rules ------------------------------------------------------------------------------------------------------------------------------
def blend_state_index(k: int, S: int) -> int:
    """The inversion state put back outside the mask after forward step ``k`` (0-based) of ``S``: ``traj[S - 1 - k]``, where ``traj[0]``
    is the input and ``traj[i]`` the state after ``i`` inverse steps.  Generation starts from ``traj[S]``; forward step ``k`` takes the
    sample from the level of ``traj[S - k]`` to the level of ``traj[S - 1 - k]``, and the last one (``k = S - 1``) to ``traj[0]``, the
    input.  The one place where the rule is written: the eager and the captured form both call it."""
    k, S = int(k), int(S)
    if not 0 <= k < S:
        raise ValueError(f"blend_state_index: forward step {k} outside [0, {S})")
    return S - 1 - k


def encode_timestep(scheduler, num_inference_steps: int, encode_strength: float) -> int:
    """The level the images are noised to for the contrast map -- diffusers' ``get_timesteps`` rule: after
    ``scheduler.set_timesteps(S)``, ``timesteps[S - min(int(S * encode_strength), S)]``.  ``encode_strength`` must lie in (0, 1] and give
    at least one step."""
    S = int(num_inference_steps)
    try:
        strength = float(encode_strength)
    except (TypeError, ValueError):
        strength = math.nan
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"encode_strength must lie in (0, 1], got {encode_strength!r}")
    init = min(int(S * strength), S)
    if init < 1:
        raise ValueError(f"encode_strength = {strength} leaves no step of {S} (int({S} * {strength}) = 0)")
    scheduler.set_timesteps(S)
    return int(scheduler.timesteps[S - init])


def _check_map_request(num_maps, threshold_ratio, who: str):
    if not (isinstance(num_maps, int) and not isinstance(num_maps, bool) and num_maps >= 1):
        raise ValueError(f"{who}: num_maps must be an integer >= 1, got {num_maps!r}")
    try:
        ratio = float(threshold_ratio)
    except (TypeError, ValueError):
        ratio = math.nan
    if not (math.isfinite(ratio) and ratio > 0.0):
        raise ValueError(f"{who}: threshold_ratio must be a finite positive number, got {threshold_ratio!r}")
    return ratio


def _check_refine_request(refine, who: str):
    """``refine`` as the normalised parameters of :class:`MaskRefine` (``None`` stays ``None``); a ``ValueError`` names the entry point."""
    if refine is None:
        return None
    if not isinstance(refine, dict):
        raise ValueError(f"{who}: refine must be a dict of MaskRefine parameters or None, got {type(refine).__name__}")
    try:
        return MaskRefine.check_params(**refine)
    except ValueError as e:
        raise ValueError(f"{who}: refine: {e}") from None


def _check_masked_request(pipe, shape, who: str):
    """What a masked transfer refuses before it packs a weight, builds a plan or launches anything.  ``shape``: (B, C, H, W)."""
    from .sd_pipeline import CustomStableDiffusionImg2ImgPipeline
    if isinstance(pipe, CustomStableDiffusionImg2ImgPipeline):
        raise NotImplementedError(f"{who}: CustomStableDiffusionImg2ImgPipeline -- the masked transfer runs in image space "
                                  "(ConditionalDDIMPipeline); the latent tier is out of scope")
    if not isinstance(pipe, ConditionalDDIMPipeline):
        raise NotImplementedError(f"{who}: {type(pipe).__name__} (a ConditionalDDIMPipeline is needed)")
    refuse_multistep(pipe.scheduler, who, MULTISTEP_NOT_MASKED)
    if len(shape) != 4:
        raise ValueError(f"{who}: expected (B, C, H, W) images, got {tuple(shape)}")
    B, Cc, H, W = (int(v) for v in shape)
    u = pipe.unet.config
    if u.in_channels != u.out_channels or Cc != u.in_channels:
        raise ValueError(f"{who}: {Cc}-channel images for a model with in_channels = {u.in_channels}, out_channels = {u.out_channels}")
    most = pipe.unet.max_batch(H, W)
    if B > most:
        raise ValueError(f"{who}: batch_size {B} exceeds what one launch plan holds at {H}x{W} ({most} images); the masked transfer has "
                         "no sliced form: split the batch")


def check_mask(mask, B: int, H: int, W: int, device, who: str = "mask") -> torch.Tensor:
    """A given mask as the (B, 1, H, W) view the kernels read: (B, 1, H, W) or (B, H, W), ``bool`` or ``uint8``, on ``device``; anything
    else is a ``ValueError``."""
    if not torch.is_tensor(mask):
        raise ValueError(f"{who}: the mask must be a tensor, got {type(mask).__name__}")
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{who}: the mask must be bool or uint8, got {mask.dtype}")
    if tuple(mask.shape) not in ((B, 1, H, W), (B, H, W)):
        raise ValueError(f"{who}: the mask must have shape {(B, 1, H, W)} or {(B, H, W)}, got {tuple(mask.shape)}")
    if mask.device != torch.device(device):
        raise ValueError(f"{who}: the mask lives on {mask.device}, the images on {torch.device(device)}")
    return mask.reshape(B, 1, H, W)


def _require_cuda(t, who):
    if not t.is_cuda:
        raise L.PhenDiffHipError(f"{who}: phendiff_amd runs on MI355X only (no CPU fallback): move the inputs to 'cuda'")


# ---- the three launches --------------------------------------------------------------------------------------------------------------------
def class_contrast_args(a: torch.Tensor, b: torch.Tensor, acc: torch.Tensor, first: bool) -> "L.ClassContrastArgs":
    """``pd_class_contrast`` over two dense fp32 (B, C, H, W) predictions into the dense fp32 (B, 1, H, W) ``acc``."""
    B, Cc, H, W = a.shape
    return L.ClassContrastArgs(B=B, C=Cc, per_pixel=H * W, a=a.data_ptr(), b=b.data_ptr(), acc=acc.data_ptr(), first=int(bool(first)))


class ContrastMask:
    """The launch of ``pd_contrast_mask`` over a dense fp32 (B, 1, H, W) ``acc``: the outputs (``mask`` uint8, ``map`` fp32 -- both
    (B, 1, H, W) -- and ``stats`` (B, 3): mean, limit, masked fraction), the workspace, the argument struct and :meth:`enqueue`.  The
    object holds every tensor the struct points at, so whoever keeps it (a runner's captured graph) keeps the memory it launches into."""

    def __init__(self, acc: torch.Tensor, threshold_ratio: float):
        B, _, H, W = acc.shape
        dev = acc.device
        size = L.lib().pd_contrast_mask_workspace(B, H * W)
        if size == 0:
            raise ValueError(f"contrast mask: no mask over a ({B}, {H * W}) batch")
        self.acc = acc
        self.mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev)
        self.map = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        self.stats = torch.empty((B, 3), dtype=torch.float32, device=dev)
        self.workspace = torch.empty((size // 8,), dtype=torch.float64, device=dev)
        self.args = L.ContrastMaskArgs(B=B, per_pixel=H * W, acc=acc.data_ptr(), ratio=float(threshold_ratio), mask=self.mask.data_ptr(),
                                       map=self.map.data_ptr(), stats=self.stats.data_ptr(), workspace=self.workspace.data_ptr())

    def enqueue(self, st: int):
        L.check(L.lib().pd_contrast_mask(C.byref(self.args), st), "pd_contrast_mask")


def mask_blend_args(x: torch.Tensor, keep: torch.Tensor, mask: torch.Tensor, out: torch.Tensor) -> "L.MaskBlendArgs":
    """``pd_mask_blend`` over dense fp32 (B, C, H, W) tensors and a dense (B, 1, H, W) uint8 mask."""
    B, Cc, H, W = x.shape
    return L.MaskBlendArgs(B=B, C=Cc, per_pixel=H * W, x=x.data_ptr(), keep=keep.data_ptr(), mask=mask.data_ptr(), out=out.data_ptr())


def _as_bytes(mask: torch.Tensor) -> torch.Tensor:
    """A checked mask as dense uint8 (a bool tensor is one byte of 0 / 1 per element: the same memory)."""
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def mask_blend(x: torch.Tensor, keep: torch.Tensor, mask: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """``out = where(mask, x, keep)`` -- one ``pd_mask_blend`` on the current stream, for a hand-written loop.  ``x`` / ``keep``: dense
    fp32 (B, C, H, W) tensors on an MI355X; ``mask``: (B, 1, H, W) or (B, H, W), bool or uint8, broadcast over the channels; ``out``
    (default: a new tensor) may be ``x``.  A selection: a NaN or an infinity on the side not taken does not reach ``out``, and a kept
    element is ``keep``'s bit for bit."""
    if not (torch.is_tensor(x) and torch.is_tensor(keep) and x.dim() == 4):
        raise ValueError("mask_blend: x and keep must be (B, C, H, W) tensors")
    B, Cc, H, W = x.shape
    m = check_mask(mask, B, H, W, x.device, "mask_blend")
    _require_cuda(x, "mask_blend")
    out = torch.empty_like(x) if out is None else out
    for name, t in (("x", x), ("keep", keep), ("out", out)):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(x.shape) or t.device != x.device:
            raise ValueError(f"mask_blend: {name} must be a dense fp32 tensor of x's shape {tuple(x.shape)} on {x.device}")
    a = mask_blend_args(x, keep, _as_bytes(m), out)
    L.check(L.lib().pd_mask_blend(C.byref(a), torch.cuda.current_stream(x.device).cuda_stream), "pd_mask_blend")
    return out


# ---- the mask --------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def class_contrast_mask(pipe, images: torch.Tensor, orig_class_labels: torch.Tensor, target_class_labels: torch.Tensor,
                        num_inference_steps: int = 50, num_maps: int = 10, encode_strength: float = 0.5, threshold_ratio: float = 3.0,
                        generator=None, refine: dict = None) -> SimpleNamespace:
    """Where the model's noise prediction under ``target_class_labels`` differs from the one under ``orig_class_labels`` (DiffEdit's mask;
    diffusers' ``generate_mask``).  Returns a namespace: ``.mask`` (B, 1, H, W) uint8 and ``.map`` (B, 1, H, W) fp32 in [0, 1] on the
    device, ``.stats`` (B, 3) -- per sample the mean of the accumulated contrast, ``threshold_ratio`` times it, and the masked fraction --
    and ``.timestep``, the encode level (:func:`encode_timestep`).

    Draw ``k`` of ``num_maps`` noises the images to that level with ``scheduler.add_noise``: from a :class:`~phendiff_amd.noise.DeviceNoise`
    with the forward-noise purpose at element ``k * C * H * W`` of each image's own stream, so image ``j``'s noise is a function of
    ``(seed, index + j, k)`` alone; from a ``torch.Generator`` (or none) with ``randn_tensor``.  Then two UNet evaluations (target class,
    source class) and one ``pd_class_contrast``; after the last draw one ``pd_contrast_mask``.  The mean is per sample (see the module's
    note).  The ``DeviceNoise`` position is not advanced: draws never do.

    ``refine`` (a dict of :class:`~phendiff_amd.mask_ops.MaskRefine` parameters): the recipe's launches follow ``pd_contrast_mask``;
    ``.mask`` is the refined mask, ``.raw_mask`` the thresholded one and ``.refine_stats`` the recipe's (B, stages, 5) int32 stats (both
    ``None`` without ``refine``; ``.map`` and ``.stats`` always describe the raw mask)."""
    who = "class_contrast_mask"
    shape = tuple(images.shape) if torch.is_tensor(images) else ()
    _check_masked_request(pipe, shape, who)
    ratio = _check_map_request(num_maps, threshold_ratio, who)
    refine = _check_refine_request(refine, who)
    t = encode_timestep(pipe.scheduler, num_inference_steps, encode_strength)
    _require_cuda(images, who)
    x = images.detach().to(torch.float32).contiguous()
    B, Cc, H, W = x.shape
    ts = torch.full((B,), t, dtype=torch.long)
    acc = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    st = torch.cuda.current_stream(x.device).cuda_stream
    for k in range(num_maps):
        if isinstance(generator, DeviceNoise):
            noised = generator.add_noise(pipe.scheduler, x, ts, elem_base=k * Cc * H * W)
        else:
            noised = pipe.scheduler.add_noise(x, randn_tensor(x.shape, generator, x.device), ts)
        eps_target = pipe.unet(noised, t, target_class_labels).sample
        eps_source = pipe.unet(noised, t, orig_class_labels).sample
        L.check(L.lib().pd_class_contrast(C.byref(class_contrast_args(eps_target, eps_source, acc, k == 0)), st), "pd_class_contrast")
    cm = ContrastMask(acc, ratio)
    cm.enqueue(st)
    if refine is None:
        return SimpleNamespace(mask=cm.mask, map=cm.map, stats=cm.stats, timestep=t, raw_mask=None, refine_stats=None)
    r = MaskRefine(B, H, W, x.device, **refine).enqueue(st, cm.mask)
    return SimpleNamespace(mask=r.mask, map=cm.map, stats=cm.stats, timestep=t, raw_mask=cm.mask, refine_stats=r.stats)


# ---- the eager transfer ------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def masked_ddib(pipe, clean_images: torch.Tensor, orig_class_labels: torch.Tensor, target_class_labels: torch.Tensor,
                num_inference_steps: int, mask: torch.Tensor = None, variant: str = "0.18.2", output_type: str = "numpy",
                refine: dict = None, **mask_kw) -> MaskedTransferOutput:
    """:func:`~phendiff_amd.img2img.ddib` that changes the image inside ``mask`` only -- the eager form (the reference-style Python loops
    over the inverse scheduler's and the forward scheduler's ``step``).  ``mask``: (B, 1, H, W) or (B, H, W), bool or uint8, on the images'
    device; ``None`` computes it first with :func:`class_contrast_mask` (``**mask_kw``: ``num_maps``, ``encode_strength``,
    ``threshold_ratio``, ``generator``).  ``refine`` (a dict of :class:`~phendiff_amd.mask_ops.MaskRefine` parameters) cleans the mask up
    -- the computed one or the given one -- before the inversion: the blend reads the refined mask, ``.mask`` is the refined mask,
    ``.raw_mask`` what the refinement read and ``.refine_stats`` its stats (both ``None`` without ``refine``).

    The inversion keeps its states: ``traj[0]`` is the input and ``traj[i]`` the state after ``i`` inverse steps, (S + 1, B, C, H, W)
    fp32 -- ``4 (S + 1) B C H W`` bytes, 1.3 GB at batch 32, S = 50, 3 x 256 x 256.  Generation starts from ``traj[S]``; after forward
    step ``k`` (0-based) ``x = where(mask, x, traj[blend_state_index(k, S)])``, that is ``traj[S - 1 - k]``.  After the last step that
    state is ``traj[0]``: outside the mask the result is the input, bit for bit.

    What the index rule means in noise levels: the state put back was reached by the inversion, the sample around it by the forward
    scheduler.  With the multistep pair the two grids would coincide exactly (those schedulers are refused for another reason: the
    blend invalidates the solver's history).  With DDIM they coincide for ``"leading"`` forward grids; for ``"trailing"`` ones against
    the 0.18.2 inverse grid they are one training timestep apart -- the mismatch plain :func:`~phendiff_amd.img2img.ddib` already lives
    with when it starts the forward scheduler from the inversion's end.

    Returns :class:`MaskedTransferOutput`: ``.images`` as :func:`ddib` returns them (``output_type``: "numpy", "pil", or "pt" for the
    NHWC device tensor), ``.mask``, ``.inverted``, ``.sample``."""
    who = "masked_ddib"
    shape = tuple(clean_images.shape) if torch.is_tensor(clean_images) else ()
    _check_masked_request(pipe, shape, who)
    if output_type not in ("numpy", "pil", "pt"):
        raise ValueError(f'output_type must be "numpy", "pil" or "pt", got {output_type!r}')
    require_pil_channels(shape[1], output_type)
    S = int(num_inference_steps)
    B, Cc, H, W = shape
    info = raw_mask = refine_stats = None
    refine = _check_refine_request(refine, who)
    if mask is None:
        _check_map_request(mask_kw.get("num_maps", 10), mask_kw.get("threshold_ratio", 3.0), who)
    else:
        if mask_kw:
            raise TypeError(f"{who}: {sorted(mask_kw)} configure the computed mask; a mask was given")
        mask = check_mask(mask, B, H, W, clean_images.device, who)
    inv, fwd, inv_ts, gen_ts = _transfer_schedules(pipe, S, variant, who)
    _require_cuda(clean_images, who)
    if mask is None:
        info = class_contrast_mask(pipe, clean_images, orig_class_labels, target_class_labels, S, refine=refine, **mask_kw)
        mask = info.mask      # (it set the forward scheduler to the same S steps: the grid above stands)
        raw_mask, refine_stats = info.raw_mask, info.refine_stats
    mask = _as_bytes(mask)
    if refine is not None and info is None:      # a given mask: refined here, before the inversion
        r = MaskRefine(B, H, W, mask.device, **refine).enqueue(torch.cuda.current_stream(mask.device).cuda_stream, mask)
        raw_mask, mask, refine_stats = mask.view(B, 1, H, W), r.mask, r.stats
    traj = torch.empty((S + 1, B, Cc, H, W), dtype=torch.float32, device=clean_images.device)
    traj[0].copy_(clean_images)
    for i, t in enumerate(inv_ts):
        model_output = pipe.unet(traj[i], t, orig_class_labels).sample
        traj[i + 1].copy_(inv.step(model_output, t, traj[i]).prev_sample)
    x = traj[S].clone()
    for k, t in enumerate(gen_ts):
        model_output = pipe.unet(x, t, target_class_labels).sample
        x = fwd.step(model_output, t, x).prev_sample
        mask_blend(x, traj[blend_state_index(k, S)], mask, out=x)
    images = torch.empty((B, H, W, Cc), dtype=torch.float32, device=x.device)
    a = L.PostprocArgs(B=B, C=Cc, H=H, W=W, x=x.data_ptr(), out_f32=images.data_ptr(), out_u8=None)
    L.check(L.lib().pd_postproc(C.byref(a), torch.cuda.current_stream(x.device).cuda_stream), "pd_postproc")
    if output_type != "pt":
        images = images.cpu().numpy()
        if output_type == "pil":
            images = numpy_to_pil(images)
    return MaskedTransferOutput(images=images, mask=mask.view(B, 1, H, W), inverted=traj[S], sample=x,
                                map=None if info is None else info.map, stats=None if info is None else info.stats, raw_mask=raw_mask,
                                refine_stats=refine_stats)


def _transfer_schedules(pipe, S: int, variant: str, who: str):
    """``trajectories._schedules`` with DDIB's choice of forward timesteps (all of them), and the refusal of two lists that differ in
    length: the blend pairs forward step ``k`` with inversion state ``S - 1 - k``."""
    inv, fwd, inv_ts, gen_ts = _schedules(pipe, S, variant, lambda fwd: fwd.timesteps[fwd.timesteps <= fwd.config.num_train_timesteps * (1 - 0)])
    if len(inv_ts) != len(gen_ts) or len(inv_ts) != S:
        raise ValueError(f"{who}: {len(inv_ts)} inversion steps against {len(gen_ts)} forward steps at num_inference_steps = {S}: the blend "
                         "pairs every forward step with an inversion state")
    return inv, fwd, inv_ts, gen_ts


# ---- the captured transfer ---------------------------------------------------------------------------------------------------------------
class MaskedDDIBGraph(_PixelTrajectory):
    """One hipGraph for the masked transfer of a batch (:func:`masked_ddib`, bit for bit), composed from the phases of
    :class:`~phendiff_amd.trajectories.DDIBGraph`:

      * ``mask="contrast"``: the mask phase first, inside the graph -- per draw ``pd_stream_noise`` (the images' forward noise, from
        ``noise``, a :class:`~phendiff_amd.noise.DeviceNoise`, at the position its state holds when the graph runs) into the working
        buffer, the UNet under the target and under the source class, ``pd_class_contrast``; then ``pd_contrast_mask``.  What
        :func:`class_contrast_mask` ``(generator=noise)`` launches.  The graph's last node is ``pd_stream_advance(batch_size)``.
      * ``mask="given"``: ``run(..., mask=...)`` copies the mask into a static buffer.
      * ``refine=dict(...)``: the launches of :class:`~phendiff_amd.mask_ops.MaskRefine` close the mask phase, inside the graph, over the
        contrast mask or the given one; ``.mask`` is the refined mask (what every blend reads), ``.raw_mask`` what the refinement read,
        ``.refine_stats`` its stats.  ``refine=None``: no launch is added, ``.raw_mask`` and ``.refine_stats`` are ``None``.
      * The inversion WITHOUT snapshots: inverse step ``i`` has the UNet read ``traj[i]`` and ``pd_ddim_step`` write ``traj[i + 1]`` --
        exactly the launches of ``DDIBGraph``'s inversion, on other pointers; ``.inverted`` is ``traj[S]``.  ``traj``:
        (S + 1, B, C, H, W) fp32, ``4 (S + 1) B C H W`` bytes.
      * Generation in the working buffer, started by one copy of ``traj[S]``; after every update (``pd_ddim_step``, or the three launches
        of ``thresholding=True``) one ``pd_mask_blend`` with ``traj[blend_state_index(k, S)]``.  Then ``pd_postproc``.

    ``run(clean_images, orig_class_labels, target_class_labels, mask=None, join=True)`` leaves ``.images`` (NHWC float in [0, 1]),
    ``.images_u8``, ``.inverted``, ``.sample`` (the final state, NCHW), ``.mask`` and -- ``mask="contrast"`` -- ``.map`` and ``.stats``
    on the device.  ``use_graph=False`` enqueues the same launches and gives the same bits."""

    sample = property(lambda self: self.x, doc="the state at the end of the transfer, NCHW in the model's range")

    def __init__(self, pipe: ConditionalDDIMPipeline, batch_size: int, num_inference_steps: int, height: int = None, width: int = None,
                 variant: str = "0.18.2", mask: str = "contrast", noise: DeviceNoise = None, num_maps: int = 10,
                 encode_strength: float = 0.5, threshold_ratio: float = 3.0, use_graph: bool = True, private_plan: bool = False,
                 refine: dict = None):
        who = "MaskedDDIBGraph"
        unet = getattr(pipe, "unet", None)
        channels = getattr(getattr(unet, "config", None), "in_channels", 0)
        H, W = _sample_hw(unet, height, width) if isinstance(pipe, ConditionalDDIMPipeline) else (height, width)
        _check_masked_request(pipe, (batch_size, channels, H, W), who)
        if mask not in ("contrast", "given"):
            raise ValueError(f'{who}: mask must be "contrast" or "given", got {mask!r}')
        S = int(num_inference_steps)
        refine = _check_refine_request(refine, who)
        self.mask_mode, self.noise, self.t_enc = mask, noise, None
        if mask == "contrast":
            ratio = _check_map_request(num_maps, threshold_ratio, who)
            if not isinstance(noise, DeviceNoise):
                raise TypeError(f'{who}: mask="contrast" draws its forward noise inside the graph from a DeviceNoise, not from a {type(noise).__name__}')
            self.t_enc = encode_timestep(pipe.scheduler, S, encode_strength)
        elif noise is not None:
            raise ValueError(f'{who}: mask="given" draws nothing: noise must be None')
        inv, fwd, inv_ts, gen_ts = _transfer_schedules(pipe, S, variant, who)
        if unet.device.type != "cuda":
            raise L.PhenDiffHipError("phendiff_amd runs on MI355X only (no CPU fallback): move the pipeline to 'cuda'")
        super().__init__(pipe, batch_size, S, height, width, None, use_graph, private_plan)
        B, dev, x = self.B, self.device, self.x
        self.inv, self.inv_ts, self.gen_ts = inv, inv_ts, gen_ts
        self.traj = torch.empty((S + 1,) + tuple(x.shape), dtype=torch.float32, device=dev)
        self.inverted = self.traj[S]      # the end of the inversion is the last state the trajectory keeps: no snapshot launch
        self.n_mask = 2 * num_maps if mask == "contrast" else 0      # row blocks of the mask phase: num_maps target, then num_maps source
        self._class_table([self.t_enc] * self.n_mask + inv_ts + gen_ts)
        if mask == "contrast":
            if noise.device != dev:
                raise L.PhenDiffHipError(f"{who}: the DeviceNoise lives on {noise.device}, the pipeline on {dev}")
            per = x[0].numel()
            self.source_out = torch.empty_like(x)
            self.acc = torch.empty((B, 1, self.H, self.W), dtype=torch.float32, device=dev)
            self._sa, self._sb = fwd._per_sample_coefs(torch.tensor([self.t_enc] * B), dev)
            self.noise_args = [noise.launch_args(x, B, per, DeviceNoise.PURPOSE_FORWARD_NOISE, x=self.traj[0], sa=self._sa, sb=self._sb,
                                                 elem_base=k * per) for k in range(num_maps)]
            self.contrast_args = [class_contrast_args(self.model_out, self.source_out, self.acc, k == 0) for k in range(num_maps)]
            self.contrast = ContrastMask(self.acc, ratio)
            self.mask, self.map, self.stats = self.contrast.mask, self.contrast.map, self.contrast.stats
        else:
            self.mask = torch.zeros((B, 1, self.H, self.W), dtype=torch.uint8, device=dev)
            self.map = self.stats = None
        self._mask_in = self.mask      # where pd_contrast_mask writes, or run() copies, the mask
        self.refine, self.raw_mask, self.refine_stats = None, None, None
        if refine is not None:
            self.refine = MaskRefine(B, self.H, self.W, dev, **refine)
            self.raw_mask, self.mask, self.refine_stats = self._mask_in, self.refine.mask, self.refine.stats
        self.inv_args = [inv.ddim_step_args(t, self.traj[i], self.model_out, self.traj[i + 1]) for i, t in enumerate(inv_ts)]
        self.inv_inputs = [self.traj[i].data_ptr() for i in range(S)]
        self.gen_args = [self._forward_step_args(fwd, t) for t in gen_ts]
        self.blend_args = [mask_blend_args(x, self.traj[blend_state_index(k, S)], self.mask, x) for k in range(S)]
        self.blends = [lambda st, a=a: L.check(self.lib.pd_mask_blend(C.byref(a), st), "pd_mask_blend") for a in self.blend_args]
        self._capture()

    def _mask_phase(self, st):
        """Per draw: the images noised to the encode level into ``x``, the UNet under the target class (row block ``k``) into
        ``model_out`` and under the source class (row block ``num_maps + k``) into ``source_out``, their contrast into ``acc``; then the
        mask (``mask="given"``: none of these) and, with ``refine``, the recipe over it."""
        step_bytes = self.rows_per_step * self.plan.w.proj_dim * 4
        M = self.n_mask // 2
        for k in range(M):
            L.check(self.lib.pd_stream_noise(C.byref(self.noise_args[k]), st), "pd_stream_noise")
            self._unet(st, self.temb.data_ptr() + k * step_bytes, self.model_out.data_ptr())
            self._unet(st, self.temb.data_ptr() + (M + k) * step_bytes, self.source_out.data_ptr())
            L.check(self.lib.pd_class_contrast(C.byref(self.contrast_args[k]), st), "pd_class_contrast")
        if M:
            self.contrast.enqueue(st)
        if self.refine is not None:
            self.refine.enqueue(st, self._mask_in)

    def _enqueue(self, st):
        self.class_rows.temb(self.ts_rows, st, self.temb)
        if self.mask_mode == "contrast" or self.refine is not None:
            self._mask_phase(st)
        self._ddim_steps(st, self.inv_args, first=self.n_mask, inputs=self.inv_inputs)
        self.x.copy_(self.traj[self.S])      # generation works in place in x; every state of the inversion stays for the blends
        self._ddim_steps(st, self.gen_args, first=self.n_mask + len(self.inv_args), after=self.blends)
        self._postproc(st)
        if self.mask_mode == "contrast":
            L.check(self.lib.pd_stream_advance(self.noise.state.data_ptr(), self.B, st), "pd_stream_advance")

    def _fill(self, clean_images, orig_class_labels, target_class_labels, mask):
        B, M, n_inv, n_gen = self.B, self.n_mask // 2, len(self.inv_ts), len(self.gen_ts)
        self.traj[0].copy_(clean_images, non_blocking=True)
        if mask is not None:
            self._mask_in.copy_(mask, non_blocking=True)
        if M:
            self.class_rows.fill(slice(0, M * B), M, B, target_class_labels)
            self.class_rows.fill(slice(M * B, 2 * M * B), M, B, orig_class_labels)
        self.class_rows.fill(slice(2 * M * B, (2 * M + n_inv) * B), n_inv, B, orig_class_labels)
        self.class_rows.fill(slice((2 * M + n_inv) * B, (2 * M + n_inv + n_gen) * B), n_gen, B, target_class_labels)

    def run(self, clean_images: torch.Tensor, orig_class_labels: torch.Tensor, target_class_labels: torch.Tensor,
            mask: torch.Tensor = None, join: bool = True):
        """``mask``: required with ``mask="given"`` ((B, 1, H, W) or (B, H, W), bool or uint8, on the runner's device), refused with
        ``mask="contrast"``.  ``join=False`` leaves the caller's stream un-joined (``self.join()`` before reading the outputs)."""
        _check_shape(clean_images, self.x)
        if self.mask_mode == "given":
            if mask is None:
                raise ValueError('MaskedDDIBGraph(mask="given"): run() needs the mask')
            mask = check_mask(mask, self.B, self.H, self.W, self.device, "MaskedDDIBGraph.run")
        elif mask is not None:
            raise ValueError('MaskedDDIBGraph(mask="contrast") computes its mask: run() takes none')
        else:
            self.noise._checked(self.noise.index, self.B)      # the shadow of the index the replay reads and then advances
        self._replay(False, clean_images, orig_class_labels, target_class_labels, mask)
        if self.mask_mode == "contrast":
            self.noise.note_advanced(self.B)
        return self.join() if join else self
