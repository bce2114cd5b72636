"""``DDIMScheduler`` / ``DDIMInverseScheduler`` with the diffusers-0.18.2 call surface the reference uses
(``src/pipeline_conditional_ddim/pipeline_conditionial_ddim.py:45,248-269,340-347``,
``src/utils_Img2Img.py:776-779,794-798``, ``src/utils_training.py:249,256,415-430``).

Host side (this file): the noise tables (``alphas_cumprod``), the int64 timestep grids (bit-exact w.r.t. the
published algorithm) and the four fp32 coefficients of one update, computed with 0-dim fp32 CPU tensors in the
same op order as the reference so that they round identically.  Device side: ``pd_ddim_step`` /
``pd_add_noise`` (one fused elementwise launch per update instead of ~10).

``DDIMScheduler(thresholding=True)`` (diffusers' ``_threshold_sample``, Imagen's dynamic thresholding) replaces the static clamp of a
step by ``s = clamp(quantile(|x0|, dynamic_thresholding_ratio, per sample), 1, sample_max_value)``, ``x0 = clamp(x0, -s, s) / s``.  The
quantile is an exact order statistic taken on the device (``pd_abs_quantile``: a radix select, no host read), so the step stays inside a
captured trajectory: :meth:`DDIMScheduler.threshold_step` builds the launches of one such step -- ``pd_ddim_raw_x0``,
``pd_abs_quantile``, ``pd_ddim_step_threshold`` -- and is what the eager ``step`` and the trajectories both enqueue; the host's part is
:func:`quantile_rank`.  With the default ``sample_max_value=1.0`` s is always 1 and thresholding equals clipping to [-1, 1].
``DDIMInverseScheduler`` does not threshold (diffusers' has ``clip_sample`` only).  ``trained_betas`` (a sequence of floats) replaces the
named beta schedule in both.

``DDIMScheduler.step(..., eta > 0, generator=DeviceNoise)`` draws the variance noise on the device: one ``pd_stream_noise`` launch in
place on ``prev_sample`` (after the thresholding, like the host-drawn term), from the stream of the step's position in ``timesteps``
(:class:`~phendiff_amd.noise.DeviceNoise`).  A ``torch.Generator`` or an explicit ``variance_noise`` keeps the torch arithmetic.

:class:`GuidanceRescale` / :func:`guidance_rescale` (diffusers' ``rescale_noise_cfg``): the classifier-free guidance combine brought back
towards the conditional prediction's per-sample standard deviation, one ``pd_guidance_rescale`` BEFORE a step, which then takes the
result as its model output -- no scheduler here knows about it.
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L
from .noise import DeviceNoise


def randn_tensor(shape, generator, device, dtype=torch.float32):
    """diffusers ``randn_tensor``: a CPU generator draws on the CPU (then moves), a device generator on the device; a LIST of
    generators draws one ``(1, ...)`` sample per generator (per-sample reproducibility) and concatenates."""
    if isinstance(generator, (list, tuple)):
        if len(generator) != shape[0]:
            raise ValueError(f"list of {len(generator)} generators for a batch of {shape[0]}")
        return torch.cat([randn_tensor((1,) + tuple(shape[1:]), g, device, dtype) for g in generator], 0)
    gdev = generator.device if generator is not None else device
    return torch.randn(tuple(shape), generator=generator, device=gdev, dtype=dtype).to(device)


class SchedulerOutput(SimpleNamespace):
    """``DDIMSchedulerOutput`` stand-in: ``.prev_sample``, ``.pred_original_sample``."""


def make_betas(schedule: str, beta_start: float, beta_end: float, n: int) -> torch.Tensor:
    if schedule == "linear":
        return torch.linspace(beta_start, beta_end, n, dtype=torch.float32)
    if schedule == "scaled_linear":  # the schedule of every shipped config (models_configs/noise_scheduler/*.json)
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float32) ** 2
    if schedule == "squaredcos_cap_v2":
        f = lambda u: math.cos((u + 0.008) / 1.008 * math.pi / 2) ** 2
        return torch.tensor([min(1 - f((i + 1) / n) / f(i / n), 0.999) for i in range(n)], dtype=torch.float32)
    raise NotImplementedError(f"beta_schedule {schedule}")


def enforce_zero_terminal_snr(betas: torch.Tensor) -> torch.Tensor:
    """Shift/scale sqrt(alpha_bar) so that the last level has exactly zero SNR (arXiv 2305.08891, alg. 1)."""
    root = torch.cumprod(1.0 - betas, dim=0).sqrt()
    first, last = root[0].clone(), root[-1].clone()
    root = (root - last) * (first / (first - last))
    bar = root ** 2
    alphas = torch.cat([bar[:1], bar[1:] / bar[:-1]])
    return 1 - alphas


def quantile_rank(n: int, q: float):
    """``torch.quantile(x, q)`` ('linear') over ``n`` fp32 values as ``(lo, hi, w)``: the value is ``lerp(sorted[lo], sorted[hi], w)``.
    torch computes the rank in the input's dtype: ``r = float32(q) * float32(n - 1)``, ``lo = floor(r)``, ``hi = ceil(r)``, ``w = r - lo``
    (fp32).  Pure host arithmetic."""
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"quantile() q values must be in the range [0, 1], got {q}")
    if not 1 <= n <= 16_000_000:
        raise ValueError(f"quantile() over {n} elements: torch.quantile takes 1 to 16 000 000")
    r = np.float32(q) * np.float32(n - 1)
    lo, hi = int(np.floor(r)), int(np.ceil(r))
    return lo, hi, float(np.float32(r - np.float32(lo)))


_PRED = L.PD_PRED


def _ptr(b):
    """A buffer as the structs take it: the device pointer of a dense tensor; a raw device pointer (int) or None as it is."""
    return b.data_ptr() if torch.is_tensor(b) else b


def step_operands(sample, model_out, uncond_out=None, w=None, guidance_cfg=False, numel=None, per_sample=None, w_per_sample=None) -> dict:
    """The operand fields the step structs share (``pd_ddim_step_args``, ``pd_ddim_step_threshold_args``, ``pd_multistep_step_args``): what
    ``step_operands`` of csrc/pd_step.h reads.  Buffers are dense fp32 tensors or raw device pointers (ints); ``numel`` / ``per_sample``
    default to ``sample``'s and ``w_per_sample`` to "``w`` holds more than one weight", so raw pointers need them spelled out."""
    if numel is None:
        numel, per_sample = sample.numel(), sample[0].numel()
    if w_per_sample is None:
        w_per_sample = torch.is_tensor(w) and w.numel() > 1
    return dict(numel=numel, per_sample=per_sample, sample=_ptr(sample), model_out=_ptr(model_out), uncond_out=_ptr(uncond_out), w=_ptr(w),
                w_per_sample=int(w_per_sample), guidance_cfg=int(guidance_cfg))


def abs_quantile_args(sample, ratio: float, x0_raw, quant, workspace) -> "L.AbsQuantileArgs":
    """``pd_abs_quantile`` over the raw x0 of a (B, ...) ``sample``: the per-sample quantile of ``|x0|`` at ``ratio`` into ``quant``."""
    B, n = sample.shape[0], sample[0].numel()
    lo, hi, wgt = quantile_rank(n, float(ratio))
    return L.AbsQuantileArgs(B=B, n=n, rank_lo=lo, rank_hi=hi, weight=wgt, x=x0_raw.data_ptr(), out=quant.data_ptr(),
                             workspace=workspace.data_ptr())


class ThresholdStep:
    """The launches of one dynamically thresholded DDIM update (:meth:`DDIMScheduler.threshold_step` builds it): the argument structs,
    and :meth:`enqueue`, the one place where the sequence is written down.  It holds the three scratch tensors the structs point at
    (``x0_raw``, ``quant``, ``workspace``): a captured graph keeps launching into them for as long as its runner keeps this object,
    whatever becomes of the scheduler that made it.  ``stream``: the stream the scratch set belongs to."""

    def __init__(self, step: "L.DdimStepThresholdArgs", quantile: "L.AbsQuantileArgs", x0_raw: torch.Tensor, quant: torch.Tensor,
                 workspace: torch.Tensor, stream: int):
        self.step, self.quantile, self.stream = step, quantile, stream
        self.x0_raw, self.quant, self.workspace = x0_raw, quant, workspace
        assert (quantile.x, quantile.out, quantile.workspace, step.quantile) == (x0_raw.data_ptr(), quant.data_ptr(), workspace.data_ptr(),
                                                                                 quant.data_ptr()), "the structs point at the tensors held"

    def enqueue(self, st: int):
        """The three launches on ``st``, which must be the stream the step was built for (its scratch set is that stream's own)."""
        if int(st) != self.stream:
            raise ValueError(f"ThresholdStep built for stream {self.stream:#x} enqueued on stream {int(st):#x}")
        lib = L.lib()
        L.check(lib.pd_ddim_raw_x0(C.byref(self.step), self.x0_raw.data_ptr(), st), "pd_ddim_raw_x0")      # before an in-place update
        L.check(lib.pd_abs_quantile(C.byref(self.quantile), st), "pd_abs_quantile")
        L.check(lib.pd_ddim_step_threshold(C.byref(self.step), st), "pd_ddim_step_threshold")


THRESHOLD_SCRATCH_SETS = 4      # scratch sets (x0, quantiles, workspace) a scheduler keeps for re-use, by last use

THRESHOLDING_NOT_GUIDED = ("the gradient-guided transfer differentiates the Lp loss of x0, and the reference defines no derivative through "
                           "the per-sample threshold s")
THRESHOLDING_NOT_LATENT = ("dynamic thresholding is a pixel-space method (diffusers documents it as unsuitable for latent-space models "
                           "such as Stable Diffusion)")


def refuse_thresholding(scheduler, who: str, why: str) -> None:
    """What does not run a ``thresholding=True`` scheduler says so, and why, before it packs or launches anything."""
    cfg = getattr(scheduler, "config", None)
    if cfg.get("thresholding", False) if isinstance(cfg, dict) else getattr(cfg, "thresholding", False):
        raise ValueError(f"{who} does not run a scheduler with thresholding=True: {why}")


# ---- classifier-free guidance rescale (arXiv 2305.08891 section 3.4; diffusers' `guidance_rescale` / rescale_noise_cfg) -------------------
# Under a zero-terminal-SNR schedule the guided prediction  cfg = u + w (c - u)  is over-scaled, which saturates the images.  The remedy
# brings cfg back towards the conditional prediction's per-sample standard deviation:  out = cfg (phi std(c) / std(cfg) + 1 - phi).
# ``pd_guidance_rescale`` does it in two launches (fp64 sums in a fixed order, a sample's result a function of that sample alone, no host
# read); the scheduler step then runs on ``out`` without an unconditional prediction, so no step kernel knows about it.
GUIDANCE_RESCALE_CHUNK = L.CONSTANTS["PD_GUIDANCE_RESCALE_CHUNK"]      # the elements one workgroup reduces: a sample has ceil(n / this) partials
GUIDANCE_RESCALE_SCRATCH_SETS = 4      # workspaces kept for re-use, by last use
_rescale_workspaces = {}               # (B, n, device, stream) -> workspace; launches on one stream are ordered, so they may share one


def check_guidance_rescale(value, who: str) -> float:
    """``guidance_rescale`` as a float in [0, 1], or a ``ValueError`` -- what every guided entry point says before it packs a weight or
    launches anything."""
    try:
        phi = float(value)
    except (TypeError, ValueError):
        phi = math.nan
    if not (math.isfinite(phi) and 0.0 <= phi <= 1.0):
        raise ValueError(f"{who}: guidance_rescale must be a finite number in [0, 1], got {value!r}")
    return phi


def guidance_weights(w, device) -> torch.Tensor:
    """The guidance weight(s) as the kernels read them: a dense fp32 (1,) or (B,) tensor on ``device``."""
    return (w if torch.is_tensor(w) else torch.tensor([float(w)])).to(device=device, dtype=torch.float32).reshape(-1).contiguous()


class GuidanceRescale:
    """The launch of one rescaled guidance combine (``pd_guidance_rescale``): the argument struct, the workspace it points at, and
    :meth:`enqueue`.  ``cond`` / ``uncond``: dense fp32 (B, ...) tensors, the two predictions; ``w``: a dense fp32 (1,) or (B,) tensor on
    their device; ``out``: where the rescaled guided prediction goes (default: ``cond`` itself -- in place, what the captured
    trajectories do).  The workspace is one per (B, n, device, stream), made on first use and kept by order of last use
    (:data:`GUIDANCE_RESCALE_SCRATCH_SETS` of them, 32 bytes per sample and chunk of :data:`GUIDANCE_RESCALE_CHUNK` elements): a capture
    finds it allocated, and the object holds it, so whoever keeps the object (a runner's captured graph) keeps the memory it launches into."""

    def __init__(self, cond: torch.Tensor, uncond: torch.Tensor, w: torch.Tensor, guidance_rescale: float, guidance_cfg: bool = False,
                 out: torch.Tensor = None, stream: int = None):
        phi = check_guidance_rescale(guidance_rescale, "GuidanceRescale")
        out = cond if out is None else out
        for name, t in (("cond", cond), ("uncond", uncond), ("out", out)):
            if not (torch.is_tensor(t) and t.is_cuda):
                raise L.PhenDiffHipError(f"GuidanceRescale: {name} must be a tensor on an MI355X (no CPU fallback)")
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(cond.shape):
                raise ValueError(f"GuidanceRescale: {name} must be a dense fp32 tensor of cond's shape {tuple(cond.shape)}")
        B, n = cond.shape[0], cond[0].numel()
        if not (torch.is_tensor(w) and w.device == cond.device and w.dtype == torch.float32 and w.is_contiguous() and w.numel() in (1, B)):
            raise ValueError(f"GuidanceRescale: w must be a dense fp32 tensor of 1 or {B} weights on {cond.device} (guidance_weights makes it)")
        self.stream = int(stream if stream is not None else torch.cuda.current_stream(cond.device).cuda_stream)
        self.cond, self.uncond, self.w, self.out = cond, uncond, w, out
        self.workspace = self._workspace(B, n, cond.device, self.stream)
        self.args = L.GuidanceRescaleArgs(numel=B * n, per_sample=n, model_out=cond.data_ptr(), uncond_out=uncond.data_ptr(),
                                          w=w.data_ptr(), w_per_sample=int(w.numel() > 1), guidance_cfg=int(bool(guidance_cfg)), rescale=phi,
                                          out=out.data_ptr(), workspace=self.workspace.data_ptr())

    @staticmethod
    def _workspace(B: int, n: int, device, stream: int) -> torch.Tensor:
        key = (B, n, device, stream)
        ws = _rescale_workspaces.pop(key, None)
        if ws is None:
            size = L.lib().pd_guidance_rescale_workspace(B, n)
            if size == 0:
                raise ValueError(f"guidance rescale: no per-sample standard deviation over a ({B}, {n}) batch (at least two elements a sample)")
            ws = torch.empty((size // 8,), dtype=torch.float64, device=device)
        _rescale_workspaces[key] = ws                           # (re-inserted: the dict's order is the order of last use)
        while len(_rescale_workspaces) > GUIDANCE_RESCALE_SCRATCH_SETS:
            del _rescale_workspaces[next(iter(_rescale_workspaces))]
        return ws

    def enqueue(self, st: int):
        """The launch on ``st``, which must be the stream the object was built for (its workspace is that stream's own)."""
        if int(st) != self.stream:
            raise ValueError(f"GuidanceRescale built for stream {self.stream:#x} enqueued on stream {int(st):#x}")
        L.check(L.lib().pd_guidance_rescale(C.byref(self.args), st), "pd_guidance_rescale")


def guidance_rescale(cond, uncond, w, guidance_rescale: float, guidance_cfg: bool = False, out=None) -> torch.Tensor:
    """The rescaled guided prediction of a conditional and an unconditional model output, a dense fp32 tensor (``out`` where given; it
    may be ``cond``): ``cfg = uncond + w (cond - uncond)`` (``guidance_cfg``: ``cond + w (cond - uncond)``) times
    ``guidance_rescale * std(cond) / std(cfg) + 1 - guidance_rescale`` per sample -- diffusers' ``rescale_noise_cfg``.  ``w``: a number
    or a (B,) tensor.  One ``pd_guidance_rescale`` on the current stream; a scheduler's ``step`` then takes the result as the model
    output.  ``guidance_rescale = 0`` returns the plain combine."""
    phi = check_guidance_rescale(guidance_rescale, "guidance_rescale")
    if not (torch.is_tensor(cond) and torch.is_tensor(uncond) and cond.is_cuda and uncond.is_cuda):
        raise L.PhenDiffHipError("phendiff_amd.guidance_rescale runs on MI355X tensors only (no CPU fallback)")
    c, u = cond.contiguous().float(), uncond.contiguous().float()
    if out is None:
        out = torch.empty_like(c)
    GuidanceRescale(c, u, guidance_weights(w, c.device), phi, guidance_cfg, out).enqueue(torch.cuda.current_stream(c.device).cuda_stream)
    return out


MULTISTEP_NOT_TILED = "the tiled trajectories step DDIM on the canvas; the solver's history is not kept per canvas yet"
MULTISTEP_NOT_GUIDED = ("the gradient-guided transfer pushes the sample between two steps, which invalidates the previous step's prediction "
                        "a multistep update reuses")
MULTISTEP_NOT_MASKED = ("the masked transfer puts the inversion's state back outside the mask between two steps, which invalidates the previous "
                        "step's prediction a multistep update reuses")
MULTISTEP_NOT_LATENT = "the multistep solvers are wired into the pixel tier (ConditionalDDIMPipeline) only"


def refuse_multistep(scheduler, who: str, why: str) -> None:
    """What does not run a DPM-Solver multistep scheduler says so, and why, before it packs or launches anything."""
    if isinstance(scheduler, (DPMSolverMultistepScheduler, DPMSolverMultistepInverseScheduler)):
        raise NotImplementedError(f"{who} does not run a {type(scheduler).__name__}: {why}")


def sampler_grid(config, num_inference_steps: int) -> np.ndarray:
    """The descending int64 timestep grid ``t_0 > ... > t_{S-1}`` of a sampler: diffusers' three spacings and ``steps_offset``
    (``DDIMScheduler.set_timesteps``; the multistep schedulers walk the same grid)."""
    n = config.num_train_timesteps
    if num_inference_steps > n:
        raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than {n}")
    mode = config.timestep_spacing
    if mode == "linspace":
        grid = np.linspace(0, n - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
    elif mode == "leading":
        grid = (np.arange(num_inference_steps) * (n // num_inference_steps)).round()[::-1].copy().astype(np.int64)
        grid += config.steps_offset
    elif mode == "trailing":
        grid = np.round(np.arange(n, 0, -(n / num_inference_steps))).astype(np.int64) - 1
    else:
        raise ValueError(f"{mode} is not supported. Choose one of 'leading', 'trailing' or 'linspace'.")
    return grid


def _beta_list(trained_betas):
    """``trained_betas`` as the config keeps it: None, or a plain list of floats (what a JSON config round-trips)."""
    if trained_betas is None:
        return None
    return [float(b) for b in (trained_betas.tolist() if hasattr(trained_betas, "tolist") else trained_betas)]


class _SchedulerBase:
    order = 1
    init_noise_sigma = 1.0
    _config_keys = ()

    def _finish_init(self, cfg: dict, rescale: bool):
        self.config = SimpleNamespace(**cfg)
        c = self.config
        if c.prediction_type not in _PRED:
            raise ValueError(f"prediction_type {c.prediction_type}")
        if c.trained_betas is not None:      # diffusers: torch.tensor(trained_betas, dtype=torch.float32), whatever beta_schedule names
            betas = torch.tensor(c.trained_betas, dtype=torch.float32)
            if betas.ndim != 1 or betas.numel() != c.num_train_timesteps:
                raise ValueError(f"trained_betas: expected {c.num_train_timesteps} values, got shape {tuple(betas.shape)}")
        else:
            betas = make_betas(c.beta_schedule, c.beta_start, c.beta_end, c.num_train_timesteps)
        if rescale:
            betas = enforce_zero_terminal_snr(betas)
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.num_inference_steps = None
        self._coef_dev = {}
        self._threshold_buffers = {}

    @classmethod
    def from_config(cls, config, **overrides):
        d = dict(config) if isinstance(config, dict) else dict(vars(config))
        d = {k: v for k, v in d.items() if not k.startswith("_")}
        d.update(overrides)
        return cls(**d)

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **overrides):
        import os
        from .checkpoint import load_scheduler
        return load_scheduler(cls, os.path.join(path, subfolder) if subfolder else path, **overrides)

    def save_pretrained(self, path):
        from .checkpoint import save_scheduler
        save_scheduler(self, path)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def __len__(self):
        return self.config.num_train_timesteps

    @staticmethod
    def _t_int(timestep) -> int:
        return int(timestep.item()) if torch.is_tensor(timestep) else int(timestep)

    # subclasses: (alpha_prod_t, alpha_prod_t_prev, sigma) as 0-dim fp32 tensors
    def _levels(self, t: int, eta: float):
        raise NotImplementedError

    def step_coefficients(self, timestep, eta: float = 0.0):
        """(sqrt_a, sqrt_b, sqrt_a_prev, dir_coef, sigma) as python floats holding fp32 values."""
        t = self._t_int(timestep)
        a, ap, sigma = self._levels(t, eta)
        sa, sb = a ** 0.5, (1 - a) ** 0.5
        sap = ap ** 0.5
        dirc = (1 - ap - sigma ** 2) ** 0.5
        return float(sa), float(sb), float(sap), float(dirc), float(sigma)

    def ddim_step_args(self, timestep, sample, model_out, prev_sample, uncond_out=None, w=None, guidance_cfg=False,
                       use_clipped_model_output=False, pred_x0=None, eta=0.0, numel=None, per_sample=None, w_per_sample=None):
        """The ``pd_ddim_step`` argument struct of one update at ``timestep``: prediction type and clipping from the config, the four
        coefficients from :meth:`step_coefficients`.  Buffers are dense fp32 tensors or raw device pointers (ints); ``numel`` /
        ``per_sample`` default to ``sample``'s and ``w_per_sample`` to "``w`` holds more than one weight", so raw pointers need them
        spelled out.  ``uncond_out`` + ``w``: the guidance combine runs inside the update (``guidance_cfg``: the "CFG" equation)."""
        if getattr(self.config, "thresholding", False):
            raise ValueError("this scheduler thresholds dynamically: a step is DDIMScheduler.threshold_step's launches, not one pd_ddim_step")
        return L.DdimStepArgs(use_clipped_model_output=int(bool(use_clipped_model_output)), prev_sample=_ptr(prev_sample), pred_x0=_ptr(pred_x0),
                              **self.step_fields(timestep, eta),
                              **step_operands(sample, model_out, uncond_out, w, guidance_cfg, numel, per_sample, w_per_sample))

    def step_fields(self, timestep, eta: float = 0.0, clip: bool = True) -> dict:
        """The scheduler's part of a DDIM-family struct (``pd_ddim_step_args``, ``pd_guided_step_args``; ``clip=False``:
        ``pd_ddim_step_threshold_args``, which has no static clamp): prediction type and clipping from the config, the four coefficients
        of the update at ``timestep`` from :meth:`step_coefficients`."""
        c = self.config
        sa, sb, sap, dirc, _ = self.step_coefficients(timestep, eta)
        fields = dict(pred_type=_PRED[c.prediction_type], sqrt_a=sa, sqrt_b=sb, sqrt_ap=sap, dir_coef=dirc)
        if clip:
            fields.update(clip=int(bool(c.clip_sample)), clip_range=float(c.clip_sample_range))
        return fields

    def _prepare_step(self, model_output, sample, uncond_output, w, out, want_x0, stream):
        """What an eager step works on: ``(x, model_out, prev, x0, uncond, weights, stream)`` -- the kernels read dense fp32; ``prev`` is
        ``out`` where given, ``x0`` None unless wanted, ``uncond`` / ``weights`` None without guidance."""
        if not (sample.is_cuda and model_output.is_cuda):
            raise L.PhenDiffHipError("phendiff_amd schedulers step on MI355X tensors only (no CPU fallback)")
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        x = sample.contiguous().float()
        mo = model_output.contiguous().float()
        prev = torch.empty_like(x) if out is None else out
        x0 = torch.empty_like(x) if want_x0 else None
        wt = uo = None
        if uncond_output is not None:
            uo, wt = uncond_output.contiguous().float(), guidance_weights(w, x.device)
        st = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
        return x, mo, prev, x0, uo, wt, st

    def _device_step(self, model_output, timestep, sample, eta, use_clipped_model_output, generator, variance_noise,
                     uncond_output=None, w=None, guidance_cfg=False, out=None, want_x0=True, stream=None):
        x, mo, prev, x0, uo, wt, st = self._prepare_step(model_output, sample, uncond_output, w, out, want_x0, stream)
        if getattr(self.config, "thresholding", False):
            self.threshold_step(timestep, x, mo, prev, st, uo, wt, guidance_cfg, use_clipped_model_output, x0, eta).enqueue(st)
        else:
            a = self.ddim_step_args(timestep, x, mo, prev, uo, wt, guidance_cfg, use_clipped_model_output, x0, eta)
            L.check(L.lib().pd_ddim_step(C.byref(a), st), "pd_ddim_step")
        if eta > 0:
            if variance_noise is None and isinstance(generator, DeviceNoise):
                # one pd_stream_noise launch in place on prev_sample (after the thresholding, like the host-drawn term below)
                generator.add_variance_noise(prev, self.step_coefficients(timestep, eta)[4], self.step_index(timestep), st)
                return prev, x0
            if variance_noise is None:
                variance_noise = randn_tensor(mo.shape, generator, mo.device, mo.dtype)
            prev = prev + self.step_coefficients(timestep, eta)[4] * variance_noise.to(device=mo.device, dtype=mo.dtype)
        return prev, x0

    def _threshold_scratch(self, sample, stream: int):
        """The scratch set (x0, quantiles, workspace) of a (B, n, device, stream), made on first use and kept by order of last use."""
        B, n = sample.shape[0], sample[0].numel()
        key = (B, n, sample.device, int(stream))
        bufs = self._threshold_buffers.pop(key, None)
        if bufs is None:
            ws = L.lib().pd_abs_quantile_workspace(B, n)
            if ws == 0:
                raise ValueError(f"dynamic thresholding: no per-sample quantile over a ({B}, {n}) batch")
            bufs = (torch.empty((B, n), dtype=torch.float32, device=sample.device), torch.empty((B,), dtype=torch.float32, device=sample.device),
                    torch.empty((ws,), dtype=torch.uint8, device=sample.device))
        self._threshold_buffers[key] = bufs                     # (re-inserted: the dict's order is the order of last use)
        while len(self._threshold_buffers) > THRESHOLD_SCRATCH_SETS:
            del self._threshold_buffers[next(iter(self._threshold_buffers))]
        return bufs

    def step_index(self, timestep) -> int:
        """The position of ``timestep`` in ``self.timesteps``: the trajectory step a ``DeviceNoise`` draws the variance noise of."""
        t = self._t_int(timestep)
        at = (self.timesteps == t).nonzero()
        if at.numel() == 0:
            raise ValueError(f"timestep {t} is not one of this scheduler's {self.timesteps.numel()} timesteps")
        return int(at[0])

    def _per_sample_coefs(self, timesteps, device):
        """sqrt(alpha_bar_t), sqrt(1 - alpha_bar_t) per sample.  The tables are computed once on the host in fp32 (the
        reference's arithmetic, bit for bit) and gathered on the device: no host sync when ``timesteps`` live there."""
        tabs = getattr(self, "_coef_tables", None)
        if tabs is None or tabs[0].device != torch.device(device):
            acp = self.alphas_cumprod
            tabs = ((acp ** 0.5).to(device), ((1 - acp) ** 0.5).to(device))
            self._coef_tables = tabs
        t = timesteps.detach().to(device=device, dtype=torch.long).reshape(-1)
        return tabs[0][t].contiguous(), tabs[1][t].contiguous()

    def _mix(self, x, noise, timesteps, velocity):
        if not x.is_cuda:
            raise L.PhenDiffHipError("phendiff_amd schedulers run on MI355X tensors only (no CPU fallback)")
        x = x.contiguous().float()
        noise = noise.contiguous().float()
        if timesteps.numel() == 1:
            timesteps = timesteps.reshape(1).expand(x.shape[0])
        sa, sb = self._per_sample_coefs(timesteps, x.device)
        out = torch.empty_like(x)
        a = L.AddNoiseArgs(numel=x.numel(), per_sample=x[0].numel(), velocity=int(velocity), x=x.data_ptr(),
                           noise=noise.data_ptr(), sa=sa.data_ptr(), sb=sb.data_ptr(), out=out.data_ptr())
        L.check(L.lib().pd_add_noise(C.byref(a), torch.cuda.current_stream(x.device).cuda_stream), "pd_add_noise")
        return out

    def add_noise(self, original_samples, noise, timesteps):
        return self._mix(original_samples, noise, timesteps, False)

    def get_velocity(self, sample, noise, timesteps):
        return self._mix(sample, noise, timesteps, True)


class DDIMScheduler(_SchedulerBase):
    """diffusers ``DDIMScheduler`` surface (constructor defaults of 0.18.2)."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                 prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                 clip_sample_range=1.0, sample_max_value=1.0, timestep_spacing="leading",
                 rescale_betas_zero_snr=False, **ignored):
        if thresholding:
            quantile_rank(1, dynamic_thresholding_ratio)      # (a ratio outside [0, 1] is refused here, not at the first step)
            if not float(sample_max_value) > 0:
                raise ValueError(f"sample_max_value must be positive, got {sample_max_value}")
        cfg = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                   beta_schedule=beta_schedule, trained_betas=_beta_list(trained_betas), clip_sample=clip_sample,
                   set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset, prediction_type=prediction_type,
                   thresholding=bool(thresholding), dynamic_thresholding_ratio=dynamic_thresholding_ratio,
                   clip_sample_range=clip_sample_range, sample_max_value=sample_max_value,
                   timestep_spacing=timestep_spacing, rescale_betas_zero_snr=rescale_betas_zero_snr)
        self._finish_init(cfg, rescale_betas_zero_snr)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.timesteps = torch.from_numpy(np.arange(num_train_timesteps)[::-1].copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps: int, device=None):
        grid = sampler_grid(self.config, num_inference_steps)
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(grid)  # kept on the host: indexing tables must not sync the device
        return self

    def _levels(self, t, eta):
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a = self.alphas_cumprod[t]
        ap = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        sigma = torch.tensor(0.0)
        if eta:
            variance = ((1 - ap) / (1 - a)) * (1 - a / ap)
            sigma = eta * variance ** 0.5
        return a, ap, sigma

    def threshold_step(self, timestep, sample, model_out, prev_sample, stream: int, uncond_out=None, w=None, guidance_cfg=False,
                       use_clipped_model_output=False, pred_x0=None, eta=0.0) -> ThresholdStep:
        """One dynamically thresholded update at ``timestep`` as a :class:`ThresholdStep` (``.enqueue(stream)`` launches it):
        the raw x0 of the step into a scratch buffer, its per-sample quantile of ``|x0|`` at ``dynamic_thresholding_ratio``, then the
        update with ``s = clamp(quantile, 1, sample_max_value)`` in the clamp's place (``prev_sample`` may be ``sample``).  ``sample``
        is a dense fp32 (B, ...) tensor; the other buffers are such tensors or raw device pointers, as for :meth:`ddim_step_args`.
        The scratch x0, the (B,) quantiles and the select's workspace come from the scheduler, one set per (B, n, device, stream): a
        capture finds them allocated, and runners that replay on their own streams do not share them.  The scheduler keeps the
        :data:`THRESHOLD_SCRATCH_SETS` sets used last (4 (B n + B) + 24 640 B bytes each) and lets older ones go; the returned step
        holds its set itself, so whoever keeps the step (a runner's captured graph) keeps the memory it launches into."""
        c = self.config
        x0_raw, quant, workspace = self._threshold_scratch(sample, stream)
        step = L.DdimStepThresholdArgs(
            use_clipped_model_output=int(bool(use_clipped_model_output)), prev_sample=_ptr(prev_sample), pred_x0=_ptr(pred_x0),
            quantile=quant.data_ptr(), sample_max_value=float(c.sample_max_value), **self.step_fields(timestep, eta, clip=False),
            **step_operands(sample, model_out, uncond_out, w, guidance_cfg))
        q = abs_quantile_args(sample, c.dynamic_thresholding_ratio, x0_raw, quant, workspace)
        return ThresholdStep(step, q, x0_raw, quant, workspace, int(stream))

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False,
             generator=None, variance_noise=None, return_dict: bool = True):
        prev, x0 = self._device_step(model_output, timestep, sample, eta, use_clipped_model_output, generator, variance_noise)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev, pred_original_sample=x0)


class DDIMInverseScheduler(_SchedulerBase):
    """diffusers ``DDIMInverseScheduler`` surface.  ``variant="0.18.2"`` (default = the version the reference
    pins, ``environment.yaml:80``): ignores ``timestep_spacing`` / ``rescale_betas_zero_snr`` (table NOT
    rescaled, ascending "leading" grid), forwards the deprecated ``set_alpha_to_one`` into ``set_alpha_to_zero``,
    and steps from level ``t`` to ``t + N//S``.  ``variant="0.20+"`` is the later rewrite."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, clip_sample=True, set_alpha_to_zero=True, steps_offset=0,
                 prediction_type="epsilon", clip_sample_range=1.0, timestep_spacing="leading",
                 rescale_betas_zero_snr=False, variant="0.18.2", **kwargs):
        if kwargs.get("set_alpha_to_one") is not None:
            set_alpha_to_zero = kwargs["set_alpha_to_one"]
        if variant not in ("0.18.2", "0.20+"):
            raise ValueError("variant must be '0.18.2' or '0.20+'")
        self.variant = variant
        cfg = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                   beta_schedule=beta_schedule, trained_betas=_beta_list(trained_betas), clip_sample=clip_sample,
                   set_alpha_to_zero=set_alpha_to_zero, steps_offset=steps_offset, prediction_type=prediction_type,
                   clip_sample_range=clip_sample_range, timestep_spacing=timestep_spacing,
                   rescale_betas_zero_snr=rescale_betas_zero_snr)
        self._finish_init(cfg, rescale_betas_zero_snr and variant == "0.20+")
        self.final_alpha_cumprod = torch.tensor(0.0) if set_alpha_to_zero else self.alphas_cumprod[-1]
        self.initial_alpha_cumprod = torch.tensor(1.0)
        self.timesteps = torch.from_numpy(np.arange(num_train_timesteps).copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = self.config.num_train_timesteps
        if num_inference_steps > n:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than {n}")
        self.num_inference_steps = num_inference_steps
        mode = "leading" if self.variant == "0.18.2" else self.config.timestep_spacing
        if mode == "leading":
            grid = (np.arange(num_inference_steps) * (n // num_inference_steps)).round().copy().astype(np.int64)
            grid += self.config.steps_offset
        elif mode == "trailing":
            grid = np.round(np.arange(n, 0, -(n / num_inference_steps))[::-1]).astype(np.int64) - 1
        else:
            raise ValueError(f"{mode} is not supported. Choose one of 'leading' or 'trailing'.")
        self.timesteps = torch.from_numpy(grid)
        return self

    def _levels(self, t, eta):
        n = self.config.num_train_timesteps
        ratio = n // self.num_inference_steps
        if self.variant == "0.18.2":
            nxt = t + ratio
            a = self.alphas_cumprod[t]
            ap = self.alphas_cumprod[nxt] if nxt < n else self.final_alpha_cumprod
        else:
            src = t - ratio
            a = self.alphas_cumprod[src] if src >= 0 else self.initial_alpha_cumprod
            ap = self.alphas_cumprod[t]
        return a, ap, torch.tensor(0.0)

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False,
             variance_noise=None, return_dict: bool = True):
        prev, x0 = self._device_step(model_output, timestep, sample, 0.0, False, None, None)
        if not return_dict:
            return (prev, x0)
        return SchedulerOutput(prev_sample=prev, pred_original_sample=x0)


# ---- second-order multistep solvers (DPM-Solver++ 2M, arXiv 2211.01095) ------------------------------------------------------------------
# One update is  x' = a x + b m0 + c (m0 - m1)  (``pd_multistep_step``): m0 the model's prediction at the level the sample is at, in the
# solver's variable (x0: the data form, the sampler's; eps: the noise form, the inversion's), m1 the previous step's.  For a step from
# level abar_s to level abar_t, with  alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = ln alpha - ln sigma, h = lambda_t - lambda_s:
#     data form    a = sigma_t / sigma_s    b = -alpha_t expm1(-h)       abar_t = 1: (0, 1)      abar_s = 0: (sigma_t, alpha_t)
#     noise form   a = alpha_t / alpha_s    b = -sigma_t expm1(h)        abar_t = 0: (0, 1)
#     c = b h / (2 h_prev)  for a second-order step whose h and h_prev (the previous step's h) are finite and non-zero; 0 otherwise
# (the limits are taken explicitly, not through inf arithmetic).  Everything in float64 on the host from ``alphas_cumprod``; the struct
# rounds each coefficient to fp32 once.  c = 0 is the first-order update: DDIM, written in the solver's variable.
DATA_FORM, NOISE_FORM = 0, 1


def _half_log_snr(abar: float) -> float:
    """lambda = ln alpha - ln sigma; +inf at abar = 1, -inf at abar = 0."""
    if abar >= 1.0:
        return math.inf
    if abar <= 0.0:
        return -math.inf
    return 0.5 * (math.log(abar) - math.log1p(-abar))


def solver_coefficients(levels, form: int, solver_order: int = 2, lower_order_final: bool = False):
    """Per step ``i`` of the path ``levels`` (n + 1 values of alpha_bar, float64) the float64 tuple ``(sqrt_a, sqrt_b, a, b, c, h)``:
    ``sqrt_a, sqrt_b`` of the level the sample is at (what turns the model's output into m0), the update's three coefficients, and h.
    ``lower_order_final``: the last of fewer than 15 steps is first-order."""
    if form not in (DATA_FORM, NOISE_FORM):
        raise ValueError(f"form must be {DATA_FORM} (data prediction) or {NOISE_FORM} (noise prediction), got {form}")
    if solver_order not in (1, 2):
        raise ValueError(f"solver_order must be 1 or 2, got {solver_order}")
    levels = [float(v) for v in levels]
    n = len(levels) - 1
    out, h_prev = [], None
    for i in range(n):
        s, t = levels[i], levels[i + 1]
        al_s, sg_s, al_t, sg_t = math.sqrt(s), math.sqrt(1.0 - s), math.sqrt(t), math.sqrt(1.0 - t)
        h = 0.0 if s == t else _half_log_snr(t) - _half_log_snr(s)
        if form == DATA_FORM:
            if t >= 1.0:
                a, b = 0.0, 1.0
            elif s <= 0.0:
                a, b = sg_t, al_t
            elif s >= 1.0:
                raise ValueError("the data form is singular going up from a noise-free level (sigma = 0): invert with the noise form")
            else:
                a, b = sg_t / sg_s, -al_t * math.expm1(-h)
        else:
            if t <= 0.0:
                a, b = 0.0, 1.0
            elif s <= 0.0:
                raise ValueError("the noise form is singular going down from pure noise (alpha = 0): sample with the data form")
            else:
                a, b = al_t / al_s, -sg_t * math.expm1(h)
        second = (solver_order == 2 and i > 0 and math.isfinite(h) and h != 0.0 and math.isfinite(h_prev) and h_prev != 0.0
                  and not (lower_order_final and i == n - 1 and n < 15))
        out.append((al_s, sg_s, a, b, 0.5 * b * h / h_prev if second else 0.0, h))
        h_prev = h
    return out


class MultistepThresholdStep(ThresholdStep):
    """The launches of one dynamically thresholded multistep update: ``pd_ddim_raw_x0``, ``pd_abs_quantile`` (:class:`ThresholdStep`'s
    structs and scratch set, whose ``step`` carries the operands the raw x0 is made of) and ``pd_multistep_step`` with the quantile."""

    def __init__(self, update: "L.MultistepStepArgs", step, quantile, x0_raw, quant, workspace, stream: int):
        super().__init__(step, quantile, x0_raw, quant, workspace, stream)
        self.update = update
        assert update.quantile == quant.data_ptr() and (update.sample, update.model_out, update.uncond_out, update.w) == (
            step.sample, step.model_out, step.uncond_out, step.w), "both structs name the same operands"

    def enqueue(self, st: int):
        if int(st) != self.stream:
            raise ValueError(f"MultistepThresholdStep built for stream {self.stream:#x} enqueued on stream {int(st):#x}")
        lib = L.lib()
        L.check(lib.pd_ddim_raw_x0(C.byref(self.step), self.x0_raw.data_ptr(), st), "pd_ddim_raw_x0")      # before an in-place update
        L.check(lib.pd_abs_quantile(C.byref(self.quantile), st), "pd_abs_quantile")
        L.check(lib.pd_multistep_step(C.byref(self.update), st), "pd_multistep_step")


class _MultistepBase(_SchedulerBase):
    """What the sampler and the inversion share: the coefficient table of the path, the one place the struct is built, the eager step
    with its two ping-pong history tensors.  A subclass sets ``form`` and, in ``set_timesteps``, ``timesteps`` and ``levels``."""
    order = 2
    form = DATA_FORM

    def _set_path(self, num_inference_steps: int, timesteps: np.ndarray, levels):
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(np.ascontiguousarray(timesteps, dtype=np.int64))      # (on the host, as the DDIM pair's)
        self.levels = np.asarray(levels, dtype=np.float64)
        c = self.config
        self._coefs = solver_coefficients(self.levels, self.form, c.solver_order, bool(getattr(c, "lower_order_final", False)))
        self._hist, self._next_index = None, None

    def _acp64(self, t: int) -> float:
        return float(self.alphas_cumprod[int(t)].double())

    def multistep_coefficients(self, i: int, first: bool = False):
        """``(sqrt_a, sqrt_b, a, b, c)`` of step ``i`` of the path as python floats holding fp32 values.  ``first``: the trajectory starts
        at this step (no history yet), so it is first-order whatever ``i``."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if not 0 <= i < len(self._coefs):
            raise ValueError(f"step {i} of a path of {len(self._coefs)} steps")
        sa, sb, a, b, c, _ = self._coefs[i]
        return tuple(float(np.float32(v)) for v in (sa, sb, a, b, 0.0 if (first or i == 0) else c))

    def step_coefficients(self, timestep, eta: float = 0.0):
        raise ValueError(f"{type(self).__name__} has no DDIM coefficients: a step is multistep_step_args' pd_multistep_step")

    def ddim_step_args(self, *args, **kw):
        raise ValueError(f"{type(self).__name__}: a step is multistep_step_args' pd_multistep_step, not a pd_ddim_step")

    def multistep_step_args(self, i: int, sample, model_out, prev_sample, hist_in, hist_out, uncond_out=None, w=None, guidance_cfg=False,
                            pred_x0=None, first: bool = False, quantile=None, numel=None, per_sample=None, w_per_sample=None):
        """The ``pd_multistep_step`` argument struct of step ``i`` of the path (``timesteps[i]`` is where the model was evaluated): form,
        prediction type and clipping from the config, the coefficients from :meth:`multistep_coefficients`.  Buffers are dense fp32 tensors
        or raw device pointers (ints), as for ``ddim_step_args``; ``hist_in`` holds the previous step's ``hist_out`` (not read by a
        first-order step, may be None then).  ``quantile``: the (B,) output of ``pd_abs_quantile`` over this step's raw x0 (the dynamic
        threshold replaces the clamp)."""
        operands = step_operands(sample, model_out, uncond_out, w, guidance_cfg, numel, per_sample, w_per_sample)
        return self._update_args(i, first, operands, prev_sample, hist_in, hist_out, pred_x0, quantile)

    def _update_args(self, i, first, operands: dict, prev_sample, hist_in, hist_out, pred_x0, quantile):
        sa, sb, a, b, c = self.multistep_coefficients(i, first)
        cfg = self.config
        clip = self.form == DATA_FORM and bool(getattr(cfg, "clip_sample", False))
        return L.MultistepStepArgs(pred_type=_PRED[cfg.prediction_type], form=self.form, clip=int(clip),
                                   clip_range=float(getattr(cfg, "clip_sample_range", 1.0)), sqrt_a=sa, sqrt_b=sb, a=a, b=b, c=c,
                                   hist_in=_ptr(hist_in) if c != 0.0 else None, prev_sample=_ptr(prev_sample), hist_out=_ptr(hist_out),
                                   pred_x0=_ptr(pred_x0), quantile=_ptr(quantile), sample_max_value=float(getattr(cfg, "sample_max_value", 1.0)),
                                   **operands)

    def solver_step(self, i: int, sample, model_out, prev_sample, hist_in, hist_out, stream: int, uncond_out=None, w=None,
                    guidance_cfg=False, pred_x0=None, first: bool = False):
        """What one update enqueues: the ``pd_multistep_step`` struct, or -- ``thresholding=True`` -- a :class:`MultistepThresholdStep`
        on ``stream`` (its scratch set is the scheduler's, one per (B, n, device, stream), as ``DDIMScheduler.threshold_step``'s).
        ``sample`` is a dense fp32 (B, ...) tensor; the other buffers are such tensors or raw device pointers."""
        cfg = self.config
        if not (self.form == DATA_FORM and getattr(cfg, "thresholding", False)):
            return self.multistep_step_args(i, sample, model_out, prev_sample, hist_in, hist_out, uncond_out, w, guidance_cfg, pred_x0, first)
        x0_raw, quant, workspace = self._threshold_scratch(sample, stream)
        operands = step_operands(sample, model_out, uncond_out, w, guidance_cfg)      # one dict: both structs name the same operands
        update = self._update_args(i, first, operands, prev_sample, hist_in, hist_out, pred_x0, quant)
        sa, sb = self.multistep_coefficients(i, first)[:2]
        raw = L.DdimStepThresholdArgs(pred_type=_PRED[cfg.prediction_type], use_clipped_model_output=0, sqrt_a=sa, sqrt_b=sb, sqrt_ap=0.0,
                                      dir_coef=0.0, prev_sample=_ptr(prev_sample), pred_x0=None, quantile=quant.data_ptr(),
                                      sample_max_value=float(cfg.sample_max_value), **operands)
        q = abs_quantile_args(sample, cfg.dynamic_thresholding_ratio, x0_raw, quant, workspace)
        return MultistepThresholdStep(update, raw, q, x0_raw, quant, workspace, int(stream))

    def _device_step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None, variance_noise=None,
                     uncond_output=None, w=None, guidance_cfg=False, out=None, want_x0=True, stream=None):
        """The eager update at ``timestep`` (``DDIMScheduler._device_step``'s signature: the pipeline calls either).  The step's position
        is ``timesteps``' index of ``timestep``; a step that does not follow the one before it (the first of a trajectory, a start
        part-way down the grid, another batch shape) has no history and is first-order.  ``use_clipped_model_output`` has no meaning
        here and is ignored; ``generator`` is not read (eta = 0: no variance noise)."""
        if eta != 0 or variance_noise is not None:
            raise ValueError(f"{type(self).__name__} is a deterministic ODE solver: eta = {eta} / variance noise has no SDE variant here")
        x, mo, prev, x0, uo, wt, st = self._prepare_step(model_output, sample, uncond_output, w, out, want_x0 and self.form == DATA_FORM, stream)
        i = self.step_index(timestep)
        hist = self._hist
        first = hist is None or self._next_index != i or hist[0].shape != x.shape or hist[0].device != x.device
        if hist is None or hist[0].shape != x.shape or hist[0].device != x.device:
            hist = self._hist = (torch.empty_like(x), torch.empty_like(x))
        a = self.solver_step(i, x, mo, prev, hist[(i + 1) % 2], hist[i % 2], st, uo, wt, guidance_cfg, x0, first)
        if isinstance(a, ThresholdStep):
            a.enqueue(st)
        else:
            L.check(L.lib().pd_multistep_step(C.byref(a), st), "pd_multistep_step")
        self._next_index = i + 1
        return prev, x0

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False, generator=None,
             variance_noise=None, return_dict: bool = True):
        if generator is not None:
            raise ValueError(f"{type(self).__name__} is a deterministic ODE solver: it draws no variance noise, so it takes no generator")
        prev, x0 = self._device_step(model_output, timestep, sample, eta, use_clipped_model_output, None, variance_noise)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev, pred_original_sample=x0)


class DPMSolverMultistepScheduler(_MultistepBase):
    """diffusers ``DPMSolverMultistepScheduler`` surface for DPM-Solver++ 2M ("dpmsolver++", "midpoint"), on ``DDIMScheduler``'s tables
    and timestep grid: ``DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`` samples in the data form.  Step ``i``
    evaluates the model at ``timesteps[i]`` and moves from ``levels[i]`` to ``levels[i + 1]``; the last level is alpha_bar = 1
    (``final_sigmas_type="zero"``) or ``alphas_cumprod[0]`` ("sigma_min").  ``clip_sample`` (default False, diffusers' behaviour; a
    scheduler made ``from_config`` of a DDIM config clips as that DDIM does) and ``thresholding`` limit x0 as ``DDIMScheduler`` does.
    ``set_alpha_to_one`` is kept in the config for the round trip and not used."""
    form = DATA_FORM

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 clip_sample=False, set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon", thresholding=False,
                 dynamic_thresholding_ratio=0.995, clip_sample_range=1.0, sample_max_value=1.0, timestep_spacing="leading",
                 rescale_betas_zero_snr=False, solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint",
                 lower_order_final=True, final_sigmas_type="zero", **ignored):
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2, got {solver_order}")
        if algorithm_type != "dpmsolver++":
            raise ValueError(f"algorithm_type {algorithm_type!r}: DPMSolverMultistepScheduler samples with 'dpmsolver++' only")
        if solver_type != "midpoint":
            raise ValueError(f"solver_type {solver_type!r}: 'midpoint' only")
        if final_sigmas_type not in ("zero", "sigma_min"):
            raise ValueError(f"final_sigmas_type must be 'zero' or 'sigma_min', got {final_sigmas_type!r}")
        if thresholding:
            quantile_rank(1, dynamic_thresholding_ratio)
            if not float(sample_max_value) > 0:
                raise ValueError(f"sample_max_value must be positive, got {sample_max_value}")
        cfg = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                   trained_betas=_beta_list(trained_betas), clip_sample=clip_sample, set_alpha_to_one=set_alpha_to_one,
                   steps_offset=steps_offset, prediction_type=prediction_type, thresholding=bool(thresholding),
                   dynamic_thresholding_ratio=dynamic_thresholding_ratio, clip_sample_range=clip_sample_range,
                   sample_max_value=sample_max_value, timestep_spacing=timestep_spacing, rescale_betas_zero_snr=rescale_betas_zero_snr,
                   solver_order=solver_order, algorithm_type=algorithm_type, solver_type=solver_type,
                   lower_order_final=bool(lower_order_final), final_sigmas_type=final_sigmas_type)
        self._finish_init(cfg, rescale_betas_zero_snr)
        self.timesteps = torch.from_numpy(np.arange(num_train_timesteps)[::-1].copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps: int, device=None):
        grid = sampler_grid(self.config, num_inference_steps)
        if self.config.final_sigmas_type == "zero":
            final = 1.0
        elif int(grid[-1]) == 0:
            raise ValueError("final_sigmas_type='sigma_min' with a grid that ends at timestep 0: the last step would not move")
        else:
            final = self._acp64(0)
        self._set_path(num_inference_steps, grid, [self._acp64(t) for t in grid] + [final])
        return self


class DPMSolverMultistepInverseScheduler(_MultistepBase):
    """The inversion that pairs with :class:`DPMSolverMultistepScheduler`: the same second-order multistep rule in the noise form
    ("dpmsolver"), climbing the sampler's own grid.  The data form is singular going up from sigma ~ 0, the noise form is not.
    Path: ``u = sorted({0} | sampler grid)``, ``timesteps = u[:-1]``; step ``j`` regards the sample as at ``alphas_cumprod[u_j]``,
    evaluates the model there and moves to ``alphas_cumprod[u_{j + 1}]``, so the inversion ends exactly at the level the sampler starts
    from (S steps; S - 1 on a grid that already holds 0).  No clamp, no thresholding (as ``DDIMInverseScheduler``), and no
    ``lower_order_final`` (the sampler's key, ignored here: the last step of an inversion is at high noise, where second order is stable)."""
    form = NOISE_FORM

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 steps_offset=0, prediction_type="epsilon", timestep_spacing="leading", rescale_betas_zero_snr=False, solver_order=2,
                 **ignored):
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2, got {solver_order}")
        cfg = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                   trained_betas=_beta_list(trained_betas), steps_offset=steps_offset, prediction_type=prediction_type,
                   timestep_spacing=timestep_spacing, rescale_betas_zero_snr=rescale_betas_zero_snr, solver_order=solver_order)
        self._finish_init(cfg, rescale_betas_zero_snr)
        self.timesteps = torch.from_numpy(np.arange(num_train_timesteps).copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps: int, device=None):
        u = sorted({0} | {int(t) for t in sampler_grid(self.config, num_inference_steps)})
        self._set_path(num_inference_steps, np.array(u[:-1], dtype=np.int64), [self._acp64(t) for t in u])
        return self

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False, variance_noise=None,
             return_dict: bool = True):
        prev, _ = self._device_step(model_output, timestep, sample, eta, False, None, variance_noise, want_x0=False)
        if not return_dict:
            return (prev, None)
        return SchedulerOutput(prev_sample=prev, pred_original_sample=None)


def inverse_scheduler(forward, variant: str = "0.18.2"):
    """The inversion that pairs with a forward scheduler, from its config: the multistep inverse for a multistep sampler,
    ``DDIMInverseScheduler(variant=...)`` otherwise.  The one place the transfers choose."""
    if isinstance(forward, DPMSolverMultistepScheduler):
        return DPMSolverMultistepInverseScheduler.from_config(forward.config)
    return DDIMInverseScheduler.from_config(forward.config, variant=variant)
