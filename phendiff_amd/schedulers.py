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
        sa, sb, sap, dirc, _ = self.step_coefficients(timestep, eta)
        ptr = lambda b: b.data_ptr() if torch.is_tensor(b) else b
        if numel is None:
            numel, per_sample = sample.numel(), sample[0].numel()
        if w_per_sample is None:
            w_per_sample = torch.is_tensor(w) and w.numel() > 1
        c = self.config
        return L.DdimStepArgs(numel=numel, per_sample=per_sample, pred_type=_PRED[c.prediction_type], clip=int(bool(c.clip_sample)),
                              clip_range=float(c.clip_sample_range), use_clipped_model_output=int(bool(use_clipped_model_output)),
                              sqrt_a=sa, sqrt_b=sb, sqrt_ap=sap, dir_coef=dirc, sample=ptr(sample), model_out=ptr(model_out),
                              uncond_out=ptr(uncond_out), w=ptr(w), w_per_sample=int(w_per_sample), guidance_cfg=int(guidance_cfg),
                              prev_sample=ptr(prev_sample), pred_x0=ptr(pred_x0))

    def _device_step(self, model_output, timestep, sample, eta, use_clipped_model_output, generator, variance_noise,
                     uncond_output=None, w=None, guidance_cfg=False, out=None, want_x0=True, stream=None):
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
            uo = uncond_output.contiguous().float()      # the kernel reads dense fp32, as it does model_output
            wt = (w if torch.is_tensor(w) else torch.tensor([float(w)])).to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
        st = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
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
        n = self.config.num_train_timesteps
        if num_inference_steps > n:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than {n}")
        self.num_inference_steps = num_inference_steps
        mode = self.config.timestep_spacing
        if mode == "linspace":
            grid = np.linspace(0, n - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        elif mode == "leading":
            grid = (np.arange(num_inference_steps) * (n // num_inference_steps)).round()[::-1].copy().astype(np.int64)
            grid += self.config.steps_offset
        elif mode == "trailing":
            grid = np.round(np.arange(n, 0, -(n / num_inference_steps))).astype(np.int64) - 1
        else:
            raise ValueError(f"{mode} is not supported. Choose one of 'leading', 'trailing' or 'linspace'.")
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
        x0_raw, quant, workspace = bufs
        sa, sb, sap, dirc, _ = self.step_coefficients(timestep, eta)
        ptr = lambda b: b.data_ptr() if torch.is_tensor(b) else b
        step = L.DdimStepThresholdArgs(
            numel=B * n, per_sample=n, pred_type=_PRED[c.prediction_type], use_clipped_model_output=int(bool(use_clipped_model_output)),
            sqrt_a=sa, sqrt_b=sb, sqrt_ap=sap, dir_coef=dirc, sample=ptr(sample), model_out=ptr(model_out), uncond_out=ptr(uncond_out),
            w=ptr(w), w_per_sample=int(torch.is_tensor(w) and w.numel() > 1), guidance_cfg=int(guidance_cfg), prev_sample=ptr(prev_sample),
            pred_x0=ptr(pred_x0), quantile=quant.data_ptr(), sample_max_value=float(c.sample_max_value))
        lo, hi, wgt = quantile_rank(n, float(c.dynamic_thresholding_ratio))
        q = L.AbsQuantileArgs(B=B, n=n, rank_lo=lo, rank_hi=hi, weight=wgt, x=x0_raw.data_ptr(), out=quant.data_ptr(),
                              workspace=workspace.data_ptr())
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
