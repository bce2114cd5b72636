"""References, bounds and shared inputs for dynamic thresholding (pd_abs_quantile, pd_ddim_raw_x0, pd_ddim_step_threshold,
DDIMScheduler(thresholding=True)), in the form of tests/flat_refs.py: an f64 reference from the same fp32 inputs, an fp32 replica that
calibrates the bound on the CPU (tests/test_host_threshold.py), and element-wise bounds (k + 1) * u * S with the roundings counted beside
them.  The ground truth of the quantile is torch.quantile on the CPU.  A plain module: tests/test_host_threshold.py and
tests/test_gpu_threshold.py import the same builders and case lists."""
import numpy as np
import torch

import flat_refs as R
from flat_refs import F32, F64, U, bound

# ================================================================================================ pd_abs_quantile
QUANTILE_QS = (0.995, 0.5, 0.0, 1.0)
# (B, n): within one wave | 16-byte loads, one chunk | several workgroups per row (8192-element chunks) | n % 4 == 0 with a ragged last
# chunk of a row that spans none whole: 2880 | the real size, once (3 x 256 x 256)
QUANTILE_SHAPES = ((3, 48), (2, 3072), (3, 20480), (5, 5 * 24 * 24))
QUANTILE_REAL_SHAPE = (2, 196608)
# n % 4 != 0: the element-load kernel, one chunk and a ragged second one
QUANTILE_ODD_SHAPES = ((3, 75), (2, 8192 + 1201))
QUANTILE_CONTENTS = ("normal", "levels", "equal", "below_one", "zeros_subnormals", "inf")
# the n x q grid on which the fp32 restatement of torch.quantile was checked bit for bit
RANK_GRID_N = (8, 48, 200, 1000, 3072, 2880, 196608, 2097152)
RANK_GRID_Q = (0.995, 0.9, 0.5, 0.999, 1.0, 0.0)


def quantile_truth(x, q):
    """torch.quantile(|x|, q, dim=1) on the CPU: fp32 [B].  A row that holds a NaN gives NaN."""
    return torch.quantile(torch.as_tensor(x).abs(), float(q), dim=1).numpy()


def quantile_input(B, n, kind):
    g = R.rng(19, B, n, QUANTILE_CONTENTS.index(kind))
    if kind == "normal":
        return R.normal(g, B, n, scale=1.7)
    if kind == "levels":       # 7 levels, both signs: heavy ties, every rank falls inside a run
        levels = np.array([0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.75], dtype=F32)
        return (levels[g.integers(0, 7, size=(B, n))] * g.choice(np.array([-1.0, 1.0], dtype=F32), size=(B, n))).astype(F32)
    if kind == "equal":        # one value a row (a saturated sample): the contention worst case
        return np.repeat(np.array([[-1.0], [2.5], [0.75], [1e-3], [4.0]], dtype=F32)[:B], n, axis=1)
    if kind == "below_one":
        return (g.random((B, n)) * 1.98 - 0.99).astype(F32)
    if kind == "zeros_subnormals":
        x = np.zeros((B, n), dtype=F32)
        x[:, 1::2] = -0.0
        k = n // 3
        x[:, :k] = (g.integers(1, 1 << 23, size=(B, k)).astype(np.uint32)).view(F32) * g.choice(np.array([-1.0, 1.0], dtype=F32), size=(B, k))
        return x
    if kind == "inf":          # one infinity a row, either sign
        x = R.normal(g, B, n, scale=1.7)
        x[np.arange(B), g.integers(0, n, size=B)] = np.array([np.inf, -np.inf] * B, dtype=F32)[:B]
        return x
    raise ValueError(kind)


def seam_input(n):
    """(x [1][n], q): half of the values tiny (~1e-30), half huge (~1e30), and q such that rank lo is the largest tiny value and rank hi the
    smallest huge one: the two order statistics differ in the TOP digit of the select.  Built, not drawn."""
    assert n % 2 == 0 and n >= 4
    g = R.rng(23, n)
    tiny = (1e-30 * (1.0 + g.random(n // 2))).astype(F32)
    huge = (1e30 * (1.0 + g.random(n // 2))).astype(F32)
    x = np.concatenate([tiny, -huge])
    g.shuffle(x)
    q = (n / 2 - 0.5) / (n - 1)                     # r = n/2 - 1/2 up to fp32 rounding: lo = n/2 - 1, hi = n/2
    from phendiff_amd.schedulers import quantile_rank
    lo, hi, w = quantile_rank(n, q)
    assert (lo, hi) == (n // 2 - 1, n // 2) and 0 < w < 1, (lo, hi, w)
    return x[None, :], q


def lerp_f32(a, b, w):
    """torch.lerp in fp32, every operation rounded on its own."""
    a, b, w = F32(a), F32(b), F32(w)
    with np.errstate(all="ignore"):
        d = F32(b - a)
        return F32(a + F32(w * d)) if w < F32(0.5) else F32(b - F32(d * F32(F32(1.0) - w)))


def quantile_numpy(x, q):
    """quantile_rank, then sort and lerp in numpy: the restatement of torch.quantile the kernel implements."""
    from phendiff_amd.schedulers import quantile_rank
    a = np.sort(np.abs(np.asarray(x, dtype=F32)), axis=1)          # (NaN sorts last)
    lo, hi, w = quantile_rank(a.shape[1], q)
    out = np.array([lerp_f32(r[lo], r[hi], w) for r in a], dtype=F32)
    out[np.isnan(a).any(axis=1)] = np.nan
    return out


def same_bits(got, want):
    """Bit-equal, or NaN where the ground truth is NaN."""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))


# ================================================================================================ pd_ddim_step_threshold, s given
STEP_SHAPES = ((8, 48), (2, 3072))                      # numel 8 * 48 and 2 * 3072
STEP_MAX_VALUES = (1.0, 1.5, 4.0)
# the raw quantiles of the rows (cycled): below 1, between 1 and the maximum, above it, for every maximum above
STEP_QUANTILES = (0.5, 1.25, 2.0, 3.0, 5.0, 0.9, 1.4, 9.0)
STEP_GUIDANCE = (None, (0, (2.5,)), (1, (0.7,)))        # none, imagen, CFG
# one weight per sample: per_sample % 4 == 3, so 4-vectors straddle two samples; numel % 4 == 3 and 1, a ragged last vector
PER_SAMPLE_SHAPES = ((5, 723), (3, 75))
PER_SAMPLE_WEIGHTS = (0.5, 1.7, 3.0, 2.5, 0.3)          # all different: an element that takes a neighbour's weight misses the bound


def step_input(B, per):
    g = R.rng(29, B, per)
    return dict(sample=R.normal(g, B, per, scale=1.3), model_out=R.normal(g, B, per, scale=1.3), uncond_out=R.normal(g, B, per, scale=1.3),
                quantile=np.array([STEP_QUANTILES[b % len(STEP_QUANTILES)] for b in range(B)], dtype=F32))


def threshold_s(quantile, max_value, dt=F64):
    """s = clamp(q, min = 1, max = sample_max_value), min first: exact in any precision (a selection, no arithmetic)."""
    return np.minimum(np.maximum(np.asarray(quantile).astype(dt), dt(1.0)), dt(max_value))[:, None]


def _combine(inp, guidance, dt):
    x, o = inp["sample"].astype(dt), inp["model_out"].astype(dt)
    if guidance is not None:
        cfg, w = guidance
        un, w = inp["uncond_out"].astype(dt), R._ddim_w(w, x.shape[0], dt)
        d = o - un
        o = (o + w * d) if cfg else (un + w * d)
    return x, o


def _step(inp, coef, pred, ucm, max_value, guidance, dt):
    sa, sb, sap, dc = (dt(c) for c in coef)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x, o = _combine(inp, guidance, dt)
        if pred == 0:
            x0, eps = (x - sb * o) / sa, o
        elif pred == 1:
            x0, eps = o, (x - sa * o) / sb
        else:
            x0, eps = sa * x - sb * o, sa * o + sb * x
        raw = x0
        s = threshold_s(inp["quantile"], max_value, dt)
        x0 = np.clip(x0, -s, s) / s
        if ucm:
            eps = (x - sa * x0) / sb
        return sap * x0 + dc * eps, x0, raw


def step_f64(inp, coef, pred, ucm, max_value, guidance=None):
    """(prev_sample, thresholded x0, raw x0) in float64 from the fp32 inputs, s from inp["quantile"]."""
    return _step(inp, coef, pred, ucm, max_value, guidance, F64)


def step_f32_replica(inp, coef, pred, ucm, max_value, guidance=None):
    return _step(inp, coef, pred, ucm, max_value, guidance, F32)


def step_bound(inp, coef, pred, ucm, max_value, guidance=None):
    """(bound of prev_sample, bound of the thresholded x0, bound of the raw x0)."""
    sa, sb, sap, dc = (float(c) for c in coef)
    x, o = np.abs(inp["sample"].astype(F64)), np.abs(inp["model_out"].astype(F64))
    s = threshold_s(inp["quantile"], max_value)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        k_o, S_o = 0, o
        if guidance is not None:
            # out = o + w (o - u)  or  u + w (o - u): sub (1), mul (1), add (1) = 3 roundings
            cfg, w = guidance
            un, w = np.abs(inp["uncond_out"].astype(F64)), np.abs(R._ddim_w(w, x.shape[0], F64))
            k_o, S_o = 3, (o if cfg else un) + w * (o + un)
        if pred == 0:
            # x0 = (x - sb * out) / sa: out (k_o), mul (1), sub (1), div (1);  eps = out
            k_r, S_r, k_e, S_e = k_o + 3, (x + sb * S_o) / sa, k_o, S_o
        elif pred == 1:
            # x0 = out;  eps = (x - sa * x0) / sb: out (k_o), mul (1), sub (1), div (1)
            k_r, S_r, k_e, S_e = k_o, S_o, k_o + 3, (x + sa * S_o) / sb
        else:
            # x0 = sa * x - sb * out, eps = sa * out + sb * x: out (k_o), mul (1), mul (1), add (1)
            k_r, S_r, k_e, S_e = k_o + 3, sa * x + sb * S_o, k_o + 3, sa * S_o + sb * x
        # clamp(x0, -s, s) is exact and 1-Lipschitz, and its error never exceeds the width 2 s of the range (finite where sqrt_a == 0 sent
        # the raw x0 to +-inf); then the division by s: one more rounding (s itself is exact: a selection among q, 1 and the maximum)
        k_t = k_r + 1
        S_t = np.minimum(S_r, 2 * s / ((k_r + 1) * U)) / s
        if ucm:
            # eps = (x - sa * x0) / sb: x0 (k_t), mul (1), sub (1), div (1)
            k_e, S_e = k_t + 3, (x + sa * S_t) / sb
        # prev = sap * x0 + dir * eps: the longer of the two paths, mul (1), mul (1), add (1)
        S_p = sap * S_t + dc * S_e
        return bound(max(k_t, k_e) + 3, S_p), bound(k_t, S_t), bound(k_r, S_r)


# ================================================================================================ eager scheduler.step
def make_threshold_ref(cfg, ratio, max_value):
    """The oracle's DDIMSchedulerRef with diffusers' _threshold_sample in the clamp's place.  The parent asserts thresholding=False, so it is
    constructed that way and the flag is set afterwards.  `.s_raw`: per step the unclamped quantiles [B] (what the pipeline tests' premise
    -- s exceeds 1 somewhere for every sample -- is asserted on)."""
    from oracle import DDIMSchedulerRef

    class ThresholdingDDIMSchedulerRef(DDIMSchedulerRef):
        def _threshold_sample(self, x0):
            shape = x0.shape
            a = x0.reshape(shape[0], -1).abs()
            s = torch.quantile(a, self.config.dynamic_thresholding_ratio, dim=1)
            self.s_raw.append(s.clone())
            s = torch.clamp(s, min=1, max=self.config.sample_max_value).unsqueeze(1)
            flat = x0.reshape(shape[0], -1)
            return (torch.clamp(flat, -s, s) / s).reshape(shape)

        def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None, variance_noise=None,
                 return_dict=True):
            prev_t = timestep - self.config.num_train_timesteps // self.num_inference_steps
            a = self.alphas_cumprod[timestep]
            ap = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
            b = 1 - a
            pt = self.config.prediction_type
            if pt == "epsilon":
                x0, eps = (sample - b ** 0.5 * model_output) / a ** 0.5, model_output
            elif pt == "sample":
                x0, eps = model_output, (sample - a ** 0.5 * model_output) / b ** 0.5
            else:
                x0, eps = (a ** 0.5) * sample - (b ** 0.5) * model_output, (a ** 0.5) * model_output + (b ** 0.5) * sample
            if self.config.thresholding:
                x0 = self._threshold_sample(x0)
            elif self.config.clip_sample:
                x0 = x0.clamp(-self.config.clip_sample_range, self.config.clip_sample_range)
            std = eta * self._get_variance(timestep, prev_t) ** 0.5
            if use_clipped_model_output:
                eps = (sample - a ** 0.5 * x0) / b ** 0.5
            prev = ap ** 0.5 * x0 + (1 - ap - std ** 2) ** 0.5 * eps
            if eta > 0:
                if variance_noise is None:
                    variance_noise = torch.randn(model_output.shape, generator=generator, dtype=model_output.dtype)
                prev = prev + std * variance_noise
            if not return_dict:
                return (prev,)
            from oracle.schedulers_ref import _Out
            return _Out(prev_sample=prev, pred_original_sample=x0)

    cfg = {k: v for k, v in cfg.items() if k not in ("thresholding", "dynamic_thresholding_ratio", "sample_max_value")}
    ref = ThresholdingDDIMSchedulerRef(thresholding=False, **cfg)
    ref.config.thresholding = True
    ref.config.dynamic_thresholding_ratio = ratio
    ref.config.sample_max_value = max_value
    ref.s_raw = []
    return ref


def eager_step_bounds(inp, coef, pred, ucm, max_value, x0_thresholded):
    """Bounds on |GPU - reference subclass| for s [B], the thresholded x0 and prev_sample of ONE eager step without guidance.  Both sides
    compute in fp32 from the same inputs, so each lies within the f64-relative bound of its own value and they differ by at most twice it.

    s: an order statistic is 1-Lipschitz in the sup norm (perturb every element by at most e and every order statistic moves by at most e)
       and the lerp is a convex combination of two of them, so |s_gpu - s_ref| <= e0 + the lerp's own roundings on either side, with
       e0 = max over the row of |x0_gpu - x0_ref| <= 2 * (bound of the raw x0).  lerp = a + w * (b - a): sub (1), mul (1), add (1) on terms of
       magnitude <= 3 * max |x0| of the row.  The clamp to [1, maximum] is 1-Lipschitz.
    x0: f(x0, s) = clamp(x0 / s, -1, 1) has |df/dx0| <= 1 / s <= 1 and |df/ds| = |x0| / s^2 <= 1 / s <= 1 (inside the range; outside it is
       constant), so |dx0| <= e0 + e_s, plus the division's rounding on either side: 2 * u * |x0_thresholded| <= 2 * u.
    prev = sap * x0 + dir * eps: eps differs by at most twice its own bound (use_clipped_model_output: eps = (x - sa x0) / sb takes x0's
       error times sa / sb and three roundings on either side); then mul, mul, add on either side."""
    sa, sb, sap, dc = (float(c) for c in coef)
    _, _, raw_b = step_bound(inp, coef, pred, False, max_value)
    _, _, raw = step_f64(inp, coef, pred, False, max_value)
    e0 = 2 * raw_b.max(axis=1)
    amax = np.abs(raw).max(axis=1)
    e_s = e0 + 2 * bound(3, 3 * amax)
    e_x0 = (e0 + e_s)[:, None] + 2 * U * np.abs(x0_thresholded)
    xs, os_ = inp["sample"].astype(F64), inp["model_out"].astype(F64)
    x, o = np.abs(xs), np.abs(os_)
    if ucm:
        eps_abs = np.abs((xs - sa * x0_thresholded) / sb)
        e_eps = sa * e_x0 / sb + 2 * bound(3, (x + sa * np.abs(x0_thresholded)) / sb)
    else:
        # the raw eps of the step: the eps path of step_bound without thresholding, on either side (epsilon prediction: eps IS the input)
        eps_abs = o if pred == 0 else (np.abs((xs - sa * os_) / sb) if pred == 1 else np.abs(sa * os_ + sb * xs))
        e_eps = 2 * (bound(0, 0 * o) if pred == 0 else bound(3, (x + sa * o) / sb) if pred == 1 else bound(3, sa * o + sb * x))
    e_prev = sap * e_x0 + dc * e_eps + 2 * bound(3, sap * np.abs(x0_thresholded) + dc * eps_abs)
    return e_s, e_x0, e_prev
