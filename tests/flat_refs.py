"""References, error bounds and shared inputs for the flat-buffer and time-embedding kernels (pd_grad_norm, pd_adamw_ema,
pd_diffusion_loss, pd_ddim_step, pd_add_noise, pd_postproc, pd_nchw_to_nhwc, pd_linear_wgrad / dgrad, pd_embedding_grad,
pd_guidance_apply).

For every operation:
    *_f64          the operation in float64 from the same fp32 inputs, written from the formula in include/phendiff_hip.h
    *_f32_replica  the same formula as separate fp32 numpy operations (what the header and the reference code describe);
                   it exists only to calibrate the bounds: tests/test_host_flat_refs.py asserts replica-within-bound on the CPU
    *_bound        element-wise bound on |fp32 result - f64 reference|, float64:

        bound = (k + 1) * u * S,   u = 2**-24

    k = the number of fp32 roundings on the path to that output (counted in a comment beside every bound), S = the sum of
    the magnitudes of the terms that are added or subtracted on that path (so that cancellation, and a division by a small
    sqrt_a, are covered).  A dot product of n terms: (n + 2) * u * sum |terms|.  No tolerance here is a free number.

A plain module (no fixtures, no hooks), in the style of tests/guard_bands.py: tests/test_host_flat_refs.py and
tests/test_gpu_flat_kernels.py import the SAME input builders and case lists, so both use the same seeds and shapes."""
import itertools
import math

import numpy as np

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
Q = 1 << 20              # 1024 blocks x 256 lanes x 4 floats: one sweep of pd_grad_norm's 16-byte loads


def rng(*key):
    return np.random.default_rng([20241018, *[int(k) for k in key]])


def normal(g, *shape, scale=1.0):
    return (g.standard_normal(shape) * scale).astype(F32)


def bound(k, S):
    """(k + 1) * u * S: k fp32 roundings on the path, S the sum of magnitudes of the terms added / subtracted on it."""
    return (np.asarray(k, dtype=F64) + 1.0) * U * np.asarray(S, dtype=F64)


def dot_bound(n, S):
    """(n + 2) * u * sum |terms| for a dot product (or running sum) of n terms."""
    return (np.asarray(n, dtype=F64) + 2.0) * U * np.asarray(S, dtype=F64)


def ulp32(x):
    """Spacing of fp32 at |x| (x: the float64 reference value)."""
    return float(np.spacing(np.abs(F32(x))))


def within(got, ref, bnd):
    """(all inside, largest error / bound).  Where the reference is not finite (a division by sqrt_a == 0) the result must be
    the same infinity, or NaN where the reference is NaN; a finite reference always has a finite bound."""
    got, ref, bnd = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64), np.asarray(bnd, dtype=F64)
    fin = np.isfinite(ref)
    assert np.all(np.isfinite(bnd[fin])), "finite reference with an unbounded error"
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        ok = np.where(fin, err <= bnd, same)
        ratio = np.where(fin & (bnd > 0), err / np.where(bnd > 0, bnd, 1.0), 0.0)
    # a zero bound (all terms zero) demands an exact result
    ok = np.where(fin & (bnd == 0), got == ref, ok)
    return bool(np.all(ok)), float(ratio.max()) if ratio.size else 0.0


# ================================================================================================ pd_grad_norm
GRAD_NORM_SIZES = (1, 3, 1027, Q, Q + 4, Q + 7, 2 * Q + 1201, 3 * Q + 5, 4 * Q + 310)
GRAD_NORM_MISALIGNED = (3, 1027, Q + 7, 2 * Q + 1201)
GRAD_NORM_MAX_NORMS = (1.0, 1e9, float("inf"))     # clips (norm > 1 from n = 3 on) / exceeds every norm here / disabled


def grad_norm_input(n, kind):
    if kind == "ones":
        return np.ones(n, dtype=F32)
    return normal(rng(1, n), n)


def grad_norm_f64(x):
    return float(np.sqrt(np.sum(np.square(x.astype(F64)))))


def grad_norm_f32_replica(x):
    """The header's two-stage reduction: squares and sums in fp64, 1024 partial sums (an order unlike numpy's pairwise one),
    the root rounded to fp32."""
    sq = np.square(x.astype(F64))
    pad = (-sq.size) % 1024
    partial = np.concatenate([sq, np.zeros(pad)]).reshape(-1, 1024).sum(axis=0)
    return F32(np.sqrt(partial.sum()))


def clip_coef_f32(norm, max_norm):
    """fp32 min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_)."""
    with np.errstate(over="ignore"):
        c = F32(max_norm) / (F32(norm) + F32(1e-6))
    return F32(1.0) if not c < F32(1.0) else c


# ================================================================================================ pd_adamw_ema
ADAMW_SMALL = (1, 255, 257)
ADAMW_LARGE = 2_097_152 + 773          # 8192 blocks x 256 lanes + 773: the grid-stride second sweep
ADAMW_STEPS = (1, 1000)
ADAMW_WD = (0.1, 1e-6)
ADAMW_GRADS = ("normal", "zero", "zero_all")       # zero_all: zero gradient AND zero moments (denom = eps)
# (name, clip_coef, ema given, zero_grad, ema_only)
ADAMW_VARIANTS = (("base", None, True, 1, 0), ("clip", 0.25, True, 1, 0), ("no_ema", None, False, 1, 0),
                  ("keep_grad", 0.25, True, 0, 0), ("ema_only", None, True, 1, 1), ("ema_only_keep_grad", None, True, 0, 1),
                  ("ema_only_no_ema", None, False, 0, 1))


def adamw_hyper(t, wd, lr=1e-4, b1=0.95, b2=0.999, eps=1e-8):
    """What FlatAdamWEMA.step hands over: python doubles, rounded to fp32 by the args struct."""
    omd = 0.05 if t == 1 else 1e-4
    h = dict(lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, step_size=lr / (1 - b1 ** t),
             bias_correction2_sqrt=math.sqrt(1 - b2 ** t), one_minus_decay=omd)
    return {k: F32(v) for k, v in h.items()}


def adamw_input(numel, grads, seed=0):
    g = rng(2, numel, seed)
    p, s = normal(g, numel), normal(g, numel)
    gr, m, v = normal(g, numel, scale=0.1), normal(g, numel, scale=0.05), np.square(normal(g, numel, scale=0.05))
    if grads != "normal":
        gr = np.zeros_like(gr)
    if grads == "zero_all":
        m, v = np.zeros_like(m), np.zeros_like(v)
    return dict(param=p, grad=gr, exp_avg=m, exp_avg_sq=v, ema=s)


def adamw_cases_small():
    """(t, wd, grads, variant) for the small sizes."""
    return list(itertools.product(ADAMW_STEPS, ADAMW_WD, ADAMW_GRADS, ADAMW_VARIANTS))


def adamw_cases_large():
    return [(1000, 0.1, "normal", ADAMW_VARIANTS[1]), (1, 1e-6, "normal", ADAMW_VARIANTS[2]), (1, 0.1, "normal", ADAMW_VARIANTS[4])]


def _adamw_d(inp, h, clip):
    d = {k: v.astype(F64) for k, v in inp.items()}
    hh = {k: float(v) for k, v in h.items()}
    return d, hh, (1.0 if clip is None else float(F32(clip)))


def adamw_f64(inp, h, clip, ema_only):
    """g = clip * grad; AdamW (decoupled decay, bias-corrected moments); EMA as a convex combination."""
    d, h, c = _adamw_d(inp, h, clip)
    if ema_only:
        p, m, v = d["param"], d["exp_avg"], d["exp_avg_sq"]
    else:
        g = c * d["grad"]
        m = h["beta1"] * d["exp_avg"] + (1 - h["beta1"]) * g
        v = h["beta2"] * d["exp_avg_sq"] + (1 - h["beta2"]) * g * g
        p = d["param"] - h["lr"] * h["weight_decay"] * d["param"] - h["step_size"] * m / (np.sqrt(v) / h["bias_correction2_sqrt"] + h["eps"])
    ema = (1 - h["one_minus_decay"]) * d["ema"] + h["one_minus_decay"] * p
    return dict(param=p, exp_avg=m, exp_avg_sq=v, ema=ema)


def adamw_f32_replica(inp, h, clip, ema_only):
    """torch.optim.AdamW's single-tensor update (mul_, lerp_, mul_.addcmul_, sqrt / bc2 + eps, addcdiv_) and EMAModel.step
    (s -= (1 - decay) * (s - p)) as separate fp32 operations."""
    one = F32(1.0)
    p, m, v, s = inp["param"], inp["exp_avg"], inp["exp_avg_sq"], inp["ema"]
    if not ema_only:
        g = inp["grad"] * (one if clip is None else F32(clip))
        p = p * (one - h["lr"] * h["weight_decay"])
        m = m + (g - m) * (one - h["beta1"])
        v = v * h["beta2"] + (g * g) * (one - h["beta2"])
        denom = np.sqrt(v) / h["bias_correction2_sqrt"] + h["eps"]
        p = p - h["step_size"] * (m / denom)
    s = s - h["one_minus_decay"] * (s - p)
    return dict(param=p, exp_avg=m, exp_avg_sq=v, ema=s)


def adamw_bound(inp, h, clip, ema_only):
    d, h, c = _adamw_d(inp, h, clip)
    p0, m0, v0, s0 = np.abs(d["param"]), np.abs(d["exp_avg"]), d["exp_avg_sq"], np.abs(d["ema"])
    omd = h["one_minus_decay"]
    zero = np.zeros_like(p0)
    if ema_only:
        # ema = s - omd * (s - p): sub, mul, sub = 3 roundings; param and the moments are not touched (exact)
        return dict(param=zero, exp_avg=zero, exp_avg_sq=zero, ema=bound(3, s0 + omd * (s0 + p0)))
    g = np.abs(c * d["grad"])
    # exp_avg = m + (g - m) * (1 - b1): g = grad * coef (1), 1 - b1 (1), g - m (1), mul (1), add (1) = 5 roundings
    S_m = m0 + (g + m0) * (1 - h["beta1"])
    # exp_avg_sq = v * b2 + (g * g) * (1 - b2): g enters twice (2), g * g (1), 1 - b2 (1), mul (1), v * b2 (1), add (1) = 7 roundings
    S_v = v0 * h["beta2"] + g * g * (1 - h["beta2"])
    # denom = sqrt(v) / bc2 + eps: v (7), sqrt (1), div (1), add (1) = 10 roundings; all its terms are positive, so the relative
    # error of denom is at most 11 u and it enters param below as 10 more roundings of the quotient
    denom = np.sqrt(S_v) / h["bias_correction2_sqrt"] + h["eps"]
    # param = p * (1 - lr * wd) - step * (m / denom): lr * wd (1), 1 - . (1), p * . (1), m (5), denom (10), div (1), step * . (1),
    # sub (1) = 21 roundings; m enters with the sum of magnitudes S_m of ITS terms (g - m cancels)
    S_p = p0 * abs(1 - h["lr"] * h["weight_decay"]) + h["step_size"] * S_m / denom
    # ema = s - omd * (s - p): p (21), sub (1), mul (1), sub (1) = 24 roundings
    S_s = s0 + omd * (s0 + S_p)
    return dict(param=bound(21, S_p), exp_avg=bound(5, S_m), exp_avg_sq=bound(7, S_v), ema=bound(24, S_s))


# ================================================================================================ pd_diffusion_loss
LOSS_SHAPES = ((3, 75), (1, 1), (3, 100_003))     # the last: numel > 262 144 = one sweep of 1024 blocks x 256 lanes
PRED_TYPES = (0, 1, 2)                            # epsilon, sample, v_prediction (pd_pred_type)


def loss_input(B, per):
    g = rng(3, B, per)
    a = np.array([0.9, 0.35, 0.02][:B], dtype=F64)              # alpha_bar per sample
    return dict(model_out=normal(g, B, per), noise=normal(g, B, per), clean=normal(g, B, per),
                weight=(a / (1 - a)).astype(F32), sa=np.sqrt(a).astype(F32), sb=np.sqrt(1 - a).astype(F32))


def _loss_target(inp, pred, dt):
    o, nz, cl = (inp[k].astype(dt) for k in ("model_out", "noise", "clean"))
    w = np.ones((o.shape[0], 1), dtype=dt)
    if pred == 0:
        t = nz
    elif pred == 1:
        t, w = cl, inp["weight"].astype(dt)[:, None]
    else:
        t = inp["sa"].astype(dt)[:, None] * nz - inp["sb"].astype(dt)[:, None] * cl
    return o, t, w


def loss_f64(inp, pred, grad_scale=1.0):
    """loss = mean(w_n (out - target)^2), grad = grad_scale * 2 w_n (out - target) / numel."""
    o, t, w = _loss_target(inp, pred, F64)
    d = o - t
    return float(np.mean(w * d * d)), float(grad_scale) * 2.0 * w * d / d.size


def loss_f32_replica(inp, pred, grad_scale=1.0):
    """fp32 element-wise terms, the header's fp64 reduction, the mean rounded to fp32."""
    o, t, w = _loss_target(inp, pred, F32)
    d = o - t
    loss = F32(np.sum((w * (d * d)).astype(F64)) / d.size)
    return loss, (F32(2.0) * w * d) * (F32(1.0) / F32(d.size)) * F32(grad_scale)


def loss_bound(inp, pred, grad_scale=1.0):
    o, _, w = _loss_target(inp, pred, F64)
    nz, cl = np.abs(inp["noise"].astype(F64)), np.abs(inp["clean"].astype(F64))
    N = o.size
    if pred == 2:
        # d = out - (sa * noise - sb * clean): mul (1), mul (1), sub (1), sub (1) = 4 roundings
        k_d, S_d = 4, np.abs(o) + inp["sa"].astype(F64)[:, None] * nz + inp["sb"].astype(F64)[:, None] * cl
    else:
        # d = out - target: 1 rounding
        k_d, S_d = 1, np.abs(o) + (nz if pred == 0 else cl)
    # grad = (2 w d) * (1 / N) * grad_scale: d (k_d), 2 w * d (1), 1 / N (1), mul (1), mul (1) = k_d + 4 roundings
    g_b = bound(k_d + 4, float(grad_scale) * 2.0 * w * S_d / N)
    # loss: term = w * (d * d) with |d~ - d| <= E_d = (k_d + 1) u S_d, so |d~^2 - d^2| <= 2 |d| E_d + E_d^2; d * d (1), w * . (1)
    # = 2 roundings of the term itself; the fp64 sum adds at most N * 2^-53 relative; the mean is rounded to fp32 once (1)
    _, d64 = loss_f64(inp, pred)
    d = np.abs(d64) * N / (2.0 * w)
    E_d = bound(k_d, S_d)
    term = w * d * d
    l_b = float(np.sum(w * (2 * d * E_d + E_d * E_d) + bound(2, term)) / N + (N * 2.0 ** -53 + 2 * U) * np.sum(term) / N)
    return l_b, g_b


# ================================================================================================ pd_ddim_step
DDIM_NUMEL = (1, 3, 5, 1023, 1024, 1025)          # 1, 3: only the cnt < 4 tail; 5, 1023, 1025: vectors + tail; 1025: two blocks
DDIM_GUIDED = (3, 75)                             # per_sample % 4 == 3: a 4-vector straddles two samples; numel % 4 == 1
# (guidance_cfg, weights): one value or one per sample; w > 1 and 0 < w < 1; three different weights
DDIM_GUIDANCE = ((0, (2.5,)), (0, (0.3,)), (0, (0.5, 1.7, 3.0)), (1, (2.5,)), (1, (0.3,)), (1, (0.5, 1.7, 3.0)))
CLIP_RANGE = 1.0


def ddim_coefficients():
    """(sqrt_a, sqrt_b, sqrt_ap, dir_coef) fp32 at the first, a middle and the last timestep of a 50-step schedule of the
    3k_steps_clipping_rescaling config.  The first has sqrt_a == 0 exactly (zero terminal SNR)."""
    from phendiff_amd.configs import SCHEDULER_CONFIGS
    from phendiff_amd.schedulers import DDIMScheduler
    s = DDIMScheduler(**SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    s.set_timesteps(50)
    return [tuple(F32(c) for c in s.step_coefficients(s.timesteps[i])[:4]) for i in (0, 25, 49)]


def ddim_input(B, per):
    """Some x0 inside, some outside the clip range for every prediction type (x, out ~ N(0, 1)); elements 0 and 1 of the
    prediction are exactly +-clip_range: for sample prediction without guidance x0 sits exactly on the boundary."""
    g = rng(4, B, per)
    out = normal(g, B, per)
    flat = out.reshape(-1)
    flat[0] = CLIP_RANGE
    if flat.size > 1:
        flat[1] = -CLIP_RANGE
    return dict(sample=normal(g, B, per), model_out=out, uncond_out=normal(g, B, per))


def _ddim_w(w, B, dt):
    w = np.asarray(w, dtype=F32).astype(dt)
    return (w if w.size > 1 else np.repeat(w, B))[:, None]


def ddim_f64(inp, coef, pred, clip, ucm, guidance=None):
    sa, sb, sap, dc = (float(c) for c in coef)
    x, o = inp["sample"].astype(F64), inp["model_out"].astype(F64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if guidance is not None:
            cfg, w = guidance
            un, w = inp["uncond_out"].astype(F64), _ddim_w(w, x.shape[0], F64)
            o = (o + w * (o - un)) if cfg else (un + w * (o - un))
        if pred == 0:
            x0, eps = (x - sb * o) / sa, o
        elif pred == 1:
            x0, eps = o, (x - sa * o) / sb
        else:
            x0, eps = sa * x - sb * o, sa * o + sb * x
        if clip:
            x0 = np.clip(x0, -CLIP_RANGE, CLIP_RANGE)
        if ucm:
            eps = (x - sa * x0) / sb
        return sap * x0 + dc * eps, x0


def ddim_f32_replica(inp, coef, pred, clip, ucm, guidance=None):
    sa, sb, sap, dc = (F32(c) for c in coef)
    x, o = inp["sample"], inp["model_out"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if guidance is not None:
            cfg, w = guidance
            un, w = inp["uncond_out"], _ddim_w(w, x.shape[0], F32)
            d = o - un
            o = (o + w * d) if cfg else (un + w * d)
        if pred == 0:
            x0, eps = (x - sb * o) / sa, o
        elif pred == 1:
            x0, eps = o, (x - sa * o) / sb
        else:
            x0, eps = sa * x - sb * o, sa * o + sb * x
        if clip:
            x0 = np.clip(x0, F32(-CLIP_RANGE), F32(CLIP_RANGE))
        if ucm:
            eps = (x - sa * x0) / sb
        return sap * x0 + dc * eps, x0


def ddim_bound(inp, coef, pred, clip, ucm, guidance=None):
    """(bound of prev_sample, bound of pred_x0)."""
    sa, sb, sap, dc = (float(c) for c in coef)
    x, o = np.abs(inp["sample"].astype(F64)), np.abs(inp["model_out"].astype(F64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        k_o, S_o = 0, o
        if guidance is not None:
            # out = o + w (o - u)  or  u + w (o - u): sub (1), mul (1), add (1) = 3 roundings
            cfg, w = guidance
            un, w = np.abs(inp["uncond_out"].astype(F64)), np.abs(_ddim_w(w, x.shape[0], F64))
            k_o, S_o = 3, (o if cfg else un) + w * (o + un)
        if pred == 0:
            # x0 = (x - sb * out) / sa: out (k_o), mul (1), sub (1), div (1);  eps = out
            k_x0, S_x0, k_e, S_e = k_o + 3, (x + sb * S_o) / sa, k_o, S_o
        elif pred == 1:
            # x0 = out;  eps = (x - sa * x0) / sb: out (k_o), mul (1), sub (1), div (1)
            k_x0, S_x0, k_e, S_e = k_o, S_o, k_o + 3, (x + sa * S_o) / sb
        else:
            # x0 = sa * x - sb * out, eps = sa * out + sb * x: out (k_o), mul (1), mul (1), add (1)
            k_x0, S_x0, k_e, S_e = k_o + 3, sa * x + sb * S_o, k_o + 3, sa * S_o + sb * x
        if clip:
            # clamp is exact and 1-Lipschitz: the error does not grow, and never exceeds the width of the range (this keeps the
            # bound finite where sqrt_a == 0 sends x0 to +-inf before the clamp)
            S_x0 = np.minimum(S_x0, 2 * CLIP_RANGE / ((k_x0 + 1) * U))
        if ucm:
            # eps = (x - sa * x0) / sb: x0 (k_x0), mul (1), sub (1), div (1)
            k_e, S_e = k_x0 + 3, (x + sa * S_x0) / sb
        # prev = sap * x0 + dir * eps: the longer of the two paths, mul (1), mul (1), add (1)
        S_p = sap * S_x0 + dc * S_e
        return bound(max(k_x0, k_e) + 3, S_p), bound(k_x0, S_x0)


def ddim_cases():
    return list(itertools.product(range(3), PRED_TYPES, (0, 1), (0, 1)))      # (timestep index, pred, clip, use_clipped_model_output)


# ================================================================================================ pd_add_noise
ADD_NOISE_SHAPES = ((3, 75), (2, 257))


def add_noise_input(B, per):
    g = rng(5, B, per)
    a = np.array([0.9, 0.35, 0.02][:B], dtype=F64)
    return dict(x=normal(g, B, per), noise=normal(g, B, per), sa=np.sqrt(a).astype(F32), sb=np.sqrt(1 - a).astype(F32))


def _add_noise(inp, velocity, dt):
    x, nz, sa, sb = inp["x"].astype(dt), inp["noise"].astype(dt), inp["sa"].astype(dt)[:, None], inp["sb"].astype(dt)[:, None]
    return (sa * nz - sb * x) if velocity else (sa * x + sb * nz)


def add_noise_f64(inp, velocity):
    return _add_noise(inp, velocity, F64)


def add_noise_f32_replica(inp, velocity):
    return _add_noise(inp, velocity, F32)


def add_noise_bound(inp, velocity):
    # sa * a +- sb * b: mul (1), mul (1), add (1) = 3 roundings
    x, nz, sa, sb = np.abs(inp["x"].astype(F64)), np.abs(inp["noise"].astype(F64)), inp["sa"].astype(F64)[:, None], inp["sb"].astype(F64)[:, None]
    return bound(3, (sa * nz + sb * x) if velocity else (sa * x + sb * nz))


# ================================================================================================ pd_postproc
POSTPROC_B = 2
POSTPROC_C = (1, 3, 4)
POSTPROC_HW = ((5, 7), (16, 16), (17, 16))        # 2 x 17 x 16 = 544 pixels: three blocks of 256; 5 x 7: a partial block
POSTPROC_HALF_MARGIN = 1e-4
POSTPROC_MAX_EXCLUDED = 1e-3


def postproc_input(C, H, W):
    g = rng(6, C, H, W)
    x = g.uniform(-1.5, 1.5, (POSTPROC_B, C, H, W)).astype(F32)
    x.reshape(-1)[:6] = np.array([-1.0, 0.0, 1.0, 3.0, -3.0, 0.0], dtype=F32)[:min(6, x.size)]
    return x


def postproc_f64(x):
    """(v = clamp(x / 2 + 0.5, 0, 1) as NHWC float64, round(255 v) as NHWC uint8)."""
    v = np.clip(x.astype(F64) / 2 + 0.5, 0.0, 1.0).transpose(0, 2, 3, 1)
    return v, np.rint(255.0 * v).astype(np.uint8)


def postproc_f32_replica(x):
    v = np.clip(x / F32(2.0) + F32(0.5), F32(0.0), F32(1.0)).transpose(0, 2, 3, 1)
    return v, np.rint(v * F32(255.0)).astype(np.uint8)


def postproc_bound(x):
    # x / 2 (1, exact in fact), + 0.5 (1) = 2 roundings; the clamp is exact
    return bound(2, np.abs(x.astype(F64)) / 2 + 0.5).transpose(0, 2, 3, 1)


def postproc_u8_checked(x):
    """NHWC mask of the elements whose uint8 value must EQUAL the reference: 255 v farther than 1e-4 from a half-integer (the
    fp32 path errs by at most about 3e-5 there: two roundings of magnitude <= 1, times 255).  x == 0 is checked as well although
    255 * 0.5 = 127.5 IS a half-integer: 0.5 and 127.5 are exact in fp32 too and both sides round half to even (128)."""
    v, _ = postproc_f64(x)
    frac = 255.0 * v - np.floor(255.0 * v)
    return (np.abs(frac - 0.5) > POSTPROC_HALF_MARGIN) | (x.transpose(0, 2, 3, 1) == 0)


# ================================================================================================ pd_nchw_to_nhwc
NHWC_SHAPES = ((2, 3, 35, 8), (1, 4, 64, 32), (2, 9, 300, 16))
NHWC_LARGE = (1, 3, 2_100_000, 16)                # 4 200 000 work items > 16384 blocks x 256: the grid-stride sweep (bf16 only)


def nhwc_input(B, C, HW):
    return normal(rng(7, B, C, HW), B, C, HW)


def nhwc_bits_replica(x, Cpad, dtype):
    """[B][HW][Cpad] raw bits (fp32 -> uint32, 16-bit types -> uint16), round to nearest even spelled out for bf16."""
    B, C, HW = x.shape
    out = np.zeros((B, HW, Cpad), dtype=F32)
    out[:, :, :C] = x.transpose(0, 2, 1)
    if dtype == "f32":
        return out.view(np.uint32)
    if dtype == "fp16":
        return out.astype(np.float16).view(np.uint16)
    bits = out.view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


# ================================================================================================ fp32 time-embedding backward
LIN_ROWS = (1, 5)
LIN_IN = (1, 31, 33, 96)        # 31 / 33: the i < in_dim mask inside a 32-wide chunk, one and two chunks
LIN_OUT = (1, 7, 9, 130)        # fewer than, one more than the 8 output groups folded through LDS
EMB = dict(num_classes=7, dim=33, rows=9)
EMB_LABELS = np.array([3, 0, 3, 6, 1, 3, 0, 5, 2], dtype=np.int64)      # repeats; class 4 is absent


def linear_input(rows, in_dim, out_dim):
    g = rng(8, rows, in_dim, out_dim)
    return dict(dy=normal(g, rows, out_dim), x=normal(g, rows, in_dim), w=normal(g, out_dim, in_dim, scale=in_dim ** -0.5),
                pre=normal(g, rows, in_dim), dw0=normal(g, out_dim, in_dim), db0=normal(g, out_dim))


def _silu(x):
    return x / (1 + np.exp(-x))


def _dsilu(y):
    s = 1 / (1 + np.exp(-y))
    return s * (1 + y * (1 - s))


def linear_wgrad_f64(inp, x_silu):
    dy, x = inp["dy"].astype(F64), inp["x"].astype(F64)
    a = _silu(x) if x_silu else x
    return inp["dw0"].astype(F64) + dy.T @ a, inp["db0"].astype(F64) + dy.sum(axis=0)


def linear_wgrad_f32_replica(inp, x_silu):
    dy, x = inp["dy"], inp["x"]
    a = (x / (F32(1) + np.exp(-x))) if x_silu else x
    s, sb = np.zeros_like(inp["dw0"]), np.zeros_like(inp["db0"])
    for r in range(dy.shape[0]):
        s = s + dy[r][:, None] * a[r][None, :]
        sb = sb + dy[r]
    return inp["dw0"] + s, inp["db0"] + sb


def silu_roundings(x):
    """fp32 roundings of x / (1 + exp(-x)) with the device's fast exponential (exp2 of x * log2 e): the argument's one rounding
    reaches the result amplified by |x| ln 2 log2 e = |x|; the hardware exp2 is good to 1 ulp = 2 u (2); 1 + e (1); the division
    (1): 4 + |x|, rounded up."""
    return 4 + np.ceil(np.abs(np.asarray(x, dtype=F64)))


def linear_wgrad_bound(inp, x_silu):
    dy, x = np.abs(inp["dy"].astype(F64)), inp["x"].astype(F64)
    rows = dy.shape[0]
    a = np.abs(_silu(x)) if x_silu else np.abs(x)
    k_act = silu_roundings(x).max(axis=0)[None, :] if x_silu else 0.0
    # dw += sum_r dy * act(x): a running sum of rows + 1 terms (the old value is one), each product carrying act's roundings
    dw = dot_bound(rows + 1 + k_act, np.abs(inp["dw0"].astype(F64)) + dy.T @ a)
    # db += sum_r dy: rows + 1 terms
    return dw, dot_bound(rows + 1, np.abs(inp["db0"].astype(F64)) + dy.sum(axis=0))


def linear_dgrad_f64(inp, with_pre):
    dx = inp["dy"].astype(F64) @ inp["w"].astype(F64)
    return dx * _dsilu(inp["pre"].astype(F64)) if with_pre else dx


def linear_dgrad_f32_replica(inp, with_pre):
    dy, w = inp["dy"], inp["w"]
    s = np.zeros((dy.shape[0], w.shape[1]), dtype=F32)
    for o in range(w.shape[0]):
        s = s + dy[:, o][:, None] * w[o][None, :]
    if with_pre:
        y = inp["pre"]
        sg = F32(1) / (F32(1) + np.exp(-y))
        s = s * (sg * (F32(1) + y * (F32(1) - sg)))
    return s


def linear_dgrad_bound(inp, with_pre):
    n = inp["w"].shape[0]
    S = np.abs(inp["dy"].astype(F64)) @ np.abs(inp["w"].astype(F64))
    if not with_pre:
        return dot_bound(n, S)                   # a dot product of out_dim terms, in whatever fixed order
    # dx = dot * silu'(y), silu'(y) = s (1 + y (1 - s)), s = 1 / (1 + exp(-y)) with relative error r_s = (|y| + 4) u (as silu_roundings).
    # 1 - s: abs error s r_s + u (1 - s); y (1 - s): |y| (s r_s + 2 u (1 - s)); 1 + .: + u |1 + y (1 - s)|; times s: + (r_s + u) |silu'|.
    # Summed: |error of silu'| <= s (1 + |y|) (r_s + 4 u) = (|y| + 8) u s (1 + |y|).  The product adds one rounding to the dot's n + 2.
    y = inp["pre"].astype(F64)
    s = 1 / (1 + np.exp(-y))
    return U * S * ((n + 3) * np.abs(_dsilu(y)) + (np.ceil(np.abs(y)) + 8) * s * (1 + np.abs(y)))


def embedding_input():
    g = rng(9)
    return dict(labels=EMB_LABELS.copy(), d=normal(g, EMB["rows"], EMB["dim"]), table0=normal(g, EMB["num_classes"], EMB["dim"]))


def embedding_grad_f64(inp):
    out = inp["table0"].astype(F64)
    np.add.at(out, inp["labels"], inp["d"].astype(F64))
    return out


def embedding_grad_f32_replica(inp):
    s = np.zeros_like(inp["table0"])
    for r, k in enumerate(inp["labels"]):
        s[k] = s[k] + inp["d"][r]
    return inp["table0"] + s


def embedding_grad_bound(inp):
    # a running sum of at most rows + 1 terms (the old value is one)
    S = np.abs(inp["table0"].astype(F64))
    np.add.at(S, inp["labels"], np.abs(inp["d"].astype(F64)))
    return dot_bound(EMB["rows"] + 1, S)


# ================================================================================================ pd_guidance_apply
GUIDANCE_APPLY_NUMEL = (1, 257, 4096 * 256 + 300)  # the last: past the 4096-block grid cap, a second grid-stride sweep
GUIDANCE_APPLY_SCALE = 0.37


def guidance_apply_input(numel):
    g = rng(10, numel)
    return dict(x=normal(g, numel), g_direct=normal(g, numel), g_unet=normal(g, numel))


def guidance_apply_f64(inp, scale=GUIDANCE_APPLY_SCALE):
    return inp["x"].astype(F64) - float(F32(scale)) * (inp["g_direct"].astype(F64) + inp["g_unet"].astype(F64))


def guidance_apply_f32_replica(inp, scale=GUIDANCE_APPLY_SCALE):
    return inp["x"] - F32(scale) * (inp["g_direct"] + inp["g_unet"])


def guidance_apply_bound(inp, scale=GUIDANCE_APPLY_SCALE):
    # x - scale * (gd + gu): add (1), mul (1), sub (1) = 3 roundings
    a = {k: np.abs(v.astype(F64)) for k, v in inp.items()}
    return bound(3, a["x"] + abs(float(F32(scale))) * (a["g_direct"] + a["g_unet"]))
