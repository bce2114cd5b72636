"""References, error bounds and shared inputs for pd_multistep_step and the two multistep schedulers (DPMSolverMultistepScheduler,
DPMSolverMultistepInverseScheduler), in the style of tests/flat_refs.py (whose `bound`, `within`, inputs and case lists are used here):

    multistep_f64           the kernel in float64 from the same fp32 inputs, written from the formula in include/phendiff_hip.h
    multistep_f32_replica   the same formula as separate fp32 numpy operations in the kernel's order; it exists only to calibrate the
                            bound: tests/test_host_multistep.py asserts replica-within-bound on the CPU
    multistep_bound         (k + 1) * u * S per output, k = fp32 roundings on the path, S = sum of magnitudes of the terms added on it
    ref_*                   the schedulers restated in float64 numpy: grid, levels, coefficients, the loop -- the definition the
                            schedulers' docstring gives, written a second time, so that a slip in either shows
    analytic_*              a model whose probability-flow ODE has a closed form: data N(0.3, 0.25) per pixel

A plain module (no fixtures, no hooks): tests/test_host_multistep.py and tests/test_gpu_multistep.py import the same builders."""
import itertools
import math

import numpy as np

import flat_refs as R

F32, F64, U = R.F32, R.F64, R.U
DATA, NOISE = 0, 1
SAMPLE_MAX_VALUE = 1.5                  # the thresholded cases: s = clamp(q, 1, 1.5) takes all three branches over the q below
THRESHOLD_Q = (0.7, 1.2, 2.5)           # per sample (B = 3): below 1 -> s = 1; inside -> s = q; above sample_max_value -> s = 1.5


# ================================================================================================ the schedulers, restated
def ref_grid(n, S, spacing, offset=0):
    """t_0 > ... > t_{S-1}: diffusers' three spacings."""
    if spacing == "linspace":
        return [int(v) for v in np.linspace(0, n - 1, S).round()[::-1]]
    if spacing == "leading":
        return [int(v) + offset for v in (np.arange(S) * (n // S)).round()[::-1]]
    assert spacing == "trailing"
    return [int(v) - 1 for v in np.round(np.arange(n, 0, -(n / S)))]


def ref_sampler_path(acp, grid, final="zero"):
    """(timesteps, levels) of the sampler: step i evaluates at grid[i] and moves from acp[grid[i]] to acp[grid[i + 1]]; last: final."""
    acp = np.asarray(acp, dtype=F64)
    return list(grid), [float(acp[t]) for t in grid] + [1.0 if final == "zero" else float(acp[0])]


def ref_inverse_path(acp, grid):
    """(timesteps, levels) of the inversion: u = sorted({0} | grid); step j evaluates at u_j and moves from acp[u_j] to acp[u_{j+1}]."""
    acp = np.asarray(acp, dtype=F64)
    u = sorted(set([0] + list(grid)))
    return u[:-1], [float(acp[t]) for t in u]


def _lam(abar):
    if abar >= 1.0:
        return math.inf
    if abar <= 0.0:
        return -math.inf
    return math.log(math.sqrt(abar)) - math.log(math.sqrt(1.0 - abar))


def ref_coefficients(levels, form, order=2, lower_order_final=False):
    """Per step (sqrt_a, sqrt_b, a, b, c) in float64."""
    n = len(levels) - 1
    out, h_prev = [], None
    for i in range(n):
        s, t = levels[i], levels[i + 1]
        al_s, sg_s, al_t, sg_t = math.sqrt(s), math.sqrt(1 - s), math.sqrt(t), math.sqrt(1 - t)
        h = _lam(t) - _lam(s) if s != t else 0.0
        if form == DATA:
            a, b = (0.0, 1.0) if t == 1.0 else ((sg_t, al_t) if s == 0.0 else (sg_t / sg_s, -al_t * math.expm1(-h)))
        else:
            a, b = (0.0, 1.0) if t == 0.0 else (al_t / al_s, -sg_t * math.expm1(h))
        c = 0.0
        if (order == 2 and i > 0 and math.isfinite(h) and h != 0 and math.isfinite(h_prev) and h_prev != 0
                and not (lower_order_final and i == n - 1 and n < 15)):
            c = 0.5 * b * h / h_prev
        out.append((al_s, sg_s, a, b, c))
        h_prev = h
    return out


def as_f32(coefs):
    """What the argument struct holds: every coefficient rounded to fp32 once (returned as float64 values)."""
    return [tuple(float(F32(v)) for v in c) for c in coefs]


def ref_m0(x, o, sa, sb, form, pred):
    """The model's output in the solver's variable: x0 (data form) or eps (noise form), by prediction type (0 eps, 1 sample, 2 v)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if pred == 0:
            x0, eps = (x - sb * o) / sa, o
        elif pred == 1:
            x0, eps = o, (x - sa * o) / sb
        else:
            x0, eps = sa * x - sb * o, sa * o + sb * x
    return x0 if form == DATA else eps


def ref_loop(x, model, timesteps, levels, coefs, form, pred=0, clip=None):
    """The scheduler's loop in float64: model(x, t, abar) at the level the sample is at, m0, the update.  Returns the list of states
    (x before every step, then the end) and of m0.  `coefs`: ref_coefficients' (or their fp32 roundings)."""
    x = np.asarray(x, dtype=F64)
    xs, ms, m1 = [x], [], None
    for i, (t, (sa, sb, a, b, c)) in enumerate(zip(timesteps, coefs)):
        m0 = ref_m0(x, model(x, t, levels[i]), sa, sb, form, pred)
        if form == DATA and clip is not None:
            m0 = np.clip(m0, -clip, clip)
        x = a * x + b * m0 + (c * (m0 - m1) if c != 0 else 0.0)
        m1 = m0
        xs.append(x)
        ms.append(m0)
    return xs, ms


# ================================================================================================ the analytic model
MU, VAR = 0.3, 0.25
Z = np.array([-1.3, 0.2, 0.9], dtype=F64)


def analytic_var(abar):
    return abar * VAR + 1.0 - abar


def analytic_eps(x, t, abar):
    """The exact noise prediction of data N(MU, VAR): eps*(x, abar) = sigma (x - alpha MU) / (abar VAR + 1 - abar)."""
    return math.sqrt(1.0 - abar) * (x - math.sqrt(abar) * MU) / analytic_var(abar)


def analytic_flow(abar, z=Z):
    """The exact solution of the probability-flow ODE through z: x(abar) = alpha MU + sqrt(abar VAR + 1 - abar) z."""
    return math.sqrt(abar) * MU + math.sqrt(analytic_var(abar)) * np.asarray(z, dtype=F64)


def analytic_constants(abar):
    """(c1, c2) fp32 values with eps*(x) = (x - c1) * c2: what a device evaluation of the model multiplies by (two fp32 operations)."""
    return float(F32(math.sqrt(abar) * MU)), float(F32(math.sqrt(1.0 - abar) / analytic_var(abar)))


def analytic_eps_rounded(x, t, abar):
    """analytic_eps with the two constants rounded to fp32: the function a device loop evaluates in fp32 and ref_loop in float64."""
    c1, c2 = analytic_constants(abar)
    return (x - c1) * c2


def loop_bound(xs, ms, levels, coefs, form, E0=None):
    """Element-wise bound on |device trajectory - ref_loop's| at the end of every step, accumulated: epsilon prediction by
    analytic_eps_rounded evaluated in fp32 on the device's own state, then pd_multistep_step.  With E_x the bound of the state:
        o = (x - c1) * c2: sub (1), mul (1) = 2 roundings of magnitude (|x| + c1) c2, plus the state's error times the slope c2
        m0: noise form  = o;   data form  (x - sb o) / sa: the operands' errors (E_x + sb E_o) / sa, plus mul (1), sub (1), div (1)
        x' = a x + b m0 + c (m0 - m1): |a| E_x + |b| E_m0 + |c| (E_m0 + E_m1), plus sub, 3 mul, 2 add = 6 roundings
    Returns the list of E_x after each step.  `E0`: the bound the state starts with (a loop that continues another one's end)."""
    E_x, E_m1, out = (np.zeros_like(xs[0]) if E0 is None else E0), None, []
    for i, (sa, sb, a, b, c) in enumerate(coefs):
        x, m0 = np.abs(xs[i]), np.abs(ms[i])
        c1, c2 = analytic_constants(levels[i])
        E_o = c2 * E_x + R.bound(2, (x + c1) * c2)
        o = (x + c1) * c2
        E_m = E_o if form == NOISE else (E_x + sb * E_o) / sa + R.bound(3, (x + sb * o) / sa)
        m1 = np.abs(ms[i - 1]) if (c != 0 and i > 0) else 0.0
        E_x = abs(a) * E_x + abs(b) * E_m + abs(c) * (E_m + (E_m1 if c != 0 else 0.0)) + R.bound(6, abs(a) * x + abs(b) * m0 + abs(c) * (m0 + m1))
        E_m1 = E_m
        out.append(E_x)
    return out


# ================================================================================================ pd_multistep_step
def schedule_coefficients():
    """{form: [(sqrt_a, sqrt_b, a, b, c) fp32 at the first, a middle and the last step]} of a 50-step schedule of the
    3k_steps_clipping_rescaling config (trailing, zero terminal SNR) and of its inverse.  Sampler: the first has sqrt_a == 0 and
    (a, b, c) = (sigma_t, alpha_t, 0), the middle one c != 0, the last (0, 1, 0).  Inverse: first c == 0, middle c != 0, last (0, 1, 0)."""
    from phendiff_amd.configs import SCHEDULER_CONFIGS
    from phendiff_amd.schedulers import DPMSolverMultistepInverseScheduler, DPMSolverMultistepScheduler
    cfg = SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
    out = {}
    for form, cls in ((DATA, DPMSolverMultistepScheduler), (NOISE, DPMSolverMultistepInverseScheduler)):
        s = cls.from_config(cfg)
        s.set_timesteps(50)
        out[form] = [tuple(F32(v) for v in s.multistep_coefficients(i)) for i in (0, 25, len(s.timesteps) - 1)]
    return out


def multistep_input(B, per):
    """flat_refs.ddim_input (some x0 inside, some outside the clip range; elements 0 and 1 of the prediction on the boundary) plus the
    previous step's prediction."""
    inp = R.ddim_input(B, per)
    inp["hist_in"] = R.normal(R.rng(11, B, per), B, per)
    return inp


def multistep_cases():
    """(form, step index into schedule_coefficients, pred, clip): the data form with and without the static clamp, the noise form
    without (it has none)."""
    return ([(DATA, ti, pred, clip) for ti, pred, clip in itertools.product(range(3), R.PRED_TYPES, (0, 1))]
            + [(NOISE, ti, pred, 0) for ti, pred in itertools.product(range(3), R.PRED_TYPES)])


def _s_of(q, dt):
    """s = min(max(q, 1), sample_max_value) per sample, as a column."""
    s = np.asarray(q, dtype=F32).astype(dt)
    s = np.where(s < 1, dt(1.0), s)
    s = np.where(s > dt(F32(SAMPLE_MAX_VALUE)), dt(F32(SAMPLE_MAX_VALUE)), s)
    return s[:, None]


def _combine(inp, guidance, dt):
    x, o = inp["sample"].astype(dt), inp["model_out"].astype(dt)
    if guidance is not None:
        cfg, w = guidance
        un, w = inp["uncond_out"].astype(dt), R._ddim_w(w, x.shape[0], dt)
        d = o - un
        o = (o + w * d) if cfg else (un + w * d)
    return x, o


def _multistep(inp, coef, form, pred, clip, guidance, quantile, dt):
    sa, sb, a, b, c = (dt(v) for v in coef)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x, o = _combine(inp, guidance, dt)
        m0 = ref_m0(x, o, sa, sb, form, pred)
        if form == DATA and quantile is not None:
            s = _s_of(quantile, dt)
            m0 = np.clip(m0, -s, s) / s
        elif form == DATA and clip:
            m0 = np.clip(m0, dt(-R.CLIP_RANGE), dt(R.CLIP_RANGE))
        prev = a * x + b * m0
        if c != 0:
            prev = prev + c * (m0 - inp["hist_in"].astype(dt))
        return prev, m0


def multistep_f64(inp, coef, form, pred, clip, guidance=None, quantile=None):
    """(prev_sample, m0 = hist_out = pred_x0).  `coef`: (sqrt_a, sqrt_b, a, b, c) fp32.  c == 0: hist_in is not looked at."""
    return _multistep(inp, coef, form, pred, clip, guidance, quantile, F64)


def multistep_f32_replica(inp, coef, form, pred, clip, guidance=None, quantile=None):
    return _multistep(inp, coef, form, pred, clip, guidance, quantile, F32)


def multistep_bound(inp, coef, form, pred, clip, guidance=None, quantile=None):
    """(bound of prev_sample, bound of m0)."""
    sa, sb, a, b, c = (abs(float(v)) for v in coef)
    x, o = np.abs(inp["sample"].astype(F64)), np.abs(inp["model_out"].astype(F64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        k_o, S_o = 0, o
        if guidance is not None:
            # out = o + w (o - u)  or  u + w (o - u): sub (1), mul (1), add (1) = 3 roundings
            cfg, w = guidance
            un, w = np.abs(inp["uncond_out"].astype(F64)), np.abs(R._ddim_w(w, x.shape[0], F64))
            k_o, S_o = 3, (o if cfg else un) + w * (o + un)
        # m0 by prediction type: as flat_refs.ddim_bound's x0 (data form) and eps (noise form)
        if pred == 0:
            k_m, S_m = (k_o + 3, (x + sb * S_o) / sa) if form == DATA else (k_o, S_o)
        elif pred == 1:
            k_m, S_m = (k_o, S_o) if form == DATA else (k_o + 3, (x + sa * S_o) / sb)
        else:
            k_m, S_m = (k_o + 3, sa * x + sb * S_o) if form == DATA else (k_o + 3, sa * S_o + sb * x)
        if form == DATA and quantile is not None:
            # clamp(x0, -s, s) / s: the clamp is exact and 1-Lipschitz and its result lies in [-s, s]; the division is one rounding
            s = _s_of(quantile, F64)
            S_m = np.minimum(S_m, 2 * s / ((k_m + 1) * U)) / s
            k_m += 1
        elif form == DATA and clip:
            # (keeps the bound finite where sqrt_a == 0 sends x0 to +-inf before the clamp)
            S_m = np.minimum(S_m, 2 * R.CLIP_RANGE / ((k_m + 1) * U))
        # prev = a x + b m0: m0 (k_m), mul (1), mul (1), add (1);  + c (m0 - m1): sub (1), mul (1), add (1)
        S_p = a * x + b * S_m
        k_p = k_m + 3
        if c != 0:
            S_p, k_p = S_p + c * (S_m + np.abs(inp["hist_in"].astype(F64))), k_m + 6
        return R.bound(k_p, S_p), R.bound(k_m, S_m)
