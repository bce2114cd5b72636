"""Cases, seeded inputs and launch helpers shared by tests/test_gpu_step_bits.py and scripts/record_step_bits.py: the five scheduler-step
entry points -- pd_ddim_step, pd_ddim_raw_x0 -> pd_abs_quantile -> pd_ddim_step_threshold, pd_multistep_step (alone and behind the same
raw-x0 / quantile chain), pd_guided_step -- compared BIT FOR BIT with what the kernels of the revision before they were put on one quad
walker and operand former (csrc/pd_step.h) wrote under tests/golden/step_bits/.

A case is ``(kind, B, per_sample, settings)``; it runs in place with every optional output given (``a``), in place with the optional
outputs NULL (``b``) and -- the shape cases -- out of place with them given (``c``); the settings sweeps run ``a`` and ``b``, the two
grid-stride cases ``a``.  Inputs come from the seeded numpy builders of tests/flat_refs.py (element-wise operations on seeded draws
only) and every fixture carries the sha256 of the inputs it was recorded on.  Rows are scaled by ROW_SCALE so that the per-row quantile
of |x0| falls below 1, between 1 and SAMPLE_MAX_VALUE, and above it.

The shapes are the smallest at which a walker can go wrong: numel 1, 3, 5, 1023, 1024, 1025 at B = 1 (tail only; vectors + tail; exactly
one block; a second block that holds only a tail); (3, 75): vectors straddle both sample boundaries, 225 % 4 = 1; (5, 1) and (4, 3): the
row changes inside a vector; 1024 * 1024 + 1029 elements for the two grid-stride kernels (kept as a sha256 plus every 127th element)."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import torch

import flat_refs as R
import multistep_refs as M
from flat_refs import F32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_bits")
KINDS = ("ddim", "thr", "ms", "ms_thr", "guided")
SAMPLE_MAX_VALUE = 1.5
RATIO = 0.9                                  # dynamic_thresholding_ratio: a tenth of a row lies above its quantile
ROW_SCALE = (1.3, 0.25, 0.5)                 # row b's operands are scaled by ROW_SCALE[b % 3]
GUIDANCE_SCALE, GRAD_SCALE = 0.37, 4.0       # pd_guided_step: guidance_loss_scale; the device scalar (a power of two)
W3 = (0.5, 1.7, 3.0)
W5 = (0.5, 1.7, 3.0, 2.5, 0.3)
BIG = (5, (1024 * 1024 + 1029) // 5)         # 5 x 209921 = 1024 * 1024 + 1029: past the 1024-block cap, a second sweep with a tail
SAMPLE_ABOVE = 65536                         # outputs with more elements are stored as a fixed sample plus the sha256 of all of them


def variants_of(name):
    if name.endswith("_big"):
        return ("a",)
    return ("a", "b") if re.search(r"_t\d_", name) else ("a", "b", "c")        # (the settings sweeps are named ..._t<step>_p<pred>...)


def _settings(ti=1, pred=0, clip=1, ucm=0, guidance=None, form=M.DATA, bad_grad=False):
    return dict(ti=ti, pred=pred, clip=clip, ucm=ucm, guidance=guidance, form=form, bad_grad=bad_grad)


def _build_cases():
    """name -> (kind, B, per_sample, settings)."""
    cases = {}
    for kind in KINDS:
        for n in R.DDIM_NUMEL:                                                      # the walker's sizes, every entry point
            cases[f"{kind}_n{n}"] = (kind, 1, n, _settings())
        if kind == "guided":                                                        # (no combine: the shapes alone)
            for B, per in (R.DDIM_GUIDED, (5, 1), (4, 3)):
                cases[f"guided_{B}x{per}"] = ("guided", B, per, _settings(pred=2))
            cases["guided_3x75_nonfinite_grad"] = ("guided", 3, 75, _settings(pred=2, bad_grad=True))
            continue
        for cfg in (0, 1):                                                          # both equations, one weight and one per sample
            for wname, w in (("w1", (2.5,)), ("w3", W3)):
                cases[f"{kind}_3x75_cfg{cfg}_{wname}"] = (kind, 3, 75, _settings(pred=2, guidance=(cfg, w)))
        cases[f"{kind}_5x1_w5"] = (kind, 5, 1, _settings(pred=2, guidance=(0, W5)))  # the row changes inside a vector
        cases[f"{kind}_4x3_w4"] = (kind, 4, 3, _settings(pred=2, guidance=(1, W5[:4])))
    # prediction type x clip x use_clipped_model_output at the first (sqrt_a == 0), a middle and the last step of the 50-step schedule
    for ti, pred, clip, ucm in R.ddim_cases():
        cases[f"ddim_t{ti}_p{pred}_c{clip}_u{ucm}"] = ("ddim", 3, 75, _settings(ti, pred, clip, ucm, (0, W3)))
        cases[f"guided_t{ti}_p{pred}_c{clip}_u{ucm}"] = ("guided", 3, 75, _settings(ti, pred, clip, ucm))
        if clip == 0:
            cases[f"thr_t{ti}_p{pred}_u{ucm}"] = ("thr", 3, 75, _settings(ti, pred, 0, ucm, (0, W3)))
    for form, ti, pred, clip in M.multistep_cases():
        cases[f"ms_f{form}_t{ti}_p{pred}_c{clip}"] = ("ms", 3, 75, _settings(ti, pred, clip, 0, (0, W3), form))
        if form == M.DATA and clip == 0:
            cases[f"ms_thr_t{ti}_p{pred}"] = ("ms_thr", 3, 75, _settings(ti, pred, 0, 0, (0, W3)))
    cases["ms_big"] = ("ms", *BIG, _settings(pred=2, guidance=(0, W5)))
    cases["guided_big"] = ("guided", *BIG, _settings(pred=2))
    return cases


CASES = _build_cases()


def cases_of(kind):
    return [n for n, c in CASES.items() if c[0] == kind]


def make_inputs(name):
    """CPU fp32 arrays [B][per_sample]: sample, model_out, uncond_out, hist_in, g_direct, g_unet (flat_refs' seeded builders)."""
    kind, B, per, s = CASES[name]
    t = M.multistep_input(B, per)
    scale = np.array([ROW_SCALE[b % 3] for b in range(B)], dtype=F32)[:, None]
    t = {k: (v * scale).astype(F32) for k, v in t.items()}
    g = R.rng(31, B, per)
    t["g_direct"], t["g_unet"] = R.normal(g, B, per), R.normal(g, B, per, scale=GRAD_SCALE)
    if s["bad_grad"]:
        t["g_unet"].reshape(-1)[B * per // 2] = np.inf
    return t


def inputs_sha256(t):
    h = hashlib.sha256()
    for key in sorted(t):
        h.update(np.ascontiguousarray(t[key]).view(np.int32).tobytes())
    return h.hexdigest()


def coefficients(name):
    """What the case's struct carries: (sqrt_a, sqrt_b, sqrt_ap, dir_coef) of flat_refs.ddim_coefficients, or for the multistep kinds
    (sqrt_a, sqrt_b, a, b, c) of multistep_refs.schedule_coefficients."""
    kind, _, _, s = CASES[name]
    if kind in ("ms", "ms_thr"):
        return tuple(float(v) for v in M.schedule_coefficients()[s["form"]][s["ti"]])
    return tuple(float(v) for v in R.ddim_coefficients()[s["ti"]])


def _quantile_args(L, B, n, x0_raw, quant, ws):
    from phendiff_amd.schedulers import quantile_rank
    lo, hi, wgt = quantile_rank(n, RATIO)
    return L.AbsQuantileArgs(B=B, n=n, rank_lo=lo, rank_hi=hi, weight=wgt, x=x0_raw.data_ptr(), out=quant.data_ptr(), workspace=ws.data_ptr())


def _run_variant(L, lib, name, t, dev, variant):
    kind, B, per, s = CASES[name]
    st = torch.cuda.current_stream().cuda_stream
    coef = coefficients(name)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in t.items()}
    nan = lambda: torch.full((B, per), float("nan"), device=dev)
    given = variant != "b"
    x = d["sample"]
    prev = x if variant != "c" else nan()                                           # a, b: prev_sample == sample
    opt = nan() if given else None                                                  # pred_x0 / pushed
    got = {}
    common = dict(numel=B * per, per_sample=per, pred_type=s["pred"], sqrt_a=coef[0], sqrt_b=coef[1], sample=x.data_ptr(),
                  model_out=d["model_out"].data_ptr(), prev_sample=prev.data_ptr())
    guide = {}
    if s["guidance"] is not None and kind != "guided":
        cfg, w = s["guidance"]
        wt = torch.tensor(w, dtype=torch.float32).to(dev)
        guide = dict(uncond_out=d["uncond_out"].data_ptr(), w=wt.data_ptr(), w_per_sample=int(len(w) > 1), guidance_cfg=cfg)
    if kind in ("thr", "ms_thr"):
        raw, quant = nan(), torch.full((B,), float("nan"), device=dev)
        ws = torch.empty((lib.pd_abs_quantile_workspace(B, per),), dtype=torch.uint8, device=dev)
        step = L.DdimStepThresholdArgs(**common, **guide, use_clipped_model_output=s["ucm"], sqrt_ap=coef[2] if kind == "thr" else 0.0,
                                       dir_coef=coef[3] if kind == "thr" else 0.0, pred_x0=L.ptr(opt) if kind == "thr" else None,
                                       quantile=quant.data_ptr(), sample_max_value=SAMPLE_MAX_VALUE)
        L.check(lib.pd_ddim_raw_x0(C.byref(step), raw.data_ptr(), st), "pd_ddim_raw_x0")
        L.check(lib.pd_abs_quantile(C.byref(_quantile_args(L, B, per, raw, quant, ws)), st), "pd_abs_quantile")
        if kind == "thr":
            L.check(lib.pd_ddim_step_threshold(C.byref(step), st), "pd_ddim_step_threshold")
        got.update(raw=raw, quant=quant)
    if kind == "ddim":
        a = L.DdimStepArgs(**common, **guide, clip=s["clip"], clip_range=R.CLIP_RANGE, use_clipped_model_output=s["ucm"], sqrt_ap=coef[2],
                           dir_coef=coef[3], pred_x0=L.ptr(opt))
        L.check(lib.pd_ddim_step(C.byref(a), st), "pd_ddim_step")
    if kind in ("ms", "ms_thr"):
        hist_out = nan()
        x0 = opt if s["form"] == M.DATA else None                                   # (the noise form has no pred_x0)
        a = L.MultistepStepArgs(**common, **guide, form=s["form"], clip=s["clip"], clip_range=R.CLIP_RANGE, a=coef[2], b=coef[3], c=coef[4],
                                hist_in=d["hist_in"].data_ptr() if coef[4] != 0.0 else None, hist_out=hist_out.data_ptr(), pred_x0=L.ptr(x0),
                                quantile=got["quant"].data_ptr() if kind == "ms_thr" else None, sample_max_value=SAMPLE_MAX_VALUE)
        L.check(lib.pd_multistep_step(C.byref(a), st), "pd_multistep_step")
        got.update(hist_out=hist_out)
        opt = x0
    if kind == "guided":
        gs = torch.tensor([GRAD_SCALE], device=dev) if given else None              # b: grad_scale NULL = 1, no flag
        flag = torch.zeros((1,), dtype=torch.int32, device=dev) if given else None
        a = L.GuidedStepArgs(**common, clip=s["clip"], clip_range=R.CLIP_RANGE, use_clipped_model_output=s["ucm"], sqrt_ap=coef[2],
                             dir_coef=coef[3], guidance_scale=GUIDANCE_SCALE, grad_scale=L.ptr(gs), g_direct=d["g_direct"].data_ptr(),
                             g_unet=d["g_unet"].data_ptr(), pushed=L.ptr(opt), overflow=L.ptr(flag))
        L.check(lib.pd_guided_step(C.byref(a), st), "pd_guided_step")
        if flag is not None:
            got.update(overflow=flag)
    got.update(prev=prev)
    if opt is not None:
        got.update(opt=opt)
    torch.cuda.synchronize()
    return {f"{variant}_{k}": v.contiguous().view(torch.int32).cpu() for k, v in got.items()}


def run_case(L, lib, name, t, dev):
    """Launch the case's variants on ``dev``; returns {array name: CPU int32-view tensor} of everything the kernels wrote
    (``prev``; ``opt``: pred_x0 / pushed; ``raw``, ``quant``: the chain's scratch; ``hist_out``; ``overflow``)."""
    got = {}
    for variant in variants_of(name):
        got.update(_run_variant(L, lib, name, t, dev, variant))
    return got


def stored_form(got):
    """What a fixture keeps of ``run_case``'s result: small arrays whole; of a large one the sha256 and every 127th element."""
    kept = {}
    for key, v in got.items():
        a = v.contiguous().numpy()
        if a.size > SAMPLE_ABOVE:
            kept[key + "__sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            kept[key + "__sample127"] = a.reshape(-1)[::127].copy()
        else:
            kept[key] = a
    return kept


def fixture_path(kind):
    """One file per entry point (kind): its arrays are named ``<case>--<array>``."""
    return os.path.join(GOLDEN, kind + ".npz")
