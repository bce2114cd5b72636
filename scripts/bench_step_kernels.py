#!/usr/bin/env python3
"""Per-launch time of the five scheduler-step entry points at the workload's shape, B x C x S x S fp32 (docs/LAB_r27.md).  GPU only.
    python scripts/bench_step_kernels.py [B C S]          (default 32 3 256)
pd_ddim_step (plain, and with the guidance combine under one weight per sample), pd_ddim_raw_x0, pd_ddim_step_threshold,
pd_multistep_step (second order, and with the guidance combine), pd_guided_step: each in place, the runners' form, ITERS back-to-back
launches between two device events after a warm one, alternated over ROUNDS rounds in ONE process.  A same-box A/B of two builds of the
library runs this script once per build and round with PD_LIB (scripts/build_rev.sh).  Prints one JSON line: microseconds per launch."""
import ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import phendiff_amd as P
from phendiff_amd import _lib as L

B, CH, S = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (32, 3, 256)
ROUNDS, ITERS = 5, 500
dev, lib = torch.device("cuda:0"), L.lib()
st = torch.cuda.current_stream(dev).cuda_stream
gen = torch.Generator(device=dev).manual_seed(0)
x, mo, un, h0, h1, gd, gu = (torch.randn((B, CH, S, S), generator=gen, device=dev) for _ in range(7))
w = torch.linspace(0.5, 3.0, B, device=dev)
quant = torch.full((B,), 2.0, device=dev)
raw = torch.empty_like(x)

cfg = P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
ddim, thr = P.DDIMScheduler(**cfg), P.DDIMScheduler(**cfg, thresholding=True, sample_max_value=4.0)
ms = P.DPMSolverMultistepScheduler.from_config(ddim.config)
for s in (ddim, thr, ms):
    s.set_timesteps(50)
t_mid = int(ddim.timesteps[25])
step_thr = thr.threshold_step(t_mid, x, mo, x, st).step
sa, sb, sap, dirc, _ = ddim.step_coefficients(t_mid)
guided = L.GuidedStepArgs(numel=x.numel(), per_sample=x[0].numel(), pred_type=L.PD_PRED[cfg["prediction_type"]], clip=1, clip_range=1.0,
                          use_clipped_model_output=0, sqrt_a=sa, sqrt_b=sb, sqrt_ap=sap, dir_coef=dirc, guidance_scale=0.1, grad_scale=None,
                          sample=x.data_ptr(), g_direct=gd.data_ptr(), g_unet=gu.data_ptr(), model_out=mo.data_ptr(), prev_sample=x.data_ptr(),
                          pushed=None, overflow=None)
LAUNCHES = {
    "pd_ddim_step": (lib.pd_ddim_step, (ddim.ddim_step_args(t_mid, x, mo, x),)),
    "pd_ddim_step_guided": (lib.pd_ddim_step, (ddim.ddim_step_args(t_mid, x, mo, x, un, w),)),
    "pd_ddim_raw_x0": (lib.pd_ddim_raw_x0, (step_thr, raw.data_ptr())),
    "pd_ddim_step_threshold": (lib.pd_ddim_step_threshold, (step_thr,)),
    "pd_multistep_step": (lib.pd_multistep_step, (ms.multistep_step_args(25, x, mo, x, h0, h1),)),
    "pd_multistep_step_guided": (lib.pd_multistep_step, (ms.multistep_step_args(25, x, mo, x, h0, h1, un, w),)),
    "pd_guided_step": (lib.pd_guided_step, (guided,)),
}
step_thr.quantile = quant.data_ptr()      # a fixed quantile: pd_abs_quantile is not part of this comparison


def launch_us(fn, args):
    call = lambda: L.check(fn(C.byref(args[0]), *args[1:], st), fn.__name__)
    call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        call()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / ITERS


times = {name: [] for name in LAUNCHES}
for _ in range(ROUNDS):
    for name, (fn, args) in LAUNCHES.items():
        times[name].append(launch_us(fn, args))
out = {"shape": [B, CH, S, S], "rounds": ROUNDS, "iters": ITERS, "library": os.path.relpath(L.LIB_PATH)}
for name, v in times.items():
    out[name] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
print(json.dumps(out))
