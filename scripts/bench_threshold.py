#!/usr/bin/env python3
"""Dynamic thresholding at the flagship size: B samples of C x S x S (docs/LAB_r19.md).  GPU only.
    python scripts/bench_threshold.py [B C S]          (default 32 3 256)
pd_abs_quantile alone (on a normal batch, a saturated one and an all-equal one); the whole thresholded step (DDIMScheduler.threshold_step:
pd_ddim_raw_x0 + pd_abs_quantile + pd_ddim_step_threshold) beside the plain pd_ddim_step, both in place, alternated in ONE process over
ROUNDS rounds of ITERS launches (UNET_ITERS for the UNet) between device events after a warm call; and, for scale, one evaluation of the
super_small UNet's launch plan at the same batch (bf16 engine, the benchmark's).  Prints one JSON line."""
import ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import phendiff_amd as P
from phendiff_amd import _lib as L
from phendiff_amd.schedulers import quantile_rank

B, CH, S = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (32, 3, 256)
ROUNDS, ITERS, UNET_ITERS = 7, 500, 10          # 500 launches of 10 to 70 us: windows of 5 to 35 ms
HBM_MEASURED = 6.29e12          # float4 copy (MI355X_MICROARCH: 79 % of the 8.0 TB/s datasheet figure)
dev, lib = torch.device("cuda:0"), L.lib()
st = torch.cuda.current_stream(dev).cuda_stream
n = CH * S * S
gen = torch.Generator(device=dev).manual_seed(0)


def timed(fn, iters=ITERS):
    """ms per call: `iters` calls between two events, after one warm call."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


out = {"shape": [B, CH, S, S], "rounds": ROUNDS, "iters": ITERS, "unet_iters": UNET_ITERS}

# ---- pd_abs_quantile alone: three passes over B * n fp32 values (the first from HBM or the infinity cache, the others likewise)
normal = torch.randn((B, n), generator=gen, device=dev) * 1.7
batches = {"normal": normal, "saturated": normal.clamp(-1, 1), "all_equal": torch.full((B, n), 0.75, device=dev)}
q_out = torch.empty((B,), dtype=torch.float32, device=dev)
ws = torch.empty((lib.pd_abs_quantile_workspace(B, n),), dtype=torch.uint8, device=dev)
lo, hi, w = quantile_rank(n, 0.995)
for name, x in batches.items():
    a = L.AbsQuantileArgs(B=B, n=n, rank_lo=lo, rank_hi=hi, weight=w, x=x.data_ptr(), out=q_out.data_ptr(), workspace=ws.data_ptr())
    L.check(lib.pd_abs_quantile(C.byref(a), st), "pd_abs_quantile")
    assert torch.equal(q_out.cpu(), torch.quantile(x.abs().cpu(), 0.995, dim=1)), name      # the figure belongs to a right answer
    t = [timed(lambda: lib.pd_abs_quantile(C.byref(a), st)) for _ in range(ROUNDS)]
    out["abs_quantile_" + name] = dict(spread(t), read_GBps=round(3 * B * n * 4 / statistics.median(t) / 1e6, 1),
                                       share_of_measured_hbm=round(3 * B * n * 4 / (statistics.median(t) * 1e-3) / HBM_MEASURED, 4))

# ---- the thresholded step beside the plain one, in place, the benchmark's scheduler config
cfg = P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
plain, thr = P.DDIMScheduler(**cfg), P.DDIMScheduler(**cfg, thresholding=True, sample_max_value=4.0)
plain.set_timesteps(50), thr.set_timesteps(50)
t_mid = int(plain.timesteps[25])
x = torch.randn((B, CH, S, S), generator=gen, device=dev)
model_out = torch.randn((B, CH, S, S), generator=gen, device=dev)
work = x.clone()
a_plain = plain.ddim_step_args(t_mid, work, model_out, work)
step = thr.threshold_step(t_mid, work, model_out, work, st)


def run_plain():
    L.check(lib.pd_ddim_step(C.byref(a_plain), st), "pd_ddim_step")


t_plain, t_thr = [], []
for _ in range(ROUNDS):
    t_plain.append(timed(run_plain))
    t_thr.append(timed(lambda: step.enqueue(st)))
out["ddim_step"] = spread(t_plain)
out["threshold_step"] = spread(t_thr)

# ---- for scale: one UNet evaluation of the same batch's launch plan
unet = P.CustomCondUNet2DModel(compute_dtype="bf16", **dict(P.UNET_CONFIGS["super_small"], sample_size=S, in_channels=CH, out_channels=CH)).to(dev)
plan = unet.plan_for(B, S, S, dev)
ts = torch.full((B,), float(t_mid), dtype=torch.float32, device=dev)
labels = (torch.arange(B, device=dev) % 2).to(torch.int64)
temb = plan.temb_rows(ts, labels, None, st)
y = torch.empty_like(x)
t_unet = [timed(lambda: plan.run(x.data_ptr(), temb.data_ptr(), y.data_ptr(), st), UNET_ITERS) for _ in range(ROUNDS)]
out["unet_eval_bf16"] = spread(t_unet)
u = statistics.median(t_unet)
out["ratio_to_one_unet_eval"] = {"abs_quantile_normal": round(out["abs_quantile_normal"]["median_ms"] / u, 4),
                                 "threshold_step": round(statistics.median(t_thr) / u, 4), "ddim_step": round(statistics.median(t_plain) / u, 4),
                                 "threshold_step_minus_ddim_step": round((statistics.median(t_thr) - statistics.median(t_plain)) / u, 4)}
print(json.dumps(out))
