#!/usr/bin/env python3
"""Captured from-noise generation under classifier-free guidance with and without the guidance rescale, in ONE process
(docs/LAB_r25.md).  GPU only.
    python scripts/bench_guidance_rescale.py [--model super_small --size 256] [--batch 32 --dtype bf16] [--steps 50] [--w 3.0] [--rounds 3]
  rescale_0    GenerationGraph(w, guidance_rescale=0): two UNet evaluations and ONE pd_ddim_step (combine + update) per step
  rescale_0.7  GenerationGraph(w, guidance_rescale=0.7): two UNet evaluations, pd_guidance_rescale (in place on the conditional
               output), pd_ddim_step on it alone
Each figure is images / s over a window of at least MIN_WINDOW_S seconds of whole batches after a warm batch, wall clock around a device
synchronise; the two configurations are alternated per round.

The launches alone, on scratch tensors of the trajectory's shape, LAUNCHES back-to-back launches between two events after a warm one:
pd_ddim_step (plain, and with the guidance combine inside: what rescale_0 launches), pd_guidance_rescale (both of its kernels; out of
place, so that 200 launches do not compound) and their share of a batch's time.  Bytes: pd_guidance_rescale reads both predictions
twice and writes once (5 streams of 4 bytes an element), pd_ddim_step 3 (+ 1 with the combine).  Prints one JSON line."""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import phendiff_amd as P
import phendiff_amd._lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="super_small")
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "f32"])
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--w", type=float, default=3.0)
ap.add_argument("--rescale", type=float, default=0.7)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
MIN_WINDOW_S, LAUNCHES = 1.0, 200
dev = torch.device("cuda:0")
B, size, S = args.batch, args.size, args.steps
torch.manual_seed(0)
unet = P.CustomCondUNet2DModel(compute_dtype=args.dtype, **dict(P.UNET_CONFIGS[args.model], sample_size=size)).to(dev)
pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
labels = (torch.arange(B, device=dev) % 2).long()
names = ("rescale_0", f"rescale_{args.rescale:g}")
# (the runners share the model's launch plan -- its activations, not their graphs: they replay one after the other)
runners = {name: P.GenerationGraph(pipe, B, S, P.DeviceNoise(1234, dev), w=args.w, guidance_rescale=phi)
           for name, phi in zip(names, (0.0, args.rescale))}
assert runners[names[0]].rescale is None and runners[names[1]].rescale is not None


def window(runner):
    """images / s: whole batches until MIN_WINDOW_S has passed, between two synchronises."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        runner.run(labels)
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= MIN_WINDOW_S:
            return B * n / dt, n


def launch_us(fn, args_struct, name):
    """Microseconds per call: LAUNCHES back-to-back calls between two events on the current stream, after a warm one."""
    lib, st = L.lib(), torch.cuda.current_stream(dev).cuda_stream
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        L.check(lib.pd_event_create(C.byref(e)), "pd_event_create")
    L.check(fn(C.byref(args_struct), st), name)
    torch.cuda.synchronize()
    L.check(lib.pd_event_record(ev[0], st), "pd_event_record")
    for _ in range(LAUNCHES):
        L.check(fn(C.byref(args_struct), st), name)
    L.check(lib.pd_event_record(ev[1], st), "pd_event_record")
    ms = C.c_float()
    L.check(lib.pd_event_elapsed_ms(ev[0], ev[1], C.byref(ms)), "pd_event_elapsed_ms")
    for e in ev:
        lib.pd_event_destroy(e)
    return 1e3 * ms.value / LAUNCHES


out = {"model": args.model, "size": size, "batch": B, "dtype": args.dtype, "steps": S, "w": args.w, "rounds": args.rounds,
       "min_window_s": MIN_WINDOW_S}
for r in runners.values():                              # warm every shape the timed windows use
    r.run(labels)
torch.cuda.synchronize()
rates = {name: [] for name in runners}
for _ in range(args.rounds):
    for name, r in runners.items():
        rates[name].append(window(r))
med = {}
for name in runners:
    v = [x for x, _ in rates[name]]
    med[name] = statistics.median(v)
    out[name] = {"images_per_s_median": round(med[name], 2), "min": round(min(v), 2), "max": round(max(v), 2),
                 "batches_per_window": rates[name][0][1]}
out[names[1]]["over_rescale_0"] = round(med[names[1]] / med[names[0]], 4)

# the launches alone (a middle step's coefficients)
x, cond, uncond, dst = (torch.randn(B, unet.config.in_channels, size, size, device=dev) for _ in range(4))
w = torch.tensor([args.w], dtype=torch.float32, device=dev)
sch = pipe.scheduler
sch.set_timesteps(S)
lib, t_mid = L.lib(), sch.timesteps[S // 2]
us_step = launch_us(lib.pd_ddim_step, sch.ddim_step_args(t_mid, x, cond, dst), "pd_ddim_step")
us_step_cfg = launch_us(lib.pd_ddim_step, sch.ddim_step_args(t_mid, x, cond, dst, uncond, w), "pd_ddim_step")
us_rescale = launch_us(lib.pd_guidance_rescale, P.GuidanceRescale(cond, uncond, w, args.rescale, out=dst).args, "pd_guidance_rescale")
nbytes = x.numel() * 4
per_batch_us = {name: 1e6 * B / med[name] for name in runners}
out["launches"] = {
    "numel": x.numel(), "launches": LAUNCHES,
    "pd_ddim_step_us": round(us_step, 2), "pd_ddim_step_streams": 3, "pd_ddim_step_gb_s": round(3 * nbytes / us_step / 1e3, 1),
    "pd_ddim_step_guided_us": round(us_step_cfg, 2), "pd_ddim_step_guided_streams": 4,
    "pd_ddim_step_guided_gb_s": round(4 * nbytes / us_step_cfg / 1e3, 1),
    "pd_guidance_rescale_us": round(us_rescale, 2), "pd_guidance_rescale_streams": 5,
    "pd_guidance_rescale_gb_s": round(5 * nbytes / us_rescale / 1e3, 1),
    "pd_guidance_rescale_over_pd_ddim_step": round(us_rescale / us_step, 3),
    "added_per_step_us": round(us_rescale + us_step - us_step_cfg, 2),
    "added_share_of_batch_time": round(S * (us_rescale + us_step - us_step_cfg) / per_batch_us[names[0]], 5)}
print(json.dumps(out))
