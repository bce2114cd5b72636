#!/usr/bin/env python3
"""Captured DDIB under DDIM against the multistep pair (DPMSolverMultistepScheduler + its inverse), in ONE process (docs/LAB_r24.md).
GPU only.
    python scripts/bench_multistep.py [--model super_small --size 256] [--batch 32 --dtype bf16] [--rounds 3] [--no-box]
  ddim_50       DDIBGraph, 50 + 50 DDIM steps: the benchmark's trajectory
  multistep_50  DDIBGraph under the multistep pair, 50 + 50 steps: the same UNet evaluations, the step kernel exchanged
  multistep_25  25 + 25 steps,  multistep_20  20 + 20 steps: what the second order is for
Each figure is images / s over a window of at least MIN_WINDOW_S seconds of whole batches after a warm batch, wall clock around a device
synchronise; the configurations are alternated per round.  What this says about image quality at the lower step counts: nothing -- that
takes trained weights (tests/test_host_multistep.py has the orders of convergence on a model with a closed-form flow).

The step launches alone: pd_ddim_step and pd_multistep_step (second order, in place, the runner's arguments) at the trajectory's shape,
LAUNCHES back-to-back launches between two events after a warm one, and their share of a trajectory's time (launches per trajectory x
time per launch / time per batch).  The clock and power of card 0 are sampled once a second through a REPEAT of ddim_50 after the timed
windows (none inside them).  Prints one JSON line."""
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-box", action="store_true")
args = ap.parse_args()
MIN_WINDOW_S, LAUNCHES = 1.0, 200
dev = torch.device("cuda:0")
B, size = args.batch, args.size
torch.manual_seed(0)
unet = P.CustomCondUNet2DModel(compute_dtype=args.dtype, **dict(P.UNET_CONFIGS[args.model], sample_size=size)).to(dev)
cfg = P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
ddim_pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**cfg))
ms_pipe = P.ConditionalDDIMPipeline(unet, P.DPMSolverMultistepScheduler.from_config(ddim_pipe.scheduler.config))
g = torch.Generator().manual_seed(1234)
images = (torch.rand(B, unet.config.in_channels, size, size, generator=g) * 2 - 1).to(dev)
labels = (torch.arange(B, device=dev) % 2).long()

CONFIGS = (("ddim_50", ddim_pipe, 50), ("multistep_50", ms_pipe, 50), ("multistep_25", ms_pipe, 25), ("multistep_20", ms_pipe, 20))
# (the runners share the model's launch plan -- its activations, not their graphs: they replay one after the other)
runners = {name: P.DDIBGraph(pipe, batch_size=B, num_inference_steps=S) for name, pipe, S in CONFIGS}


def window(runner):
    """images / s: whole batches until MIN_WINDOW_S has passed, between two synchronises."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        runner.run(images, labels, 1 - labels)
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= MIN_WINDOW_S:
            return B * n / dt, n


def launch_us(fn, args_struct, name):
    """Microseconds per launch: LAUNCHES back-to-back launches between two events on the current stream, after a warm one."""
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


out = {"model": args.model, "size": size, "batch": B, "dtype": args.dtype, "rounds": args.rounds, "min_window_s": MIN_WINDOW_S}
for r in runners.values():                              # warm every shape the timed windows use
    r.run(images, labels, 1 - labels)
torch.cuda.synchronize()
rates = {name: [] for name in runners}
for _ in range(args.rounds):
    for name, r in runners.items():
        rates[name].append(window(r))
med = {}
for name, (_, _, S) in zip(runners, CONFIGS):
    v = [x for x, _ in rates[name]]
    med[name] = statistics.median(v)
    out[name] = {"steps": f"{S} + {S}", "images_per_s_median": round(med[name], 2), "min": round(min(v), 2), "max": round(max(v), 2),
                 "batches_per_window": rates[name][0][1], "step_launches_per_batch": len(runners[name].inv_args) + len(runners[name].gen_args)}
for name in list(runners)[1:]:
    out[name]["over_ddim_50"] = round(med[name] / med["ddim_50"], 3)

# the step launches alone, on scratch tensors of the trajectory's shape (the runner's in-place form; a middle step: c != 0)
x, mo, h0, h1 = (torch.randn(B, unet.config.in_channels, size, size, device=dev) for _ in range(4))
sd, sm = ddim_pipe.scheduler, ms_pipe.scheduler
sd.set_timesteps(50), sm.set_timesteps(50)
lib = L.lib()
us_ddim = launch_us(lib.pd_ddim_step, sd.ddim_step_args(sd.timesteps[25], x, mo, x), "pd_ddim_step")
us_ms = launch_us(lib.pd_multistep_step, sm.multistep_step_args(25, x, mo, x, h0, h1), "pd_multistep_step")
us_ms_first = launch_us(lib.pd_multistep_step, sm.multistep_step_args(0, x, mo, x, None, h1), "pd_multistep_step")
nbytes = x.numel() * 4
out["step_kernel"] = {"numel": x.numel(), "launches": LAUNCHES,
                      "pd_ddim_step_us": round(us_ddim, 2), "pd_ddim_step_streams": 3, "pd_ddim_step_gb_s": round(3 * nbytes / us_ddim / 1e3, 1),
                      "pd_multistep_step_us": round(us_ms, 2), "pd_multistep_step_streams": 5, "pd_multistep_step_gb_s": round(5 * nbytes / us_ms / 1e3, 1),
                      "pd_multistep_step_first_order_us": round(us_ms_first, 2), "pd_multistep_step_first_order_streams": 4,
                      "multistep_over_ddim": round(us_ms / us_ddim, 3)}
for name, us in (("ddim_50", us_ddim), ("multistep_50", us_ms), ("multistep_25", us_ms), ("multistep_20", us_ms)):
    per_batch_us = 1e6 * B / med[name]
    out[name]["step_share_of_batch_time"] = round(out[name]["step_launches_per_batch"] * us / per_batch_us, 5)

if not args.no_box:
    import re, subprocess, threading

    def box_sample():
        try:
            r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                               text=True, timeout=10)
            j = json.loads(r.stdout[r.stdout.index("{"):])
            card = j[sorted(k for k in j if k.startswith("card"))[0]]
            num = lambda v: float(re.search(r"[-+]?\d+(\.\d+)?", str(v)).group(0))
            return (next((num(v) for k, v in card.items() if "sclk" in k.lower()), None),
                    next((num(v) for k, v in card.items() if "power" in k.lower() and "(w)" in k.lower()), None))
        except Exception:
            return None

    samples, stop = [], threading.Event()

    def poll():
        while not stop.is_set():
            s = box_sample()
            if s:
                samples.append(s)
            stop.wait(1.0)
    th = threading.Thread(target=poll)
    th.start()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 4.0:
        runners["ddim_50"].run(images, labels, 1 - labels)
        torch.cuda.synchronize()
    stop.set()
    th.join()
    m = lambda v: statistics.median(v) if v else None
    out["box"] = {"sclk_mhz_median": m([s[0] for s in samples if s[0]]), "power_w_median": m([s[1] for s in samples if s[1]]),
                  "samples": len(samples), "source": "rocm-smi --showclocks --showpower, every 1 s through a repeat of ddim_50 after the timed windows"}
print(json.dumps(out))
