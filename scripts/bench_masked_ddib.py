#!/usr/bin/env python3
"""The masked class transfer against plain captured DDIB, in ONE process (docs/LAB_r29.md).  GPU only.
    python scripts/bench_masked_ddib.py [--model super_small --size 256] [--batch 32 --dtype bf16] [--steps 50] [--num-maps 10] [--rounds 3]
  ddib       DDIBGraph: S inversion steps, the snapshot, S denoising steps (the code path of before this feature, unchanged)
  given      MaskedDDIBGraph(mask="given"): the inversion writes each step into the next kept state (no snapshot), one copy, S denoising
             steps with one pd_mask_blend each
  contrast   MaskedDDIBGraph(mask="contrast", num_maps): 2 * num_maps more UNet evaluations, num_maps pd_stream_noise and
             pd_class_contrast, one pd_contrast_mask and pd_stream_advance in front of / behind the same
Each figure is images / s over a window of at least MIN_WINDOW_S seconds of whole batches after a warm batch, wall clock around a device
synchronise; the three configurations are alternated per round.

The new launches alone, on scratch tensors of the trajectory's shape, LAUNCHES back-to-back launches between two events after a warm one:
pd_class_contrast (2 C + 1 streams of 4 bytes a pixel in, 1 out; the first draw reads one less), pd_contrast_mask (both of its kernels:
acc read three times with stats, map and mask written), pd_mask_blend (x and keep in, out out: 3 streams of 4 bytes an element, plus a byte
a pixel), next to pd_ddim_step.  Prints one JSON line."""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import phendiff_amd as P
import phendiff_amd._lib as L
from phendiff_amd.masked import class_contrast_args, mask_blend_args

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="super_small")
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "f32"])
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--num-maps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
MIN_WINDOW_S, LAUNCHES = 2.0, 200
dev = torch.device("cuda:0")
B, size, S, M = args.batch, args.size, args.steps, args.num_maps
torch.manual_seed(0)
unet = P.CustomCondUNet2DModel(compute_dtype=args.dtype, **dict(P.UNET_CONFIGS[args.model], sample_size=size)).to(dev)
pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
Cc = unet.config.in_channels
g = torch.Generator().manual_seed(1)
images = (torch.rand(B, Cc, size, size, generator=g) * 2 - 1).to(dev)
labels = (torch.arange(B, device=dev) % 2).long()
target = 1 - labels
half = torch.zeros((B, 1, size, size), dtype=torch.uint8, device=dev)
half[:, :, :, :size // 2] = 1
# (the runners share the model's launch plan -- its activations, not their graphs: they replay one after the other)
runners = {"ddib": P.DDIBGraph(pipe, B, S),
           "given": P.MaskedDDIBGraph(pipe, B, S, mask="given"),
           "contrast": P.MaskedDDIBGraph(pipe, B, S, mask="contrast", noise=P.DeviceNoise(1234, dev), num_maps=M)}
run = {"ddib": lambda r: r.run(images, labels, target), "given": lambda r: r.run(images, labels, target, mask=half),
       "contrast": lambda r: r.run(images, labels, target)}


def window(name):
    """images / s: whole batches until MIN_WINDOW_S has passed, between two synchronises."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        run[name](runners[name])
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


out = {"model": args.model, "size": size, "batch": B, "dtype": args.dtype, "steps": S, "num_maps": M, "rounds": args.rounds,
       "min_window_s": MIN_WINDOW_S, "unet_evaluations": {"ddib": 2 * S, "given": 2 * S, "contrast": 2 * S + 2 * M}}
for name in runners:                                    # warm every shape the timed windows use
    run[name](runners[name])
torch.cuda.synchronize()
out["masked_fraction_contrast"] = [round(float(v), 4) for v in runners["contrast"].stats[:4, 2].cpu()]
rates = {name: [] for name in runners}
for _ in range(args.rounds):
    for name in runners:
        rates[name].append(window(name))
med = {}
for name in runners:
    v = [x for x, _ in rates[name]]
    med[name] = statistics.median(v)
    out[name] = {"images_per_s_median": round(med[name], 2), "min": round(min(v), 2), "max": round(max(v), 2),
                 "batches_per_window": rates[name][0][1], "ms_per_batch": round(1e3 * B / med[name], 2)}
for name in ("given", "contrast"):
    out[name]["time_over_ddib"] = round(med["ddib"] / med[name], 4)

# the launches alone (a middle step's coefficients)
x, a_, b_, dst = (torch.randn(B, Cc, size, size, device=dev) for _ in range(4))
acc = torch.empty((B, 1, size, size), dtype=torch.float32, device=dev)
sch = pipe.scheduler
sch.set_timesteps(S)
lib = L.lib()
us_step = launch_us(lib.pd_ddim_step, sch.ddim_step_args(sch.timesteps[S // 2], x, a_, dst), "pd_ddim_step")
us_first = launch_us(lib.pd_class_contrast, class_contrast_args(a_, b_, acc, True), "pd_class_contrast")
acc.zero_()      # (200 accumulations of |N(0, 2)| stay finite)
us_contrast = launch_us(lib.pd_class_contrast, class_contrast_args(a_, b_, acc, False), "pd_class_contrast")
cm = P.ContrastMask(acc, 3.0)
us_mask = launch_us(lib.pd_contrast_mask, cm.args, "pd_contrast_mask")
us_blend = launch_us(lib.pd_mask_blend, mask_blend_args(x, a_, half, dst), "pd_mask_blend")
us_blend_inplace = launch_us(lib.pd_mask_blend, mask_blend_args(x, a_, half, x), "pd_mask_blend")
nbytes, pix = x.numel() * 4, B * size * size
per_batch_us = {name: 1e6 * B / med[name] for name in runners}
out["launches"] = {
    "numel": x.numel(), "pixels": pix, "launches": LAUNCHES,
    "pd_ddim_step_us": round(us_step, 2), "pd_ddim_step_gb_s": round(3 * nbytes / us_step / 1e3, 1),
    "pd_class_contrast_first_us": round(us_first, 2), "pd_class_contrast_first_gb_s": round((2 * nbytes + 4 * pix) / us_first / 1e3, 1),
    "pd_class_contrast_us": round(us_contrast, 2), "pd_class_contrast_gb_s": round((2 * nbytes + 8 * pix) / us_contrast / 1e3, 1),
    "pd_contrast_mask_us": round(us_mask, 2), "pd_contrast_mask_gb_s": round((3 * 4 + 4 + 1) * pix / us_mask / 1e3, 1),
    "pd_mask_blend_us": round(us_blend, 2), "pd_mask_blend_gb_s": round((3 * nbytes + pix) / us_blend / 1e3, 1),
    "pd_mask_blend_inplace_us": round(us_blend_inplace, 2),
    "blends_share_of_given_batch": round(S * us_blend_inplace / per_batch_us["given"], 5),
    "mask_kernels_share_of_contrast_batch": round((us_first + (M - 1) * us_contrast + us_mask) / per_batch_us["contrast"], 6)}
print(json.dumps(out))
