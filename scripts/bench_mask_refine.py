#!/usr/bin/env python3
"""The mask refinement (phendiff_amd.mask_ops, csrc/mask_morph.hip) at batch 32, 256 x 256, in ONE process (docs/LAB_r30.md).  GPU only.
    python scripts/bench_mask_refine.py [--model super_small --size 256] [--batch 32 --dtype bf16] [--steps 50] [--num-maps 10] [--rounds 3]
  primitives   every entry point alone over a speckled mask (blobs with pin-holes, specks on the background: what a contrast mask looks
               like): LAUNCHES back-to-back calls between two events after a warm one, microseconds per call
  recipe       MaskRefine(close=1.5, open=1.5, fill_holes=-1, min_area=64, dilate=3).enqueue, the same way
  transfer     MaskedDDIBGraph(mask="contrast") without and with refine=<that recipe>: images / s over windows of at least MIN_WINDOW_S
               seconds of whole batches after a warm batch, alternated per round; the added time per batch and its share
Prints one JSON line."""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import phendiff_amd as P
import phendiff_amd._lib as L
from phendiff_amd import mask_ops as M

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="super_small")
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "f32"])
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--num-maps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-transfer", action="store_true", help="the primitives and the recipe only")
args = ap.parse_args()
MIN_WINDOW_S, LAUNCHES = 2.0, 100
RECIPE = dict(close=1.5, open=1.5, fill_holes=-1, min_area=64, dilate=3)
dev = torch.device("cuda:0")
B, size, S = args.batch, args.size, args.steps
lib, st = L.lib(), torch.cuda.current_stream(dev).cuda_stream


def speckled_mask():
    g = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    m = torch.zeros((B, size, size), dtype=torch.bool)
    for s in range(B):
        for _ in range(6):
            cy, cx = (torch.rand(2, generator=g) * size).tolist()
            ry, rx = (size / 12 + torch.rand(2, generator=g) * size / 8).tolist()
            m[s] |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    m &= torch.rand(m.shape, generator=g) > 0.03
    m |= torch.rand(m.shape, generator=g) < 0.02
    return m.to(torch.uint8).to(dev)


def timed_us(enqueue, launches=LAUNCHES):
    """Microseconds per call of enqueue(): `launches` back-to-back calls between two events on the current stream, after a warm one."""
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        L.check(lib.pd_event_create(C.byref(e)), "pd_event_create")
    enqueue()
    torch.cuda.synchronize()
    L.check(lib.pd_event_record(ev[0], st), "pd_event_record")
    for _ in range(launches):
        enqueue()
    L.check(lib.pd_event_record(ev[1], st), "pd_event_record")
    ms = C.c_float()
    L.check(lib.pd_event_elapsed_ms(ev[0], ev[1], C.byref(ms)), "pd_event_elapsed_ms")
    for e in ev:
        lib.pd_event_destroy(e)
    return round(1e3 * ms.value / launches, 2)


mask = speckled_mask()
H = W = size
i32 = dict(dtype=torch.int32, device=dev)
d2, out = torch.empty((B, H, W), **i32), torch.empty((B, H, W), dtype=torch.uint8, device=dev)
ws = torch.empty((lib.pd_mask_components_workspace(B, H, W) // 4,), **i32)
label, area, count, status = torch.empty((B, H, W), **i32), torch.empty((B, H, W), **i32), torch.empty((B,), **i32), torch.empty((B,), **i32)
border, stats = torch.empty((B, H, W), dtype=torch.uint8, device=dev), torch.empty((B, 5), **i32)


def call(fn, a, name):
    return lambda: L.check(fn(C.byref(a), st), name)


prim = {}
for to_set in (True, False):
    prim[f"pd_mask_distance_to_{'set' if to_set else 'clear'}_us"] = timed_us(call(lib.pd_mask_distance, M.mask_distance_args(mask, d2, to_set, 0, B, H, W), "pd_mask_distance"))
for radius in (1.5, 3, 8):
    for op, nm in ((M.DILATE, "dilate"), (M.ERODE, "erode")):
        prim[f"pd_mask_morph_{nm}_r{radius}_us"] = timed_us(call(lib.pd_mask_morph, M.mask_morph_args(mask, out, op, M.disc_r2(radius), ws, B, H, W), "pd_mask_morph"))
for conn, phase in ((8, 1), (4, 0)):
    a = M.mask_components_args(mask, phase, conn, ws, B, H, W, label, area, border, count, status)
    prim[f"pd_mask_components_c{conn}_phase{phase}_us"] = timed_us(call(lib.pd_mask_components, a, "pd_mask_components"))
    rule, limit = (M.DROP_SMALL, 64) if phase else (M.FILL_HOLES, -1)
    a = M.mask_filter_args(mask, label, area, border, rule, limit, out, B, H, W, status=status, stats=stats, stats_stride=5)
    prim[f"pd_mask_filter_{'drop_small' if phase else 'fill_holes'}_us"] = timed_us(call(lib.pd_mask_filter, a, "pd_mask_filter"))
torch.cuda.synchronize()
result = {"size": size, "batch": B, "launches": LAUNCHES, "set_fraction": round(float((mask != 0).float().mean()), 4), "components_status": int(status.abs().sum()),
          "components_per_sample_mean": round(float(count.float().mean()), 1), "primitives": prim}
r = M.MaskRefine(B, H, W, dev, **RECIPE)
result["recipe"] = {"params": RECIPE, "launch_calls": len(r.ops), "us": timed_us(lambda: r.enqueue(st, mask))}
torch.cuda.synchronize()
result["recipe"]["stats_sample0"] = r.stats[0].cpu().tolist()

if not args.no_transfer:
    torch.manual_seed(0)
    unet = P.CustomCondUNet2DModel(compute_dtype=args.dtype, **dict(P.UNET_CONFIGS[args.model], sample_size=size)).to(dev)
    pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
    g = torch.Generator().manual_seed(1)
    images = (torch.rand(B, unet.config.in_channels, size, size, generator=g) * 2 - 1).to(dev)
    labels = (torch.arange(B, device=dev) % 2).long()
    runners = {"contrast": P.MaskedDDIBGraph(pipe, B, S, mask="contrast", noise=P.DeviceNoise(1234, dev), num_maps=args.num_maps),
               "contrast_refine": P.MaskedDDIBGraph(pipe, B, S, mask="contrast", noise=P.DeviceNoise(1234, dev), num_maps=args.num_maps, refine=RECIPE)}

    def window(runner):
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while True:
            runner.run(images, labels, 1 - labels)
            torch.cuda.synchronize()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= MIN_WINDOW_S:
                return B * n / dt

    for runner in runners.values():
        runner.run(images, labels, 1 - labels)
    torch.cuda.synchronize()
    rates = {name: [] for name in runners}
    for _ in range(args.rounds):
        for name, runner in runners.items():
            rates[name].append(window(runner))
    tr = {"model": args.model, "dtype": args.dtype, "steps": S, "num_maps": args.num_maps, "rounds": args.rounds, "min_window_s": MIN_WINDOW_S}
    for name, v in rates.items():
        med = statistics.median(v)
        tr[name] = {"images_per_s_median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2), "ms_per_batch": round(1e3 * B / med, 2),
                    "ms_per_batch_range": [round(1e3 * B / max(v), 2), round(1e3 * B / min(v), 2)]}
    added = tr["contrast_refine"]["ms_per_batch"] - tr["contrast"]["ms_per_batch"]
    rr = runners["contrast_refine"]
    tr["refine_added_ms_per_batch"] = round(added, 3)
    tr["refine_share_of_batch"] = round(added / tr["contrast_refine"]["ms_per_batch"], 5)
    tr["raw_masked_fraction"] = [round(float(v), 4) for v in rr.stats[:4, 2].cpu()]
    tr["refined_masked_fraction"] = [round(float(v), 4) for v in rr.mask[:4].float().mean(dim=(1, 2, 3)).cpu()]
    rm = M.MaskRefine(B, H, W, dev, **RECIPE)
    raw = rr.raw_mask.clone()
    tr["recipe_on_the_contrast_mask_us"] = timed_us(lambda: rm.enqueue(st, raw))
    result["transfer"] = tr
print(json.dumps(result))
