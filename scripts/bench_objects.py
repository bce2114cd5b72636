#!/usr/bin/env python3
"""The per-object measurements (phendiff_amd.objects, csrc/object_stats.hip) at batch 32, 256 x 256, C = 3, in ONE process
(docs/LAB_r31.md).  GPU only.
    python scripts/bench_objects.py [--size 256 --batch 32 --channels 3 --max-objects 1024] [--rounds 5] [--no-transfer] [--model super_small --dtype bf16 --steps 50 --num-maps 10]
  masks        speckled (blobs with pin-holes and specks on the background: what a raw contrast mask looks like) and contrast (a
               smoothed noise field thresholded at a multiple of its mean, the shape class_contrast_mask gives: fewer, larger regions)
  entry points pd_mask_components / pd_object_index / pd_object_geometry / pd_object_intensity alone, and ObjectMeasure.enqueue (all 12
               launches, no allocation): CALLS back-to-back calls between two events after a warm one, the median of ROUNDS such windows
  eager        label_objects + measure_intensity (allocations and the derived torch tables included), the same way
  torch        the same geometry and intensity tables from the dense index map with index_add / scatter_reduce over the foreground
               pixels on the same device (float64 atomics: not reproducible in the last bits), 5 calls a window, and its agreement with
               the kernels' tables.  It is slow (tens to hundreds of milliseconds a call: float64 min / max atomics on a few hot rows)
  progress     one timestamped line per stage on stderr
  transfer     MaskedDDIBGraph(mask="contrast"): milliseconds a batch over windows of at least MIN_WINDOW_S seconds, and the share of a
               batch that ObjectMeasure.enqueue over the same batch would take
Prints one JSON line."""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

MIN_WINDOW_S, CALLS = 2.0, 100


def speckled_mask(B, size, seed=3):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    m = torch.zeros((B, size, size), dtype=torch.bool)
    for s in range(B):
        for _ in range(6):
            cy, cx = (torch.rand(2, generator=g) * size).tolist()
            ry, rx = (size / 12 + torch.rand(2, generator=g) * size / 8).tolist()
            m[s] |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    m &= torch.rand(m.shape, generator=g) > 0.03
    m |= torch.rand(m.shape, generator=g) < 0.02
    return m.to(torch.uint8)


def contrast_mask(B, size, seed=5, ratio=1.6):
    """|smoothed noise| thresholded at `ratio` times its mean: the DiffEdit rule over a field with the correlation length of a cell."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((B, 1, size, size), generator=g)
    for _ in range(3):
        f = F.avg_pool2d(f, 9, stride=1, padding=4)
    f = f.abs()
    return (f > ratio * f.mean(dim=(1, 2, 3), keepdim=True))[:, 0].to(torch.uint8)


def torch_tables(index, images, K):
    """(geometry int64 (B, K, 12), intensity float64 (B, K, C, 4)) from the dense index map by index_add / scatter_reduce over the
    foreground pixels (the background is dropped first: its one key per sample would take most of the atomics)."""
    B, H, W = index.shape
    Cn, dev = images.shape[1], index.device
    n = B * K
    fg = (index > 0).reshape(-1)
    key = (index.long() - 1 + (torch.arange(B, device=dev) * K)[:, None, None]).reshape(-1)[fg]
    y = torch.arange(H, device=dev)[None, :, None].expand(B, H, W).reshape(-1)[fg]
    x = torch.arange(W, device=dev)[None, None, :].expand(B, H, W).reshape(-1)[fg]
    p = F.pad(index, (1, 1, 1, 1), value=-1)
    edges = ((p[:, :-2, 1:-1] != index).long() + (p[:, 2:, 1:-1] != index) + (p[:, 1:-1, :-2] != index) + (p[:, 1:-1, 2:] != index)).reshape(-1)[fg]
    onb = ((y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)).long()
    sums = torch.zeros((n, 7), dtype=torch.int64, device=dev).index_add_(0, key, torch.stack([torch.ones_like(y), y, x, y * y, x * x, y * x, edges], -1))
    big = torch.iinfo(torch.int64).max

    def red(src, how, init):
        return torch.full((n,), init, dtype=torch.int64, device=dev).scatter_reduce_(0, key, src, how, include_self=True)

    y0, y1, x0, x1, border = red(y, "amin", big), red(y, "amax", 0), red(x, "amin", big), red(x, "amax", 0), red(onb, "amax", 0)
    has = sums[:, 0] > 0
    geom = torch.stack([sums[:, 0], y0 * has, y1, x0 * has, x1, sums[:, 1], sums[:, 2], sums[:, 3], sums[:, 4], sums[:, 5], sums[:, 6], border], -1)
    v = images.permute(0, 2, 3, 1).reshape(-1, Cn)[fg].to(torch.float64)
    keyc = key[:, None].expand(-1, Cn)
    s1 = torch.zeros((n, Cn), dtype=torch.float64, device=dev).index_add_(0, key, v)
    s2 = torch.zeros((n, Cn), dtype=torch.float64, device=dev).index_add_(0, key, v * v)
    lo = torch.full((n, Cn), float("inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, keyc, v, "amin", include_self=True)
    hi = torch.full((n, Cn), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, keyc, v, "amax", include_self=True)
    inten = torch.where(has[:, None, None], torch.stack([s1, s2, lo, hi], -1), torch.zeros((), dtype=torch.float64, device=dev))
    return geom.view(B, K, 12), inten.view(B, K, Cn, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--max-objects", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--model", default="super_small")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "f32"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--num-maps", type=int, default=10)
    ap.add_argument("--no-transfer", action="store_true", help="the measurements only")
    args = ap.parse_args()
    import phendiff_amd as P
    import phendiff_amd._lib as L
    from phendiff_amd import mask_ops as M, objects as O
    dev = torch.device("cuda:0")
    B, size, Cn, K = args.batch, args.size, args.channels, args.max_objects
    H = W = size
    lib, st = L.lib(), torch.cuda.current_stream(dev).cuda_stream

    def window_us(enqueue, calls=CALLS):
        ev = [C.c_void_p(), C.c_void_p()]
        for e in ev:
            L.check(lib.pd_event_create(C.byref(e)), "pd_event_create")
        L.check(lib.pd_event_record(ev[0], st), "pd_event_record")
        for _ in range(calls):
            enqueue()
        L.check(lib.pd_event_record(ev[1], st), "pd_event_record")
        ms = C.c_float()
        L.check(lib.pd_event_elapsed_ms(ev[0], ev[1], C.byref(ms)), "pd_event_elapsed_ms")
        for e in ev:
            lib.pd_event_destroy(e)
        return 1e3 * ms.value / calls

    t_start = time.perf_counter()

    def log(what):      # progress on stderr: where the time of a run went
        print(f"[{time.perf_counter() - t_start:7.1f} s] {what}", file=sys.stderr, flush=True)

    def timed(enqueue, calls=CALLS, what=""):
        """Median, least and largest microseconds per call over the rounds, after a warm call."""
        enqueue()
        torch.cuda.synchronize()
        v = [window_us(enqueue, calls) for _ in range(args.rounds)]
        log(f"{what}: {statistics.median(v):.1f} us")
        return {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}

    g = torch.Generator().manual_seed(11)
    images = torch.rand((B, Cn, H, W), generator=g).to(dev)
    result = {"size": size, "batch": B, "channels": Cn, "max_objects": K, "calls": CALLS, "rounds": args.rounds, "masks": {}}
    measure_us = {}
    for name, mask in (("speckled", speckled_mask(B, size)), ("contrast", contrast_mask(B, size))):
        mask = mask.to(dev)
        om = O.ObjectMeasure(B, H, W, Cn, dev, max_objects=K)
        om.enqueue(st, mask, images)
        torch.cuda.synchronize()
        log(name + ": first ObjectMeasure.enqueue done")
        area = om.geometry[..., 0]
        boxes = ((om.geometry[..., 2] - om.geometry[..., 1] + 1) * (om.geometry[..., 4] - om.geometry[..., 3] + 1) * (area > 0)).sum().item()
        r = {"set_fraction": round(float((mask != 0).float().mean()), 4), "objects_per_sample_mean": round(float(om.count.float().mean()), 1),
             "objects_per_sample_max": int(om.count.max()), "status_max": int(om.status.max()),
             "box_pixels_over_object_pixels": round(boxes / max(int(area.sum()), 1), 3)}
        label = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        comp_status = torch.empty((B,), dtype=torch.int32, device=dev)
        comp = M.mask_components_args(mask, 1, 8, om._comp_ws, B, H, W, label=label, status=comp_status)
        index = torch.empty_like(label)
        ia = O.object_index_args(label, index, om.count, om.status, om._index_ws, K, B, H, W, label_status=comp_status)
        ga = O.object_geometry_args(index, om.geometry, K, B, H, W)
        na = O.object_intensity_args(index, om.geometry, images, om.intensity, K, B, H, W, Cn, torch.float32)
        r["pd_mask_components"] = timed(lambda: L.check(lib.pd_mask_components(C.byref(comp), st), "pd_mask_components"), what=name + " pd_mask_components")
        r["pd_object_index"] = timed(lambda: L.check(lib.pd_object_index(C.byref(ia), st), "pd_object_index"), what=name + " pd_object_index")
        r["pd_object_geometry"] = timed(lambda: L.check(lib.pd_object_geometry(C.byref(ga), st), "pd_object_geometry"), what=name + " pd_object_geometry")
        r["pd_object_intensity"] = timed(lambda: L.check(lib.pd_object_intensity(C.byref(na), st), "pd_object_intensity"), what=name + " pd_object_intensity")
        r["ObjectMeasure_enqueue"] = timed(lambda: om.enqueue(st, mask, images), what=name + " ObjectMeasure.enqueue")
        r["label_objects_plus_measure_intensity"] = timed(lambda: O.measure_intensity(O.label_objects(mask, max_objects=K), images), calls=CALLS // 4, what=name + " label_objects + measure_intensity")
        r["torch_tables_from_index"] = timed(lambda: torch_tables(om.index, images, K), calls=5, what=name + " torch tables")
        tg, ti = torch_tables(om.index, images, K)
        torch.cuda.synchronize()
        r["torch_geometry_equals"] = bool(torch.equal(tg, om.geometry))
        r["torch_intensity_max_rel_diff"] = float(((ti - om.intensity).abs() / om.intensity.abs().clamp(min=1e-300)).max())
        r["after_labelling_over_torch"] = round((r["pd_object_index"]["us_median"] + r["pd_object_geometry"]["us_median"] + r["pd_object_intensity"]["us_median"])
                                                / r["torch_tables_from_index"]["us_median"], 4)
        measure_us[name] = r["ObjectMeasure_enqueue"]["us_median"]
        result["masks"][name] = r

    if not args.no_transfer:
        torch.manual_seed(0)
        S = args.steps
        unet = P.CustomCondUNet2DModel(compute_dtype=args.dtype, **dict(P.UNET_CONFIGS[args.model], sample_size=size)).to(dev)
        pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
        g = torch.Generator().manual_seed(1)
        x = (torch.rand(B, unet.config.in_channels, size, size, generator=g) * 2 - 1).to(dev)
        labels = (torch.arange(B, device=dev) % 2).long()
        runner = P.MaskedDDIBGraph(pipe, B, S, mask="contrast", noise=P.DeviceNoise(1234, dev), num_maps=args.num_maps)
        log("transfer: runner built")
        runner.run(x, labels, 1 - labels)
        torch.cuda.synchronize()
        log("transfer: warm batch done")
        ms = []
        for _ in range(3):
            t0, n = time.perf_counter(), 0
            while True:
                runner.run(x, labels, 1 - labels)
                torch.cuda.synchronize()
                n += 1
                dt = time.perf_counter() - t0
                if dt >= MIN_WINDOW_S:
                    ms.append(1e3 * dt / n)
                    break
        batch_ms = statistics.median(ms)
        result["transfer"] = {"model": args.model, "dtype": args.dtype, "steps": S, "num_maps": args.num_maps, "min_window_s": MIN_WINDOW_S,
                              "ms_per_batch_median": round(batch_ms, 2), "ms_per_batch_range": [round(min(ms), 2), round(max(ms), 2)],
                              "measure_share_of_batch": {k: round(v / 1e3 / batch_ms, 6) for k, v in measure_us.items()}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
