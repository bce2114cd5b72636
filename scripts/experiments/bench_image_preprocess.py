#!/usr/bin/env python3
"""pd_image_preprocess alone: images/s and achieved bytes/s at the training shape (N = 112, 1024 x 1280 x 3 -> 128 x 128) and the transfer
shape (N = 32, 512 x 512 x 3 -> 256 x 256), next to the same batch resized by PIL on 16 host threads (docs/LAB_r8.md).

GPU side: device events around `--batch-launches` launches, a warm-up first, the median of `--repeats` such windows.  The bytes are what the
algorithm needs, from the shapes: the source read once plus both outputs written once.  The source batch is device resident (the upload
of decoded bytes is the caller's, as in the trainers).  Host side: PIL resize -> ToTensor -> Normalize per image on a 16-thread pool (PIL
releases the GIL inside resize), median of `--pil-repeats` batches.

    python scripts/experiments/bench_image_preprocess.py [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 6.29e12          # measured HBM peak, bytes/s of the MI355X
SHAPES = {"training": (112, 1024, 1280, 128, 128), "transfer": (32, 512, 512, 256, 256)}


def gpu_time(pre, x, raw, launches, repeats, warmup):
    from phendiff_amd import _lib as L
    lib = L.lib()
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        L.check(lib.pd_event_create(C.byref(e)), "pd_event_create")
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(warmup):
        pre(x, return_raw=raw)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        L.check(lib.pd_event_record(ev[0], st))
        for _ in range(launches):
            pre(x, return_raw=raw)
        L.check(lib.pd_event_record(ev[1], st))
        ms = C.c_float()
        L.check(lib.pd_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
        times.append(ms.value * 1e-3 / launches)
    for e in ev:
        lib.pd_event_destroy(e)
    return statistics.median(times), min(times), max(times)


def pil_one(a, OH, OW):
    from PIL import Image
    r = np.asarray(Image.fromarray(a).resize((OW, OH), Image.BILINEAR))
    return torch.from_numpy(r.copy()).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5)


def pil_time(x, OH, OW, threads, repeats):
    torch.set_num_threads(1)        # the per-image torch ops are tiny: the pool is the parallelism
    times = []
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(lambda a: pil_one(a, OH, OW), x[:threads]))
        for _ in range(repeats):
            t0 = time.perf_counter()
            torch.stack(list(pool.map(lambda a: pil_one(a, OH, OW), x)))
            times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pil-repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import phendiff_amd as P
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: a measurement does not fall back")
    out = []
    for name, (N, H, W, OH, OW) in SHAPES.items():
        x_host = np.random.default_rng(0).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        x = torch.from_numpy(x_host).cuda()
        pre = P.ImagePreprocessor((OH, OW))
        for raw in (False, True):
            med, lo, hi = gpu_time(pre, x, raw, args.batch_launches, args.repeats, args.warmup)
            nbytes = N * H * W * 3 + N * OH * OW * 3 * (4 + (1 if raw else 0))
            rec = dict(shape=name, N=N, src=[H, W], dst=[OH, OW], raw_twin=raw, seconds=med, seconds_min=lo, seconds_max=hi,
                       images_per_s=N / med, bytes=nbytes, bytes_per_s=nbytes / med, share_of_hbm_peak=nbytes / med / HBM_PEAK)
            out.append(rec)
            print(f"{name:9s} N={N} {H}x{W}->{OH}x{OW} raw={int(raw)}: {med * 1e6:8.1f} us/batch (min {lo * 1e6:.1f}, max {hi * 1e6:.1f})  "
                  f"{N / med:10.0f} images/s  {nbytes / med / 1e12:.3f} TB/s = {100 * nbytes / med / HBM_PEAK:.1f} % of {HBM_PEAK / 1e12:.2f} TB/s", flush=True)
        t = pil_time(x_host, OH, OW, args.threads, args.pil_repeats)
        out.append(dict(shape=name, N=N, pil_threads=args.threads, seconds=t, images_per_s=N / t))
        print(f"{name:9s} PIL on {args.threads} host threads: {t * 1e3:8.1f} ms/batch  {N / t:10.0f} images/s", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
