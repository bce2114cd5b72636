#!/usr/bin/env python3
"""The 16-bit image kernels at a plate's size: N stacks of H x W x C uint16 -> OUT x OUT (docs/LAB_r17.md, docs/LAB_r18.md).  GPU only.
    python scripts/bench_image16.py [N H W C OUT]          (default 32 1080 1080 5 256)
pd_image_preprocess_bands16 beside pd_image_preprocess_bands (the same tiled resampler on the high bytes of the same data: half the bytes, integer
instead of float64 arithmetic), the two alternated in ONE process over ROUNDS rounds of ITERS launches between device events; then
pd_band_histogram16 on the same batch, on its 12-bit version and on an all-equal batch, as bytes read per second.  Prints one JSON line."""
import ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import phendiff_amd as P
from phendiff_amd import _lib as L

N, H, W, CH, OUT = (int(v) for v in sys.argv[1:6]) if len(sys.argv) > 5 else (32, 1080, 1080, 5, 256)
ROUNDS, ITERS = 7, 10
HBM_MEASURED = 6.29e12          # float4 copy (MI355X_MICROARCH: 79 % of the 8.0 TB/s datasheet figure)
dev, lib = torch.device("cuda:0"), L.lib()
gen = torch.Generator(device=dev).manual_seed(0)
x16 = torch.randint(-32768, 32768, (N, H, W, CH), dtype=torch.int16, device=dev, generator=gen).view(torch.uint16)
x8 = (x16.view(torch.int16).to(torch.int32) >> 8).to(torch.uint8)      # the high bytes: the same pictures at 8 bits
pre = P.ImagePreprocessor((OUT, OUT), device=dev, channels=CH)


def timed(fn):
    """ms per call: ITERS calls between two events, after one warm call."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / ITERS


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


t8, t16 = [], []
for _ in range(ROUNDS):
    t8.append(timed(lambda: pre(x8)))
    t16.append(timed(lambda: pre(x16)))
out = {"shape": [N, H, W, CH, OUT], "rounds": ROUNDS, "iters": ITERS, "resize_8bit": spread(t8), "resize_16bit": spread(t16),
       "ratio_16_over_8_median": round(statistics.median(t16) / statistics.median(t8), 3)}
src_bytes = N * H * W * CH * 2
out["resize_16bit"]["source_GBps"] = round(src_bytes / statistics.median(t16) / 1e6, 1)
out["resize_8bit"]["source_GBps"] = round(src_bytes / 2 / statistics.median(t8) / 1e6, 1)

counts = torch.zeros((CH, 65536), dtype=torch.int32, device=dev)
st = torch.cuda.current_stream(dev).cuda_stream
batches = {"full_range": x16, "12bit": (x16.view(torch.int16) & 0x0FFF).view(torch.uint16),
           "all_equal": torch.full((N, H, W, CH), 1234, dtype=torch.int16, device=dev).view(torch.uint16)}
for name, x in batches.items():
    a = L.BandHistogram16Args(N=N, H=H, W=W, C=CH, image_stride=H * W * CH * 2, row_stride=W * CH * 2, pixel_stride=CH * 2, x=x.data_ptr(),
                              counts=counts.data_ptr())
    counts.zero_()
    L.check(lib.pd_band_histogram16(C.byref(a), st), "pd_band_histogram16")
    assert int((counts.to(torch.int64) & 0xFFFFFFFF).sum()) == N * H * W * CH          # every sample counted once
    t = [timed(lambda: lib.pd_band_histogram16(C.byref(a), st)) for _ in range(ROUNDS)]
    out["histogram_" + name] = dict(spread(t), source_GBps=round(src_bytes / statistics.median(t) / 1e6, 1),
                                    share_of_measured_hbm=round(src_bytes / (statistics.median(t) * 1e-3) / HBM_MEASURED, 4))
print(json.dumps(out))
