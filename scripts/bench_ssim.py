#!/usr/bin/env python3
"""pd_ssim beside the torch formulation of the same definition ON THE SAME DEVICE (docs/LAB_r21.md).  GPU only.
    python scripts/bench_ssim.py [--dtype f32|bf16|f16]
The torch formulation is what a user would write without the kernel: per scale five depthwise F.conv2d calls in float64 (x, y, x^2, y^2, xy
with the outer-product window, groups = C), the elementwise ssim / cs formula and the means, F.avg_pool2d between scales.  Shapes:
32 x 3 x 256 x 256 (levels 1 and 5) and 1 x 5 x 2048 x 2048 (levels 5).  Both legs are warmed at every shape, then alternated for ROUNDS
rounds in ONE process; a round times `iters` calls between two device events, `iters` chosen from the warm call so that a window lasts
about WINDOW_S.  The two legs' outputs are compared at the sizes timed (bound 1e-9).  Prints one JSON line."""
import json, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from phendiff_amd import diagnostics as D

if not torch.cuda.is_available():
    raise SystemExit("needs an MI355X: a measurement does not fall back")
DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[sys.argv[sys.argv.index("--dtype") + 1] if "--dtype" in sys.argv else "f32"]
CASES = [((32, 3, 256, 256), 1), ((32, 3, 256, 256), 5), ((1, 5, 2048, 2048), 5)]
ROUNDS, WINDOW_S, MAX_ITERS = 5, 0.5, 500
WIN, SIGMA, RANGE = 11, 1.5, 2.0
dev = torch.device("cuda:0")


def box_state():
    """Clock and power as the box reports them (read-only query; absent tool: empty)."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else {}
    except Exception:      # noqa: BLE001
        return {}


def torch_ssim(x, y, levels):
    """[B, C, levels, 2] float64 on the device, from library calls only."""
    C = x.shape[1]
    g = torch.from_numpy(D.gaussian_window(WIN, SIGMA)).to(dev)
    k = torch.outer(g, g).expand(C, 1, -1, -1).contiguous()
    c1, c2 = (D.SSIM_K1 * RANGE) ** 2, (D.SSIM_K2 * RANGE) ** 2
    x, y = x.double(), y.double()
    out = []
    for s in range(levels):
        if s:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        mx, my = F.conv2d(x, k, groups=C), F.conv2d(y, k, groups=C)
        vx = F.conv2d(x * x, k, groups=C) - mx * mx
        vy = F.conv2d(y * y, k, groups=C) - my * my
        vxy = F.conv2d(x * y, k, groups=C) - mx * my
        cs = (2.0 * vxy + c2) / (vx + vy + c2)
        ssim = cs * (2.0 * mx * my + c1) / (mx * mx + my * my + c1)
        out.append(torch.stack([ssim.mean(dim=(2, 3)), cs.mean(dim=(2, 3))], dim=-1))
    return torch.stack(out, dim=2)


def warm(fn):
    """One call for code objects and algorithm choices, a second one timed by the host clock around a synchronise: seconds per call."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


res = {"dtype": str(DTYPE), "win": WIN, "rounds": ROUNDS, "window_s": WINDOW_S, "cases": []}
gen = torch.Generator(device=dev).manual_seed(0)
for shape, levels in CASES:
    x = (torch.rand(shape, generator=gen, device=dev) * 2 - 1).to(DTYPE)
    y = (x.float() + 0.1 * torch.randn(shape, generator=gen, device=dev)).clamp(-1, 1).to(DTYPE)
    legs = {"pd_ssim": lambda: D.ssim_maps_means(x, y, data_range=RANGE, levels=levels, win_size=WIN, sigma=SIGMA),
            "torch_conv2d_fp64": lambda: torch_ssim(x, y, levels)}
    diff = float((legs["pd_ssim"]() - legs["torch_conv2d_fp64"]()).abs().max())
    assert diff <= 1e-9, (shape, levels, diff)
    iters = {n: max(1, min(MAX_ITERS, int(WINDOW_S / max(warm(f), 1e-6)))) for n, f in legs.items()}
    times = {n: [] for n in legs}
    for _ in range(ROUNDS):
        for n, f in legs.items():
            times[n].append(timed(f, iters[n]))
    case = {"shape": list(shape), "levels": levels, "max_abs_difference": diff, "iters": iters}
    case.update({n: spread(t) for n, t in times.items()})
    case["torch_over_pd_ssim"] = round(statistics.median(times["torch_conv2d_fp64"]) / statistics.median(times["pd_ssim"]), 2)
    res["cases"].append(case)
    del x, y
    torch.cuda.empty_cache()
res["box_state_after"] = box_state()
print(json.dumps(res))
