#!/usr/bin/env python3
"""The inversion diagnostics at (32, 3 x 256 x 256) fp32: `phendiff_amd.check_gaussianity` (one pd_sample_stats call, B x 110 numbers to the
host) next to the host route the reference takes per sample -- `.cpu()`, numpy mean / std / 100-bin histogram and `scipy.stats.normaltest`
(utils_Img2Img.py:79-93, without the figure) -- docs/LAB_r12.md.

Each leg runs in a child process under its own time limit.  Wall time per call, the device synchronised before the clock starts and the
result on the host when it stops (both routes end with numbers on the host).  Median of `--repeats` (>= 20) calls after 5 warm-up calls.
The host leg needs SciPy; without it the leg says so and the run stops (a measurement does not fall back).

    python scripts/experiments/bench_sample_stats.py [--repeats 30]"""
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SHAPE = (32, 3, 256, 256)
LEG_LIMIT_S = 240


def leg(name, repeats, warmup):
    import numpy as np
    import torch
    import phendiff_amd as P
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: a measurement does not fall back")
    gauss = torch.randn(SHAPE, generator=torch.Generator().manual_seed(0)).to("cuda:0")
    if name == "host":
        from scipy.stats import normaltest

        def call():
            out = []
            for itm in gauss:
                v = itm.cpu().numpy().flatten()
                out.append((itm.mean().item(), itm.std().item(), np.histogram(v, bins=100, range=(-3, 3))[0], normaltest(v)[1]))
            return out
    else:
        call = lambda: P.check_gaussianity(gauss)      # noqa: E731
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        wall.append(time.perf_counter() - t0)
    print(json.dumps(dict(leg=name, shape=list(SHAPE), repeats=repeats, wall_ms_median=round(statistics.median(wall) * 1e3, 4),
                          wall_ms_min=round(min(wall) * 1e3, 4), wall_ms_max=round(max(wall) * 1e3, 4))), flush=True)


def main():
    argv = sys.argv[1:]
    repeats = max(20, int(argv[argv.index("--repeats") + 1])) if "--repeats" in argv else 30
    if "--leg" in argv:
        return leg(argv[argv.index("--leg") + 1], repeats, warmup=5)
    for name in ("host", "device"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--repeats", str(repeats)], timeout=LEG_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(stopped_after=name, exit_status=rc)), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
