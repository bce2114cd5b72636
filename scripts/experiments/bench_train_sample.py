#!/usr/bin/env python3
"""The training step's input sampling at the training shape (B = 112, 3 x 128 x 128 fp32): `sample_training_inputs` with a CPU generator
(host randn + H2D copy + device randint + pd_add_noise) next to `DeviceTrainingSampler.sample` (one pd_train_sample launch) -- docs/LAB_r11.md.

Each leg runs in a child process under its own time limit.  Wall time per call with a device synchronisation after it (the host path's cost
is host work and a copy, which device events alone would not see); the device leg also reports device-event time per launch over a window
of back-to-back launches, and the share of the HBM peak its 12 bytes per element amount to.  Median of `--repeats` (>= 20) after a warm-up.

    python scripts/experiments/bench_train_sample.py [--repeats 30]"""
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

HBM_PEAK = 6.29e12          # measured HBM peak, bytes/s of the MI355X
SHAPE = (112, 3, 128, 128)
LEG_LIMIT_S = 240


def box_state():
    """Clock and power as the box reports them (read-only query; absent tool: empty)."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else {}
    except Exception:
        return {}


def leg(name, repeats, warmup):
    import torch
    import phendiff_amd as P
    from phendiff_amd.training import sample_training_inputs
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: a measurement does not fall back")
    dev = "cuda:0"
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    clean = torch.rand(SHAPE, device=dev) * 2 - 1
    if name == "host":
        g = torch.Generator().manual_seed(0)
        call = lambda: sample_training_inputs(clean, sched, cpu_generator=g)      # noqa: E731
    else:
        sampler = P.DeviceTrainingSampler(sched, 0, dev)
        call = lambda: sampler.sample(clean)                                      # noqa: E731
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    rec = dict(leg=name, shape=list(SHAPE), repeats=repeats, wall_ms_median=round(statistics.median(wall) * 1e3, 4),
               wall_ms_min=round(min(wall) * 1e3, 4), wall_ms_max=round(max(wall) * 1e3, 4))
    if name == "device":
        launches, dev_t = 20, []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                call()
            e1.record()
            e1.synchronize()
            dev_t.append(e0.elapsed_time(e1) * 1e-3 / launches)
        med = statistics.median(dev_t)
        nbytes = clean.numel() * 12
        # (the window includes torch.empty_like of both outputs per call: what a training loop pays too)
        rec.update(device_us_median=round(med * 1e6, 2), device_us_min=round(min(dev_t) * 1e6, 2), bytes=nbytes,
                   bytes_per_s=round(nbytes / med), share_of_hbm_peak=round(nbytes / med / HBM_PEAK, 4))
    print(json.dumps(rec), flush=True)


def main():
    argv = sys.argv[1:]
    repeats = max(20, int(argv[argv.index("--repeats") + 1])) if "--repeats" in argv else 30
    if "--leg" in argv:
        return leg(argv[argv.index("--leg") + 1], repeats, warmup=5)
    print(json.dumps(dict(box_before=box_state())), flush=True)
    for name in ("host", "device"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--repeats", str(repeats)], timeout=LEG_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(stopped_after=name, exit_status=rc)), flush=True)
            return rc
    print(json.dumps(dict(box_after=box_state())), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
