#!/usr/bin/env python3
"""From-noise generation of one evaluation batch, three ways, in ONE process (docs/LAB_r23.md).  GPU only.
    python scripts/bench_generation.py [--model small_denoiser_config --size 128] [--batch 32 --steps 50 --w 2.0 --dtype bf16]
                                       [--rounds 3] [--only c] [--no-box]
  (a) the eager pipeline with a CPU torch.Generator and output_type="numpy", then the host quantisation (images_to_uint8) and the H2D
      copy of the uint8 array: the evaluation path before GenerationGraph (a torch.Generator keeps that path, bit for bit);
  (b) GenerationGraph(use_graph=False): noise drawn on the device, the same launches enqueued from Python, uint8 stays on the device;
  (c) GenerationGraph captured: one hipGraph replay per batch.
Each figure is images / s over a window of at least MIN_WINDOW_S seconds of whole batches after a warm batch, wall clock around a device
synchronise; the three are alternated per round.  `--only c` runs one configuration alone, ROUNDS batches after a warm one, and prints
how many pd_stream_noise launches a batch holds: the form a `rocprofv3 --kernel-trace --stats -- python scripts/bench_generation.py
--only c ...` run takes for the noise launches' share.  The clock and power of card 0 are sampled once a second through a REPEAT of (c)
after the timed windows (none inside them).  Prints one JSON line."""
import argparse, json, os, re, statistics, subprocess, sys, threading, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import phendiff_amd as P
from phendiff_amd.eval_generation import images_to_uint8

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="small_denoiser_config")
ap.add_argument("--size", type=int, default=None, help="image size (default: the config's sample_size, its training size)")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--w", type=float, default=2.0)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "f32"])
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--only", default=None, choices=["a", "b", "c"])
ap.add_argument("--no-box", action="store_true")
args = ap.parse_args()
MIN_WINDOW_S = 1.0
dev = torch.device("cuda:0")
size = args.size or P.UNET_CONFIGS[args.model]["sample_size"]
torch.manual_seed(0)
unet = P.CustomCondUNet2DModel(compute_dtype=args.dtype, **dict(P.UNET_CONFIGS[args.model], sample_size=size)).to(dev)
pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
labels = (torch.arange(args.batch, device=dev) % 2).long()
B, S, w = args.batch, args.steps, args.w


def eager_cpu_generator():
    gen = torch.Generator().manual_seed(5742877512)

    def batch():
        images = pipe(labels, None, w, generator=gen, num_inference_steps=S, output_type="numpy").images
        return torch.from_numpy(images_to_uint8(images)).to(dev)
    return batch


def graph(use_graph):
    runner = P.GenerationGraph(pipe, B, S, P.DeviceNoise(5742877512, dev), w=w, use_graph=use_graph)
    return lambda: runner.run(labels)


def window(batch):
    """images / s: whole batches until MIN_WINDOW_S has passed, between two synchronises."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        u8 = batch()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= MIN_WINDOW_S:
            assert u8.dtype == torch.uint8 and u8.is_cuda and tuple(u8.shape) == (B, size, size, unet.config.in_channels)
            return B * n / dt, n


def box_sample():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                           text=True, timeout=10)
        j = json.loads(r.stdout[r.stdout.index("{"):])
        card = j[sorted(k for k in j if k.startswith("card"))[0]]
        num = lambda v: float(re.search(r"[-+]?\d+(\.\d+)?", str(v)).group(0))
        sclk = next((num(v) for k, v in card.items() if "sclk" in k.lower()), None)
        power = next((num(v) for k, v in card.items() if "power" in k.lower() and "(w)" in k.lower()), None)
        return sclk, power
    except Exception:
        return None


def box_under(batch, seconds=4.0):
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
    while time.perf_counter() - t0 < seconds:
        batch()
        torch.cuda.synchronize()
    stop.set()
    th.join()
    med = lambda v: statistics.median(v) if v else None
    return {"sclk_mhz_median": med([s[0] for s in samples if s[0]]), "power_w_median": med([s[1] for s in samples if s[1]]),
            "samples": len(samples), "source": "rocm-smi --showclocks --showpower, every 1 s through a repeat of (c) after the timed windows"}


out = {"model": args.model, "size": size, "batch": B, "steps": S, "w": w, "dtype": args.dtype, "rounds": args.rounds,
       "min_window_s": MIN_WINDOW_S}
makers = {"a": eager_cpu_generator, "b": lambda: graph(False), "c": lambda: graph(True)}
names = {"a": "a_eager_cpu_generator", "b": "b_generation_enqueued", "c": "c_generation_graph"}
if args.only:
    batch = makers[args.only]()
    batch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.rounds):
        batch()
    torch.cuda.synchronize()
    out[names[args.only]] = {"images_per_s": round(B * args.rounds / (time.perf_counter() - t0), 2), "batches": args.rounds, "warm_batches": 1}
    out["pd_stream_noise_launches_per_batch"] = 1      # the initial sample (eta = 0: no variance noise); pd_stream_advance: 1
else:
    batches = {k: makers[k]() for k in "abc"}
    for k in "abc":                                     # warm every shape the timed windows use
        batches[k]()
    torch.cuda.synchronize()
    rates = {k: [] for k in "abc"}
    for _ in range(args.rounds):
        for k in "abc":
            rates[k].append(window(batches[k]))
    for k in "abc":
        v = [r for r, _ in rates[k]]
        out[names[k]] = {"images_per_s_median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                         "batches_per_window": rates[k][0][1]}
    med = {k: statistics.median([r for r, _ in rates[k]]) for k in "abc"}
    out["c_over_a"], out["c_over_b"] = round(med["c"] / med["a"], 3), round(med["c"] / med["b"], 3)
    if not args.no_box:
        out["box"] = box_under(batches["c"])
print(json.dumps(out))
