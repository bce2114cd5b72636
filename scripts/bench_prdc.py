#!/usr/bin/env python3
"""precision / recall / f_score / density / coverage from pd_knn_radii + pd_manifold_query beside the torch formulation of the same
definitions ON THE SAME DEVICE (docs/LAB_r22.md).  GPU only.
    python scripts/bench_prdc.py [--sizes 2000,10000,50000]
The torch formulation is what a user would write without the kernels: float64 ``torch.cdist`` over blocks of rows (a block's distance matrix
is held to 1 GiB), ``kthvalue(k + 1)`` for the radii (the block's diagonal set to 0), ``<=`` against the radii and ``any`` / ``sum`` / ``min``
per row -- in distances, which decide as the squared ones do.  Both legs compute all five metrics (neighbourhood 3 for precision / recall, 5
for density / coverage) of N generated against N real rows of D = 2048 fp32 features.  Both legs are warmed at every size, then alternated
for ROUNDS rounds in ONE process; a round times `iters` calls between two device events, `iters` chosen from the warm call so that a window
lasts about WINDOW_S.  The two legs' metrics are compared at the sizes timed.  Prints one JSON line."""
import json, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from phendiff_amd import metrics as M

if not torch.cuda.is_available():
    raise SystemExit("needs an MI355X: a measurement does not fall back")
SIZES = [int(v) for v in (sys.argv[sys.argv.index("--sizes") + 1] if "--sizes" in sys.argv else "2000,10000,50000").split(",")]
D, K_PRC, K_DC = 2048, 3, 5
ROUNDS, WINDOW_S, MAX_ITERS = 3, 0.5, 200
BLOCK_BYTES = 1 << 30
dev = torch.device("cuda:0")


def box_state():
    """Clock and power as the box reports them (read-only query; absent tool: empty)."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else {}
    except Exception:      # noqa: BLE001
        return {}


def sheet(n, seed, axis):
    """A low-dimensional sheet (8 latent directions) in D dimensions, half of it shifted along `axis`: precision and recall well inside
    (0, 1), which i.i.d. clouds in 2048 dimensions do not give."""
    g = torch.Generator(device=dev).manual_seed(seed)
    w = torch.rand((8, D), generator=torch.Generator(device=dev).manual_seed(40), device=dev)
    z = torch.randn((n, 8), generator=g, device=dev).abs()
    z[: n // 2, axis] += 2.5
    return (z @ w + 0.02 * torch.randn((n, D), generator=g, device=dev).abs()).float().contiguous()


def blocks(n, cols):
    step = max(1, min(n, BLOCK_BYTES // (8 * cols)))
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def torch_radii(f, k):
    out = torch.empty(len(f), dtype=torch.float64, device=dev)
    for i, j in blocks(len(f), len(f)):
        d = torch.cdist(f[i:j], f)
        r = torch.arange(j - i, device=dev)
        d[r, i + r] = 0.0
        out[i:j] = d.kthvalue(k + 1, dim=1).values
    return out


def torch_query(q, r, rad=None):
    count = None if rad is None else torch.empty(len(q), dtype=torch.int64, device=dev)
    dmin = torch.empty(len(q), dtype=torch.float64, device=dev)
    for i, j in blocks(len(q), len(r)):
        d = torch.cdist(q[i:j], r)
        dmin[i:j] = d.min(dim=1).values
        if rad is not None:
            count[i:j] = (d <= rad[None, :]).sum(dim=1)
    return count, dmin


def torch_five(gen, real):
    g, x = gen.double(), real.double()
    in_real, _ = torch_query(g, x, torch_radii(x, K_PRC))
    in_gen, _ = torch_query(x, g, torch_radii(g, K_PRC))
    rad = torch_radii(x, K_DC)
    count, _ = torch_query(g, x, rad)
    _, dmin = torch_query(x, g)
    n_p, n_r, n_d, n_c = (int(v) for v in torch.stack([(in_real > 0).sum(), (in_gen > 0).sum(), count.sum(), (dmin <= rad).sum()]).cpu())
    p, r, d, c = n_p / len(g), n_r / len(x), n_d / (K_DC * len(g)), n_c / len(x)
    return {M.KEY_PRECISION: p, M.KEY_RECALL: r, M.KEY_F_SCORE: M._f_score(p, r), M.KEY_DENSITY: d, M.KEY_COVERAGE: c}


def pd_five(gen, real):
    return dict(M.precision_recall_device(gen, real, K_PRC), **M.density_coverage_device(gen, real, K_DC))


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
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


res = {"D": D, "prc_neighborhood": K_PRC, "dc_nearest_k": K_DC, "rounds": ROUNDS, "window_s": WINDOW_S, "box_state_before": box_state(), "cases": []}
for n in SIZES:
    gen, real = sheet(n, 22, 0), sheet(n, 21, 1)
    legs = {"pd_manifold": lambda: pd_five(gen, real), "torch_cdist_fp64": lambda: torch_five(gen, real)}
    values = {name: f() for name, f in legs.items()}
    diff = max(abs(values["pd_manifold"][k] - values["torch_cdist_fp64"][k]) for k in values["pd_manifold"])
    assert diff <= 1e-2, (n, values)      # (a distance within rounding of a radius may fall either way: a few rows of N)
    iters = {name: max(1, min(MAX_ITERS, int(WINDOW_S / max(warm(f), 1e-6)))) for name, f in legs.items()}
    times = {name: [] for name in legs}
    for _ in range(ROUNDS):
        for name, f in legs.items():
            times[name].append(timed(f, iters[name]))
    case = {"N": n, "values": values["pd_manifold"], "max_abs_difference": diff, "iters": iters}
    case.update({name: spread(t) for name, t in times.items()})
    case["torch_over_pd"] = round(statistics.median(times["torch_cdist_fp64"]) / statistics.median(times["pd_manifold"]), 2)
    # fp64 flops of the seven Gram products (2 radii + 2 queries, 1 radii + 2 queries) per second of the kernel leg
    case["pd_tflops_fp64"] = round(7 * 2.0 * n * n * D / (statistics.median(times["pd_manifold"]) * 1e-3) / 1e12, 2)
    res["cases"].append(case)
    print(json.dumps(case), file=sys.stderr, flush=True)      # (progress: the large size takes a while)
    del gen, real
    torch.cuda.empty_cache()
res["box_state_after"] = box_state()
print(json.dumps(res))
