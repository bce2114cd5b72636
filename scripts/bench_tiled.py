#!/usr/bin/env python3
"""A tiled step at field-of-view size: one C x S x S canvas, tile T, overlap O (docs/LAB_r20.md).  GPU only.
    python scripts/bench_tiled.py [C S T O] [--no-single-plan]          (default 3 1024 256 32: 5 x 5 = 25 tiles)
pd_tile_gather and pd_tile_blend alone, with their bytes moved per second beside the measured copy rate; the UNet's launch plan over the
tiles (bf16 engine, the benchmark's); the share of gather + blend in a step; a captured TiledDDIBGraph step beside a plain DDIBGraph step
at B = tiles, T x T (the same UNet work without the two kernels), alternated in ONE process; and whether ONE launch plan of the whole
canvas can be built, with its time per evaluation if so.  ROUNDS rounds of ITERS launches (fewer for the UNet and the trajectories)
between device events after a warm call.  Prints one JSON line."""
import ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import phendiff_amd as P
from phendiff_amd import _lib as L
from phendiff_amd.img2img import _TiledForward

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
CH, S, TILE, OV = (int(v) for v in argv[:4]) if len(argv) > 3 else (3, 1024, 256, 32)
SINGLE_PLAN = "--no-single-plan" not in sys.argv
ROUNDS, ITERS, UNET_ITERS, STEPS, RUNS = 7, 200, 5, 3, 3          # 200 launches of ~10 us: windows of a few ms; a trajectory is 2 * STEPS steps
HBM_MEASURED = 6.29e12          # float4 copy (MI355X_MICROARCH: 79 % of the 8.0 TB/s datasheet figure)
dev, lib = torch.device("cuda:0"), L.lib()
st = torch.cuda.current_stream(dev).cuda_stream
gen = torch.Generator(device=dev).manual_seed(0)


def timed(fn, iters=ITERS):
    """ms per call: `iters` calls between two events, after one warm call."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


grid = P.TileGrid(S, S, TILE, OV)
T = grid.tiles_per_image
out = {"canvas": [1, CH, S, S], "tile": TILE, "overlap": OV, "tiles": T, "rounds": ROUNDS, "iters": ITERS, "unet_iters": UNET_ITERS}
unet = P.CustomCondUNet2DModel(compute_dtype="bf16", **dict(P.UNET_CONFIGS["super_small"], sample_size=TILE, in_channels=CH, out_channels=CH)).to(dev)
pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))

# ---- the two kernels alone, and the plan over the tiles between them
canvas = torch.randn((1, CH, S, S), generator=gen, device=dev)
model_out = torch.empty_like(canvas)
fwd = _TiledForward(unet, grid, 1, None, dev).bind(canvas, model_out)
assert fwd.chunks == [(0, T)], fwd.chunks
fwd.tiles_out.copy_(torch.randn(fwd.tiles_out.shape, generator=gen, device=dev))
tile_bytes = fwd.tiles_in.numel() * 4
t_gather = [timed(lambda: lib.pd_tile_gather(C.byref(fwd.gather_args), st)) for _ in range(ROUNDS)]
t_blend = [timed(lambda: lib.pd_tile_blend(C.byref(fwd.blend_args), st)) for _ in range(ROUNDS)]
# the figures belong to right answers: a tile is the canvas's window, and constant tile outputs blend to that constant within rounding
y0, x0 = grid.origins()[T - 1]
assert torch.equal(fwd.tiles_in[T - 1], canvas[0, :, y0:y0 + TILE, x0:x0 + TILE])
fwd.tiles_out.fill_(0.75)
lib.pd_tile_blend(C.byref(fwd.blend_args), st)
assert float((model_out - 0.75).abs().max()) < 1e-6
moved = {"gather": 2 * tile_bytes, "blend": tile_bytes + canvas.numel() * 4}      # read + written (the weight tables: a few KiB)
for name, t in (("gather", t_gather), ("blend", t_blend)):
    m = statistics.median(t)
    out["tile_" + name] = dict(spread(t), bytes=moved[name], GBps=round(moved[name] / m / 1e6, 1),
                               share_of_measured_hbm=round(moved[name] / (m * 1e-3) / HBM_MEASURED, 4))
ts = torch.full((T,), 1500.0, dtype=torch.float32, device=dev)
labels = (torch.arange(T, device=dev) % 2).to(torch.int64)
temb = fwd.plan.temb_rows(ts, labels, None, st, rows=T)
t_unet = [timed(lambda: fwd.plan.run(fwd.tiles_in.data_ptr(), temb.data_ptr(), fwd.tiles_out.data_ptr(), st), UNET_ITERS) for _ in range(ROUNDS)]
out["unet_over_tiles_bf16"] = spread(t_unet)
u, gb = statistics.median(t_unet), statistics.median(t_gather) + statistics.median(t_blend)
out["gather_plus_blend_share_of_step"] = round(gb / (gb + u), 5)

# ---- captured: a TiledDDIBGraph step beside a DDIBGraph step over the same UNet work (B = tiles, tile x tile), alternated
x_tiles = torch.randn((T, CH, TILE, TILE), generator=gen, device=dev).clamp(-1, 1)
one, zero = torch.ones((1,), dtype=torch.int64, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev)
tiled = P.TiledDDIBGraph(pipe, 1, STEPS, S, S, TILE, overlap=OV)
plain = P.DDIBGraph(pipe, T, STEPS, TILE, TILE)
canvas.clamp_(-1, 1)
t_tiled, t_plain = [], []
for _ in range(ROUNDS):
    t_tiled.append(timed(lambda: tiled.run(canvas, zero, one), RUNS) / (2 * STEPS))
    t_plain.append(timed(lambda: plain.run(x_tiles, labels, 1 - labels), RUNS) / (2 * STEPS))
out["tiled_graph_step"] = spread(t_tiled)
out["plain_graph_step_same_unet_work"] = spread(t_plain)
out["tiled_minus_plain_step_ms"] = round(statistics.median(t_tiled) - statistics.median(t_plain), 4)
del tiled, plain
torch.cuda.empty_cache()

# ---- one launch plan of the whole canvas: can it be built, and what does an evaluation cost
if SINGLE_PLAN:
    out["single_plan"] = {"max_batch": unet.max_batch(S, S)}
    try:
        big = unet.new_plan(1, S, S, dev)
        temb1 = big.temb_rows(ts[:1].contiguous(), labels[:1].contiguous(), None, st, rows=1)
        t_big = [timed(lambda: big.run(canvas.data_ptr(), temb1.data_ptr(), model_out.data_ptr(), st), 2) for _ in range(3)]
        out["single_plan"].update(built=True, **spread(t_big), ratio_to_tiled_unet=round(statistics.median(t_big) / u, 2))
    except Exception as e:      # (a refusal is a result here: it is reported, not hidden)
        out["single_plan"].update(built=False, error=f"{type(e).__name__}: {e}"[:300])
print(json.dumps(out))
