"""Tiled trajectories on MI355X: pd_tile_gather / pd_tile_blend against the CPU references of tests/tiled_refs.py (bit for bit), their guard
bands, and tiled_inversion / tiled_ddib / TiledDDIBGraph against the tiled reference trajectory over the oracle's UNet and schedulers
(the `super_small` denoiser at sample_size 32 on a 72 x 88 canvas: 3 x 4 tiles of 32 x 32, overlap 8, the last row and column flush).

Trajectory tolerances are those of test_gpu_unet_ddib.test_ddib_eager_and_graph_vs_oracle (f32 2e-5, bf16 1.5e-2, fp16 2e-3): the blend is
a convex combination of tile outputs, so it adds no error source of its own."""
import functools

import numpy as np
import pytest
import torch

import threshold_refs as TH
import tiled_refs as T
from guard_bands import MIN_GUARD_BYTES
from test_gpu_guard_bands import Case, Op, out_op, p1_poisoned_surroundings, p2_canaried_outputs, p3_sample_isolation
from test_gpu_unet_ddib import make_pair, rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
TRAJ_TOL = {"f32": 2e-5, "bf16": 1.5e-2, "fp16": 2e-3}
CANVAS = dict(B=2, H=72, W=88, tile=32, overlap=8, S=3)
THRESHOLD_RATIO, THRESHOLD_MAX, THRESHOLD_SEED = 0.995, 2.0, 1234      # (the seed: chosen on the CPU, the premise is asserted below)


def _case_id(c):
    return "x".join(str(v) for v in c[:4]) + f"-t{c[4]}-ov{c[5]}".replace(" ", "")


def _kernel_inputs(case):
    B, Cc, H, W, tile, ov = case
    gen = torch.Generator().manual_seed(7 + H + W)
    g = T.GridRef(H, W, tile, ov)
    canvas = torch.randn(B, Cc, H, W, generator=gen)
    outs = torch.randn(B * g.per_image, Cc, g.th, g.tw, generator=gen)
    return g, canvas, outs


# ================================================================================================ the two kernels
@pytest.mark.parametrize("case", T.KERNEL_CASES, ids=_case_id)
def test_gather_and_blend_equal_the_reference(case):
    import phendiff_amd as P
    B, Cc, H, W, tile, ov = case
    g, canvas, outs = _kernel_inputs(case)
    grid = P.TileGrid(H, W, tile, ov)
    Tn = B * g.per_image
    canvas_d, outs_d = canvas.to(DEV), outs.to(DEV)
    for first, count in sorted({(0, Tn), (min(5, Tn - 1), min(7, Tn - min(5, Tn - 1))), (Tn - 1, 1)}):
        want = T.gather_ref(canvas, g, first, count)
        got = torch.full((count, Cc, g.th, g.tw), NAN, device=DEV)
        grid.gather(canvas_d, first, count, out=got)
        again = torch.full_like(got, NAN)
        grid.gather(canvas_d, first, count, out=again)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(got).any()), "every element of the tile batch is written"
        assert torch.equal(got.cpu(), want), (first, count)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    want = T.blend_ref(outs, g, B)
    got = torch.full((B, Cc, H, W), NAN, device=DEV)
    grid.blend(outs_d, got)
    again = torch.full_like(got, NAN)
    grid.blend(outs_d, again)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(got).any()), "every element of the canvas is written"
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    if g.per_image == 1:                        # one tile with weight 1: the blend is a copy, bit for bit
        assert torch.equal(got.view(torch.int32), outs_d.view(torch.int32).view(got.shape))


def _gather_case(case):
    import phendiff_amd as P
    B, Cc, H, W, tile, ov = case
    g, canvas, _ = _kernel_inputs(case)
    grid = P.TileGrid(H, W, tile, ov)
    want = T.gather_ref(canvas, g).view(B, g.per_image, Cc, g.th, g.tw)

    def launch(t):
        grid.gather(t["canvas"], out=t["tiles"].view(-1, Cc, g.th, g.tw))

    def check(o):
        assert torch.equal(o["tiles"], want)
    return Case(dict(canvas=Op(canvas, sample_dim=0)), dict(tiles=out_op(tuple(want.shape), torch.float32, sample_dim=0)), launch, check, nsamples=B)


def _blend_case(case):
    import phendiff_amd as P
    import phendiff_amd._lib as L
    import ctypes as C
    B, Cc, H, W, tile, ov = case
    g, _, outs = _kernel_inputs(case)
    grid = P.TileGrid(H, W, tile, ov)
    want = T.blend_ref(outs, g, B)

    def launch(t):      # (the weight tables guarded too: the argument struct is built by hand around them)
        a = L.TileBlendArgs(tiles=t["tiles"].data_ptr(), wy=t["wy"].data_ptr(), wx=t["wx"].data_ptr(), out=t["out"].data_ptr(),
                            **grid._geometry(B, Cc))
        L.check(L.lib().pd_tile_blend(C.byref(a), torch.cuda.current_stream().cuda_stream), "pd_tile_blend")

    def check(o):
        assert torch.equal(o["out"], want)
    ins = dict(tiles=Op(outs.view(B, g.per_image, Cc, g.th, g.tw), sample_dim=0), wy=Op(g.wy), wx=Op(g.wx))
    return Case(ins, dict(out=out_op((B, Cc, H, W), torch.float32, sample_dim=0)), launch, check, nsamples=B)


@pytest.mark.parametrize("prop", [p1_poisoned_surroundings, p2_canaried_outputs, p3_sample_isolation], ids=["P1", "P2", "P3"])
@pytest.mark.parametrize("case", [T.KERNEL_CASES[0], T.KERNEL_CASES[2]], ids=_case_id)
@pytest.mark.parametrize("build", [_gather_case, _blend_case], ids=["gather", "blend"])
def test_guard_bands(build, case, prop, monkeypatch):
    assert MIN_GUARD_BYTES >= 2 * 4 * case[3] * 4       # at least two groups of four canvas rows on either side of every operand
    prop(build(case), DEV, monkeypatch)


@pytest.mark.parametrize("case", [T.KERNEL_CASES[0], T.KERNEL_CASES[2]], ids=_case_id)
def test_blend_nan_in_one_tile_changes_exactly_the_pixels_it_covers(case):
    import phendiff_amd as P
    B, Cc, H, W, tile, ov = case
    g, _, outs = _kernel_inputs(case)
    grid = P.TileGrid(H, W, tile, ov)
    base = grid.blend(outs.to(DEV), torch.full((B, Cc, H, W), NAN, device=DEV)).cpu()
    Tn = B * g.per_image
    for i in sorted({0, Tn // 2, Tn - 1}):
        bad = outs.clone()
        bad[i] = NAN
        got = grid.blend(bad.to(DEV), torch.full((B, Cc, H, W), NAN, device=DEV)).cpu()
        covered = T.covered_by(g, B, i)[:, None].expand(B, Cc, H, W)
        assert bool(torch.isnan(got[covered]).all()), i
        assert torch.equal(got[~covered].view(torch.int32), base[~covered].view(torch.int32)), i


# ================================================================================================ trajectories
@functools.lru_cache(maxsize=None)
def pipes(mode, channels=3):
    """(oracle UNet, the engine's pipeline) on identical weights; the oracle's weights do not depend on `mode` (seed 0)."""
    import phendiff_amd as P
    if channels == 3:
        r, m = make_pair("super_small", 32, mode)
    else:
        from oracle import CondUNet2DRef
        torch.manual_seed(0)
        cfg = dict(P.UNET_CONFIGS["super_small"], sample_size=32, in_channels=channels, out_channels=channels)
        keys = CondUNet2DRef.__init__.__code__.co_varnames
        r = CondUNet2DRef(**{k: v for k, v in cfg.items() if k in keys}).eval()
        m = P.CustomCondUNet2DModel(compute_dtype=mode, **cfg)
        m.load_state_dict(r.state_dict())
        m = m.to(DEV)
    return r, P.ConditionalDDIMPipeline(m, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))


def _ref_scheduler():
    import phendiff_amd as P
    from oracle import DDIMSchedulerRef
    return DDIMSchedulerRef(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])


@functools.lru_cache(maxsize=None)
def reference(seed=1234, channels=3):
    """The tiled reference trajectory of the canvas batch, computed once: (x, labels, images, inverted)."""
    c = CANVAS
    r, _ = pipes("f32", channels)
    x, labels = T.canvas_batch(c["B"], channels, c["H"], c["W"], seed)
    img, inv = T.tiled_ddib_ref(r, _ref_scheduler(), x, labels, 1 - labels, c["S"], T.GridRef(c["H"], c["W"], c["tile"], c["overlap"]))
    return x, labels, img, inv


@functools.lru_cache(maxsize=None)
def eager_f32():
    import phendiff_amd as P
    c = CANVAS
    x, labels, _, _ = reference()
    _, pipe = pipes("f32")
    return P.tiled_ddib(pipe, x.to(DEV), labels.to(DEV), (1 - labels).to(DEV), c["S"], c["tile"], overlap=c["overlap"])


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
def test_tiled_inversion_and_ddib_vs_reference(mode):
    import phendiff_amd as P
    c, tol = CANVAS, TRAJ_TOL[mode]
    x, labels, ref_img, ref_inv = reference()
    _, pipe = pipes(mode)
    inv = P.tiled_inversion(pipe, x.to(DEV), labels.to(DEV), c["S"], c["tile"], overlap=c["overlap"])
    e_inv = rel(inv, ref_inv)
    out = eager_f32() if mode == "f32" else P.tiled_ddib(pipe, x.to(DEV), labels.to(DEV), (1 - labels).to(DEV), c["S"], c["tile"],
                                                         overlap=c["overlap"])
    e_img = rel(out.images, ref_img)
    print(f"tiled trajectory {mode}: rel-L2 inverted {e_inv:.3e}, images {e_img:.3e} (bound {tol})")
    assert e_inv < tol and e_img < tol, (mode, e_inv, e_img)
    assert out.images.shape == ref_img.shape == (c["B"], c["H"], c["W"], 3) and out.images.dtype == np.float32
    assert out.images_u8.dtype == np.uint8 and out.images_u8.shape == out.images.shape
    assert torch.equal(out.inverted, inv)                               # the inversion half of the transfer IS tiled_inversion
    lsb = int(np.abs(out.images_u8.astype(int) - (ref_img * 255).round().astype(int)).max())
    assert lsb <= {"f32": 1, "fp16": 2, "bf16": 12}[mode], lsb         # (the bounds of test_ddib_eager_and_graph_vs_oracle)


def test_one_tile_canvas_is_ddib_bit_for_bit():
    import phendiff_amd as P
    _, pipe = pipes("f32")
    x, labels = T.canvas_batch(2, 3, 32, 32, seed=5)
    xd, ld, td = x.to(DEV), labels.to(DEV), (1 - labels).to(DEV)
    want_img, want_inv = P.ddib(pipe, xd, ld, td, 3), P.inversion(pipe, xd, ld, 3)
    got = P.tiled_ddib(pipe, xd, ld, td, 3, 32, overlap=0)
    assert np.array_equal(got.images.view(np.int32), want_img.view(np.int32))
    assert torch.equal(got.inverted.view(torch.int32), want_inv.view(torch.int32))
    regen = P.tiled_inverted_regeneration(pipe, xd, ld, 3, 32, overlap=0)
    assert np.array_equal(regen.images, P.inverted_regeneration(pipe, xd, ld, 3))


def test_result_does_not_depend_on_the_tile_batch():
    import phendiff_amd as P
    c = CANVAS
    x, labels, _, _ = reference()
    _, pipe = pipes("f32")
    whole = eager_f32()
    from phendiff_amd.img2img import _TiledForward
    fwd = _TiledForward(pipe.unet, P.TileGrid(c["H"], c["W"], c["tile"], c["overlap"]), c["B"], 5, torch.device(DEV))
    assert fwd.T == 24 and fwd.chunks == [(0, 5), (5, 5), (10, 5), (15, 5), (20, 4)] and sorted(fwd.plans) == [4, 5]
    got = P.tiled_ddib(pipe, x.to(DEV), labels.to(DEV), (1 - labels).to(DEV), c["S"], c["tile"], overlap=c["overlap"], tile_batch=5)
    assert np.array_equal(got.images.view(np.int32), whole.images.view(np.int32)) and np.array_equal(got.images_u8, whole.images_u8)
    assert torch.equal(got.inverted.view(torch.int32), whole.inverted.view(torch.int32))
    with pytest.raises(ValueError, match="tile_batch"):
        P.tiled_ddib(pipe, x.to(DEV), labels.to(DEV), (1 - labels).to(DEV), c["S"], c["tile"], overlap=c["overlap"], tile_batch=0)


def test_captured_trajectory_equals_eager_and_replays():
    import phendiff_amd as P
    c = CANVAS
    x, labels, _, _ = reference()
    _, pipe = pipes("f32")
    eager = eager_f32()
    g = P.TiledDDIBGraph(pipe, c["B"], c["S"], c["H"], c["W"], c["tile"], overlap=c["overlap"])
    out = g.run(x.to(DEV), labels.to(DEV), (1 - labels).to(DEV))
    torch.cuda.synchronize()
    assert np.array_equal(out.images.cpu().numpy().view(np.int32), eager.images.view(np.int32))
    assert np.array_equal(out.images_u8.cpu().numpy(), eager.images_u8)
    assert torch.equal(out.inverted.view(torch.int32), eager.inverted.view(torch.int32))
    # a second run with other inputs: the buffers, not the nodes
    x2, l2, ref2, inv2 = reference(99)
    out2 = g.run(x2.to(DEV), l2.to(DEV), (1 - l2).to(DEV))
    torch.cuda.synchronize()
    assert rel(out2.images, ref2) < TRAJ_TOL["f32"] and rel(out2.inverted, inv2) < TRAJ_TOL["f32"]
    g.images.fill_(-7.0)
    with pytest.raises(ValueError, match=r"expected images of shape \(2, 3, 72, 88\), got \(1, 3, 72, 88\)"):
        g.run(x[:1].to(DEV), labels.to(DEV), (1 - labels).to(DEV))
    with pytest.raises(ValueError, match=r"expected images of shape"):
        g.run(x[:, :, :64].to(DEV), labels.to(DEV), (1 - labels).to(DEV))
    torch.cuda.synchronize()
    assert bool((g.images == -7.0).all())                               # nothing was launched


@functools.lru_cache(maxsize=None)
def threshold_reference():
    import phendiff_amd as P
    c = CANVAS
    r, _ = pipes("f32")
    x, labels = T.canvas_batch(c["B"], 3, c["H"], c["W"], THRESHOLD_SEED)
    fwd = TH.make_threshold_ref(P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"], THRESHOLD_RATIO, THRESHOLD_MAX)
    img, inv = T.tiled_ddib_ref(r, fwd, x, labels, 1 - labels, c["S"], T.GridRef(c["H"], c["W"], c["tile"], c["overlap"]))
    s = torch.stack(fwd.s_raw)
    assert s.shape == (c["S"], c["B"]) and bool((s > 1.0).any()), s      # the premise: the reference's unclamped s exceeds 1 somewhere
    return x, labels, img, inv


def test_thresholding_scheduler_takes_the_quantile_over_the_whole_canvas():
    import phendiff_amd as P
    c = CANVAS
    x, labels, ref_img, ref_inv = threshold_reference()
    r, base = pipes("f32")
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"], thresholding=True, dynamic_thresholding_ratio=THRESHOLD_RATIO,
                            sample_max_value=THRESHOLD_MAX)
    pipe = P.ConditionalDDIMPipeline(base.unet, sched)
    out = P.tiled_ddib(pipe, x.to(DEV), labels.to(DEV), (1 - labels).to(DEV), c["S"], c["tile"], overlap=c["overlap"])
    e_img, e_inv = rel(out.images, ref_img), rel(out.inverted, ref_inv)
    print(f"tiled trajectory f32, thresholding: rel-L2 inverted {e_inv:.3e}, images {e_img:.3e}")
    assert e_img < TRAJ_TOL["f32"] and e_inv < TRAJ_TOL["f32"]
    g = P.TiledDDIBGraph(pipe, c["B"], c["S"], c["H"], c["W"], c["tile"], overlap=c["overlap"])
    got = g.run(x.to(DEV), labels.to(DEV), (1 - labels).to(DEV))
    torch.cuda.synchronize()
    assert np.array_equal(got.images.cpu().numpy().view(np.int32), out.images.view(np.int32))
    # a canvas over torch.quantile's limit is refused on the host, before anything is launched
    big = torch.empty((1, 3, 2400, 2400), device="meta")
    with pytest.raises(ValueError, match="16 000 000"):
        P.tiled_ddib(pipe, big, labels[:1].to(DEV), labels[:1].to(DEV), c["S"], c["tile"])
    with pytest.raises(ValueError, match="16 000 000"):
        P.TiledDDIBGraph(pipe, 1, c["S"], 2400, 2400, c["tile"])


def test_five_channel_stack_f32():
    import phendiff_amd as P
    c = CANVAS
    x, labels, ref_img, ref_inv = reference(1234, 5)
    _, pipe = pipes("f32", 5)
    out = P.tiled_ddib(pipe, x.to(DEV), labels.to(DEV), (1 - labels).to(DEV), c["S"], c["tile"], overlap=c["overlap"])
    assert out.images.shape == (c["B"], c["H"], c["W"], 5)
    assert rel(out.images, ref_img) < TRAJ_TOL["f32"] and rel(out.inverted, ref_inv) < TRAJ_TOL["f32"]
