"""GuidedTransferGraph / SDGuidedTransferGraph on MI355X: the gradient-guided transfer (utils_Img2Img.py:651-760) as ONE captured
trajectory against the eager ``linear_interp_custom_guidance_inverted_start`` (bit for bit) and the committed oracle vectors (the bounds
of the eager tests, read from their parametrisation), the fp16 overflow protocol (scale and flag on the device, retry by replay), replay
with other inputs, and the SD UNet's stale-context check."""
import os

import numpy as np
import pytest
import torch

import test_gpu_sd_pipeline as SP
import test_gpu_unet_backward as UB
from test_gpu_unet_ddib import rel

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
S = 3


def _marks(fn, argnames):
    return next(m.args[1] for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == argnames)


# pixel tier: the 16-bit bounds of test_gradient_guided_transfer_16_bit_engines_vs_golden; fp32: the 2e-3 that
# test_golden_fixture_guided_transfer_f32 asserts (a literal in its body)
PIXEL_TOL = dict(_marks(UB.test_gradient_guided_transfer_16_bit_engines_vs_golden, "mode,tol"), f32=2e-3)
# SD tier: (latents, images) of test_sd_gradient_guided_transfer_matches_golden
SD_TOL = {m: (tl, ti) for m, tl, ti in _marks(SP.test_sd_gradient_guided_transfer_matches_golden, "mode,tol_lat,tol_img")}


def pixel_fixture():
    d = np.load(os.path.join(GOLDEN, "guided_super_small_32_s3.npz"))
    x, labels = torch.from_numpy(d["images"]).cuda(), torch.from_numpy(d["labels"]).cuda()
    return d, x, labels, float(d["p"]), float(d["guidance_loss_scale"])


def eager_pixel(P, pp, x, orig, target, p, gls):
    """(pt output, numpy output, inverted, [losses per step]) of the eager functions."""
    pt = P.linear_interp_custom_guidance_inverted_start(pp, x, orig, target, p, gls, S, output_type="pt")
    arr = P.linear_interp_custom_guidance_inverted_start(pp, x, orig, target, p, gls, S, output_type="numpy")
    inv = P.inversion(pp, x, orig, S)
    again, losses = P.custom_guided_generation(pp, inv, target, p, gls, S, return_losses=True)
    assert torch.equal(again, pt)
    return pt, arr, inv, torch.stack(losses)


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
def test_pixel_runner_equals_the_eager_function_and_the_golden_vectors(mode):
    import phendiff_amd as P
    d, x, labels, p, gls = pixel_fixture()
    _, pp = UB._pipes(mode)
    pt, arr, inv, losses = eager_pixel(P, pp, x, labels, 1 - labels, p, gls)
    runner = P.GuidedTransferGraph(pp, 2, S, p, gls)
    out = runner.run(x, labels, 1 - labels)
    torch.cuda.synchronize()
    assert out is runner and runner.losses.shape == (S, 2) and runner.grad_scale == (4096.0 if mode == "fp16" else 1.0)
    print(f"{mode}: guided differs from eager in {int((runner.guided != pt).sum())} of {pt.numel()} elements; "
          f"vs golden {rel(runner.guided, d['out']):.3e} (bound {PIXEL_TOL[mode]})")
    assert torch.equal(runner.guided, pt)
    assert torch.equal(runner.inverted, inv)
    assert torch.equal(runner.losses, losses)
    assert torch.equal(runner.images.cpu(), torch.from_numpy(arr))
    assert torch.equal(runner.images_u8.cpu(), (runner.images * 255).round().to(torch.uint8).cpu())
    keep = [t.clone() for t in (runner.guided, runner.inverted, runner.losses, runner.images)]
    # the same launches without the capture
    plain = P.GuidedTransferGraph(pp, 2, S, p, gls, use_graph=False).run(x, labels, 1 - labels)
    torch.cuda.synchronize()
    assert not plain.graph
    for a, b in zip(keep, (plain.guided, plain.inverted, plain.losses, plain.images)):
        assert torch.equal(a, b)
    # the committed oracle vectors, and the guidance must have had an effect
    assert rel(keep[0], d["out"]) < PIXEL_TOL[mode]
    ddib = P.DDIBGraph(pp, 2, S).run(x, labels, 1 - labels)
    torch.cuda.synchronize()
    assert torch.equal(ddib.inverted, keep[1])
    assert float((keep[3] - ddib.images).abs().max()) > 1e-2


def test_fp16_overflow_halves_the_device_scale_and_replays(monkeypatch):
    """The runner starts at 2^30 (overflows fp16 on the first cast of the backward): the flag comes back set, the scale is halved on the
    device and the whole trajectory replayed until it is finite.  Not bit-equal to the eager loop, which halves per step and so may have
    run earlier steps at a larger scale (the two differ by fp16 subnormal rounding only): the golden bound holds."""
    import phendiff_amd as P
    import phendiff_amd.img2img as I
    d, x, labels, p, gls = pixel_fixture()
    _, pp = UB._pipes("fp16")
    monkeypatch.setattr(I, "GUIDANCE_GRAD_SCALE", 2.0 ** 30)
    runner = P.GuidedTransferGraph(pp, 2, S, p, gls)
    assert runner.grad_scale == 2.0 ** 30
    launches = []
    launch = runner._launch
    monkeypatch.setattr(runner, "_launch", lambda: (launches.append(runner.grad_scale), launch())[1])
    runner.run(x, labels, 1 - labels)
    torch.cuda.synchronize()
    reached = runner.grad_scale
    print(f"fp16 forced overflow: {len(launches)} launches, scale 2^30 -> 2^{int(np.log2(reached))}; vs golden {rel(runner.guided, d['out']):.3e}")
    assert len(launches) >= 2 and launches == [2.0 ** (30 - i) for i in range(len(launches))]
    assert 0 < reached < 2.0 ** 30 and np.log2(reached) == int(np.log2(reached)) and reached >= 2.0 ** -10
    assert float(runner.steps.scale_dev) == reached and int(runner.steps.overflow) == 0
    assert torch.isfinite(runner.guided).all() and torch.isfinite(runner.losses).all()
    assert rel(runner.guided, d["out"]) < PIXEL_TOL["fp16"]
    first = runner.guided.clone()
    del launches[:]
    runner.run(x, labels, 1 - labels)                   # starts from the scale reached: no retry
    torch.cuda.synchronize()
    assert launches == [reached] and runner.grad_scale == reached and torch.equal(runner.guided, first)


def test_fp16_gives_up_below_the_floor(monkeypatch):
    """A gradient that is not finite at any scale (a NaN in the batch): the same FloatingPointError as the eager loop, the scale kept at
    the floor."""
    import phendiff_amd as P
    import phendiff_amd.img2img as I
    d, x, labels, p, gls = pixel_fixture()
    _, pp = UB._pipes("fp16")
    monkeypatch.setattr(I, "GUIDANCE_GRAD_SCALE", 2.0 ** -8)
    runner = P.GuidedTransferGraph(pp, 2, S, p, gls)
    bad = x.clone()
    bad[0, 0, 0, 0] = float("nan")
    with pytest.raises(FloatingPointError, match="not finite at any scale"):
        runner.run(bad, labels, 1 - labels)
    torch.cuda.synchronize()
    assert runner.grad_scale == 2.0 ** -10 == float(runner.steps.scale_dev)


@pytest.mark.parametrize("mode", ["f32", "fp16"])
def test_pixel_runner_replays(mode):
    import phendiff_amd as P
    d, x, labels, p, gls = pixel_fixture()
    _, pp = UB._pipes(mode)
    runner = P.GuidedTransferGraph(pp, 2, S, p, gls)
    runner.run(x, labels, 1 - labels)
    first = [t.clone() for t in (runner.guided, runner.inverted, runner.losses, runner.images, runner.images_u8)]
    runner.run(x, labels, 1 - labels)
    torch.cuda.synchronize()
    for a, b in zip(first, (runner.guided, runner.inverted, runner.losses, runner.images, runner.images_u8)):
        assert torch.equal(a, b)
    # another batch, the classes the other way round: nothing of the first may linger in a static buffer
    x2 = (x.flip(0) * 0.9).contiguous()
    runner.run(x2, 1 - labels, labels)
    torch.cuda.synchronize()
    got = [t.clone() for t in (runner.guided, runner.inverted, runner.losses)]
    pt, arr, inv, losses = eager_pixel(P, pp, x2, 1 - labels, labels, p, gls)
    assert torch.equal(got[0], pt) and torch.equal(got[1], inv) and torch.equal(got[2], losses)
    assert not torch.equal(got[0], first[0])
    with pytest.raises(ValueError, match="expected images of shape"):
        runner.run(x[:1], labels[:1], 1 - labels[:1])
    with pytest.raises(ValueError, match="expected images of shape"):
        runner.run(torch.zeros(2, 3, 16, 16, device="cuda"), labels, 1 - labels)


def test_batch_above_one_plan_is_refused(monkeypatch):
    import phendiff_amd as P
    _, pp = UB._pipes("bf16")
    monkeypatch.setattr(type(pp.unet), "max_batch", lambda self, H, W: 1)
    with pytest.raises(ValueError, match="exceeds what one launch plan holds"):
        P.GuidedTransferGraph(pp, 2, S, 2, 0.5)
    assert not pp.unet._plans


# ---- latent-diffusion tier -----------------------------------------------------------------------------------------------------------
def sd_fixture():
    d = np.load(os.path.join(GOLDEN, "guided_sd_tiny_32_s3.npz"))
    x, labels = torch.from_numpy(d["images"]).cuda(), torch.from_numpy(d["labels"]).cuda()
    # the posterior noise the vectors were made with (make_golden.py --sd-guided draws it from this generator)
    noise = torch.randn((2, 4, 16, 16), generator=torch.Generator().manual_seed(13)).cuda()
    return d, x, labels, noise, float(d["p"]), float(d["guidance_loss_scale"])


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
def test_sd_runner_equals_the_eager_function_and_the_golden_vectors(mode):
    import phendiff_amd as P
    d, x, labels, noise, p, gls = sd_fixture()
    tol_lat, tol_img = SD_TOL[mode]
    _, pipe = SP.make_pipe(mode)
    runner = P.SDGuidedTransferGraph(pipe, 2, S, p, gls, 32, 32)
    runner.run(x, labels, 1 - labels, noise=noise)
    torch.cuda.synchronize()
    lat, inv, guided, images, losses = (t.clone() for t in (runner.guided_latents, runner.inverted, runner.guided, runner.images, runner.losses))
    e_lat, e_inv = rel(lat, torch.from_numpy(d["guided_latents"])), rel(inv, torch.from_numpy(d["inverted"]))
    print(f"SD {mode}: guided latents vs golden {e_lat:.3e}, inverted {e_inv:.3e} (bound {tol_lat})")
    assert e_lat < tol_lat and e_inv < tol_lat
    assert tuple(guided.shape) == (2, 3, 32, 32) and float(guided.min()) == -1.0 and float(guided.max()) == 1.0
    assert tuple(images.shape) == (2, 32, 32, 3) and float(images.min()) >= 0 and float(images.max()) <= 1
    ref = torch.from_numpy(d["out"])
    if mode == "f32":
        assert rel(guided, ref) < tol_img
    else:       # up to the affine map the min-max renormalisation fixes by two extreme pixels, as the eager test compares
        a, b = guided.cpu() - guided.mean().cpu(), ref - ref.mean()
        assert float((a / a.norm() - b / b.norm()).norm()) < tol_img
    if mode == "fp16":
        return
    gen = lambda: torch.Generator().manual_seed(13)
    pt = P.linear_interp_custom_guidance_inverted_start(pipe, x, labels, 1 - labels, p, gls, S, output_type="pt", generator=gen())
    arr = P.linear_interp_custom_guidance_inverted_start(pipe, x, labels, 1 - labels, p, gls, S, generator=gen())
    e_lat0, (c_orig, c_target) = P.LDM_preprocess(pipe, x, [labels, 1 - labels], generator=gen())
    e_inv = P.inversion(pipe, e_lat0, c_orig, S)
    e_guided, e_losses = P.custom_guided_generation(pipe, e_inv, c_target, p, gls, S, return_losses=True)
    print(f"SD {mode}: latents differ from eager in {int((lat != e_guided).sum())} elements, images in {int((guided != pt).sum())}")
    assert torch.equal(inv, e_inv) and torch.equal(lat, e_guided) and torch.equal(losses, torch.stack(e_losses))
    assert torch.equal(guided, pt) and torch.equal(images.cpu(), torch.from_numpy(arr))
    # replay, then another batch under swapped classes
    runner.run(x, labels, 1 - labels, noise=noise)
    torch.cuda.synchronize()
    assert torch.equal(runner.guided, guided) and torch.equal(runner.guided_latents, lat)
    x2 = (x.flip(0) * 0.9).contiguous()
    runner.run(x2, 1 - labels, labels, generator=torch.Generator().manual_seed(5))
    torch.cuda.synchronize()
    pt2 = P.linear_interp_custom_guidance_inverted_start(pipe, x2, 1 - labels, labels, p, gls, S, output_type="pt",
                                                         generator=torch.Generator().manual_seed(5))
    assert torch.equal(runner.guided, pt2)
    with pytest.raises(ValueError, match="expected images of shape"):
        runner.run(x[:1], labels[:1], 1 - labels[:1], noise=noise[:1])


@pytest.mark.parametrize("use_graph", [True, False])
def test_eager_forward_after_an_sd_guided_graph_projects_its_context_again(use_graph):
    """As for SDDDIBGraph: the inversion half runs on the UNet's shared inference plan and leaves its class context there."""
    import phendiff_amd as P
    from phendiff_amd.sd_pipeline import hack_class_embedding
    _, pipe = SP.make_pipe("f32")
    unet = pipe.unet
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(2, 4, 16, 16, generator=g).cuda()
    x = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).cuda()
    noise = torch.randn(2, 4, 16, 16, generator=g).cuda()
    labels = torch.tensor([0, 1]).cuda()
    E = hack_class_embedding(pipe._encode_class(class_labels=labels, device=lat.device, do_classifier_free_guidance=False)).contiguous()
    o1 = unet(lat, 500, E, return_dict=False)[0].clone()
    runner = P.SDGuidedTransferGraph(pipe, 2, 2, 2, 0.5, 32, 32, use_graph=use_graph)
    assert runner.plan is unet.plan_for(2, 16, 16, 77, lat.device)
    runner.run(x, 1 - labels, 1 - labels, noise=noise)             # both halves under the other context
    o2 = unet(lat, 500, E, return_dict=False)[0]
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)
