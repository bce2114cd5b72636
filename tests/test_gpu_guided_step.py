"""``pd_guided_step`` and ``pd_lp_guidance_scaled`` on MI355X against the launches they replace, bit for bit:
``g_unet *= 1 / scale`` -> ``pd_guidance_apply`` -> ``pd_ddim_step(sample = pushed)`` resp. ``pd_lp_guidance`` -> ``d_model_out * scale``;
the overflow flag; guard bands (tests/guard_bands.py through the engine of tests/test_gpu_guard_bands.py); run-to-run determinism."""
import ctypes as C

import pytest
import torch

from test_gpu_guard_bands import Case, Op, out_op, p1_poisoned_surroundings, p2_canaried_outputs, p3_sample_isolation
from test_gpu_kernels import env, stream  # noqa: F401

pytestmark = pytest.mark.gpu

# (sqrt_a, sqrt_b, sqrt_ap, dir_coef): a mid-trajectory level, and one near t = N where epsilon-prediction divides by a small sqrt_a
# (a fused multiply-add in the numerator would show there)
COEFS = [(0.8, 0.6, 0.9, 0.4358899), (0.0123, 0.99992436, 0.05, 0.99874922)]
# the last exceeds the grid cap (1024 blocks x 1024 elements): the grid-stride loop runs; (2, 3, 5, 7): numel % 4 == 2, the partial vector
SHAPES = [(2, 3, 4, 4), (3, 3, 10, 6), (2, 3, 32, 32), (6, 3, 256, 256), (2, 3, 5, 7)]
SCALES = [None, 1.0, 4096.0, 2.0 ** -3]


def operands(shape, scale, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
    out = torch.randn(shape, generator=g).to(dev)
    gd = (torch.randn(shape, generator=g) * 0.05).to(dev)
    gu = (torch.randn(shape, generator=g) * 0.05 * (scale or 1.0)).to(dev)
    return x, out, gd, gu


def step_fields(x, pred, clip, coefs):
    sa, sb, sap, dirc = coefs
    return dict(numel=x.numel(), per_sample=x[0].numel(), pred_type=pred, clip=clip, clip_range=1.0, use_clipped_model_output=0,
                sqrt_a=sa, sqrt_b=sb, sqrt_ap=sap, dir_coef=dirc)


def three_launches(L, lib, x, out, gd, gu, pred, clip, coefs, gls, scale):
    """(prev_sample, pushed) the way ``custom_guided_generation`` gets them."""
    u = gu.clone()
    if scale is not None:
        u.mul_(1.0 / scale)
    pushed, prev = torch.empty_like(x), torch.empty_like(x)
    a = L.GuidanceApplyArgs(numel=x.numel(), scale=gls, x=x.data_ptr(), g_direct=gd.data_ptr(), g_unet=u.data_ptr(), out=pushed.data_ptr())
    L.check(lib.pd_guidance_apply(C.byref(a), stream()), "pd_guidance_apply")
    d = L.DdimStepArgs(sample=pushed.data_ptr(), model_out=out.data_ptr(), uncond_out=None, w=None, w_per_sample=0, guidance_cfg=0,
                       prev_sample=prev.data_ptr(), pred_x0=None, **step_fields(x, pred, clip, coefs))
    L.check(lib.pd_ddim_step(C.byref(d), stream()), "pd_ddim_step")
    return prev, pushed


def guided_step(L, lib, x, out, gd, gu, pred, clip, coefs, gls, scale_dev, prev, pushed, overflow):
    a = L.GuidedStepArgs(guidance_scale=gls, grad_scale=L.ptr(scale_dev), sample=x.data_ptr(), g_direct=gd.data_ptr(), g_unet=gu.data_ptr(),
                         model_out=out.data_ptr(), prev_sample=prev.data_ptr(), pushed=L.ptr(pushed), overflow=L.ptr(overflow),
                         **step_fields(x, pred, clip, coefs))
    L.check(lib.pd_guided_step(C.byref(a), stream()), "pd_guided_step")


@pytest.mark.parametrize("alias", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("scale", SCALES, ids=lambda s: f"scale-{s}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_guided_step_equals_the_three_launches(env, shape, scale, alias):
    L, lib, _, dev = env
    x, out, gd, gu = operands(shape, scale, dev)
    scale_dev = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=dev)
    worst = 0
    for pred in (0, 1, 2):
        for clip in (0, 1):
            for coefs in COEFS:
                want_prev, want_pushed = three_launches(L, lib, x, out, gd, gu, pred, clip, coefs, 0.5, scale)
                sample = x.clone()
                prev = sample if alias else torch.full_like(x, float("nan"))
                pushed = torch.full_like(x, float("nan"))
                guided_step(L, lib, sample, out, gd, gu, pred, clip, coefs, 0.5, scale_dev, prev, pushed, None)
                torch.cuda.synchronize()
                worst = max(worst, int((prev != want_prev).sum()), int((pushed != want_pushed).sum()))
                assert torch.equal(pushed, want_pushed), (pred, clip, coefs)
                assert torch.equal(prev, want_prev), (pred, clip, coefs)
                if not alias:
                    assert torch.equal(sample, x)
    print(f"pd_guided_step {shape} scale {scale} {'in place' if alias else 'out of place'}: {worst} elements differ from the three launches")
    # `pushed` is optional
    prev = torch.empty_like(x)
    guided_step(L, lib, x, out, gd, gu, 2, 1, COEFS[0], 0.5, scale_dev, prev, None, None)
    torch.cuda.synchronize()
    assert torch.equal(prev, three_launches(L, lib, x, out, gd, gu, 2, 1, COEFS[0], 0.5, scale)[0])


BIG = (6, 3, 256, 256)      # 1 179 648 elements: those from 1 048 576 on belong to the second pass of the grid-stride loop


@pytest.mark.parametrize("where", ["first", "last", "stride-tail"])
@pytest.mark.parametrize("what", [float("inf"), float("-inf"), float("nan")], ids=["inf", "-inf", "nan"])
def test_overflow_flag_is_set_by_one_non_finite_gradient(env, where, what):
    L, lib, _, dev = env
    x, out, gd, gu = operands(BIG, 4096.0, dev)
    scale_dev = torch.tensor([4096.0], dtype=torch.float32, device=dev)
    flag = torch.tensor([-7, 0, -9], dtype=torch.int32, device=dev)      # canaries on both sides of the flag
    prev = torch.empty_like(x)
    guided_step(L, lib, x, out, gd, gu, 2, 1, COEFS[0], 0.5, scale_dev, prev, None, flag[1:2])
    torch.cuda.synchronize()
    assert flag.tolist() == [-7, 0, -9], "finite gradients must leave the flag alone"
    index = {"first": 0, "last": x.numel() - 1, "stride-tail": 1024 * 1024 + 4 * 1000 + 1}[where]
    gu.view(-1)[index] = what
    guided_step(L, lib, x, out, gd, gu, 2, 1, COEFS[0], 0.5, scale_dev, prev, None, flag[1:2])
    torch.cuda.synchronize()
    assert flag.tolist() == [-7, 1, -9]
    # no flag to set: the launch runs and returns, and every other element is what it was
    again = torch.empty_like(x)
    guided_step(L, lib, x, out, gd, gu, 2, 1, COEFS[0], 0.5, scale_dev, again, None, None)
    torch.cuda.synchronize()
    keep = torch.ones(x.numel(), dtype=torch.bool, device=dev)
    keep[index] = False
    assert torch.equal(again.view(-1)[keep], prev.view(-1)[keep]) and not torch.isfinite(again.view(-1)[index])


def test_overflow_flag_small_tensors_and_partial_vector(env):
    """The flag at sizes below one block, and with the non-finite element in the partial last vector (numel % 4 == 2)."""
    L, lib, _, dev = env
    for shape in ((2, 3, 4, 4), (2, 3, 5, 7)):
        x, out, gd, gu = operands(shape, None, dev)
        flag = torch.tensor([-7, 0, -9], dtype=torch.int32, device=dev)
        prev = torch.empty_like(x)
        guided_step(L, lib, x, out, gd, gu, 0, 1, COEFS[1], 0.5, None, prev, None, flag[1:2])
        torch.cuda.synchronize()
        assert flag.tolist() == [-7, 0, -9]
        gu.view(-1)[-1] = float("inf")
        guided_step(L, lib, x, out, gd, gu, 0, 1, COEFS[1], 0.5, None, prev, None, flag[1:2])
        torch.cuda.synchronize()
        assert flag.tolist() == [-7, 1, -9]


def lp_args(L, x, out, target, p, pred, splits, partial, d_out, d_dir, losses, coefs=COEFS[0]):
    return L.LpGuidanceArgs(numel=x.numel(), per_sample=x[0].numel(), pred_type=pred, clip=1, clip_range=1.0, sqrt_a=coefs[0], sqrt_b=coefs[1],
                            p=float(p), sample=x.data_ptr(), model_out=out.data_ptr(), target=target.data_ptr(), partial=partial.data_ptr(),
                            splits=splits, d_model_out=d_out.data_ptr(), d_sample_direct=d_dir.data_ptr(), losses=losses.data_ptr())


def lp_operands(shape, dev):
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
    out = (torch.randn(shape, generator=g) * 0.7).to(dev)
    target = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
    return x, out, target


@pytest.mark.parametrize("scale", [1.0, 4096.0])
@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("shape,splits", [((2, 3, 10, 6), 1), ((3, 3, 64, 64), 3)], ids=["2x3x10x6", "3x3x64x64-splits3"])
def test_lp_guidance_scaled_equals_lp_guidance_times_scale(env, shape, splits, p, scale):
    L, lib, _, dev = env
    x, out, target = lp_operands(shape, dev)
    B = shape[0]
    new = lambda: (torch.empty(B * splits, dtype=torch.float64, device=dev), torch.empty_like(x), torch.empty_like(x), torch.empty(B, device=dev))
    scale_dev = torch.tensor([scale], dtype=torch.float32, device=dev)
    for pred in (0, 1, 2):
        want, got = new(), new()
        L.check(lib.pd_lp_guidance(C.byref(lp_args(L, x, out, target, p, pred, splits, *want)), stream()), "pd_lp_guidance")
        L.check(lib.pd_lp_guidance_scaled(C.byref(lp_args(L, x, out, target, p, pred, splits, *got)), scale_dev.data_ptr(), stream()),
                "pd_lp_guidance_scaled")
        torch.cuda.synchronize()
        assert float(want[1].abs().max()) > 0
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
        assert torch.equal(got[1], want[1] * scale), pred


# ---- guard bands: B = 2, numel % 4 == 2 (the partial vector sits against the back guard), the second sample starts inside a vector ----
GB_SHAPE = (2, 3, 5, 7)


def guided_step_case(env_, scale):
    L, lib, _, dev = env_
    x, out, gd, gu = (t.cpu() for t in operands(GB_SHAPE, scale, "cpu"))
    ins = {"sample": Op(x, sample_dim=0), "model_out": Op(out, sample_dim=0), "g_direct": Op(gd, sample_dim=0), "g_unet": Op(gu, sample_dim=0)}
    if scale is not None:
        ins["grad_scale"] = Op(torch.tensor([scale], dtype=torch.float32))
    outs = {"prev_sample": out_op(GB_SHAPE, torch.float32, sample_dim=0), "pushed": out_op(GB_SHAPE, torch.float32, sample_dim=0),
            "overflow": Op(torch.zeros(1, dtype=torch.int32))}

    def launch(T):
        guided_step(L, lib, T["sample"], T["model_out"], T["g_direct"], T["g_unet"], 0, 1, COEFS[1], 0.5, T.get("grad_scale"),
                    T["prev_sample"], T["pushed"], T["overflow"])

    def check(O):
        prev, pushed = three_launches(L, lib, x.to(dev), out.to(dev), gd.to(dev), gu.to(dev), 0, 1, COEFS[1], 0.5, scale)
        torch.cuda.synchronize()
        assert torch.equal(O["prev_sample"], prev.cpu()) and torch.equal(O["pushed"], pushed.cpu()) and int(O["overflow"]) == 0

    return Case(ins, outs, launch, check, nsamples=GB_SHAPE[0])


def lp_scaled_case(env_, p):
    L, lib, _, dev = env_
    x, out, target = lp_operands(GB_SHAPE, "cpu")
    B, splits, scale = GB_SHAPE[0], 2, 4096.0
    ins = {"sample": Op(x, sample_dim=0), "model_out": Op(out, sample_dim=0), "target": Op(target, sample_dim=0),
           "grad_scale": Op(torch.tensor([scale], dtype=torch.float32))}
    outs = {"partial": out_op((B, splits), torch.float64, sample_dim=0), "d_model_out": out_op(GB_SHAPE, torch.float32, sample_dim=0),
            "d_sample_direct": out_op(GB_SHAPE, torch.float32, sample_dim=0), "losses": out_op((B,), torch.float32, sample_dim=0)}

    def launch(T):
        a = lp_args(L, T["sample"], T["model_out"], T["target"], p, 2, splits, T["partial"], T["d_model_out"], T["d_sample_direct"], T["losses"])
        L.check(lib.pd_lp_guidance_scaled(C.byref(a), T["grad_scale"].data_ptr(), stream()), "pd_lp_guidance_scaled")

    def check(O):
        w = (torch.empty(B * splits, dtype=torch.float64, device=dev), torch.empty(GB_SHAPE, device=dev), torch.empty(GB_SHAPE, device=dev),
             torch.empty(B, device=dev))
        L.check(lib.pd_lp_guidance(C.byref(lp_args(L, x.to(dev), out.to(dev), target.to(dev), p, 2, splits, *w)), stream()), "pd_lp_guidance")
        torch.cuda.synchronize()
        assert torch.equal(O["d_model_out"], (w[1] * scale).cpu()) and torch.equal(O["d_sample_direct"], w[2].cpu())
        assert torch.equal(O["losses"], w[3].cpu()) and torch.equal(O["partial"].view(-1), w[0].cpu())

    return Case(ins, outs, launch, check, nsamples=B)


GB_CASES = [("pd_guided_step", guided_step_case, None), ("pd_guided_step", guided_step_case, 4096.0),
            ("pd_lp_guidance_scaled", lp_scaled_case, 2), ("pd_lp_guidance_scaled", lp_scaled_case, 3)]
_gb_id = lambda c: f"{c[0]}-{c[2]}"


@pytest.mark.parametrize("c", GB_CASES, ids=_gb_id)
def test_guided_p1_poisoned_surroundings(env, monkeypatch, c):
    p1_poisoned_surroundings(c[1](env, c[2]), env[3], monkeypatch)


@pytest.mark.parametrize("c", GB_CASES, ids=_gb_id)
def test_guided_p2_canaried_outputs(env, monkeypatch, c):
    p2_canaried_outputs(c[1](env, c[2]), env[3], monkeypatch)


@pytest.mark.parametrize("c", GB_CASES, ids=_gb_id)
def test_guided_p3_sample_isolation(env, monkeypatch, c):
    p3_sample_isolation(c[1](env, c[2]), env[3], monkeypatch)


def test_two_calls_are_bit_identical(env):
    L, lib, _, dev = env
    x, out, gd, gu = operands(BIG, 4096.0, dev)
    scale_dev = torch.tensor([4096.0], dtype=torch.float32, device=dev)
    runs = []
    for _ in range(2):
        prev, pushed = torch.empty_like(x), torch.empty_like(x)
        guided_step(L, lib, x, out, gd, gu, 0, 1, COEFS[1], 0.5, scale_dev, prev, pushed, None)
        runs.append((prev, pushed))
    x2, out2, target = lp_operands((3, 3, 64, 64), dev)
    for _ in range(2):
        w = (torch.empty(9, dtype=torch.float64, device=dev), torch.empty_like(x2), torch.empty_like(x2), torch.empty(3, device=dev))
        L.check(lib.pd_lp_guidance_scaled(C.byref(lp_args(L, x2, out2, target, 3, 2, 3, *w)), scale_dev.data_ptr(), stream()), "pd_lp_guidance_scaled")
        runs.append(w)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert all(torch.equal(a, b) for a, b in zip(runs[2], runs[3]))
