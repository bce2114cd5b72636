"""The three mask kernels on MI355X against their float64 restatement (tests/contrast_mask_ref.py) on the shared seeded cases
(tests/contrast_mask_cases.py), their exact properties, and the guard-band properties P1 / P2 / P3 of tests/test_gpu_guard_bands.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from contrast_mask_cases import CASES, GUARD_CASES, RATIO, case_id, inputs, reference
from test_gpu_guard_bands import Case, Op, out_op, p1_poisoned_surroundings, p2_canaried_outputs, p3_sample_isolation
from test_gpu_kernels import env, stream  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ulps(got, ref):
    """|got - ref| in units of the fp32 spacing at ref (got: float32; ref: float32, or float64 taken as it is)."""
    got, ref = np.asarray(got, np.float32).astype(np.float64), np.asarray(ref).astype(np.float64)
    return np.abs(got - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def class_contrast(env_, a, b, acc, first):
    L, lib = env_[0], env_[1]
    B, Cc, H, W = a.shape
    args = L.ClassContrastArgs(B=B, C=Cc, per_pixel=H * W, a=a.data_ptr(), b=b.data_ptr(), acc=acc.data_ptr(), first=int(first))
    L.check(lib.pd_class_contrast(C.byref(args), stream()), "pd_class_contrast")


def contrast_mask(env_, acc, ratio=RATIO, want_map=True, want_stats=True):
    """(mask, map, stats) of a device (B, H, W) fp32 ``acc``."""
    L, lib = env_[0], env_[1]
    B, n = acc.shape[0], acc[0].numel()
    mask = torch.full(acc.shape, 7, dtype=torch.uint8, device=acc.device)
    cmap = torch.full(acc.shape, float("nan"), dtype=torch.float32, device=acc.device) if want_map else None
    stats = torch.full((B, 3), float("nan"), dtype=torch.float32, device=acc.device) if want_stats else None
    ws = torch.empty((lib.pd_contrast_mask_workspace(B, n) // 8,), dtype=torch.float64, device=acc.device)
    args = L.ContrastMaskArgs(B=B, per_pixel=n, acc=acc.data_ptr(), ratio=ratio, mask=mask.data_ptr(), map=L.ptr(cmap), stats=L.ptr(stats),
                              workspace=ws.data_ptr())
    L.check(lib.pd_contrast_mask(C.byref(args), stream()), "pd_contrast_mask")
    torch.cuda.synchronize()
    return mask, cmap, stats


def blend(env_, x, keep, mask, out):
    L, lib = env_[0], env_[1]
    B, Cc, H, W = x.shape
    args = L.MaskBlendArgs(B=B, C=Cc, per_pixel=H * W, x=x.data_ptr(), keep=keep.data_ptr(), mask=mask.data_ptr(), out=out.data_ptr())
    L.check(lib.pd_mask_blend(C.byref(args), stream()), "pd_mask_blend")


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- pd_class_contrast -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_class_contrast_against_float64(env, case):
    """Every acc element within 4 * C * num_maps * 2^-24 * max|acc_ref| of the reference: the fp32 rounding of C additions per draw and
    num_maps accumulations at half an ulp each, with a factor 4 of head-room (derived, not measured).  The first draw is written over a
    NaN-filled acc."""
    B, Cc, H, W, M = case
    a, b = inputs(case)
    ref = reference(case)["acc"]
    acc = torch.full((B, 1, H, W), float("nan"), dtype=torch.float32, device=DEV)
    for k in range(M):
        class_contrast(env, torch.tensor(a[k]).to(DEV), torch.tensor(b[k]).to(DEV), acc, first=(k == 0))
        if k == 0:
            assert bool(torch.isfinite(acc).all()), "first = 1 must not read acc"
    got = acc.cpu().numpy().reshape(B, H, W).astype(np.float64)
    bound = 4 * Cc * M * 2.0 ** -24 * float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print(f"pd_class_contrast {case_id(case)}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


# ---- pd_contrast_mask ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_contrast_mask_against_reference(env, case):
    """From the reference's fp32-rounded acc: the mask exactly (tests/test_host_contrast_mask.py::test_margin_condition makes that fair),
    the map within 2 fp32 ulp, the mean within 1 ulp of the float64 mean rounded to fp32, the fraction exactly."""
    ref = reference(case)
    mask, cmap, stats = contrast_mask(env, torch.tensor(ref["acc32"]).to(DEV))
    assert np.array_equal(mask.cpu().numpy(), ref["mask"])
    map_ulps = float(ulps(cmap.cpu().numpy(), ref["map"]).max())      # (against the float64 map itself)
    mean_ulps = float(ulps(stats[:, 0].cpu().numpy(), ref["stats"][:, 0]).max())
    print(f"pd_contrast_mask {case_id(case)}: map {map_ulps:.2f} ulp, mean {mean_ulps:.2f} ulp")
    assert map_ulps <= 2
    assert mean_ulps <= 1
    assert np.array_equal(stats[:, 2].cpu().numpy(), ref["stats"][:, 2])
    limit = stats[:, 1].cpu().numpy()
    assert np.array_equal(limit, (np.float32(RATIO) * stats[:, 0].cpu().numpy()).astype(np.float32))      # limit = ratio * mean, one fp32 product
    # the optional outputs are optional: the mask alone is the same mask
    alone, _, _ = contrast_mask(env, torch.tensor(ref["acc32"]).to(DEV), want_map=False, want_stats=False)
    assert torch.equal(alone, mask)


@pytest.mark.parametrize("case", [CASES[1], CASES[5]], ids=case_id)
def test_contrast_mask_exact_properties(env, case):
    B = case[0]
    acc = torch.tensor(reference(case)["acc32"]).to(DEV)
    mask, cmap, stats = contrast_mask(env, acc)
    again = contrast_mask(env, acc)
    for got, first in zip(again, (mask, cmap, stats)):      # two runs: bitwise equal
        assert same_bits(got, first)
    for s in range(B):                                       # a row alone equals the row in its batch, bitwise
        m1, c1, s1 = contrast_mask(env, acc[s:s + 1].clone())
        assert same_bits(m1[0], mask[s]) and same_bits(c1[0], cmap[s]) and same_bits(s1[0], stats[s])
    for s in range(B):                                       # a NaN sample: an empty mask of its own, its neighbours unchanged
        bad = acc.clone()
        bad[s].view(-1)[bad[s].numel() // 2] = float("nan")
        mb, cb, sb = contrast_mask(env, bad)
        assert not bool(mb[s].any()) and not bool(cb[s].any()) and float(sb[s, 2]) == 0.0 and bool(torch.isnan(sb[s, 0]))
        for o in range(B):
            if o != s:
                assert same_bits(mb[o], mask[o]) and same_bits(cb[o], cmap[o]) and same_bits(sb[o], stats[o])
    zero = acc.clone()                                       # an all-zero sample: an empty mask and stats {0, 0, 0}
    zero[B - 1].zero_()
    mz, cz, sz = contrast_mask(env, zero)
    assert not bool(mz[B - 1].any()) and not bool(cz[B - 1].any()) and sz[B - 1].tolist() == [0.0, 0.0, 0.0]
    assert same_bits(mz[:B - 1], mask[:B - 1]) and same_bits(sz[:B - 1], stats[:B - 1])
    inf = acc.clone()                                        # an infinity: the limit is not finite
    inf[0].view(-1)[0] = float("inf")
    mi, ci, _ = contrast_mask(env, inf)
    assert not bool(mi[0].any()) and not bool(ci[0].any())


# ---- pd_mask_blend ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 5, 7), (3, 1, 5, 7), (3, 3, 8, 8), (2, 32, 4, 4), (3, 2, 67, 61), (5, 1, 1, 1)], ids=str)
def test_mask_blend(env, shape):
    B, Cc, H, W = shape
    rng = np.random.default_rng([7, B, Cc, H, W])
    x, keep = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    mask = (rng.random((B, 1, H, W)) < 0.5).astype(np.uint8)
    mask[rng.random(mask.shape) < 0.1] *= 200                                       # any non-zero byte takes x
    # NaN / Inf on the side NOT taken must not reach out
    x_p, keep_p = x.copy(), keep.copy()
    taken = np.broadcast_to(mask != 0, shape)
    x_p[~taken] = np.where(rng.random(int((~taken).sum())) < 0.5, np.nan, np.inf)
    keep_p[taken] = np.where(rng.random(int(taken.sum())) < 0.5, np.nan, -np.inf)
    want = np.where(taken, x, keep)
    xd, kd, md = torch.tensor(x_p).to(DEV), torch.tensor(keep_p).to(DEV), torch.tensor(mask).to(DEV)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    blend(env, xd, kd, md, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))      # bitwise np.where; nothing of the other side
    inplace = xd.clone()                                                                 # out == x
    blend(env, inplace, kd, md, inplace)
    assert same_bits(inplace, out)
    into_keep = kd.clone()                                                               # out == keep
    blend(env, xd, into_keep, md, into_keep)
    assert same_bits(into_keep, out)
    ones, zeros = torch.ones_like(md), torch.zeros_like(md)
    xc, kc = torch.tensor(x).to(DEV), torch.tensor(keep).to(DEV)
    blend(env, xc, kc, ones, out)
    assert same_bits(out, xc)                                                            # all ones: x
    blend(env, xc, kc, zeros, out)
    assert same_bits(out, kc)                                                            # all zeros: keep


def test_mask_blend_host_function(env):
    import phendiff_amd as P
    g = torch.Generator().manual_seed(3)
    x, keep = torch.randn(3, 3, 8, 8, generator=g).to(DEV), torch.randn(3, 3, 8, 8, generator=g).to(DEV)
    m = (torch.rand(3, 8, 8, generator=g) < 0.5).to(DEV)
    want = torch.where(m[:, None], x, keep)
    assert same_bits(P.mask_blend(x, keep, m), want)                          # (B, H, W) bool
    assert same_bits(P.mask_blend(x, keep, m[:, None].to(torch.uint8)), want)      # (B, 1, H, W) uint8
    xc = x.clone()
    assert P.mask_blend(xc, keep, m, out=xc) is xc and same_bits(xc, want)


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------------
def class_contrast_guard_case(env_, case, first):
    B, Cc, H, W, _ = case
    a, b = inputs(case)
    prior = torch.tensor(reference(case)["acc32"]).view(B, 1, H, W)
    ins = {"a": Op(torch.tensor(a[0]), sample_dim=0), "b": Op(torch.tensor(b[0]), sample_dim=0)}
    # first: acc is NaN before the launch and must be finite after it; else it is read AND written: an input whose body the launch updates
    outs = {"acc": out_op((B, 1, H, W), torch.float32, sample_dim=0) if first else Op(prior.clone(), sample_dim=0)}

    def launch(T):
        class_contrast(env_, T["a"], T["b"], T["acc"], first)

    def check(O):
        ref = np.abs(a[0].astype(np.float64) - b[0].astype(np.float64)).sum(1) / Cc + (0 if first else prior.numpy().reshape(B, H, W).astype(np.float64))
        assert np.abs(O["acc"].numpy().reshape(B, H, W) - ref).max() <= 4 * (Cc + 1) * 2.0 ** -24 * np.abs(ref).max()
    return Case(ins, outs, launch, check, nsamples=B)


def contrast_mask_guard_case(env_, case):
    L, lib = env_[0], env_[1]
    B, _, H, W, _ = case
    ref = reference(case)
    n = H * W
    ins = {"acc": Op(torch.tensor(ref["acc32"]).view(B, 1, H, W), sample_dim=0)}
    outs = {"mask": Op(torch.full((B, 1, H, W), 255, dtype=torch.uint8), sample_dim=0), "map": out_op((B, 1, H, W), torch.float32, sample_dim=0),
            "stats": out_op((B, 3), torch.float32, sample_dim=0),
            "workspace": out_op((lib.pd_contrast_mask_workspace(B, n) // 8,), torch.float64)}

    def launch(T):
        args = L.ContrastMaskArgs(B=B, per_pixel=n, acc=T["acc"].data_ptr(), ratio=RATIO, mask=T["mask"].data_ptr(), map=T["map"].data_ptr(),
                                  stats=T["stats"].data_ptr(), workspace=T["workspace"].data_ptr())
        L.check(lib.pd_contrast_mask(C.byref(args), stream()), "pd_contrast_mask")

    def check(O):
        assert np.array_equal(O["mask"].numpy().reshape(B, H, W), ref["mask"])
        assert np.array_equal(O["stats"][:, 2].numpy(), ref["stats"][:, 2])
    return Case(ins, outs, launch, check, nsamples=B)


def mask_blend_guard_case(env_, case):
    B, _, H, W, _ = case
    Cc = 3
    rng = np.random.default_rng([11, B, H, W])
    x, keep = (torch.tensor(rng.standard_normal((B, Cc, H, W)).astype(np.float32)) for _ in range(2))
    mask = torch.tensor((rng.random((B, 1, H, W)) < 0.5).astype(np.uint8))
    ins = {"x": Op(x, sample_dim=0), "keep": Op(keep, sample_dim=0), "mask": Op(mask, sample_dim=0)}
    outs = {"out": out_op((B, Cc, H, W), torch.float32, sample_dim=0)}

    def launch(T):
        blend(env_, T["x"], T["keep"], T["mask"], T["out"])

    def check(O):
        assert torch.equal(O["out"], torch.where(mask != 0, x, keep))
    return Case(ins, outs, launch, check, nsamples=B)


GUARDED = ([("pd_class_contrast-first", lambda e, c: class_contrast_guard_case(e, c, True), c) for c in GUARD_CASES]
           + [("pd_class_contrast-accumulate", lambda e, c: class_contrast_guard_case(e, c, False), c) for c in GUARD_CASES]
           + [("pd_contrast_mask", contrast_mask_guard_case, c) for c in GUARD_CASES]
           + [("pd_mask_blend", mask_blend_guard_case, c) for c in GUARD_CASES])
_gid = lambda g: f"{g[0]}-{case_id(g[2])}"


@pytest.mark.parametrize("g", GUARDED, ids=_gid)
def test_p1_poisoned_surroundings(env, g, monkeypatch):
    p1_poisoned_surroundings(g[1](env, g[2]), env[3], monkeypatch)


@pytest.mark.parametrize("g", GUARDED, ids=_gid)
def test_p2_canaried_outputs(env, g, monkeypatch):
    p2_canaried_outputs(g[1](env, g[2]), env[3], monkeypatch)


# (P3 over one sample has no other sample to watch: the 35-pixel shape also at B = 3, where sample boundaries fall inside a quad)
@pytest.mark.parametrize("g", GUARDED + [(name, build, CASES[1]) for name, build, c in GUARDED if c == CASES[0]], ids=_gid)
def test_p3_sample_isolation(env, g, monkeypatch):
    p3_sample_isolation(g[1](env, g[2]), env[3], monkeypatch)
