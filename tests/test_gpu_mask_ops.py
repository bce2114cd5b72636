"""The mask refinement on MI355X (``phendiff_amd.mask_ops`` / ``csrc/mask_morph.hip``) against the numpy references of
``tests/mask_ops_ref.py`` over the shared cases of ``tests/mask_ops_cases.py``.  Everything is integers: every comparison is exact equality.
A reference is computed once per (case, request) and shared (``mask_ops_cases.reference``)."""
import numpy as np
import pytest
import torch

from mask_ops_cases import BIG, CASES, NAMES, RADII, RECIPES, SMALL, reference
from mask_ops_ref import FAR, r2_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(name):
    return torch.from_numpy(CASES[name].copy()).to(DEV)


def same(t, ref):
    got = t.cpu().numpy()
    return got.shape == ref.shape and np.array_equal(got, ref)


def radii(name):
    return RADII if name != BIG else RADII[1:2]


@pytest.mark.parametrize("name", NAMES)
def test_distance(name):
    import phendiff_amd as P
    m = dev(name)
    for to_set in (False, True):
        d = P.mask_distance(m, to_set=to_set)
        assert d.dtype == torch.int32 and same(d, reference(name, "d2", to_set)), to_set
        for limit in (1, 5):      # saturation: every value above limit, PD_MASK_FAR included, is limit + 1
            ref = reference(name, "d2", to_set)
            want = np.where(ref > limit, limit + 1, ref)
            assert same(P.mask_distance(m, to_set=to_set, limit=limit), want), (to_set, limit)
    assert P.mask_ops.MASK_FAR == FAR
    as_bool = (m != 0)[:, None]      # (B, 1, H, W) bool: the same numbers in the input's shape
    d = P.mask_distance(as_bool)
    assert tuple(d.shape) == tuple(as_bool.shape) and same(d[:, 0], reference(name, "d2", False))


@pytest.mark.parametrize("name", NAMES)
def test_morphology(name):
    import phendiff_amd as P
    m = dev(name)
    for radius in radii(name):
        r2 = r2_of(radius)
        for fn, what in ((P.mask_dilate, "dilate"), (P.mask_erode, "erode"), (P.mask_open, "open"), (P.mask_close, "close")):
            out = fn(m, radius)
            assert out.dtype == torch.uint8 and same(out, reference(name, what, r2)), (what, radius)
            if what in ("open", "close"):      # idempotent
                assert torch.equal(fn(out, radius), out), (what, radius)
    assert torch.equal(m, dev(name))      # the input is never written


@pytest.mark.parametrize("name", NAMES)
def test_components(name):
    import phendiff_amd as P
    m = dev(name)
    for conn, phase in ((8, 1), (4, 1), (4, 0), (8, 0)):
        label, area, border, count = reference(name, "label", conn, phase)
        c = P.mask_components(m, connectivity=conn, phase=phase)
        assert c.label.dtype == c.area.dtype == c.count.dtype == torch.int32 and c.border.dtype == torch.uint8
        assert same(c.label, label) and same(c.area, area) and same(c.border, border) and same(c.count, count), (conn, phase)
        assert not bool(c.status.any()), (conn, phase)


@pytest.mark.parametrize("name", NAMES)
def test_filters(name):
    import phendiff_amd as P
    m = dev(name)
    for min_area, conn in ((2, 8), (9, 4)) if name != BIG else ((9, 8),):
        assert same(P.remove_small_components(m, min_area, connectivity=conn), reference(name, "drop_small", min_area, conn)[0]), (min_area, conn)
    for max_area, conn in ((None, 8), (5, 8), (None, 4)) if name != BIG else ((None, 8),):
        assert same(P.fill_holes(m, max_area, connectivity=conn), reference(name, "fill_holes", max_area, conn)[0]), (max_area, conn)
    if name != BIG:
        assert torch.equal(P.remove_small_components(m, 0), (m != 0).to(torch.uint8)) and torch.equal(P.fill_holes(m, 0), (m != 0).to(torch.uint8))


@pytest.mark.parametrize("name", NAMES)
def test_recipe(name):
    """The recipe and its stats rows (pixels in, pixels out, components seen, components kept / filled, status = 0) per enabled stage."""
    import phendiff_amd as P
    m = dev(name)
    B, H, W = m.shape
    for k, params in enumerate(RECIPES if name != BIG else RECIPES[:1]):
        want, stats = reference(name, "refine", k)
        r = P.MaskRefine(B, H, W, DEV, **params)
        r.enqueue(torch.cuda.current_stream().cuda_stream, m)
        assert tuple(r.mask.shape) == (B, 1, H, W) and same(r.mask[:, 0], want), k
        assert tuple(r.stats.shape) == stats.shape and r.stats.dtype == torch.int32 and same(r.stats, stats), (k, r.stats.cpu(), stats)
        assert r.stages == tuple(s for s in P.mask_ops.STAGES if params.get(s))
        assert same(P.refine_mask(m, **params), want) and same(P.refine_mask(m[:, None] != 0, **params)[:, 0], want)
    assert torch.equal(m, dev(name))      # src is never written


def everything(m):
    """Every primitive's result and the recipe's over one batch, as a dict of CPU tensors."""
    import phendiff_amd as P
    B, H, W = m.shape
    out = {"d2_clear": P.mask_distance(m), "d2_set": P.mask_distance(m, to_set=True), "d2_limit": P.mask_distance(m, to_set=True, limit=4),
           "dilate": P.mask_dilate(m, 2.9), "erode": P.mask_erode(m, 1), "open": P.mask_open(m, 1.5), "close": P.mask_close(m, 1.5),
           "drop": P.remove_small_components(m, 3), "fill": P.fill_holes(m)}
    for conn, phase in ((8, 1), (4, 0)):
        c = P.mask_components(m, connectivity=conn, phase=phase)
        out.update({f"{k}{conn}{phase}": getattr(c, k) for k in ("label", "area", "border", "count", "status")})
    r = P.MaskRefine(B, H, W, DEV, **RECIPES[0]).enqueue(torch.cuda.current_stream().cuda_stream, m)
    out.update(recipe=r.mask[:, 0], stats=r.stats)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("name", [n for n in SMALL if "1x1" not in n])
def test_a_sample_does_not_see_its_batch(name):
    """Every result of a sample in the batch of 3 is the result for that sample alone, and unchanged when the batch order is reversed;
    two runs give equal bytes."""
    m = dev(name)
    whole, again = everything(m), everything(m)
    flipped = everything(m.flip(0).contiguous())
    for k, v in whole.items():
        assert torch.equal(v, again[k]), k
        assert torch.equal(v, flipped[k].flip(0)), k
    for s in range(m.shape[0]):
        alone = everything(m[s:s + 1].contiguous())
        for k, v in whole.items():
            assert torch.equal(v[s:s + 1], alone[k]), (k, s)


def test_two_runs_of_the_large_case_give_equal_bytes():
    m = dev(BIG)
    a, b = everything(m), everything(m)
    for k, v in a.items():
        assert torch.equal(v, b[k]), k
    assert not bool(a["status81"].any()) and not bool(a["status40"].any())


@pytest.mark.parametrize("name", ["long_64x64", "speckled_64x64"])
def test_captured_equals_eager_over_three_replays(name):
    import phendiff_amd as P
    m = dev(name)
    B, H, W = m.shape
    eager = everything(m)
    src = torch.zeros_like(m)
    r = P.MaskRefine(B, H, W, DEV, **RECIPES[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # a warm-up outside the capture
        r.enqueue(side.cuda_stream, src)
        P.mask_distance(src, to_set=True)
        P.mask_components(src)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        r.enqueue(st, src)
        d2 = P.mask_distance(src, to_set=True)
        c = P.mask_components(src, connectivity=8, phase=1)
    other = dev("random_64x64")
    for replay in range(3):
        src.copy_(other if replay == 1 else m)      # the second replay runs on other contents: nothing is carried across
        r.mask.fill_(0xA5)
        r.stats.fill_(-7)
        d2.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        if replay == 1:
            assert same(r.mask[:, 0], reference("random_64x64", "refine", 0)[0]) and same(d2, reference("random_64x64", "d2", True))
            continue
        assert torch.equal(r.mask[:, 0].cpu(), eager["recipe"]) and torch.equal(r.stats.cpu(), eager["stats"]), replay
        assert torch.equal(d2.cpu(), eager["d2_set"]) and torch.equal(c.label.cpu(), eager["label81"]) and torch.equal(c.area.cpu(), eager["area81"]), replay
        assert torch.equal(c.count.cpu(), eager["count81"]) and not bool(c.status.any())
