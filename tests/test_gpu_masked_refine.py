"""``refine=`` in the masked class transfer on MI355X: ``class_contrast_mask``, ``masked_ddib`` and ``MaskedDDIBGraph`` with the mask
refinement of ``phendiff_amd.mask_ops`` between the mask and its use.  The smallest model and sizes of ``test_gpu_masked_ddib.py``
(``super_small`` at its SIZE, B and S, seeded random weights, bf16).

With random weights a contrast mask can be anything, all clear or all set included.  Every assertion about the contrast path is therefore a
bit-equality between two forms of the same launches, and the given-mask path -- a speckled mask of ``mask_ops_cases.speckled``, whose
refinement is checked on the CPU reference to keep at least one set and one clear pixel per sample -- carries the assertions about
what the refinement does to a transfer."""
import numpy as np
import pytest
import torch

import mask_ops_ref as R
from mask_ops_cases import speckled
from test_gpu_masked_ddib import B, S, SIZE, Recorder, same_bits
from test_gpu_unet_ddib import make_pair, synth_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REFINE = dict(close=1.5, open=1.5, fill_holes=-1, min_area=6, dilate=2)
MASK_ENTRY_POINTS = ("pd_mask_morph", "pd_mask_components", "pd_mask_filter", "pd_mask_distance")


@pytest.fixture(scope="module")
def world():
    """The pipeline, a batch, a speckled mask and its reference refinement -- computed once, left unchanged."""
    import phendiff_amd as P
    _, unet = make_pair("super_small", SIZE, "bf16")
    w = type("World", (), {})()
    w.pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
    x, labels = synth_batch(B, SIZE)
    w.x, w.labels, w.target = x.to(DEV), labels.to(DEV), (1 - labels).to(DEV)
    speck = speckled(np.random.default_rng(77), SIZE, SIZE).astype(np.uint8)
    assert speck.shape == (B, SIZE, SIZE)
    w.speck_ref, w.stats_ref = R.refine_ref(speck, **REFINE)
    # the refinement must leave something to transfer and something to keep in every sample -- and must have changed the mask
    for s in range(B):
        n = int(w.speck_ref[s].sum())
        assert 0 < n < SIZE * SIZE, f"sample {s}: the refined reference mask is degenerate ({n} of {SIZE * SIZE} pixels set)"
        assert not np.array_equal(w.speck_ref[s], speck[s])
    w.speck = torch.from_numpy(speck).to(DEV)
    return w


def test_given_mask_refined_eager(world):
    import phendiff_amd as P
    w = world
    out = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=w.speck, refine=REFINE, output_type="pt")
    assert np.array_equal(out.mask[:, 0].cpu().numpy(), w.speck_ref) and tuple(out.mask.shape) == (B, 1, SIZE, SIZE)
    assert np.array_equal(out.refine_stats.cpu().numpy(), w.stats_ref)
    assert torch.equal(out.raw_mask[:, 0], w.speck) and torch.equal(P.refine_mask(w.speck, **REFINE), out.mask[:, 0])
    by_hand = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=P.refine_mask(w.speck, **REFINE), output_type="pt")
    assert same_bits(out.sample, by_hand.sample) and same_bits(out.images, by_hand.images) and same_bits(out.inverted, by_hand.inverted)
    assert by_hand.raw_mask is None and by_hand.refine_stats is None
    keep = (out.mask == 0).expand_as(w.x)
    assert same_bits(out.sample[keep], w.x[keep])                                  # outside the refined mask: the input, bit for bit
    inside = ~keep
    assert int(((out.sample != w.x) & inside).sum()) > 0.5 * int(inside.sum())      # inside it the transfer happened
    unrefined = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=w.speck, refine=None, output_type="pt")
    assert unrefined.raw_mask is None and torch.equal(unrefined.mask[:, 0], w.speck) and not same_bits(unrefined.sample, out.sample)


@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "enqueued"])
def test_given_mask_refined_in_the_graph(world, use_graph):
    import phendiff_amd as P
    w = world
    eager = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=w.speck, refine=REFINE, output_type="pt")
    g = P.MaskedDDIBGraph(w.pipe, B, S, mask="given", refine=REFINE, use_graph=use_graph)
    for replay in range(2):
        g.run(w.x, w.labels, w.target, mask=w.speck if replay == 0 else (w.speck != 0)[:, None])
        torch.cuda.synchronize()
        assert torch.equal(g.mask, eager.mask) and torch.equal(g.raw_mask[:, 0], w.speck) and torch.equal(g.refine_stats, eager.refine_stats)
        assert same_bits(g.sample, eager.sample) and same_bits(g.images, eager.images) and same_bits(g.inverted, eager.inverted)
    plain = P.MaskedDDIBGraph(w.pipe, B, S, mask="given", use_graph=use_graph)      # refine=None: the unrefined call's bits
    plain.run(w.x, w.labels, w.target, mask=w.speck)
    torch.cuda.synchronize()
    unrefined = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=w.speck, output_type="pt")
    assert plain.raw_mask is None and plain.refine_stats is None and plain.refine is None
    assert torch.equal(plain.mask[:, 0], w.speck) and same_bits(plain.sample, unrefined.sample) and not same_bits(plain.sample, g.sample)


def test_contrast_mask_refined(world):
    import phendiff_amd as P
    w = world
    seed, start = 4321, 5
    kw = dict(num_maps=2, encode_strength=0.5, threshold_ratio=3.0)
    raw = P.class_contrast_mask(w.pipe, w.x, w.labels, w.target, S, generator=P.DeviceNoise(seed, DEV, first_index=start), **kw)
    assert raw.raw_mask is None and raw.refine_stats is None
    m = P.class_contrast_mask(w.pipe, w.x, w.labels, w.target, S, generator=P.DeviceNoise(seed, DEV, first_index=start), refine=REFINE, **kw)
    assert same_bits(m.raw_mask, raw.mask) and same_bits(m.map, raw.map) and same_bits(m.stats, raw.stats)
    assert torch.equal(m.mask, P.refine_mask(raw.mask, **REFINE))
    want, stats = R.refine_ref(raw.mask[:, 0].cpu().numpy(), **REFINE)
    assert np.array_equal(m.mask[:, 0].cpu().numpy(), want) and np.array_equal(m.refine_stats.cpu().numpy(), stats)
    degenerate = [s for s in range(B) if int(want[s].sum()) in (0, SIZE * SIZE)]
    print(f"refined contrast mask: {[int(want[s].sum()) for s in range(B)]} of {SIZE * SIZE} pixels set; degenerate samples: {degenerate}")
    # the eager transfer: masked_ddib(refine=...) is masked_ddib(mask=refine_mask(raw))
    out = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, refine=REFINE, generator=P.DeviceNoise(seed, DEV, first_index=start),
                        output_type="pt", **kw)
    assert torch.equal(out.mask, m.mask) and same_bits(out.raw_mask, raw.mask) and torch.equal(out.refine_stats, m.refine_stats)
    by_hand = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=P.refine_mask(raw.mask, **REFINE), output_type="pt")
    assert same_bits(out.sample, by_hand.sample) and same_bits(out.images, by_hand.images)
    keep = (out.mask == 0).expand_as(w.x)
    assert same_bits(out.sample[keep], w.x[keep])
    # the captured transfer gives the eager function's bits
    for use_graph in (True, False):
        noise = P.DeviceNoise(seed, DEV, first_index=start)
        g = P.MaskedDDIBGraph(w.pipe, B, S, mask="contrast", noise=noise, refine=REFINE, use_graph=use_graph, **kw)
        g.run(w.x, w.labels, w.target)
        torch.cuda.synchronize()
        assert noise.index == start + B
        assert torch.equal(g.mask, out.mask) and same_bits(g.raw_mask, raw.mask) and torch.equal(g.refine_stats, out.refine_stats), use_graph
        assert same_bits(g.map, raw.map) and same_bits(g.stats, raw.stats)
        assert same_bits(g.sample, out.sample) and same_bits(g.images, out.images) and same_bits(g.inverted, out.inverted), use_graph
    # refine=None: the unrefined graph's bits, and .raw_mask is None
    plain = P.MaskedDDIBGraph(w.pipe, B, S, mask="contrast", noise=P.DeviceNoise(seed, DEV, first_index=start), refine=None, **kw)
    plain.run(w.x, w.labels, w.target)
    torch.cuda.synchronize()
    unrefined = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=raw.mask, output_type="pt")
    assert plain.raw_mask is None and same_bits(plain.mask, raw.mask) and same_bits(plain.sample, unrefined.sample)


def test_refine_none_adds_no_launch(world, monkeypatch):
    """Without refine the sequence of entry-point calls holds none of the refinement's; with it, exactly MaskRefine.plan's, in the mask
    phase -- before the first inversion step."""
    import phendiff_amd as P
    import phendiff_amd._lib as L
    w = world
    rec = Recorder(L.lib())
    monkeypatch.setattr(L, "_lib", rec)
    plain = P.MaskedDDIBGraph(w.pipe, B, S, mask="given", use_graph=False, private_plan=True)
    refined = P.MaskedDDIBGraph(w.pipe, B, S, mask="given", refine=REFINE, use_graph=False, private_plan=True)
    rec.calls = []
    plain.run(w.x, w.labels, w.target, mask=w.speck)
    plain_calls, rec.calls = rec.calls, []
    refined.run(w.x, w.labels, w.target, mask=w.speck)
    refined_calls, rec.calls = rec.calls, []
    torch.cuda.synchronize()
    assert not [c for c in plain_calls if c in MASK_ENTRY_POINTS]
    added = [c for c in refined_calls if c in MASK_ENTRY_POINTS]
    assert added == [fn for _, fn, _ in P.MaskRefine.plan(**REFINE)]
    assert [c for c in refined_calls if c not in MASK_ENTRY_POINTS] == plain_calls
    first, last = refined_calls.index(added[0]), len(refined_calls) - 1 - refined_calls[::-1].index(added[-1])
    assert refined_calls[first:last + 1] == added and "pd_ddim_step" not in refined_calls[:first]
    rec.calls = []
    P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=w.speck, output_type="pt")
    assert not [c for c in rec.calls if c in MASK_ENTRY_POINTS]
