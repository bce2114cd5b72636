"""The masked class transfer on MI355X: ``masked_ddib`` (eager), ``MaskedDDIBGraph`` (enqueued and captured) and ``class_contrast_mask``.
``super_small`` at 32 x 32 with seeded random weights, S = 4, B = 3, bf16, the scheduler config the DDIB tests use (a "trailing" grid),
and its thresholded form for one case.

With random weights a contrast map can sit anywhere relative to the threshold, so masks are NOT compared across precisions or against a
CPU oracle here: only bit-equalities between forms of the same launches are asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_unet_ddib import make_pair, synth_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, S, SIZE = 3, 4, 32


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.fixture(scope="module")
def world():
    """The pipelines (plain and thresholded, one UNet), two batches, and plain DDIB's results -- computed once, left unchanged."""
    import phendiff_amd as P
    _, unet = make_pair("super_small", SIZE, "bf16")
    cfg = P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
    w = type("World", (), {})()
    w.pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**cfg))
    w.pipe_th = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**cfg, thresholding=True, dynamic_thresholding_ratio=0.9, sample_max_value=1.5))
    x, labels = synth_batch(B, SIZE)
    w.x, w.labels, w.target = x.to(DEV), labels.to(DEV), (1 - labels).to(DEV)
    x2, l2 = synth_batch(B, SIZE, seed=99)
    w.x2, w.labels2, w.target2 = x2.to(DEV), (1 - l2).to(DEV), l2.to(DEV)
    w.ones = torch.ones((B, 1, SIZE, SIZE), dtype=torch.uint8, device=DEV)
    half = torch.zeros((B, SIZE, SIZE), dtype=torch.bool, device=DEV)      # a half plane, different per sample
    half[0, :, :SIZE // 2] = True
    half[1, :SIZE // 2, :] = True
    half[2, :, SIZE // 2 + 3:] = True
    w.half = half
    return w


def run_given(pipe, w, mask, x=None, labels=None, target=None, **kw):
    import phendiff_amd as P
    g = P.MaskedDDIBGraph(pipe, B, S, mask="given", **kw)
    g.run(w.x if x is None else x, w.labels if labels is None else labels, w.target if target is None else target, mask=mask)
    torch.cuda.synchronize()
    return g


def postproc_u8(x):
    import phendiff_amd._lib as L
    n, c, h, wd = x.shape
    f32 = torch.empty((n, h, wd, c), dtype=torch.float32, device=x.device)
    u8 = torch.empty((n, h, wd, c), dtype=torch.uint8, device=x.device)
    a = L.PostprocArgs(B=n, C=c, H=h, W=wd, x=x.data_ptr(), out_f32=f32.data_ptr(), out_u8=u8.data_ptr())
    L.check(L.lib().pd_postproc(C.byref(a), torch.cuda.current_stream().cuda_stream), "pd_postproc")
    torch.cuda.synchronize()
    return u8


def test_all_ones_mask_is_plain_ddib(world):
    import phendiff_amd as P
    w = world
    d = P.DDIBGraph(w.pipe, B, S).run(w.x, w.labels, w.target)
    torch.cuda.synchronize()
    g = run_given(w.pipe, w, w.ones)
    assert same_bits(g.images, d.images) and same_bits(g.images_u8, d.images_u8) and same_bits(g.inverted, d.inverted)
    assert g.mask.dtype == torch.uint8 and tuple(g.mask.shape) == (B, 1, SIZE, SIZE) and bool(g.mask.all())
    eager = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=w.ones)
    plain = P.ddib(w.pipe, w.x, w.labels, w.target, S)
    assert isinstance(eager.images, np.ndarray) and np.array_equal(eager.images, plain)
    assert same_bits(eager.inverted, d.inverted) and same_bits(eager.sample, g.sample)


def test_all_zeros_mask_returns_the_input(world):
    import phendiff_amd as P
    w = world
    zeros = torch.zeros_like(w.ones)
    g = run_given(w.pipe, w, zeros)
    assert same_bits(g.sample, w.x)
    assert same_bits(P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=zeros).sample, w.x)
    assert same_bits(g.images_u8, postproc_u8(w.x))


def test_half_plane_mask_keeps_the_rest(world):
    w = world
    g = run_given(w.pipe, w, w.half)
    inside = w.half[:, None].expand_as(w.x)
    assert torch.equal(g.mask, w.half[:, None].to(torch.uint8))
    assert same_bits(g.sample[~inside], w.x[~inside])                       # outside the mask: the input, bit for bit
    u8_in = postproc_u8(w.x)
    nhwc = w.half[:, :, :, None].expand_as(u8_in)
    assert torch.equal(g.images_u8[~nhwc], u8_in[~nhwc])                      # ... and its pd_postproc
    for b in range(B):                                                        # inside the mask the transfer happened
        changed = (g.sample[b] != w.x[b]) & inside[b]
        assert int(changed.sum()) > 0.5 * int(inside[b].sum()), b      # (not all: clipped pixels of the input may come back clipped)
    assert bool(torch.isfinite(g.sample).all())


def test_eager_enqueued_and_captured_give_the_same_bits(world):
    import phendiff_amd as P
    w = world
    captured = run_given(w.pipe, w, w.half)
    first = {k: getattr(captured, k).clone() for k in ("images", "images_u8", "inverted", "sample", "mask")}
    enqueued = run_given(w.pipe, w, w.half, use_graph=False)
    eager = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=w.half, output_type="pt")
    for k, v in first.items():
        assert same_bits(getattr(enqueued, k), v), k
    assert same_bits(eager.images, first["images"]) and same_bits(eager.inverted, first["inverted"]) and same_bits(eager.sample, first["sample"])
    assert torch.equal(eager.mask, first["mask"])
    captured.run(w.x, w.labels, w.target, mask=w.half)                       # a second replay
    torch.cuda.synchronize()
    for k, v in first.items():
        assert same_bits(getattr(captured, k), v), k
    captured.run(w.x2, w.labels2, w.target2, mask=w.ones)                     # other inputs, another mask ...
    torch.cuda.synchronize()
    assert not same_bits(captured.sample, first["sample"])
    captured.run(w.x, w.labels, w.target, mask=w.half[:, None].to(torch.uint8))      # ... then the first again: nothing is carried across
    torch.cuda.synchronize()
    for k, v in first.items():
        assert same_bits(getattr(captured, k), v), k


def hand_contrast(pipe, noise, x, labels, target, num_maps, encode_strength, ratio):
    """The mask phase as a hand loop: DeviceNoise.add_noise, pipe.unet and the three kernels' first two."""
    import phendiff_amd as P
    import phendiff_amd._lib as L
    lib = L.lib()
    t = P.encode_timestep(pipe.scheduler, S, encode_strength)
    n, c, h, wd = x.shape
    acc = torch.full((n, 1, h, wd), float("nan"), dtype=torch.float32, device=x.device)
    st = torch.cuda.current_stream().cuda_stream
    for k in range(num_maps):
        noised = noise.add_noise(pipe.scheduler, x, torch.full((n,), t, dtype=torch.long), elem_base=k * c * h * wd)
        eps_t = pipe.unet(noised, t, target).sample
        eps_s = pipe.unet(noised, t, labels).sample
        a = L.ClassContrastArgs(B=n, C=c, per_pixel=h * wd, a=eps_t.data_ptr(), b=eps_s.data_ptr(), acc=acc.data_ptr(), first=int(k == 0))
        L.check(lib.pd_class_contrast(C.byref(a), st), "pd_class_contrast")
    mask = torch.empty((n, 1, h, wd), dtype=torch.uint8, device=x.device)
    cmap = torch.empty((n, 1, h, wd), dtype=torch.float32, device=x.device)
    stats = torch.empty((n, 3), dtype=torch.float32, device=x.device)
    ws = torch.empty((lib.pd_contrast_mask_workspace(n, h * wd) // 8,), dtype=torch.float64, device=x.device)
    a = L.ContrastMaskArgs(B=n, per_pixel=h * wd, acc=acc.data_ptr(), ratio=ratio, mask=mask.data_ptr(), map=cmap.data_ptr(),
                           stats=stats.data_ptr(), workspace=ws.data_ptr())
    L.check(lib.pd_contrast_mask(C.byref(a), st), "pd_contrast_mask")
    torch.cuda.synchronize()
    return mask, cmap, stats, t


@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "enqueued"])
def test_contrast_mask_in_the_graph_is_the_hand_loop(world, use_graph):
    import phendiff_amd as P
    w = world
    seed, start = 4321, 5
    noise = P.DeviceNoise(seed, DEV, first_index=start)
    g = P.MaskedDDIBGraph(w.pipe, B, S, mask="contrast", noise=noise, num_maps=2, encode_strength=0.5, threshold_ratio=3.0, use_graph=use_graph)
    g.run(w.x, w.labels, w.target)
    torch.cuda.synchronize()
    assert noise.index == start + B and int(noise.state.cpu()[1]) == start + B      # the shadow and the device position
    mask, cmap, stats, t = hand_contrast(w.pipe, P.DeviceNoise(seed, DEV, first_index=start), w.x, w.labels, w.target, 2, 0.5, 3.0)
    assert g.t_enc == t
    assert same_bits(g.mask, mask) and same_bits(g.map, cmap) and same_bits(g.stats, stats)
    assert bool(torch.isfinite(g.map).all()) and float(g.map.min()) >= 0.0 and float(g.map.max()) <= 1.0
    assert torch.equal(g.mask, (g.map > 0.5).to(torch.uint8))
    # class_contrast_mask with a DeviceNoise at the same position: the same mask; it does not advance the position
    at = P.DeviceNoise(seed, DEV, first_index=start)
    m = P.class_contrast_mask(w.pipe, w.x, w.labels, w.target, S, num_maps=2, encode_strength=0.5, threshold_ratio=3.0, generator=at)
    torch.cuda.synchronize()
    assert at.index == start and m.timestep == t
    assert same_bits(m.mask, mask) and same_bits(m.map, cmap) and same_bits(m.stats, stats)
    assert tuple(m.mask.shape) == (B, 1, SIZE, SIZE) and m.mask.dtype == torch.uint8 and tuple(m.stats.shape) == (B, 3)
    # the transfer under that mask is the given-mask transfer
    given = run_given(w.pipe, w, mask, use_graph=use_graph)
    assert same_bits(g.sample, given.sample) and same_bits(g.images_u8, given.images_u8) and same_bits(g.inverted, given.inverted)
    # the next replay draws for the next B images: the mask of a DeviceNoise at start + B
    g.run(w.x, w.labels, w.target)
    torch.cuda.synchronize()
    assert noise.index == start + 2 * B
    nxt = P.class_contrast_mask(w.pipe, w.x, w.labels, w.target, S, num_maps=2, generator=P.DeviceNoise(seed, DEV, first_index=start + B))
    assert same_bits(g.mask, nxt.mask) and same_bits(g.map, nxt.map)
    assert not same_bits(g.map, cmap)


def test_eager_masked_ddib_computes_its_mask(world):
    import phendiff_amd as P
    w = world
    out = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, num_maps=2, generator=P.DeviceNoise(77, DEV), output_type="pt")
    m = P.class_contrast_mask(w.pipe, w.x, w.labels, w.target, S, num_maps=2, generator=P.DeviceNoise(77, DEV))
    assert same_bits(out.mask, m.mask) and same_bits(out.map, m.map)
    given = P.masked_ddib(w.pipe, w.x, w.labels, w.target, S, mask=m.mask, output_type="pt")
    assert same_bits(out.sample, given.sample) and same_bits(out.images, given.images)
    keep = (m.mask == 0).expand_as(w.x)
    assert same_bits(out.sample[keep], w.x[keep])
    g = torch.Generator().manual_seed(5)      # a torch.Generator draws with randn_tensor
    a = P.class_contrast_mask(w.pipe, w.x, w.labels, w.target, S, num_maps=2, generator=g)
    b = P.class_contrast_mask(w.pipe, w.x, w.labels, w.target, S, num_maps=2, generator=torch.Generator().manual_seed(5))
    assert same_bits(a.map, b.map)


class Recorder:
    """The loaded library with every entry point wrapped: the names of the calls, in order (scripts/trajectory_signature.py's mechanism)."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if not callable(real) or name in ("pd_last_error", "pd_abi_version"):
            return real

        def fn(*args):
            self.calls.append(name)
            return real(*args)
        return fn


def test_inversion_enqueues_ddib_graphs_launches(world, monkeypatch):
    """The inversion half of MaskedDDIBGraph enqueues no launch DDIBGraph's inversion does not (it keeps its states by writing each step
    into the next state, not by snapshots), and the generation half adds exactly one pd_mask_blend after every update."""
    import phendiff_amd as P
    import phendiff_amd._lib as L
    w = world
    rec = Recorder(L.lib())
    monkeypatch.setattr(L, "_lib", rec)
    plain = P.DDIBGraph(w.pipe, B, S, use_graph=False, private_plan=True)
    masked = P.MaskedDDIBGraph(w.pipe, B, S, mask="given", use_graph=False, private_plan=True)
    rec.calls = []
    plain.run(w.x, w.labels, w.target)
    ddib_calls, rec.calls = rec.calls, []
    masked.run(w.x, w.labels, w.target, mask=w.ones)
    masked_calls, rec.calls = rec.calls, []
    torch.cuda.synchronize()
    assert ddib_calls.count("pd_add_noise") == 1 and ddib_calls.count("pd_ddim_step") == 2 * S      # the snapshot between the halves
    cut = ddib_calls.index("pd_add_noise")
    inversion = ddib_calls[:cut]
    assert inversion.count("pd_ddim_step") == S and len(inversion) > 10 * S                         # (the UNet's launches were recorded)
    assert masked_calls[:cut] == inversion
    rest = masked_calls[cut:]
    assert "pd_add_noise" not in masked_calls
    assert [c for c in rest if c != "pd_mask_blend"] == ddib_calls[cut + 1:]
    assert rest.count("pd_mask_blend") == S
    assert all(rest[i - 1] == "pd_ddim_step" for i, c in enumerate(rest) if c == "pd_mask_blend")
    assert same_bits(masked.images, plain.images)


def test_thresholded_forward_scheduler(world):
    import phendiff_amd as P
    w = world
    assert w.pipe_th.scheduler.config.thresholding and w.pipe_th.scheduler.config.timestep_spacing == "trailing"
    d = P.DDIBGraph(w.pipe_th, B, S).run(w.x, w.labels, w.target)
    torch.cuda.synchronize()
    g = run_given(w.pipe_th, w, w.ones)
    assert same_bits(g.images, d.images) and same_bits(g.images_u8, d.images_u8) and same_bits(g.inverted, d.inverted)
    h = run_given(w.pipe_th, w, w.half)
    inside = w.half[:, None].expand_as(w.x)
    assert same_bits(h.sample[~inside], w.x[~inside])
    assert int(((h.sample != w.x) & inside).sum()) > 0.5 * int(inside.sum())
    eager = P.masked_ddib(w.pipe_th, w.x, w.labels, w.target, S, mask=w.half, output_type="pt")
    assert same_bits(eager.sample, h.sample) and same_bits(eager.images, h.images)
