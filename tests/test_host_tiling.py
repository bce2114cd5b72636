"""Tiled trajectories without a GPU: the grid and its weights (known answers, coverage, partition of unity, TileGrid against the
restatement in tests/tiled_refs.py, the refusals), the reference's self-check (with a zero-output and a pointwise model the tiled
reference trajectory is the untiled oracle trajectory, so the reference -- not the kernel -- defines the blend), the C ABI of the two entry
points (struct layout, exports, every refusal before a launch) and what the tiled trajectories refuse before they pack anything."""
import ctypes as C

import numpy as np
import pytest
import torch

import tiled_refs as T
from abi_header import header_fields

AXES = tuple(k for k, _ in T.KNOWN_ORIGINS) + ((1024, 256, 32), (1080, 256, 32), (2048, 256, 64), (100, 7, 6), (50, 32, 31))


def test_grid_known_origins():
    from phendiff_amd.tiling import axis_origins
    for (L, t, ov), want in T.KNOWN_ORIGINS:
        assert tuple(T.origins_1d(L, t, ov)) == want == axis_origins(L, t, ov), (L, t, ov)
    assert T.coverage_1d(72, 32, 16)[40:48].tolist() == [3] * 8 and T.coverage_1d(72, 32, 16).max() == 3      # more than two tiles on a row
    assert len(T.origins_1d(1024, 256, 32)) == 5


def test_every_pixel_is_covered_and_weights_sum_to_one():
    for L, t, ov in AXES:
        cover, orig, w = T.coverage_1d(L, t, ov), T.origins_1d(L, t, ov), T.weights_1d(L, t, ov)
        assert cover.min() >= 1, (L, t, ov)
        assert orig[0] == 0 and orig[-1] == L - t and all(b > a for a, b in zip(orig, orig[1:]))
        total = np.zeros(L)
        for k, o in enumerate(orig):
            total[o:o + t] += w[k]
        assert np.abs(total - 1.0).max() <= 4 * np.finfo(np.float64).eps, (L, t, ov)
        assert (w > 0).all()
        # a position covered once has weight exactly 1.0f there
        w32 = w.astype(np.float32)
        for k, o in enumerate(orig):
            once = cover[o:o + t] == 1
            assert (w32[k][once] == np.float32(1.0)).all()
            assert (w32[k][~once] < np.float32(1.0)).all()


def test_tilegrid_agrees_with_the_reference_tables():
    import phendiff_amd as P
    from phendiff_amd.tiling import axis_weights
    for L, t, ov in AXES:
        assert np.array_equal(axis_weights(L, t, ov), T.weights_1d(L, t, ov)), (L, t, ov)
    for B, Cc, H, W, tile, ov in T.KERNEL_CASES + ((1, 3, 1080, 1080, 256, 32), (1, 3, 96, 200, (32, 64), (8, 16))):
        g, r = P.TileGrid(H, W, tile, ov), T.GridRef(H, W, tile, ov)
        assert list(g.origins_y) == r.oy and list(g.origins_x) == r.ox and g.tiles_per_image == r.per_image
        assert (g.th, g.tw, g.sy, g.sx) == (r.th, r.tw, r.th - r.ovy, r.tw - r.ovx) and (g.nty, g.ntx) == (len(r.oy), len(r.ox))
        assert g.weights_y.dtype == torch.float32 and torch.equal(g.weights_y, r.wy) and torch.equal(g.weights_x, r.wx)
        assert g.origins() == [(y0, x0) for _, _, _, y0, x0 in r.tiles(1)]
    # the 2-D weights of a position sum to one (fp32 tables, summed in float64: within the rounding of the tables)
    r = T.GridRef(72, 88, 32, 8)
    total = torch.zeros(72, 88, dtype=torch.float64)
    for _, ky, kx, y0, x0 in r.tiles(1):
        total[y0:y0 + 32, x0:x0 + 32] += r.wy[ky].double()[:, None] * r.wx[kx].double()[None, :]
    assert float((total - 1).abs().max()) < 4 * 2.0 ** -24


def test_tilegrid_refusals():
    import phendiff_amd as P
    for H, W, tile, ov in ((72, 88, 32, -1), (72, 88, 32, 32), (72, 88, 32, 40), (31, 88, 32, 8), (72, 31, 32, 8), (72, 88, (32, 96), 8),
                           (72, 88, 32, (8, 32)), (72, 88, 32, (-2, 0))):
        with pytest.raises(ValueError):
            P.TileGrid(H, W, tile, ov)
    with pytest.raises(ValueError):
        P.TileGrid(72, 88, (32, 32, 32), 8)
    g = P.TileGrid(32, 32, 32, 31)                     # L == t: one tile whatever the overlap
    assert (g.nty, g.ntx) == (1, 1) and bool((g.weights_y == 1).all())


# ---------------------------------------------------------------------------------------------------------------- reference self-check
def _schedulers():
    import phendiff_amd as P
    from oracle import DDIMSchedulerRef
    return DDIMSchedulerRef(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])


@pytest.mark.parametrize("model", ["zero", "pointwise"])
def test_reference_tiled_trajectory_equals_the_untiled_one_for_pointwise_models(model):
    """model_out = a(t, class) * x commutes with cutting tiles out, and the blend of equal values is that value up to the rounding of a
    convex combination: per step at most (n + 1) u |m| for n covering tiles (weight product, term, n - 1 additions, the fp32 weights' own
    1 u each); over 2 S steps of a trajectory whose per-step amplification is about 1 the bound below is generous and fixed in advance."""
    a = 0.0 if model == "zero" else 0.37

    def unet(x, t, labels):
        return (a * (1.0 + 0.5 * labels.float()).view(-1, 1, 1, 1) * (1.0 + float(t) / 3000.0)) * x
    x, labels = T.canvas_batch(2, 3, 72, 88)
    g = T.GridRef(72, 88, 32, 8)
    got_img, got_inv = T.tiled_ddib_ref(unet, _schedulers(), x, labels, 1 - labels, 3, g)
    want_img, want_inv = T.untiled_ddib_ref(unet, _schedulers(), x, labels, 1 - labels, 3)
    u = 2.0 ** -24
    bound = 6 * (9 + 1) * u * 8                          # 6 steps, up to 9 covering tiles, values below 8
    assert float((got_inv - want_inv).abs().max()) <= bound and float(np.abs(got_img - want_img).max()) <= bound
    if model == "zero":                                  # every term is +-0: exactly the untiled trajectory
        assert torch.equal(got_inv, want_inv) and np.array_equal(got_img, want_img)
    assert float(want_inv.abs().max()) < 8


def test_reference_gather_and_blend_invert_each_other_on_one_tile():
    x, _ = T.canvas_batch(3, 32, 32, 32)
    g = T.GridRef(32, 32, 32, 0)
    tiles = T.gather_ref(x, g)
    assert torch.equal(tiles, x) and torch.equal(T.blend_ref(tiles, g, 3), x)
    x2, _ = T.canvas_batch(2, 3, 72, 88)
    g2 = T.GridRef(72, 88, 32, 8)
    assert T.gather_ref(x2, g2, 5, 7).shape == (7, 3, 32, 32) and torch.equal(T.gather_ref(x2, g2, 5, 7), T.gather_ref(x2, g2)[5:12])


# ---------------------------------------------------------------------------------------------------------------- ABI
GRID_FIELDS = ["B", "C", "Hc", "Wc", "th", "tw", "nty", "ntx", "sy", "sx"]
GATHER_FIELDS = GRID_FIELDS + ["first", "count", "canvas", "tiles"]
BLEND_FIELDS = GRID_FIELDS + ["tiles", "wy", "wx", "out"]


def test_structs_and_exports():
    import phendiff_amd._lib as L
    assert header_fields("pd_tile_gather_args") == GATHER_FIELDS == [f[0] for f in L.TileGatherArgs._fields_]
    assert header_fields("pd_tile_blend_args") == BLEND_FIELDS == [f[0] for f in L.TileBlendArgs._fields_]
    lib = L.lib()
    for name in ("pd_tile_gather", "pd_tile_blend"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == 8


def test_args_builders_describe_the_grid():
    """Host tensors stand in for device ones (nothing is launched)."""
    import phendiff_amd as P
    g = P.TileGrid(72, 88, 32, 8)
    canvas, tiles = torch.zeros(2, 3, 72, 88), torch.zeros(24, 3, 32, 32)
    a = g.gather_args(canvas, tiles, 5, 7)
    want = dict(B=2, C=3, Hc=72, Wc=88, th=32, tw=32, nty=3, ntx=4, sy=24, sx=24)
    assert {k: getattr(a, k) for k in want} == want and (a.first, a.count, a.canvas, a.tiles) == (5, 7, canvas.data_ptr(), tiles.data_ptr())
    assert g.gather_args(canvas, tiles).count == 24
    b = g.blend_args(tiles, canvas)
    wy, wx = g.device_weights("cpu")
    assert {k: getattr(b, k) for k in want} == want and (b.tiles, b.wy, b.wx, b.out) == (tiles.data_ptr(), wy.data_ptr(), wx.data_ptr(), canvas.data_ptr())
    assert g.device_weights("cpu")[0] is wy                                  # (made once per device)


def _aligned():
    buf = (C.c_char * 8192)()
    return buf, (C.addressof(buf) + 255) // 256 * 256


GRID_OK = dict(B=2, C=3, Hc=72, Wc=88, th=32, tw=32, nty=3, ntx=4, sy=24, sx=24)
GRID_REFUSALS = [(dict(B=0), b"canvas"), (dict(C=0), b"canvas"), (dict(Hc=0), b"canvas"), (dict(Wc=-1), b"canvas"), (dict(th=0), b"tile 0 x 32"),
                 (dict(tw=0), b"tile 32 x 0"), (dict(th=80, sy=24), b"larger than the canvas"), (dict(tw=96), b"larger than the canvas"),
                 (dict(sy=0), b"stride"), (dict(sx=33), b"stride"), (dict(sy=-3), b"stride"), (dict(nty=2), b"tile counts"),
                 (dict(ntx=5), b"tile counts"), (dict(nty=0), b"tile counts"),
                 (dict(B=1 << 20, C=64), b"overflows 32-bit offsets")]


def test_tile_gather_validates_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf, p = _aligned()
    ok = dict(GRID_OK, first=0, count=24, canvas=p, tiles=p)
    cases = GRID_REFUSALS + [(dict(canvas=None), b"null pointer"), (dict(tiles=None), b"null pointer"), (dict(first=-1), b"first"),
                             (dict(count=0), b"count"), (dict(first=20, count=5), b"first + count"), (dict(first=24, count=1), b"first + count"),
                             (dict(canvas=p + 2), b"4-byte aligned"), (dict(tiles=p + 1), b"4-byte aligned"),
                             # the canvas fits 32-bit offsets, the tile batch (4x overlap: 25 tiles a canvas) does not
                             (dict(B=450, C=4, Hc=1024, Wc=1024, th=256, tw=256, sy=192, sx=192, nty=5, ntx=5, count=11250), b"a tile batch")]
    for change, word in cases:
        rc = lib.pd_tile_gather(C.byref(L.TileGatherArgs(**dict(ok, **change))), None)
        assert rc < 0, change
        assert word in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_tile_gather:"), (change, lib.pd_last_error())
    assert lib.pd_tile_gather(None, None) < 0 and b"null args" in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_tile_gather:")


def test_tile_blend_validates_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf, p = _aligned()
    ok = dict(GRID_OK, tiles=p, wy=p, wx=p, out=p)
    cases = GRID_REFUSALS + [(dict(tiles=None), b"null pointer"), (dict(wy=None), b"null pointer"), (dict(wx=None), b"null pointer"),
                             (dict(out=None), b"null pointer"), (dict(tiles=p + 2), b"4-byte aligned"), (dict(wy=p + 1), b"4-byte aligned"),
                             (dict(wx=p + 3), b"4-byte aligned"), (dict(out=p + 2), b"4-byte aligned"),
                             (dict(B=450, C=4, Hc=1024, Wc=1024, th=256, tw=256, sy=192, sx=192, nty=5, ntx=5), b"a tile batch")]
    for change, word in cases:
        rc = lib.pd_tile_blend(C.byref(L.TileBlendArgs(**dict(ok, **change))), None)
        assert rc < 0, change
        assert word in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_tile_blend:"), (change, lib.pd_last_error())
    assert lib.pd_tile_blend(None, None) < 0 and b"null args" in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_tile_blend:")


# ---------------------------------------------------------------------------------------------------------------- what is refused early
def _meta_pipe(scheduler=None, **unet_kw):
    import phendiff_amd as P
    with torch.device("meta"):
        unet = P.CustomCondUNet2DModel(**dict(P.UNET_CONFIGS["super_small"], sample_size=32, **unet_kw))
    return P.ConditionalDDIMPipeline(unet, scheduler or P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))


def test_tiled_trajectories_refuse_before_anything_is_packed():
    """Meta-device models: whatever is raised comes before a weight is packed or a plan built."""
    import os
    import sys
    import phendiff_amd as P
    pipe = _meta_pipe()
    x, labels = torch.zeros(2, 3, 72, 88), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="overlap"):
        P.tiled_ddib(pipe, x, labels, 1 - labels, 3, 32, overlap=32)
    with pytest.raises(ValueError, match="exceeds the canvas"):
        P.tiled_inversion(pipe, x, labels, 3, 96)
    with pytest.raises(ValueError, match="5-channel images"):
        P.tiled_ddib(pipe, torch.zeros(2, 5, 72, 88), labels, 1 - labels, 3, 32)
    with pytest.raises(ValueError, match="output_type"):
        P.tiled_ddib(pipe, x, labels, 1 - labels, 3, 32, output_type="pil")
    with pytest.raises(P.PhenDiffHipError, match="no CPU fallback"):
        P.tiled_ddib(pipe, x, labels, 1 - labels, 3, 32)
    with pytest.raises(ValueError, match="overlap"):
        P.TiledDDIBGraph(pipe, 2, 3, 72, 88, 32, overlap=40)
    with pytest.raises(NotImplementedError):
        P.tiled_ddib(object(), x, labels, 1 - labels, 3, 32)
    # a thresholding scheduler takes its quantile over the whole canvas: 3 x 2400 x 2400 is past torch.quantile's 16 000 000 elements
    th = _meta_pipe(P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"], thresholding=True, sample_max_value=2.0))
    big = torch.zeros(1, 3, 2400, 2400, device="meta")
    with pytest.raises(ValueError, match="16 000 000"):
        P.tiled_ddib(th, big, labels[:1], labels[:1], 3, 32)
    with pytest.raises(ValueError, match="16 000 000"):
        P.TiledDDIBGraph(th, 1, 3, 2400, 2400, 32)
    for p in (pipe, th):
        assert not p.unet._plans and p.unet._weights is None
    # the latent tier is not tiled
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import SD_SCHED, SD_TINY_UNET, SD_TINY_VAE
    with torch.device("meta"):
        unet, vae = P.SDUNet2DConditionModel(**SD_TINY_UNET), P.AutoencoderKL(**SD_TINY_VAE)
        emb = P.CustomEmbedding(2, SD_TINY_UNET["cross_attention_dim"])
    sd = P.CustomStableDiffusionImg2ImgPipeline(vae, unet, P.DDIMScheduler(**SD_SCHED), emb)
    for call in (lambda: P.tiled_ddib(sd, x, labels, 1 - labels, 3, 32), lambda: P.tiled_inversion(sd, x, labels, 3, 32),
                 lambda: P.tiled_inverted_regeneration(sd, x, labels, 3, 32), lambda: P.TiledDDIBGraph(sd, 2, 3, 72, 88, 32)):
        with pytest.raises(NotImplementedError, match="latent tier"):
            call()
    assert not unet._plans
