"""SSIM without a GPU: the reference (tests/ssim_ref.py) against closed forms that need no second implementation, ``gaussian_window`` against
the reference's own taps, the C ABI of ``pd_ssim`` / ``pd_ssim_workspace`` (struct, exports, every refusal before a launch) and the host
argument checks of ``sample_ssim``."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssim_ref as R
from abi_header import header_fields

C1, C2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2      # data_range 2.0


def smooth_pair(B, Cc, H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 3, H), np.linspace(0, 4, W), indexing="ij")
    base = 0.6 * np.sin(2.1 * xx + 0.3) * np.cos(1.7 * yy) + 0.1
    x = base + 0.05 * rng.standard_normal((B, Cc, H, W))
    y = base + 0.15 * rng.standard_normal((B, Cc, H, W))
    return torch.from_numpy(x), torch.from_numpy(y)


# ---------------------------------------------------------------------------------------------------------------- the reference is right
def test_identical_images_score_one():
    x, _ = smooth_pair(2, 3, 40, 45)
    m = R.maps_means(x, x, levels=2)
    assert m.shape == (2, 3, 2, 2)
    assert np.abs(m - 1.0).max() <= 1e-12
    s = R.scores(m)
    assert np.abs(s["ssim"] - 1.0).max() <= 1e-12 and np.abs(s["ms_ssim"] - 1.0).max() <= 1e-12


@pytest.mark.parametrize("a,b", [(0.5, 0.5), (0.9, -0.3), (0.0, 0.7), (-1.0, 1.0)])
def test_constant_images(a, b):
    x = torch.full((1, 2, 20, 23), a, dtype=torch.float64)
    y = torch.full((1, 2, 20, 23), b, dtype=torch.float64)
    m = R.maps_means(x, y)
    assert np.abs(m[..., 1] - 1.0).max() <= 1e-12                                   # no variance, no covariance: cs = C2 / C2
    assert np.abs(m[..., 0] - (2 * a * b + C1) / (a * a + b * b + C1)).max() <= 1e-12


def test_negated_checkerboard():
    """x = a +-1 checkerboard, y = -x.  Every window sees the same picture up to a sign: its mean is mu = +-(sum_i g_i (-1)^i)^2 (1.9e-8 for
    the default taps), its variance v = 1 - mu^2, and vxy = -v exactly, so cs = (C2 - 2 v) / (2 v + C2) at every position -- the analytic
    value with v = 1, up to mu^2 = 3.7e-16."""
    i, j = np.meshgrid(np.arange(30), np.arange(37), indexing="ij")
    x = torch.from_numpy(((-1.0) ** (i + j))[None, None])
    _, cs = R.ssim_cs_maps(x, -x)
    want = (C2 - 2.0) / (2.0 + C2)
    assert want < -0.99
    assert (cs - want).abs().max() <= 1e-12
    m = R.maps_means(x, -x)
    assert abs(m[0, 0, 0, 1] - want) <= 1e-12
    assert R.scores(np.repeat(m, 2, axis=2))["ms_ssim"][0] == 0.0              # the clamp: a negative cs contributes 0, not a NaN


def test_symmetry():
    x, y = smooth_pair(2, 2, 33, 40, seed=3)
    a, b = R.maps_means(x, y, levels=2), R.maps_means(y, x, levels=2)
    assert np.abs(a - b).max() <= 1e-14
    assert 0.0 < a[..., 0].min() < a[..., 0].max() < 1.0


def test_shared_y_and_pyramid():
    x, y = smooth_pair(3, 2, 45, 51, seed=4)
    m = R.maps_means(x, y[1], levels=3)
    for b in range(3):
        assert np.array_equal(m[b], R.maps_means(x[b:b + 1], y[1:2], levels=3)[0])
    # scale 1 is scale 0 of the 2x2 means, an odd trailing row / column dropped
    h = x[:, :, :44, :50].reshape(3, 2, 22, 2, 25, 2).mean(dim=(3, 5))
    hy = y[1:2, :, :44, :50].reshape(1, 2, 22, 2, 25, 2).mean(dim=(3, 5)).expand(3, -1, -1, -1)
    assert np.abs(R.maps_means(h, hy)[:, :, 0] - m[:, :, 1]).max() <= 1e-13
    w = R.weights_of(3)
    assert abs(w.sum() - 1.0) <= 1e-15 and np.allclose(w, np.array(R.WEIGHTS[:3]) / sum(R.WEIGHTS[:3]))
    assert np.array_equal(R.weights_of(5), np.array(R.WEIGHTS))


def test_against_skimage_if_present():
    metrics = pytest.importorskip("skimage.metrics")
    x, y = smooth_pair(1, 1, 40, 45, seed=5)
    got = R.maps_means(x, y)[0, 0, 0, 0]
    _, full = metrics.structural_similarity(x[0, 0].numpy(), y[0, 0].numpy(), data_range=2.0, gaussian_weights=True, sigma=1.5,
                                            use_sample_covariance=False, full=True)
    assert abs(got - full[5:-5, 5:-5].mean()) <= 1e-9      # (skimage pads; its interior is the valid map)


def test_against_pytorch_msssim_if_present():
    pm = pytest.importorskip("pytorch_msssim")
    x, y = smooth_pair(2, 3, 180, 190, seed=6)
    s = R.scores(R.maps_means(x, y, levels=5))
    assert np.abs(s["ssim"] - pm.ssim(x, y, data_range=2.0, size_average=False).numpy()).max() <= 1e-9
    assert np.abs(s["ms_ssim"] - pm.ms_ssim(x, y, data_range=2.0, size_average=False).numpy()).max() <= 1e-9


# ---------------------------------------------------------------------------------------------------------------- gaussian_window
@pytest.mark.parametrize("win,sigma", [(11, 1.5), (3, 0.5), (33, 5.0)])
def test_gaussian_window_equals_the_reference_taps(win, sigma):
    from phendiff_amd import gaussian_window
    g = gaussian_window(win, sigma)
    assert g.dtype == np.float64 and g.shape == (win,)
    assert np.array_equal(g, R.window(win, sigma))
    assert abs(g.sum() - 1.0) <= 2.0 ** -52
    assert np.array_equal(g, g[::-1]) and g.argmax() == win // 2


def test_gaussian_window_refuses():
    from phendiff_amd import gaussian_window
    for win in (10, 1, 35, 0):
        with pytest.raises(ValueError):
            gaussian_window(win, 1.5)
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gaussian_window(11, sigma)


# ---------------------------------------------------------------------------------------------------------------- C ABI
FIELDS = (["dtype", "C", "H", "W", "win", "levels", "B", "y_sample_stride"] + [f"w{i}" for i in range(33)]
          + ["c1", "c2", "x", "y", "out", "workspace", "workspace_bytes"])


def test_ssim_struct_and_export():
    import phendiff_amd._lib as L
    assert header_fields("pd_ssim_args") == FIELDS == [f[0] for f in L.SsimArgs._fields_]
    assert all(t is C.c_double for n, t in L.SsimArgs._fields_ if n[0] == "w" and n[1:].isdigit())
    # the taps are one run of doubles, as the library reads them
    assert L.SsimArgs.w32.offset - L.SsimArgs.w0.offset == 32 * 8
    assert L.CONSTANTS["PD_SSIM_MAX_WIN"] == 33 and L.CONSTANTS["PD_SSIM_MAX_LEVELS"] == 5
    lib = L.lib()
    for name in ("pd_ssim", "pd_ssim_workspace"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert L.SYMBOLS["pd_ssim_workspace"] == (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int])
    assert lib.pd_abi_version() == L.ABI_VERSION == 8


def ok_args(L, **change):
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    base = dict(dtype=1, C=3, H=45, W=67, win=11, levels=2, B=2, y_sample_stride=3 * 45 * 67, c1=C1, c2=C2, x=p, y=p, out=p, workspace=p,
                workspace_bytes=1 << 40)
    base.update({f"w{i}": g for i, g in enumerate(R.window(11, 1.5))})
    base.update(change)
    a = L.SsimArgs(**base)
    a._keep = buf
    return a


def test_ssim_validates_without_gpu():
    """Every refusal comes before any launch: no device is needed, and the pointers are never dereferenced."""
    import phendiff_amd._lib as L
    lib = L.lib()
    ERR_ARG, ERR_SHAPE = L.CONSTANTS["PD_ERR_ARG"], L.PD_ERR_SHAPE
    nan, inf = float("nan"), float("inf")
    cases = [({name: None}, ERR_ARG, b"null") for name in ("x", "y", "out", "workspace")]
    cases += [(dict(dtype=d), ERR_ARG, b"dtype") for d in (3, -1, 7)]
    cases += [(dict(workspace_bytes=lib.pd_ssim_workspace(2, 3, 45, 67, 2) - 1), ERR_ARG, b"workspace_bytes"), (dict(workspace_bytes=0), ERR_ARG, b"workspace_bytes")]
    cases += [({k: v}, ERR_ARG, k.encode()) for k in ("c1", "c2") for v in (0.0, -1.0, nan, inf)]
    cases += [({f"w{i}": v}, ERR_ARG, b"window") for i in (0, 5, 10) for v in (nan, inf)]
    cases += [({k: v}, ERR_SHAPE, b"shape") for k in ("B", "C", "H", "W") for v in (0, -3)]
    cases += [(dict(win=w), ERR_SHAPE, b"window") for w in (10, 1, 35, 2, 0, -11)]
    cases += [(dict(levels=v), ERR_SHAPE, b"levels") for v in (0, 6, -1)]
    cases += [(dict(levels=4), ERR_SHAPE, b"window"), (dict(H=21), ERR_SHAPE, b"shape"), (dict(W=20, levels=1, win=21), ERR_SHAPE, b"levels")]
    cases += [(dict(y_sample_stride=v), ERR_SHAPE, b"stride") for v in (1, 3 * 45 * 67 - 1, 45 * 67, -1)]
    cases += [(dict(B=1 << 40), ERR_SHAPE, b"shape"), (dict(B=1 << 31, H=11, W=11, levels=1, y_sample_stride=0), ERR_SHAPE, b"index range")]
    for change, code, word in cases:
        rc = lib.pd_ssim(C.byref(ok_args(L, **change)), None)
        assert rc == code, (change, rc, lib.pd_last_error())
        assert word in lib.pd_last_error(), (change, lib.pd_last_error())
    # a tap past win is not looked at
    a = ok_args(L, w11=nan, workspace_bytes=0)
    assert lib.pd_ssim(C.byref(a), None) == ERR_ARG and b"workspace_bytes" in lib.pd_last_error()
    assert lib.pd_ssim(None, None) < 0 and b"null args" in lib.pd_last_error()


def test_ssim_workspace_query():
    import phendiff_amd._lib as L
    lib = L.lib()
    for args in ((0, 3, 45, 67, 1), (2, 0, 45, 67, 1), (2, 3, 0, 67, 1), (2, 3, 45, -1, 1), (2, 3, 45, 67, 0), (2, 3, 45, 67, 6),
                 (2, 3, 45, 5, 2), (2, 3, 2, 67, 1), (1 << 40, 3, 45, 67, 1), (1 << 31, 1, 3, 3, 1)):
        assert lib.pd_ssim_workspace(*args) == 0, args
    sizes = {}
    for args in ((1, 1, 3, 3, 1), (2, 3, 11, 11, 1), (2, 3, 45, 67, 1), (2, 3, 45, 67, 3), (1, 2, 176, 176, 5), (1, 5, 2048, 2048, 5)):
        n = lib.pd_ssim_workspace(*args)
        assert n > 0 and n % 8 == 0, args
        sizes[args] = n
    assert sizes[(1, 1, 3, 3, 1)] == 16                                   # one tile's pair
    assert sizes[(2, 3, 45, 67, 3)] > sizes[(2, 3, 45, 67, 1)]           # the pyramid and the other scales' partials
    # the pyramid of both images in fp64: levels 1 .. 4 of 5 x 2048 x 2048
    pyramid = 2 * 8 * 5 * sum((2048 >> s) ** 2 for s in range(1, 5))
    assert pyramid < sizes[(1, 5, 2048, 2048, 5)] < pyramid * 1.02


# ---------------------------------------------------------------------------------------------------------------- host argument checks
def test_public_names_and_argument_checks():
    import phendiff_amd as P
    from phendiff_amd import diagnostics as D
    assert P.sample_ssim is D.sample_ssim and P.ssim_maps_means is D.ssim_maps_means and P.gaussian_window is D.gaussian_window
    x = torch.zeros(2, 3, 40, 40)
    with pytest.raises(P.PhenDiffHipError):
        P.sample_ssim(x, x)                                              # a CPU tensor: no fallback
    with pytest.raises(P.PhenDiffHipError):
        P.ssim_maps_means(x, x[0].contiguous())
    with pytest.raises(ValueError, match="B, C, H, W"):
        P.sample_ssim(x[0], x[0])                                        # rank
    with pytest.raises(ValueError, match="B, C, H, W"):
        P.sample_ssim(x.reshape(2, 3, 40, 8, 5), x)
    with pytest.raises(ValueError, match="contiguous"):
        P.sample_ssim(x.transpose(2, 3), x)
    with pytest.raises(ValueError, match="dtype"):
        P.sample_ssim(x, x.to(torch.bfloat16))
    with pytest.raises(TypeError, match="float64"):
        P.sample_ssim(x.double(), x.double())
    for bad in (x[:1], x[:, :2].contiguous(), x[0, 0].contiguous(), torch.zeros(3, 40, 41)):
        with pytest.raises(ValueError, match="x.shape or x.shape"):
            P.sample_ssim(x, bad)
    with pytest.raises(ValueError, match="at least 176"):
        P.sample_ssim(torch.zeros(1, 1, 175, 300), torch.zeros(1, 1, 175, 300), levels=5)
    with pytest.raises(ValueError, match="at least 11"):
        P.sample_ssim(torch.zeros(1, 1, 300, 10), torch.zeros(1, 300, 10))
    for levels in (0, 6):
        with pytest.raises(ValueError, match="levels"):
            P.sample_ssim(x, x, levels=levels)
    with pytest.raises(ValueError, match="win_size"):
        P.sample_ssim(x, x, win_size=8)
    with pytest.raises(ValueError, match="data_range"):
        P.sample_ssim(x, x, data_range=0.0)
    for weights in ((0.5, 0.5, 0.5), (0.5, -0.5), (0.5, float("nan"))):
        with pytest.raises(ValueError, match="weights"):
            P.sample_ssim(x, x, levels=2, win_size=3, weights=weights)


def test_ms_ssim_weights():
    from phendiff_amd import diagnostics as D
    for levels in range(1, 6):
        assert np.array_equal(D.ms_ssim_weights(levels), R.weights_of(levels))
    assert np.array_equal(D.ms_ssim_weights(2, (0.25, 0.75)), np.array([0.25, 0.75]))
