"""16-bit image stacks -- what needs no GPU: the float64 tables and the arithmetic they stand for (a numpy emulation held to EQUALITY with
PIL's mode I;16 resize), the three new entry points' structs, symbols and refusals, the argument checks of ImagePreprocessor's 16-bit path
and the rank rule of band_percentiles."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from abi_header import define, header_fields
from image16_ref import KINDS, contents, emulate_resize16, pil_bands16

# (H, W) -> (OH, OW): down, up, one axis unchanged (either one), both changed by a hair, nothing changed, the 32 x limit (65 taps)
SHAPES = [((37, 53), (16, 16)), ((16, 16), (37, 53)), ((64, 48), (64, 16)), ((33, 70), (8, 70)), ((130, 97), (32, 24)), ((9, 9), (9, 9)),
          ((21, 40), (20, 41)), ((256, 256), (8, 8))]
NEW = {"pd_image_preprocess_bands16": ("pd_image_preprocess_bands16_args", "ImagePreprocessBands16Args"),
       "pd_band_histogram16": ("pd_band_histogram16_args", "BandHistogram16Args"),
       "pd_postproc_bands16": ("pd_postproc_bands16_args", "PostprocBands16Args")}


@pytest.mark.parametrize("sizes", [(53, 16), (16, 53), (48, 16), (97, 24), (40, 41), (256, 8), (1, 7), (40, 1), (1080, 256)])
def test_f64_tables_share_bounds_and_ksize_with_the_8_bit_tables(sizes):
    from phendiff_amd.data import PRECISION_BITS, resample_tables, resample_tables_f64
    i, o = sizes
    coef8, bounds8 = resample_tables(i, o)
    coef, bounds = resample_tables_f64(i, o)
    assert coef.dtype == np.float64 and bounds.dtype == np.int32 and coef.flags.c_contiguous
    assert coef.shape == coef8.shape == (o, 2 * math.ceil(max(i / o, 1.0)) + 1) and np.array_equal(bounds, bounds8)
    # the 8-bit table is this one in 22-bit fixed point, and nothing lies past a row's count
    assert np.array_equal(np.where(coef < 0, -0.5 + coef * (1 << PRECISION_BITS), 0.5 + coef * (1 << PRECISION_BITS)).astype(np.int64), coef8)
    past = np.arange(coef.shape[1])[None, :] >= bounds[:, 1:2]
    assert (coef[past] == 0.0).all() and (coef >= 0.0).all()
    assert np.abs(np.cumsum(coef, axis=1)[:, -1] - 1.0).max() < 1e-14
    with pytest.raises(ValueError):
        resample_tables_f64(0, 4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SHAPES])
def test_emulated_arithmetic_equals_pil_i16_resize(src, dst, kind):
    """One float64 accumulator per sample, taps in order, product and sum rounded separately, (int)(ss + 0.5), horizontal pass first into
    uint16: equal to PIL.Image.resize of a mode I;16 image, sample for sample."""
    (H, W), (OH, OW) = src, dst
    a = contents(kind, (H, W))
    got, want = emulate_resize16(a, OH, OW), pil_bands16(a, OH, OW)
    assert got.dtype == np.uint16 and got.shape == want.shape == (OH, OW)
    assert int((got != want).sum()) == 0


def test_new_symbols_are_exported_prototyped_and_laid_out_as_the_header_says():
    import phendiff_amd._lib as L
    lib = L.lib()
    for fn, (cname, pyname) in NEW.items():
        assert fn in L.SYMBOLS and hasattr(lib, fn)
        cls = getattr(L, pyname)
        assert L.SYMBOLS[fn] == (C.c_int, [C.POINTER(cls), C.c_void_p])
        assert header_fields(cname) == [f[0] for f in cls._fields_], cname
    b16 = dict(L.ImagePreprocessBands16Args._fields_)
    assert b16["image_stride"] is C.c_longlong and b16["row_stride"] is C.c_longlong and b16["pixel_stride"] is C.c_int
    # the 16-bit struct is the 8-bit band struct with lo / hi ahead of mean and y_u16 for y_u8
    want = [f[0] for f in L.ImagePreprocessBandsArgs._fields_]
    want[want.index("mean"):want.index("mean")] = ["lo", "hi"]
    want[want.index("y_u8")] = "y_u16"
    assert [f[0] for f in L.ImagePreprocessBands16Args._fields_] == want
    # added entry points, no struct changed: the ABI version stays
    assert define("PD_ABI_VERSION") == L.ABI_VERSION == lib.pd_abi_version() == 8


def _args(**kw):
    """Well-formed arguments of a 64 x 64 x 5 -> 32 x 32 call (the pointers are never dereferenced: validation comes first)."""
    import phendiff_amd._lib as L
    d = dict(N=1, H=64, W=64, C=5, OH=32, OW=32, out_slots=1, image_stride=64 * 64 * 10, row_stride=64 * 10, pixel_stride=10, ksize_x=5,
             ksize_y=5, x=256, coef_x=256, bounds_x=256, coef_y=256, bounds_y=256, lo=256, hi=256, mean=256, std=256, y_f32=256, y_u16=256)
    d.update(kw)
    return L.ImagePreprocessBands16Args(**d)


def test_bands16_validates_before_launching():
    import phendiff_amd._lib as L
    lib = L.lib()
    call = lambda a: lib.pd_image_preprocess_bands16(C.byref(a), None)      # noqa: E731
    assert lib.pd_image_preprocess_bands16(None, None) == -1 and b"null pointer" in lib.pd_last_error()
    assert call(_args(x=None)) == -1 and b"null pointer" in lib.pd_last_error()
    assert call(_args(y_f32=None, y_u16=None)) == -1 and b"null pointer" in lib.pd_last_error()
    for bad in (0, 33):
        assert call(_args(C=bad, pixel_stride=128)) == -1 and b"C must be in 1..32" in lib.pd_last_error()
    assert call(_args(lo=None)) == -1 and b"lo" in lib.pd_last_error()
    assert call(_args(hi=None)) == -1 and b"lo / hi" in lib.pd_last_error()
    assert call(_args(mean=None)) == -1 and b"mean" in lib.pd_last_error()
    # (none of the four is needed without y_f32: the refusal that follows is a later one)
    assert call(_args(lo=None, hi=None, mean=None, std=None, y_f32=None, ksize_x=3)) == -2 and b"ksize" in lib.pd_last_error()
    assert call(_args(x=257)) == -1 and b"aligned" in lib.pd_last_error()
    assert call(_args(pixel_stride=11, row_stride=64 * 11 + 1)) == -2 and b"pixel_stride" in lib.pd_last_error() and b"even" in lib.pd_last_error()
    assert call(_args(row_stride=64 * 10 + 1)) == -2 and b"row_stride" in lib.pd_last_error() and b"even" in lib.pd_last_error()
    assert call(_args(N=2, image_stride=64 * 64 * 10 + 1)) == -2 and b"image_stride" in lib.pd_last_error()
    assert call(_args(pixel_stride=8)) == -2 and b"pixel_stride" in lib.pd_last_error() and b"2 * C" in lib.pd_last_error()
    assert call(_args(pixel_stride=130, row_stride=64 * 130, image_stride=64 * 64 * 130)) == -2 and b"pixel_stride" in lib.pd_last_error()
    assert call(_args(H=33 * 32, image_stride=33 * 32 * 64 * 10, ksize_y=67)) == -2 and b"above 32" in lib.pd_last_error()
    assert call(_args(W=33 * 32, row_stride=33 * 32 * 10, image_stride=33 * 32 * 64 * 10, ksize_x=67)) == -2 and b"above 32" in lib.pd_last_error()
    assert call(_args(ksize_x=3)) == -2 and b"ksize" in lib.pd_last_error()
    assert call(_args(ksize_y=7)) == -2 and b"ksize" in lib.pd_last_error()
    assert call(_args(coef_y=None)) == -1 and b"table" in lib.pd_last_error()
    assert call(_args(OH=0)) == -2 and b"positive" in lib.pd_last_error()
    assert call(_args(N=0)) == -2 and call(_args(out_slots=0)) == -2
    assert call(_args(row_stride=64 * 10 - 2)) == -2 and b"row_stride" in lib.pd_last_error()
    assert call(_args(N=2, image_stride=64 * 64 * 10 - 2)) == -2 and b"image_stride" in lib.pd_last_error()
    assert call(_args(N=400, image_stride=1 << 24)) == -2 and b"source beyond 32-bit" in lib.pd_last_error()
    assert call(_args(out_slots=1 << 18)) == -2 and b"output beyond 32-bit" in lib.pd_last_error()
    # a view into 128-byte pixels under a 32 x horizontal down-scale: one staged source row is beyond a workgroup's 64 KiB for every band
    # group (ImagePreprocessor then reads a dense copy)
    assert call(_args(W=1024, pixel_stride=128, row_stride=1024 * 128, image_stride=64 * 1024 * 128, ksize_x=65)) == -2 \
        and b"LDS budget" in lib.pd_last_error()
    assert lib.pd_last_error().startswith(b"pd_image_preprocess_bands16:")


def test_histogram_and_postproc_validate_before_launching():
    import phendiff_amd._lib as L
    lib = L.lib()
    good = dict(N=2, H=64, W=64, C=5, image_stride=64 * 64 * 10, row_stride=64 * 10, pixel_stride=10, x=256, counts=256)
    hist = lambda **kw: lib.pd_band_histogram16(C.byref(L.BandHistogram16Args(**dict(good, **kw))), None)      # noqa: E731
    assert lib.pd_band_histogram16(None, None) == -1 and b"null pointer" in lib.pd_last_error()
    assert hist(x=None) == -1 and hist(counts=None) == -1 and b"null pointer" in lib.pd_last_error()
    assert hist(C=0) == -1 and hist(C=33, pixel_stride=66) == -1 and b"C must be in 1..32" in lib.pd_last_error()
    assert hist(x=257) == -1 and b"aligned" in lib.pd_last_error()
    assert hist(N=0) == -2 and b"positive" in lib.pd_last_error()
    assert hist(N=1 << 20, H=64, W=64) == -2 and b"below 2^32" in lib.pd_last_error()          # 2^32 samples a band, exactly
    assert hist(pixel_stride=8) == -2 and b"pixel_stride" in lib.pd_last_error()
    assert hist(pixel_stride=11, row_stride=64 * 11 + 1) == -2 and b"even" in lib.pd_last_error()
    assert hist(row_stride=64 * 10 - 2) == -2 and b"row_stride" in lib.pd_last_error()
    assert hist(image_stride=64 * 64 * 10 - 2) == -2 and b"image_stride" in lib.pd_last_error()
    assert lib.pd_last_error().startswith(b"pd_band_histogram16:")
    good = dict(N=2, C=5, H=8, W=8, x=256, lo=256, hi=256, mean=256, std=256, y=256)
    post = lambda **kw: lib.pd_postproc_bands16(C.byref(L.PostprocBands16Args(**dict(good, **kw))), None)      # noqa: E731
    assert lib.pd_postproc_bands16(None, None) == -1
    for name in ("x", "lo", "hi", "mean", "std", "y"):
        assert post(**{name: None}) == -1 and b"null pointer" in lib.pd_last_error(), name
    assert post(C=0) == -1 and post(C=33) == -1 and b"C must be in 1..32" in lib.pd_last_error()
    assert post(H=0) == -2 and b"positive" in lib.pd_last_error()
    assert lib.pd_last_error().startswith(b"pd_postproc_bands16:")


def test_preprocessor_16_bit_host_side_checks():
    """Every refusal below is raised before any device call (there is no device here)."""
    import phendiff_amd as P
    u16 = np.zeros((1, 8, 8, 5), np.uint16)
    with pytest.raises(TypeError, match="channels"):
        P.ImagePreprocessor((8, 8))(np.zeros((1, 8, 8, 3), np.uint16))                      # 16-bit RGB without channels
    with pytest.raises(TypeError, match="channels"):
        P.ImagePreprocessor((8, 8))([np.zeros((8, 8, 3), np.uint16)])
    pre = P.ImagePreprocessor((8, 8), channels=5)
    assert pre.window is None
    for bad in (np.int16, np.int32, np.float32, np.float64):
        with pytest.raises(TypeError, match="uint8 or uint16"):
            pre(np.zeros((1, 8, 8, 5), bad))
        with pytest.raises(TypeError, match="uint8 or uint16"):
            pre([np.zeros((8, 8, 5), bad)])
    with pytest.raises(TypeError):
        pre(torch.zeros((1, 8, 8, 5), dtype=torch.int16))
    with pytest.raises(TypeError, match="uint8 and uint16"):
        pre([np.zeros((8, 8, 5), np.uint8), np.zeros((8, 8, 5), np.uint16)])
    with pytest.raises(ValueError, match=r"\(N, H, W, 5\)"):
        pre(np.zeros((1, 8, 8, 3), np.uint16))
    with pytest.raises(ValueError):
        pre(np.zeros((2, 8, 8), np.uint16))                                                 # (N, H, W) is the one-band form only
    with pytest.raises(ValueError, match="down-scale"):
        P.ImagePreprocessor((2, 2), channels=5)(np.zeros((1, 65, 8, 5), np.uint16))
    # window
    win = P.ImagePreprocessor((8, 8), channels=5, window=(100, 4000))
    assert win.window == ([100.0] * 5, [4000.0] * 5)
    with pytest.raises(ValueError, match="window"):
        win(np.zeros((1, 8, 8, 5), np.uint8))                                               # a uint8 source has no window
    with pytest.raises(ValueError, match="window"):
        P.ImagePreprocessor((8, 8), window=(0, 1))                                          # ... nor has the RGB path
    for lo, hi in ((5, 5), (6, 5), ([0, 0, 0, 0, 9], [1, 1, 1, 1, 9])):
        with pytest.raises(ValueError, match="hi must be above lo"):
            P.ImagePreprocessor((8, 8), channels=5, window=(lo, hi))
    with pytest.raises(ValueError, match="window lo"):
        P.ImagePreprocessor((8, 8), channels=5, window=([0, 1, 2], 9))
    with pytest.raises(ValueError, match="window hi"):
        P.ImagePreprocessor((8, 8), channels=5, window=(0, torch.ones(4)))
    with pytest.raises(ValueError, match="window"):
        P.ImagePreprocessor((8, 8), channels=5, window=(0, 1, 2))
    kept = torch.full((5,), 7.0)
    assert P.ImagePreprocessor((8, 8), channels=5, window=(0, kept)).window[1] is kept        # a tensor is used as it is
    with pytest.raises(ValueError, match="restore"):
        P.ImagePreprocessor((8, 8)).restore(torch.zeros(1, 3, 8, 8))
    with pytest.raises(TypeError):
        P.band_percentiles(np.zeros((1, 8, 8, 5), np.uint8), channels=5)
    with pytest.raises(ValueError, match="channels"):
        P.band_percentiles(u16)
    with pytest.raises(ValueError, match="q must be"):
        P.band_percentiles(u16, q=(50, 10), channels=5)
    with pytest.raises(TypeError):
        P.restore_bands16(torch.zeros(1, 5, 8, 8, dtype=torch.float64), (0, 1), 0.5, 0.5)
    if not torch.cuda.is_available():
        for call in (lambda: pre(u16), lambda: P.band_percentiles(u16, channels=5), lambda: pre.restore(torch.zeros(1, 5, 8, 8)),
                     lambda: P.restore_bands16(torch.zeros(1, 5, 8, 8), (0, 1), 0.5, 0.5)):
            with pytest.raises(P.PhenDiffHipError, match="no CPU fallback"):
                call()


def test_percentile_rank_rule():
    """k = max(1, ceil(n * q / 100)) in float64; the percentile is the k-th smallest sample."""
    from phendiff_amd.data import percentile_rank
    assert percentile_rank(1000, 0.1) == 1 and percentile_rank(1000, 99.9) == 999 and percentile_rank(1000, 100) == 1000
    assert percentile_rank(1000, 0) == 1 and percentile_rank(1, 50) == 1 and percentile_rank(1001, 0.1) == 2
    assert percentile_rank(3 * 64 * 64, 99.9) == math.ceil(3 * 64 * 64 * 99.9 / 100) == 12276
    for n in (1, 7, 4096, 37 * 53 * 3, (1 << 32) - 1):
        for q in (0, 0.1, 1, 50, 99.9, 100):
            k = percentile_rank(n, q)
            assert k == max(1, math.ceil(n * q / 100)) and 1 <= k <= n
    band = np.random.default_rng(5).integers(0, 65536, 5000, dtype=np.uint16)
    assert np.sort(band)[percentile_rank(band.size, 100) - 1] == band.max() and np.sort(band)[percentile_rank(band.size, 0) - 1] == band.min()
    for bad in ((0, 50), (10, -1), (10, 100.5)):
        with pytest.raises(ValueError):
            percentile_rank(*bad)
