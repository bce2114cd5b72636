"""Image preprocessing (phendiff_amd/data.py, pd_image_preprocess) -- what needs no GPU: the resampling tables against PIL itself, the output
size rule, the order in which flip codes consume the RNG, and the C entry point's argument validation."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_header import define, header_fields

# (H, W) -> (OH, OW): up-scaling, down-scaling, 1-pixel sources, one axis unchanged, nothing to do, and the training shape
SHAPES = [((37, 53), (16, 16)), ((16, 16), (37, 53)), ((64, 64), (32, 32)), ((97, 61), (128, 128)), ((200, 300), (128, 128)),
          ((33, 33), (33, 17)), ((1, 7), (5, 3)), ((5, 5), (5, 5)), ((48, 80), (32, 32)), ((1024, 1280), (128, 128))]


def apply_tables(a, coef, bounds, axis):
    """Pillow's 8-bit pass along one axis in integers: acc = 1 << 21; acc += src * coef; out = clamp(acc >> 22)."""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((coef.shape[0],) + a.shape[1:], np.uint8)
    for i in range(coef.shape[0]):
        first, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << 21) + np.tensordot(coef[i, :n].astype(np.int64), a[first:first + n], axes=(0, 0))
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_with_tables(a, OH, OW):
    """Horizontal pass first, into uint8, then the vertical pass; an axis whose size does not change is skipped."""
    from phendiff_amd.data import resample_tables
    H, W = a.shape[:2]
    if W != OW:
        a = apply_tables(a, *resample_tables(W, OW), axis=1)
    if H != OH:
        a = apply_tables(a, *resample_tables(H, OH), axis=0)
    return a


@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SHAPES])
def test_tables_reproduce_pil_bilinear(src, dst):
    from PIL import Image
    (H, W), (OH, OW) = src, dst
    a = np.random.default_rng(H * 10007 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(a).resize((OW, OH), Image.BILINEAR))
    got = resize_with_tables(a, OH, OW)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert int((got != want).sum()) == 0


def test_table_layout():
    from phendiff_amd.data import resample_tables
    coef, bounds = resample_tables(1280, 128)
    assert coef.dtype == np.int32 and bounds.dtype == np.int32 and coef.shape == (128, 21) and bounds.shape == (128, 2)
    assert resample_tables(16, 37)[0].shape == (37, 3) and resample_tables(320, 10)[0].shape == (10, 65)
    first, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (n >= 1).all() and (n <= 21).all() and (first >= 0).all() and (first + n <= 1280).all()
    assert (np.diff(first) >= 0).all() and (np.diff(first + n) >= 0).all()          # the kernel's tile window relies on monotone bounds
    assert (coef >= 0).all() and (np.abs(coef.sum(axis=1) - (1 << 22)) <= 21).all()  # rows are normalised to 1.0 in 22-bit fixed point
    assert all((coef[i, n[i]:] == 0).all() for i in range(128))
    with pytest.raises(ValueError):
        resample_tables(0, 4)


def test_resized_output_size():
    from phendiff_amd.data import resized_output_size
    assert resized_output_size(100, 200, 64) == (64, 128)
    assert resized_output_size(200, 100, 64) == (128, 64)
    assert resized_output_size(50, 75, 32) == (32, 48)
    assert resized_output_size(40, 60, 16) == (16, 24)
    assert resized_output_size(100, 200, (17, 31)) == (17, 31) and resized_output_size(5, 5, [128, 96]) == (128, 96)


def test_draw_flips_consumes_the_rng_like_the_composed_transform():
    from phendiff_amd.data import draw_flips
    got = draw_flips(9, torch.Generator().manual_seed(77))
    g = torch.Generator().manual_seed(77)
    want = []
    for _ in range(9):          # RandomHorizontalFlip then RandomVerticalFlip, image after image
        h = bool(torch.rand(1, generator=g) < 0.5)
        v = bool(torch.rand(1, generator=g) < 0.5)
        want.append(int(h) + 2 * int(v))
    assert got.dtype == torch.uint8 and got.tolist() == want and len(set(want)) > 1
    assert draw_flips(5, torch.Generator().manual_seed(1), p=0.0).tolist() == [0] * 5
    assert draw_flips(5, torch.Generator().manual_seed(1), p=1.0).tolist() == [3] * 5
    torch.manual_seed(5)
    a = draw_flips(6)
    torch.manual_seed(5)
    assert torch.equal(a, draw_flips(6))      # no generator: the global RNG, like the transforms


def test_struct_matches_header_and_is_bound():
    import phendiff_amd as P
    import phendiff_amd._lib as L
    assert header_fields("pd_image_preprocess_args") == [f[0] for f in L.ImagePreprocessArgs._fields_]
    assert "pd_image_preprocess" in L.SYMBOLS and hasattr(L.lib(), "pd_image_preprocess")
    assert define("PD_ABI_VERSION") == L.ABI_VERSION == L.lib().pd_abi_version()
    assert P.data.ImagePreprocessor is P.ImagePreprocessor


def test_the_three_structs_keep_their_abi_8_layout():
    """The three image structs share their 19 leading fields: their sizes and offsets are pinned to what the C
    structs of ABI 8 have (ints, two long longs, pointers and floats under the x86-64 rules)."""
    import phendiff_amd._lib as L
    rgb, bands, bands16 = L.ImagePreprocessArgs, L.ImagePreprocessBandsArgs, L.ImagePreprocessBands16Args
    assert [C.sizeof(s) for s in (rgb, bands, bands16)] == [160, 152, 168]
    shared = [f[0] for f in rgb._fields_[:19]]
    assert shared[3] == "Cin" and shared[-1] == "flips"
    for s in (bands, bands16):
        assert [f[0] for f in s._fields_[:19]] == shared[:3] + ["C"] + shared[4:]
    for s in (rgb, bands, bands16):
        assert [getattr(s, f).offset for f in ("N", "OH", "image_stride", "pixel_stride", "x", "flips")] == [0, 16, 32, 48, 64, 112]
        assert getattr(s, s._fields_[3][0]).offset == 12
    assert [getattr(rgb, f).offset for f in ("mean0", "std0", "y_f32", "y_u8")] == [120, 132, 144, 152]
    assert [getattr(bands, f).offset for f in ("mean", "std", "y_f32", "y_u8")] == [120, 128, 136, 144]
    assert [getattr(bands16, f).offset for f in ("lo", "hi", "mean", "std", "y_f32", "y_u16")] == [120, 128, 136, 144, 152, 160]


def _args(**kw):
    """Well-formed arguments of a 64 x 64 x 3 -> 32 x 32 call (the pointers are never dereferenced: validation comes first)."""
    import phendiff_amd._lib as L
    d = dict(N=1, H=64, W=64, Cin=3, OH=32, OW=32, out_slots=1, image_stride=64 * 64 * 3, row_stride=64 * 3, pixel_stride=3, ksize_x=5,
             ksize_y=5, x=256, coef_x=256, bounds_x=256, coef_y=256, bounds_y=256, y_f32=256, y_u8=256, std0=0.5, std1=0.5, std2=0.5)
    d.update(kw)
    return L.ImagePreprocessArgs(**d)


def test_validates_before_launching():
    import phendiff_amd._lib as L
    lib = L.lib()
    call = lambda a: lib.pd_image_preprocess(C.byref(a), None)      # noqa: E731
    assert lib.pd_image_preprocess(None, None) == -1 and b"null pointer" in lib.pd_last_error()
    assert call(_args(x=None)) == -1 and b"null pointer" in lib.pd_last_error()
    assert call(_args(y_f32=None, y_u8=None)) == -1 and b"null pointer" in lib.pd_last_error()
    assert call(_args(coef_y=None)) == -1 and b"table" in lib.pd_last_error()
    assert call(_args(Cin=2)) == -1 and b"Cin" in lib.pd_last_error()
    assert call(_args(H=33 * 32, image_stride=33 * 32 * 64 * 3, ksize_y=67)) == -2 and b"above 32" in lib.pd_last_error()
    assert call(_args(W=33 * 32, row_stride=33 * 32 * 3, image_stride=33 * 32 * 64 * 3, ksize_x=67)) == -2 and b"above 32" in lib.pd_last_error()
    assert call(_args(OH=0)) == -2 and b"positive" in lib.pd_last_error()
    assert call(_args(N=0)) == -2 and call(_args(out_slots=0)) == -2
    assert call(_args(ksize_x=3)) == -2 and b"ksize" in lib.pd_last_error()
    assert call(_args(pixel_stride=2)) == -2 and b"pixel_stride" in lib.pd_last_error()
    assert call(_args(row_stride=64 * 3 - 1)) == -2 and b"row_stride" in lib.pd_last_error()
    assert call(_args(N=2, image_stride=64 * 64 * 3 - 1)) == -2 and b"image_stride" in lib.pd_last_error()
    # 32-bit byte offsets per launch: source (N x image_stride) and output (slots x 3 x OH x OW x 4 bytes)
    assert call(_args(N=400, image_stride=1 << 24)) == -2 and b"source beyond 32-bit" in lib.pd_last_error()
    assert call(_args(out_slots=1 << 19)) == -2 and b"output beyond 32-bit" in lib.pd_last_error()


def test_preprocessor_host_side_checks():
    """What ImagePreprocessor decides before it touches a device: argument errors, and no CPU fallback."""
    import phendiff_amd as P
    pre = P.ImagePreprocessor(16)
    mixed = [np.zeros((40, 60, 3), np.uint8), np.zeros((40, 40, 3), np.uint8)]       # -> (16, 24) and (16, 16)
    with pytest.raises(ValueError, match="different output sizes"):
        pre(mixed)
    with pytest.raises(TypeError):
        pre(np.zeros((1, 8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        pre(np.zeros((1, 8, 8, 2), np.uint8))
    with pytest.raises(ValueError, match="down-scale"):
        P.ImagePreprocessor((2, 2))(np.zeros((1, 65, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="flips"):
        P.ImagePreprocessor((8, 8))(np.zeros((2, 8, 8, 3), np.uint8), flips=torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        P.ImagePreprocessor((8, 8), std=0.0)
    assert P.ImagePreprocessor((8, 8), mean=(0.1, 0.2, 0.3)).mean == [0.1, 0.2, 0.3] and pre.std == [0.5] * 3
    if not torch.cuda.is_available():
        with pytest.raises(P.PhenDiffHipError, match="no CPU fallback"):
            P.ImagePreprocessor((8, 8))(np.zeros((1, 8, 8, 3), np.uint8))
