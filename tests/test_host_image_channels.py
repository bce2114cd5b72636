"""Image stacks of 4 to 32 channels -- what needs no GPU: pd_image_preprocess_bands' struct, symbol and refusals, the argument checks of
ImagePreprocessor(channels=C), the channel range of the pixel UNet and the PIL refusal of the pipeline."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_header import define, header_fields


def test_bands_struct_matches_header_and_is_bound():
    import phendiff_amd._lib as L
    assert header_fields("pd_image_preprocess_bands_args") == [f[0] for f in L.ImagePreprocessBandsArgs._fields_]
    assert "pd_image_preprocess_bands" in L.SYMBOLS and hasattr(L.lib(), "pd_image_preprocess_bands")
    # an added entry point, no struct changed: the ABI version stays
    assert define("PD_ABI_VERSION") == L.ABI_VERSION == L.lib().pd_abi_version() == 8
    # the RGB entry's struct is what it was
    assert [f[0] for f in L.ImagePreprocessArgs._fields_][19:25] == ["mean0", "mean1", "mean2", "std0", "std1", "std2"]


def _args(**kw):
    """Well-formed arguments of a 64 x 64 x 5 -> 32 x 32 call (the pointers are never dereferenced: validation comes first)."""
    import phendiff_amd._lib as L
    d = dict(N=1, H=64, W=64, C=5, OH=32, OW=32, out_slots=1, image_stride=64 * 64 * 5, row_stride=64 * 5, pixel_stride=5, ksize_x=5,
             ksize_y=5, x=256, coef_x=256, bounds_x=256, coef_y=256, bounds_y=256, mean=256, std=256, y_f32=256, y_u8=256)
    d.update(kw)
    return L.ImagePreprocessBandsArgs(**d)


def test_bands_validates_before_launching():
    import phendiff_amd._lib as L
    lib = L.lib()
    call = lambda a: lib.pd_image_preprocess_bands(C.byref(a), None)      # noqa: E731
    assert lib.pd_image_preprocess_bands(None, None) == -1 and b"null pointer" in lib.pd_last_error()
    assert call(_args(x=None)) == -1 and b"null pointer" in lib.pd_last_error()
    assert call(_args(y_f32=None, y_u8=None)) == -1 and b"null pointer" in lib.pd_last_error()
    for bad in (0, 33, -1):
        assert call(_args(C=bad, pixel_stride=64)) == -1 and b"C must be in 1..32" in lib.pd_last_error()
    assert call(_args(mean=None)) == -1 and b"mean" in lib.pd_last_error()
    assert call(_args(std=None)) == -1 and b"mean / std" in lib.pd_last_error()
    assert call(_args(pixel_stride=4)) == -2 and b"pixel_stride" in lib.pd_last_error()
    assert call(_args(pixel_stride=65, row_stride=64 * 65, image_stride=64 * 64 * 65)) == -2 and b"pixel_stride" in lib.pd_last_error()
    assert call(_args(coef_y=None)) == -1 and b"table" in lib.pd_last_error()
    assert call(_args(H=33 * 32, image_stride=33 * 32 * 64 * 5, ksize_y=67)) == -2 and b"above 32" in lib.pd_last_error()
    assert call(_args(W=33 * 32, row_stride=33 * 32 * 5, image_stride=33 * 32 * 64 * 5, ksize_x=67)) == -2 and b"above 32" in lib.pd_last_error()
    assert call(_args(OH=0)) == -2 and b"positive" in lib.pd_last_error()
    assert call(_args(N=0)) == -2 and call(_args(out_slots=0)) == -2
    assert call(_args(ksize_x=3)) == -2 and b"ksize" in lib.pd_last_error()
    assert call(_args(row_stride=64 * 5 - 1)) == -2 and b"row_stride" in lib.pd_last_error()
    assert call(_args(N=2, image_stride=64 * 64 * 5 - 1)) == -2 and b"image_stride" in lib.pd_last_error()
    assert call(_args(N=400, image_stride=1 << 24)) == -2 and b"source beyond 32-bit" in lib.pd_last_error()
    # output: slots x C x OH x OW x 4 bytes
    assert call(_args(out_slots=1 << 18)) == -2 and b"output beyond 32-bit" in lib.pd_last_error()
    # a view into 64-byte pixels under a 32 x horizontal down-scale: one staged source row (1059 columns x 64 bytes) is beyond the 64 KiB of a
    # workgroup for every band group (documented in the header; ImagePreprocessor then reads a dense copy)
    assert call(_args(W=1024, pixel_stride=64, row_stride=1024 * 64, image_stride=64 * 1024 * 64, ksize_x=65)) == -2 \
        and b"LDS budget" in lib.pd_last_error()
    # every message names the entry that refused
    assert lib.pd_last_error().startswith(b"pd_image_preprocess_bands:")


def test_preprocessor_channels_host_side_checks():
    import phendiff_amd as P
    pre = P.ImagePreprocessor((8, 8), channels=5)
    assert pre.channels == 5 and pre.mean == [0.5] * 5 and pre.std == [0.5] * 5
    assert P.ImagePreprocessor((8, 8), channels=5, mean=[.1, .2, .3, .4, .5]).mean == [.1, .2, .3, .4, .5]
    with pytest.raises(ValueError, match="mean"):
        P.ImagePreprocessor((8, 8), channels=5, mean=(0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match="std"):
        P.ImagePreprocessor((8, 8), channels=5, std=(0.1, 0.2, 0.3))
    with pytest.raises(ValueError):
        P.ImagePreprocessor((8, 8), channels=5, std=[.5, .5, 0.0, .5, .5])
    for bad in (0, 33, 2.5):
        with pytest.raises(ValueError, match="channels"):
            P.ImagePreprocessor((8, 8), channels=bad)
    with pytest.raises(ValueError, match=r"\(N, H, W, 5\)"):
        pre(np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        pre(np.zeros((2, 8, 8), np.uint8))                   # (N, H, W) is the one-band form only
    with pytest.raises(ValueError, match=r"\(H, W, 5\)"):
        pre([np.zeros((8, 8, 5), np.uint8), np.zeros((8, 8, 4), np.uint8)])
    with pytest.raises(TypeError):
        pre(np.zeros((1, 8, 8, 5), np.float32))
    from PIL import Image
    with pytest.raises(TypeError, match="PIL"):
        pre([Image.fromarray(np.zeros((8, 8, 3), np.uint8))])
    with pytest.raises(TypeError, match="PIL"):
        P.ImagePreprocessor((8, 8), channels=3)([Image.fromarray(np.zeros((8, 8, 3), np.uint8))])
    with pytest.raises(ValueError, match="down-scale"):
        P.ImagePreprocessor((2, 2), channels=5)(np.zeros((1, 65, 8, 5), np.uint8))
    with pytest.raises(ValueError, match="flips"):
        pre(np.zeros((2, 8, 8, 5), np.uint8), flips=torch.zeros(3, dtype=torch.uint8))
    # the default-constructed object is what it was
    default = P.ImagePreprocessor((8, 8))
    assert default.channels is None and default.mean == [0.5] * 3
    with pytest.raises(ValueError):
        default(np.zeros((1, 8, 8, 2), np.uint8))
    with pytest.raises(ValueError):
        default(np.zeros((1, 8, 8, 5), np.uint8))
    with pytest.raises(ValueError, match="three"):
        P.ImagePreprocessor((8, 8), mean=(0.1, 0.2))
    if not torch.cuda.is_available():
        with pytest.raises(P.PhenDiffHipError, match="no CPU fallback"):
            pre(np.zeros((1, 8, 8, 5), np.uint8))


def _cfg(**kw):
    import phendiff_amd as P
    return dict(P.UNET_CONFIGS["super_small"], sample_size=32, **kw)


def test_channel_range_is_checked_at_construction():
    import phendiff_amd as P
    for key in ("in_channels", "out_channels"):
        for bad in (33, 64, 0):
            with pytest.raises(NotImplementedError, match=r"1\.\.32"):
                P.CustomCondUNet2DModel(**_cfg(**{key: bad}))
    for cin, cout in ((1, 1), (4, 4), (5, 2), (32, 32)):
        m = P.CustomCondUNet2DModel(**_cfg(in_channels=cin, out_channels=cout))
        assert tuple(m.conv_in.weight.shape[:2]) == (m.config.block_out_channels[0], cin) and m.conv_out.weight.shape[0] == cout


def test_pil_output_is_refused_before_sampling():
    """output_type="pil" with a channel count PIL cannot hold: ValueError naming output_type="numpy", raised before any device work (the model
    sits on the CPU here: a forward would raise PhenDiffHipError instead)."""
    import phendiff_amd as P
    unet = P.CustomCondUNet2DModel(compute_dtype="f32", **_cfg(in_channels=5, out_channels=5))
    pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
    labels = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match='output_type="numpy"'):
        pipe(labels, num_inference_steps=2)                                   # "pil" is the default
    x = torch.zeros(2, 5, 32, 32)
    with pytest.raises(ValueError, match='output_type="numpy"'):
        P.ddib(pipe, x, labels, 1 - labels, 2, output_type="pil")              # not after the inversion half
    with pytest.raises(ValueError, match='output_type="numpy"'):
        P.inverted_regeneration(pipe, x, labels, 2, output_type="pil")
    with pytest.raises(ValueError, match='output_type="numpy"'):
        P.classifier_free_guidance_forward_start(pipe, x, labels, 2.5, 0.5, 2, output_type="pil")
    with pytest.raises(P.PhenDiffHipError):
        P.ddib(pipe, x, labels, 1 - labels, 2)                                  # "numpy": the refusal is about PIL alone
    with pytest.raises(ValueError, match='output_type="numpy"'):
        P.linear_interp_custom_guidance_inverted_start(pipe, torch.zeros(2, 5, 32, 32), labels, 1 - labels, 2, 0.001, 2, output_type="pil")
