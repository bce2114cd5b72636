"""Guard bands (tests/guard_bands.py; the three properties of tests/test_gpu_guard_bands.py) for the two kernels routes that image
stacks of 4 to 32 channels add: pd_image_preprocess_bands at C = 5, and the padded conv_in route of the pixel UNet
(pd_nchw_to_nhwc over C fp32 NCHW planes -> 32-channel NHWC -> 3x3 pd_conv).
P1: what surrounds an input never reaches the output.  P2: an output is written completely, and nothing beside it.  P3: one sample's
bytes never reach another sample's output."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_image_bands import DEV, check, pil_bands, reference, stack
from test_gpu_unet_channels import make_pair, synth

pytestmark = pytest.mark.gpu
BANDS = 5


def launch_bands(x, n, strides, c, H, W, OH, OW, y_f32, y_u8, out_slots, mean, std, out_index=None, flips=None):
    """pd_image_preprocess_bands through ctypes on explicit pointers and byte strides."""
    import phendiff_amd._lib as L
    from phendiff_amd.data import resample_tables
    a = L.ImagePreprocessBandsArgs(N=n, H=H, W=W, C=c, OH=OH, OW=OW, out_slots=out_slots, image_stride=strides[0], row_stride=strides[1],
                                   pixel_stride=strides[2], x=x.data_ptr(), mean=mean.data_ptr(), std=std.data_ptr(), y_f32=L.ptr(y_f32),
                                   y_u8=L.ptr(y_u8), out_index=L.ptr(out_index), flips=L.ptr(flips))
    keep = []
    for axis, (i, o) in (("x", (W, OW)), ("y", (H, OH))):
        if i != o:
            coef, bounds = (torch.from_numpy(t).to(DEV) for t in resample_tables(i, o))
            keep += [coef, bounds]
            setattr(a, f"coef_{axis}", coef.data_ptr())
            setattr(a, f"bounds_{axis}", bounds.data_ptr())
            setattr(a, f"ksize_{axis}", coef.shape[1])
    L.check(L.lib().pd_image_preprocess_bands(C.byref(a), torch.cuda.current_stream().cuda_stream), "pd_image_preprocess_bands")
    torch.cuda.synchronize()


def half(c):
    return torch.full((c,), 0.5, device=DEV), torch.full((c,), 0.5, device=DEV)


@pytest.mark.parametrize("pad", [13, 64], ids=["odd-stride", "dword-stride"])
def test_bands_p1_row_gaps_and_ends_never_reach_the_output(pad):
    """Rows `pad` bytes apart more than their width, the gap columns and both ends of the allocation filled with 0xFF, then with 0x00:
    identical output bits, equal to the reference."""
    from guard_bands import guarded_rows
    N, H, W, OH, OW, c = 3, 50, 150, 19, 70, BANDS
    src = torch.from_numpy(stack(N, H, W, c))
    rs = W * c + pad
    view, h = guarded_rows(src.view(N * H, W * c), rs, device=DEV, name="source rows")
    mean, std = half(c)
    results = []
    for fill in (h.poison, h.clear):
        fill()
        y = torch.full((N, c, OH, OW), float("nan"), device=DEV)
        raw = torch.full((N, OH, OW, c), 0xAB, dtype=torch.uint8, device=DEV)
        launch_bands(view, N, (H * rs, rs, c), c, H, W, OH, OW, y, raw, N, mean, std)
        check(y, raw, reference(N, H, W, c, OH, OW), [0.5] * c, [0.5] * c)
        results.append((y, raw))
    assert torch.equal(results[0][0].view(torch.int32), results[1][0].view(torch.int32)) and torch.equal(results[0][1], results[1][1])


def test_bands_p1_unread_bands_of_a_wider_pixel_never_reach_the_output():
    """pixel_stride 8 > C = 5: bands 5..7 of every pixel are poison (0xFF), then zero."""
    N, H, W, OH, OW, c = 2, 50, 150, 19, 70, BANDS
    wide = torch.zeros((N, H, W, 8), dtype=torch.uint8)
    wide[..., :c] = torch.from_numpy(stack(N, H, W, c))
    dev = wide.to(DEV)
    mean, std = half(c)
    results = []
    for fill in (0xFF, 0x00):
        dev[..., c:] = fill
        y = torch.full((N, c, OH, OW), float("nan"), device=DEV)
        raw = torch.full((N, OH, OW, c), 0xAB, dtype=torch.uint8, device=DEV)
        launch_bands(dev, N, (H * W * 8, W * 8, 8), c, H, W, OH, OW, y, raw, N, mean, std)
        check(y, raw, reference(N, H, W, c, OH, OW), [0.5] * c, [0.5] * c)
        results.append((y, raw))
    assert torch.equal(results[0][0].view(torch.int32), results[1][0].view(torch.int32)) and torch.equal(results[0][1], results[1][1])


def test_bands_p2_outputs_are_written_completely_and_nothing_else():
    """Both outputs sit between canaries; every element is written, the canaries survive.  Flipped and out_index-scattered writes."""
    from guard_bands import guarded
    N, H, W, OH, OW, c = 3, 50, 150, 19, 70, BANDS
    x = torch.from_numpy(stack(N, H, W, c)).to(DEV)
    y, hy = guarded(torch.full((N, c, OH, OW), float("nan")), device=DEV, name="y_f32")
    raw, hr = guarded(torch.full((N, OH, OW, c), 0xAB, dtype=torch.uint8), device=DEV, name="y_u8")
    hy.canary()
    hr.canary()
    slots = torch.tensor([2, 0, 1], dtype=torch.int32, device=DEV)
    flips = torch.tensor([3, 1, 2], dtype=torch.uint8, device=DEV)
    mean, std = half(c)
    launch_bands(x, N, (H * W * c, W * c, c), c, H, W, OH, OW, y, raw, N, mean, std, out_index=slots, flips=flips)
    assert hy.intact() and hr.intact()
    assert not torch.isnan(y).any()
    order = [1, 2, 0]                        # slot s holds image order[s]
    want = np.asarray(reference(N, H, W, c, OH, OW))[order]
    check(y, raw, want, [0.5] * c, [0.5] * c, flips.cpu()[order])


def test_bands_p3_images_do_not_leak_into_other_slots():
    import phendiff_amd as P
    H, W, OH, OW, c = 50, 150, 19, 70, BANDS
    a = stack(3, H, W, c)
    pre = P.ImagePreprocessor((OH, OW), device=DEV, channels=c)
    y0, raw0 = pre(a, return_raw=True)
    b = a.copy()
    b[1] ^= 0xFF
    y1, raw1 = pre(b, return_raw=True)
    torch.cuda.synchronize()
    for s in (0, 2):
        assert torch.equal(y0[s].view(torch.int32), y1[s].view(torch.int32)) and torch.equal(raw0[s], raw1[s])
    assert not torch.equal(raw0[1], raw1[1]) and not torch.equal(y0[1], y1[1])
    assert np.array_equal(raw1[1].cpu().numpy(), pil_bands(b[1], OH, OW))


# ---- the padded conv_in route -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_conv_in_p1_nan_around_the_input_planes_changes_no_output_bit(mode):
    """The C fp32 NCHW planes of the batch sit between NaN, then between zeros: the transpose reads C planes, not 32."""
    from guard_bands import guarded
    _, m = make_pair(5, 5, mode)
    x, labels = synth(2, 5)
    view, h = guarded(x, device=DEV, name="sample")
    outs = []
    for fill in (h.poison, h.clear):
        fill()
        outs.append(m(view, 640, class_labels=labels.cuda()).sample.clone())
        assert m._plans and next(iter(m._plans.values()))._in_args.x == view.data_ptr()      # read in place
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_conv_in_p3_nan_in_the_other_sample_changes_no_output_bit(mode):
    _, m = make_pair(5, 5, mode)
    x, labels = synth(2, 5)
    clean = m(x.cuda(), 640, class_labels=labels.cuda()).sample.clone()
    for other in (0, 1):
        bad = x.clone()
        bad[other] = float("nan")
        out = m(bad.cuda(), 640, class_labels=labels.cuda()).sample
        torch.cuda.synchronize()
        keep = 1 - other
        assert torch.isfinite(out[keep]).all() and torch.equal(out[keep].view(torch.int32), clean[keep].view(torch.int32))
        assert not torch.isfinite(out[other]).all()
