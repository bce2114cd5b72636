"""pd_image_preprocess_bands / ImagePreprocessor(channels=C) on the GPU: every band is an independent mode-L image through PIL's own
resize, then ToTensor -> Normalize -> flips with torch on the CPU.  Integer arithmetic and three correctly rounded float operations in a
fixed order: every comparison is for EQUALITY."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# up-scaling and down-scaling, tiles ragged in both directions (8 x 32 output tiles), one axis unchanged, the down-scale limit (factor 32:
# 65 taps -- with 32 bands the workgroups carry band GROUPS, see csrc/data_kernels.hip)
SHAPES = [((37, 53), (16, 16)), ((16, 16), (37, 53)), ((50, 150), (19, 70)), ((33, 33), (33, 17)), ((320, 64), (10, 8))]
BANDS = [2, 5, 32]


def stack(n, H, W, c, seed=0):
    return np.random.default_rng(seed + 1000 * H + 10 * W + c).integers(0, 256, (n, H, W, c), dtype=np.uint8)


def pil_bands(a, OH, OW):
    """One stack (H, W, C) uint8 -> (OH, OW, C): every band resized as a mode-L image."""
    from PIL import Image
    return np.stack([np.array(Image.fromarray(np.ascontiguousarray(a[..., c]), "L").resize((OW, OH), Image.BILINEAR))
                     for c in range(a.shape[-1])], axis=-1)


@functools.lru_cache(maxsize=None)
def reference(n, H, W, c, OH, OW, seed=0):
    """PIL's bytes for stack(n, H, W, c, seed): computed once per shape, shared, read-only."""
    r = np.stack([pil_bands(a, OH, OW) for a in stack(n, H, W, c, seed)])
    r.setflags(write=False)
    return r


def norms(c):
    return [0.1 + 0.02 * i for i in range(c)], [0.5 + 0.01 * i for i in range(c)]


def to_tensor_normalize(raw, mean, std, flips=None):
    m = torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)
    out = []
    for i, r in enumerate(np.asarray(raw)):
        t = torch.from_numpy(np.array(r)).permute(2, 0, 1).float().div(255)
        t = t.sub(m).div(s)
        code = 0 if flips is None else int(flips[i])
        if code & 1:
            t = torch.flip(t, [2])
        if code & 2:
            t = torch.flip(t, [1])
        out.append(t)
    return torch.stack(out)


def check(y, raw, want_raw, mean, std, flips=None):
    torch.cuda.synchronize()
    want_raw = np.asarray(want_raw)
    if raw is not None:
        assert raw.dtype == torch.uint8 and tuple(raw.shape) == want_raw.shape
        diff = int((raw.cpu().numpy() != want_raw).sum())
        assert diff == 0, f"{diff} of {want_raw.size} resized bytes differ from PIL"
    want = to_tensor_normalize(want_raw, mean, std, flips)
    assert y.dtype == torch.float32 and y.shape == want.shape
    got = y.cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} float32 values differ (max |d| {float((got - want).abs().max())})"


@pytest.mark.parametrize("c", BANDS)
@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SHAPES])
def test_bit_equal_to_pil_per_band(src, dst, c):
    import phendiff_amd as P
    (H, W), (OH, OW) = src, dst
    mean, std = norms(c)
    pre = P.ImagePreprocessor((OH, OW), mean=mean, std=std, device=DEV, channels=c)
    y, raw = pre(stack(2, H, W, c), return_raw=True)
    assert tuple(y.shape) == (2, c, OH, OW) and tuple(raw.shape) == (2, OH, OW, c)
    check(y, raw, reference(2, H, W, c, OH, OW), mean, std)


def test_one_band_and_float_only():
    """channels=1 takes (N, H, W) and (N, H, W, 1); without return_raw only the float tensor is written."""
    import phendiff_amd as P
    g = stack(3, 45, 150, 1, seed=3)
    pre = P.ImagePreprocessor((19, 70), device=DEV, channels=1)
    want = reference(3, 45, 150, 1, 19, 70, seed=3)
    for x in (g[..., 0], g, torch.from_numpy(g).to(DEV)):
        y = pre(x)
        assert isinstance(y, torch.Tensor) and tuple(y.shape) == (3, 1, 19, 70)
        check(y, None, want, [0.5], [0.5])


def test_three_bands_equal_the_rgb_entry():
    """C = 3 through the band entry gives the RGB entry's bytes and floats for RGB input."""
    import phendiff_amd as P
    x = stack(3, 50, 150, 3, seed=4)
    y0, raw0 = P.ImagePreprocessor((19, 70), mean=(0.1, 0.2, 0.3), std=(0.7, 0.8, 0.9), device=DEV)(x, return_raw=True)
    y1, raw1 = P.ImagePreprocessor((19, 70), mean=(0.1, 0.2, 0.3), std=(0.7, 0.8, 0.9), device=DEV, channels=3)(x, return_raw=True)
    torch.cuda.synchronize()
    assert torch.equal(raw0, raw1) and torch.equal(y0.view(torch.int32), y1.view(torch.int32))


def test_all_four_flip_codes():
    import phendiff_amd as P
    H, W, OH, OW, c = 50, 150, 19, 70, 5
    flips = torch.tensor([0, 1, 2, 3], dtype=torch.uint8)
    mean, std = norms(c)
    pre = P.ImagePreprocessor((OH, OW), mean=mean, std=std, device=DEV, channels=c)
    y, raw = pre(stack(4, H, W, c), flips=flips, return_raw=True)
    check(y, raw, reference(4, H, W, c, OH, OW), mean, std, flips)


def test_ragged_source_sizes_fill_one_batch_in_list_order():
    """Two source sizes interleaved in one list, arrays and tensors: one launch per size through out_index, slot order = list order."""
    import phendiff_amd as P
    c = 5
    a, b = stack(3, 50, 150, c, seed=5), stack(2, 64, 40, c, seed=6)
    items = [a[0], torch.from_numpy(b[0]), a[1], torch.from_numpy(b[1]).to(DEV), a[2]]
    order = [a[0], b[0], a[1], b[1], a[2]]
    want = np.stack([pil_bands(x, 19, 70) for x in order])
    flips = torch.tensor([1, 2, 3, 0, 1], dtype=torch.uint8)
    mean, std = norms(c)
    y, raw = P.ImagePreprocessor((19, 70), mean=mean, std=std, device=DEV, channels=c)(items, flips=flips, return_raw=True)
    check(y, raw, want, mean, std, flips)


def test_strided_device_view_is_read_in_place():
    """Five bands of an eight-band device tensor (pixel_stride 8 > C): read through the strides, the other three bands never enter."""
    import phendiff_amd as P
    wide = stack(2, 50, 150, 8, seed=7)
    dev = torch.from_numpy(wide).to(DEV)
    view = dev[..., :5]
    assert view.stride() == (50 * 150 * 8, 150 * 8, 8, 1)
    pre = P.ImagePreprocessor((19, 70), device=DEV, channels=5)
    assert pre._strided(view)[0].data_ptr() == dev.data_ptr() and pre._strided(view)[3] == 8        # no copy
    want = np.stack([pil_bands(a[..., :5], 19, 70) for a in wide])
    y, raw = pre(view, return_raw=True)
    check(y, raw, want, [0.5] * 5, [0.5] * 5)
    dev[..., 5:] ^= 0xFF
    y2, raw2 = pre(view, return_raw=True)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(raw, raw2)


def test_wide_pixel_view_under_a_steep_horizontal_downscale_falls_back_to_a_dense_copy():
    """Five bands of 64-byte pixels, 1024 -> 32 columns: a staged source row at that pixel stride does not fit a workgroup's LDS (the entry
    refuses it before launch), the same bands dense do -- the preprocessor reads a dense copy and gives PIL's bytes."""
    import phendiff_amd as P
    wide = stack(2, 8, 1024, 64, seed=9)
    view = torch.from_numpy(wide).to(DEV)[..., :5]
    pre = P.ImagePreprocessor((8, 32), device=DEV, channels=5)
    assert pre._strided(view)[3] == 64                       # the view itself is within what the entry reads in place
    want = np.stack([pil_bands(a[..., :5], 8, 32) for a in wide])
    y, raw = pre(view, return_raw=True)
    check(y, raw, want, [0.5] * 5, [0.5] * 5)


def test_graph_capture_follows_the_input():
    import phendiff_amd as P
    H, W, OH, OW, c = 50, 150, 19, 70, 5
    pre = P.ImagePreprocessor((OH, OW), device=DEV, channels=c)
    x = torch.from_numpy(stack(4, H, W, c)).to(DEV)
    flips = torch.tensor([3, 0, 1, 2], dtype=torch.uint8, device=DEV)
    pre(x, flips=flips)                      # builds the tables and the mean / std vectors outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, raw = pre(x, flips=flips, return_raw=True)
    new = stack(4, H, W, c, seed=21)
    x.copy_(torch.from_numpy(new).to(DEV))
    graph.replay()
    check(y, raw, np.stack([pil_bands(a, OH, OW) for a in new]), [0.5] * c, [0.5] * c, flips.cpu())
