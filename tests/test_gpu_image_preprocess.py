"""pd_image_preprocess / phendiff_amd.data.ImagePreprocessor on the GPU against the reference's own transform stack run on the CPU:
PIL resize per image -> ToTensor -> Normalize -> flips.  The resize is integer arithmetic and the float tail is three correctly rounded
operations in a fixed order, so every comparison is for EQUALITY (torch.equal on float32, byte equality on uint8)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TILE_H, TILE_W = 8, 32          # the kernel's output tile (csrc/data_kernels.hip IP_TOH x IP_TOW)

# the list of tests/test_host_image_preprocess.py without the 1024 x 1280 case (its own test below), plus
#   (50, 150) -> (19, 70): 3 x 3 tiles of 8 x 32, the last row of tiles 3 high and the last column 6 wide (ragged in both directions)
#   (70, 19) -> (50, 150): the same raggedness when up-scaling (tiles overlap in their source window, 7 x 5 tiles)
#   (320, 64) -> (10, 8): the down-scale limit, factor 32 vertically (65 taps), 8 horizontally
SHAPES = [((37, 53), (16, 16)), ((16, 16), (37, 53)), ((64, 64), (32, 32)), ((97, 61), (128, 128)), ((200, 300), (128, 128)),
          ((33, 33), (33, 17)), ((1, 7), (5, 3)), ((5, 5), (5, 5)), ((48, 80), (32, 32)),
          ((50, 150), (19, 70)), ((70, 19), (50, 150)), ((320, 64), (10, 8))]
NORMS = [(0.5, 0.5), ((0.1, 0.2, 0.3), (0.7, 0.8, 0.9))]


def images(n, H, W, c=3, seed=0):
    shape = (n, H, W) if c is None else (n, H, W, c)
    return np.random.default_rng(seed + 1000 * H + W).integers(0, 256, shape, dtype=np.uint8)


def pil_resize(a, OH, OW):
    """One image (H, W, 3) uint8 through PIL -> (OH, OW, 3) uint8."""
    from PIL import Image
    return np.array(Image.fromarray(a).resize((OW, OH), Image.BILINEAR))


@functools.lru_cache(maxsize=None)
def resized_reference(n, H, W, OH, OW):
    """PIL's bytes for images(n, H, W): computed once per shape, shared by the tests, never modified (callers only read)."""
    r = np.stack([pil_resize(a, OH, OW) for a in images(n, H, W)])
    r.setflags(write=False)
    return r


def to_tensor_normalize(raw, mean, std, flips=None):
    """ToTensor -> Normalize -> flips of resized uint8 NHWC images, with the reference's torch ops on the CPU."""
    m = torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)
    out = []
    for i, r in enumerate(raw):
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


@pytest.mark.parametrize("mean,std", NORMS, ids=["half", "per-channel"])
@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SHAPES])
def test_bit_equal_to_pil_and_torch(src, dst, mean, std):
    import phendiff_amd as P
    (H, W), (OH, OW) = src, dst
    pre = P.ImagePreprocessor((OH, OW), mean=mean, std=std, device=DEV)
    y, raw = pre(images(3, H, W), return_raw=True)
    check(y, raw, resized_reference(3, H, W, OH, OW), mean, std)


def test_training_shape():
    """1024 x 1280 microscopy crops -> 128 x 128 (scale 8 x 10: 17 x 21 taps, 16 x 4 tiles per image)."""
    import phendiff_amd as P
    y, raw = P.ImagePreprocessor((128, 128), device=DEV)(images(2, 1024, 1280), return_raw=True)
    check(y, raw, resized_reference(2, 1024, 1280, 128, 128), 0.5, 0.5)


def test_float_only_and_device_input():
    """Without return_raw only the float tensor is written; a device-resident batch is read in place."""
    import phendiff_amd as P
    x = torch.from_numpy(images(3, 37, 53)).to(DEV)
    y = P.ImagePreprocessor((16, 16), device=DEV)(x)
    assert isinstance(y, torch.Tensor)
    check(y, None, resized_reference(3, 37, 53, 16, 16), 0.5, 0.5)


@pytest.mark.parametrize("dst", [(19, 70), (45, 23)], ids=["down", "one-axis-unchanged"])
def test_single_channel_is_replicated(dst):
    """Mode L: (N, H, W) and (N, H, W, 1) give what PIL's convert("RGB") of the same data gives."""
    from PIL import Image
    import phendiff_amd as P
    OH, OW = dst
    g = images(3, 45, 150, c=None, seed=3)
    want = np.stack([np.array(Image.fromarray(a).convert("RGB").resize((OW, OH), Image.BILINEAR)) for a in g])
    pre = P.ImagePreprocessor((OH, OW), mean=(0.1, 0.2, 0.3), std=(0.7, 0.8, 0.9), device=DEV)
    for x in (g, g[..., None]):
        y, raw = pre(x, return_raw=True)
        check(y, raw, want, (0.1, 0.2, 0.3), (0.7, 0.8, 0.9))


def test_rgba_drops_alpha():
    """Pixel stride 4: RGBA bytes are read in place, alpha never enters the result."""
    from PIL import Image
    import phendiff_amd as P
    rgba = images(3, 50, 150, c=4, seed=4)
    want = np.stack([np.array(Image.fromarray(a).convert("RGB").resize((70, 19), Image.BILINEAR)) for a in rgba])
    pre = P.ImagePreprocessor((19, 70), device=DEV)
    y, raw = pre(rgba, return_raw=True)
    check(y, raw, want, 0.5, 0.5)
    other_alpha = rgba.copy()
    other_alpha[..., 3] ^= 0xFF
    y2, raw2 = pre(torch.from_numpy(other_alpha).to(DEV), return_raw=True)
    assert torch.equal(y, y2) and torch.equal(raw, raw2)


def test_all_four_flip_codes():
    """Codes 0..3 in one batch: the float tensor is mirrored, the raw twin never is."""
    import phendiff_amd as P
    H, W, OH, OW = 50, 150, 19, 70
    flips = torch.tensor([0, 1, 2, 3], dtype=torch.uint8)
    want_raw = resized_reference(4, H, W, OH, OW)
    pre = P.ImagePreprocessor((OH, OW), device=DEV)
    y, raw = pre(images(4, H, W), flips=flips, return_raw=True)
    check(y, raw, want_raw, 0.5, 0.5, flips)
    plain = pre(images(4, H, W))
    assert torch.equal(plain[0], y[0]) and not torch.equal(plain[3], y[3])
    assert torch.equal(torch.flip(plain[3], [1, 2]), y[3])


def test_data_aug_on_the_fly_draws_the_codes():
    import phendiff_amd as P
    from phendiff_amd.data import draw_flips
    H, W, OH, OW = 37, 53, 16, 16
    pre = P.ImagePreprocessor((OH, OW), data_aug_on_the_fly=True, device=DEV)
    y = pre(images(3, H, W), generator=torch.Generator().manual_seed(11))
    codes = draw_flips(3, torch.Generator().manual_seed(11))
    check(y, None, resized_reference(3, H, W, OH, OW), 0.5, 0.5, codes)


def test_mixed_sizes_fill_one_batch_in_list_order():
    """Two source sizes, interleaved, as arrays and PIL images: one launch per size through out_index, slot order = list order."""
    from PIL import Image
    import phendiff_amd as P
    a, b = images(3, 50, 150, seed=5), images(2, 64, 40, seed=6)
    items = [a[0], Image.fromarray(b[0]), a[1], torch.from_numpy(b[1]), a[2]]
    order = [a[0], b[0], a[1], b[1], a[2]]
    want = np.stack([pil_resize(x, 19, 70) for x in order])
    flips = torch.tensor([1, 2, 3, 0, 1], dtype=torch.uint8)
    y, raw = P.ImagePreprocessor((19, 70), device=DEV)(items, flips=flips, return_raw=True)
    check(y, raw, want, 0.5, 0.5, flips)


def test_int_definition_keeps_the_aspect_ratio():
    import phendiff_amd as P
    pre = P.ImagePreprocessor(16, device=DEV)
    y, raw = pre(images(3, 40, 60), return_raw=True)
    assert tuple(y.shape) == (3, 3, 16, 24) and tuple(raw.shape) == (3, 16, 24, 3)
    check(y, raw, resized_reference(3, 40, 60, 16, 24), 0.5, 0.5)
    with pytest.raises(ValueError):
        pre([images(1, 40, 60)[0], images(1, 40, 40)[0]])


def test_graph_capture_follows_the_input():
    """The call is one kernel launch on the current stream: captured once, replayed with new bytes in the same input tensor."""
    import phendiff_amd as P
    H, W, OH, OW = 50, 150, 19, 70
    pre = P.ImagePreprocessor((OH, OW), device=DEV)
    x = torch.from_numpy(images(4, H, W)).to(DEV)
    flips = torch.tensor([3, 0, 1, 2], dtype=torch.uint8, device=DEV)
    pre(x, flips=flips)                      # builds the tables of this shape outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, raw = pre(x, flips=flips, return_raw=True)
    for seed in (21, 22):
        new = images(4, H, W, seed=seed)
        x.copy_(torch.from_numpy(new).to(DEV))
        graph.replay()
        check(y, raw, np.stack([pil_resize(a, OH, OW) for a in new]), 0.5, 0.5, flips.cpu())


# ---- guard bands (tests/guard_bands.py; the three properties of tests/test_gpu_guard_bands.py) ----------------------------------------------

def launch(x, n, strides, cin, H, W, OH, OW, y_f32, y_u8, out_slots, out_index=None, flips=None):
    """pd_image_preprocess through ctypes on explicit pointers and byte strides (what ImagePreprocessor does for its own tensors)."""
    import phendiff_amd._lib as L
    from phendiff_amd.data import resample_tables
    a = L.ImagePreprocessArgs(N=n, H=H, W=W, Cin=cin, OH=OH, OW=OW, out_slots=out_slots, image_stride=strides[0],
                              row_stride=strides[1], pixel_stride=strides[2], x=x.data_ptr(), mean0=0.5, mean1=0.5, mean2=0.5,
                              std0=0.5, std1=0.5, std2=0.5, y_f32=L.ptr(y_f32), y_u8=L.ptr(y_u8), out_index=L.ptr(out_index), flips=L.ptr(flips))
    keep = []
    for axis, (i, o) in (("x", (W, OW)), ("y", (H, OH))):
        if i != o:
            coef, bounds = (torch.from_numpy(t).to(DEV) for t in resample_tables(i, o))
            keep += [coef, bounds]
            setattr(a, f"coef_{axis}", coef.data_ptr())
            setattr(a, f"bounds_{axis}", bounds.data_ptr())
            setattr(a, f"ksize_{axis}", coef.shape[1])
    L.check(L.lib().pd_image_preprocess(C.byref(a), torch.cuda.current_stream().cuda_stream), "pd_image_preprocess")
    torch.cuda.synchronize()


@pytest.mark.parametrize("pad", [13, 64], ids=["odd-stride", "dword-stride"])
def test_p1_row_gaps_and_ends_never_reach_the_output(pad):
    """P1: rows `pad` bytes apart more than their width (13: every row starts at another byte offset within its dword), the gap columns
    and both ends of the allocation filled with 0xFF, then with 0x00: identical output bits, equal to the reference."""
    from guard_bands import guarded_rows
    N, H, W, OH, OW = 3, 50, 150, 19, 70
    src = torch.from_numpy(images(N, H, W))
    rs = W * 3 + pad
    view, h = guarded_rows(src.view(N * H, W * 3), rs, device=DEV, name="source rows")
    results = []
    for fill in (h.poison, h.clear):
        fill()
        y = torch.full((N, 3, OH, OW), float("nan"), device=DEV)
        raw = torch.full((N, OH, OW, 3), 0xAB, dtype=torch.uint8, device=DEV)
        launch(view, N, (H * rs, rs, 3), 3, H, W, OH, OW, y, raw, N)
        check(y, raw, resized_reference(N, H, W, OH, OW), 0.5, 0.5)
        results.append((y, raw))
    assert torch.equal(results[0][0].view(torch.int32), results[1][0].view(torch.int32)) and torch.equal(results[0][1], results[1][1])


def test_p2_outputs_are_written_completely_and_nothing_else():
    """P2: both outputs sit between canaries; every element is written (NaN / 0xAB pre-fill gone, values equal the reference), the
    canaries survive.  Flipped and out_index-scattered writes included."""
    from guard_bands import guarded
    N, H, W, OH, OW = 3, 50, 150, 19, 70
    x = torch.from_numpy(images(N, H, W)).to(DEV)
    y, hy = guarded(torch.full((N, 3, OH, OW), float("nan")), device=DEV, name="y_f32")
    raw, hr = guarded(torch.full((N, OH, OW, 3), 0xAB, dtype=torch.uint8), device=DEV, name="y_u8")
    hy.canary()
    hr.canary()
    slots = torch.tensor([2, 0, 1], dtype=torch.int32, device=DEV)
    flips = torch.tensor([3, 1, 2], dtype=torch.uint8, device=DEV)
    launch(x, N, (H * W * 3, W * 3, 3), 3, H, W, OH, OW, y, raw, N, out_index=slots, flips=flips)
    assert hy.intact() and hr.intact()
    assert not torch.isnan(y).any()
    order = [1, 2, 0]                        # slot s holds image order[s]
    want = np.asarray(resized_reference(N, H, W, OH, OW))[order]
    check(y, raw, want, 0.5, 0.5, flips.cpu()[order])


def test_p3_images_do_not_leak_into_other_slots():
    """P3: changing every byte of one image changes its own slot and no other."""
    import phendiff_amd as P
    H, W, OH, OW = 50, 150, 19, 70
    a = images(3, H, W)
    pre = P.ImagePreprocessor((OH, OW), device=DEV)
    y0, raw0 = pre(a, return_raw=True)
    b = a.copy()
    b[1] ^= 0xFF
    y1, raw1 = pre(b, return_raw=True)
    torch.cuda.synchronize()
    for s in (0, 2):
        assert torch.equal(y0[s].view(torch.int32), y1[s].view(torch.int32)) and torch.equal(raw0[s], raw1[s])
    assert not torch.equal(raw0[1], raw1[1]) and not torch.equal(y0[1], y1[1])
