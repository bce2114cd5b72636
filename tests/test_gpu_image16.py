"""pd_image_preprocess_bands16 / pd_band_histogram16 / pd_postproc_bands16 and their host surface on the GPU.  The resize is held to
EQUALITY with PIL's mode I;16 resize per band, the float tail to equality with the same fp32 torch operations on the CPU, the histogram
to np.bincount, the percentiles to the np.sort rank rule, the way back to its fp32 restatement: integer arithmetic, float64 sums in a
fixed order and correctly rounded fp32 operations leave no room for a tolerance.  Shapes are the smallest that reach every path of an
8 x 32-tile kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from image16_ref import KINDS, as_int, contents, pil_bands16, postproc16, reference16, stack16, window_normalize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 3

# source (H, W) -> output (OH, OW)
SHAPES = [((37, 53), (9, 33)),        # ragged tile in both axes
          ((16, 16), (37, 53)),       # up-scale
          ((64, 48), (64, 16)),       # vertical axis skipped
          ((33, 70), (8, 70)),        # horizontal axis skipped
          ((9, 9), (9, 9)),           # both skipped
          ((256, 256), (8, 8)),       # 32 x, ksize 65
          ((1, 1), (5, 7)),           # one-sample source
          ((32, 32), (1, 1))]         # one-sample output, at the 32 x limit (40 x 40 -> 1 x 1 is beyond it: refused, see below)
CASES = [(s, d, c) for s, d in SHAPES for c in ((5,) if s == (256, 256) else (1, 5, 32))]


def norms(c):
    return [0.1 + 0.02 * i for i in range(c)], [0.5 + 0.01 * i for i in range(c)]


def clipping_window(kind, c):
    """A per-band window inside the data's range: both ends clip."""
    if kind == "12bit":
        return [300.0 + 7 * i for i in range(c)], [3500.0 + 11 * i for i in range(c)]
    return [8000.0 + 37 * i for i in range(c)], [50000.0 + 911 * i for i in range(c)]


def check(y, raw, want_raw, lo, hi, mean, std, flips=None):
    torch.cuda.synchronize()
    want_raw = np.asarray(want_raw)
    if raw is not None:
        assert raw.dtype == torch.uint16 and tuple(raw.shape) == want_raw.shape
        got_raw, want_t = as_int(raw), torch.from_numpy(want_raw.astype(np.int32))
        assert torch.equal(got_raw, want_t), f"{int((got_raw != want_t).sum())} of {want_raw.size} resized samples differ from PIL"
    want = window_normalize(want_raw, lo, hi, mean, std, flips)
    assert y.dtype == torch.float32 and y.shape == want.shape
    got = y.cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} float32 values differ (max |d| {float((got - want).abs().max())})"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("src,dst,c", CASES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}-c{c}" for s, d, c in CASES])
def test_bit_equal_to_pil_i16_per_band(src, dst, c, kind):
    """y_u16 equals PIL per band; y_f32 equals the torch restatement, under the default window and under a per-band one that clips."""
    import phendiff_amd as P
    (H, W), (OH, OW) = src, dst
    mean, std = norms(c)
    x = stack16(kind, N, H, W, c)
    want = reference16(kind, N, H, W, c, OH, OW)
    pre = P.ImagePreprocessor((OH, OW), mean=mean, std=std, device=DEV, channels=c)
    y, raw = pre(x[..., 0] if c == 1 else x, return_raw=True)
    assert tuple(y.shape) == (N, c, OH, OW) and tuple(raw.shape) == (N, OH, OW, c)
    check(y, raw, want, 0.0, 65535.0, mean, std)
    lo, hi = clipping_window(kind, c)
    y = P.ImagePreprocessor((OH, OW), mean=mean, std=std, device=DEV, channels=c, window=(lo, hi))(x)          # float only: y_u16 null
    assert isinstance(y, torch.Tensor)
    check(y, None, want, lo, hi, mean, std)


def test_one_sample_output_beyond_the_downscale_limit_is_refused_as_on_the_8_bit_path():
    """40 x 40 -> 1 x 1 is a 40 x down-scale: both band paths refuse it the same way, and the entry point itself does."""
    import phendiff_amd as P
    import phendiff_amd._lib as L
    for dtype in (np.uint8, np.uint16):
        with pytest.raises(ValueError, match="down-scale factor above 32"):
            P.ImagePreprocessor((1, 1), device=DEV, channels=5)(np.zeros((N, 40, 40, 5), dtype))
    x, y = torch.zeros((1, 40, 40, 5), dtype=torch.int16, device=DEV), torch.zeros((1, 5, 1, 1), device=DEV)
    with pytest.raises(L.PhenDiffHipError, match="down-scale factor above 32"):
        launch16(x, 1, (40 * 40 * 10, 40 * 10, 10), 5, 40, 40, 1, 1, y, None, 1, default_vecs(5))


def test_all_four_flip_codes_mirror_the_floats_only():
    import phendiff_amd as P
    H, W, OH, OW, c = 37, 53, 9, 33, 5
    flips = torch.tensor([0, 1, 2, 3], dtype=torch.uint8)
    mean, std = norms(c)
    x = stack16("full", 4, H, W, c)
    y, raw = P.ImagePreprocessor((OH, OW), mean=mean, std=std, device=DEV, channels=c)(x, flips=flips, return_raw=True)
    check(y, raw, reference16("full", 4, H, W, c, OH, OW), 0.0, 65535.0, mean, std, flips)


def test_three_source_sizes_fill_slots_in_list_order():
    import phendiff_amd as P
    c, OH, OW = 5, 9, 33
    a, b, d = contents("full", (2, 37, 53, c), 5), contents("12bit", (2, 64, 40, c), 6), contents("saturated", (1, 20, 90, c), 7)
    items = [a[0], torch.from_numpy(b[0]), d[0], a[1], torch.from_numpy(b[1]).to(DEV)]
    order = [a[0], b[0], d[0], a[1], b[1]]
    want = np.stack([pil_bands16(x, OH, OW) for x in order])
    flips = torch.tensor([1, 2, 3, 0, 1], dtype=torch.uint8)
    mean, std = norms(c)
    y, raw = P.ImagePreprocessor((OH, OW), mean=mean, std=std, device=DEV, channels=c, window=(100, 60000))(items, flips=flips, return_raw=True)
    check(y, raw, want, 100.0, 60000.0, mean, std, flips)


def test_strided_device_view_is_read_in_place():
    """Five bands of an eight-band device tensor (pixel_stride 16 bytes > 2 * C): read through the strides, equal to the dense copy's result."""
    import phendiff_amd as P
    H, W, OH, OW = 37, 53, 9, 33
    wide = contents("full", (2, H, W, 8), 8)
    dev = torch.from_numpy(wide).to(DEV)
    view = dev[..., :5]
    assert view.stride() == (H * W * 8, W * 8, 8, 1)
    pre = P.ImagePreprocessor((OH, OW), device=DEV, channels=5)
    t, s_img, s_row, s_pix, cin = pre._strided(view)
    assert t.data_ptr() == dev.data_ptr() and (s_img, s_row, s_pix, cin) == (H * W * 16, W * 16, 16, 5)        # no copy, byte strides
    y, raw = pre(view, return_raw=True)
    check(y, raw, np.stack([pil_bands16(a[..., :5], OH, OW) for a in wide]), 0.0, 65535.0, [0.5] * 5, [0.5] * 5)
    y1, raw1 = pre(np.ascontiguousarray(wide[..., :5]), return_raw=True)
    dev.view(torch.int16)[..., 5:] = -1                      # the three bands the view leaves out never enter
    y2, raw2 = pre(view, return_raw=True)
    torch.cuda.synchronize()
    for a, b in ((y1, raw1), (y2, raw2)):
        assert torch.equal(y.view(torch.int32), a.view(torch.int32)) and torch.equal(as_int(raw), as_int(b))


def test_wide_pixel_view_under_a_steep_downscale_falls_back_to_a_dense_copy():
    """Five bands of 128-byte pixels, 1024 -> 32 columns: a staged row at that stride is beyond the LDS budget (refused before launch)."""
    import phendiff_amd as P
    wide = contents("12bit", (2, 8, 1024, 64), 9)
    view = torch.from_numpy(wide).to(DEV)[..., :5]
    pre = P.ImagePreprocessor((8, 32), device=DEV, channels=5)
    assert pre._strided(view)[3] == 128                      # the view itself is within what the entry reads in place
    y, raw = pre(view, return_raw=True)
    check(y, raw, np.stack([pil_bands16(a[..., :5], 8, 32) for a in wide]), 0.0, 65535.0, [0.5] * 5, [0.5] * 5)


def test_graph_capture_follows_the_input_and_runs_are_bitwise_equal():
    import phendiff_amd as P
    H, W, OH, OW, c = 37, 53, 9, 33, 5
    lo, hi = clipping_window("full", c)
    pre = P.ImagePreprocessor((OH, OW), device=DEV, channels=c, window=(lo, hi))
    x = torch.from_numpy(contents("full", (4, H, W, c), 11)).to(DEV)
    flips = torch.tensor([3, 0, 1, 2], dtype=torch.uint8, device=DEV)
    pre(x, flips=flips)                      # builds the tables and the window / mean / std vectors outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, raw = pre(x, flips=flips, return_raw=True)
    new = contents("full", (4, H, W, c), 21)
    x.view(torch.int16).copy_(torch.from_numpy(new.view(np.int16)).to(DEV))
    graph.replay()
    check(y, raw, np.stack([pil_bands16(a, OH, OW) for a in new]), lo, hi, [0.5] * c, [0.5] * c, flips.cpu())
    eager = [pre(x, flips=flips, return_raw=True) for _ in range(2)]
    torch.cuda.synchronize()
    for ye, re_ in eager:
        assert torch.equal(ye.view(torch.int32), y.view(torch.int32)) and torch.equal(as_int(re_), as_int(raw))


# ---- guard bands (tests/guard_bands.py): the doubled row widths brought no over-read, no stray write ----------------------------------
def launch16(x, n, strides, c, H, W, OH, OW, y_f32, y_u16, out_slots, vecs, out_index=None, flips=None):
    """pd_image_preprocess_bands16 through ctypes on explicit pointers and BYTE strides; vecs = (lo, hi, mean, std) device fp32 [C]."""
    import phendiff_amd._lib as L
    from phendiff_amd.data import resample_tables_f64
    a = L.ImagePreprocessBands16Args(N=n, H=H, W=W, C=c, OH=OH, OW=OW, out_slots=out_slots, image_stride=strides[0], row_stride=strides[1],
                                     pixel_stride=strides[2], x=x.data_ptr(), lo=vecs[0].data_ptr(), hi=vecs[1].data_ptr(),
                                     mean=vecs[2].data_ptr(), std=vecs[3].data_ptr(), y_f32=L.ptr(y_f32), y_u16=L.ptr(y_u16),
                                     out_index=L.ptr(out_index), flips=L.ptr(flips))
    keep = []
    for axis, (i, o) in (("x", (W, OW)), ("y", (H, OH))):
        if i != o:
            coef, bounds = (torch.from_numpy(t).to(DEV) for t in resample_tables_f64(i, o))
            keep += [coef, bounds]
            setattr(a, f"coef_{axis}", coef.data_ptr())
            setattr(a, f"bounds_{axis}", bounds.data_ptr())
            setattr(a, f"ksize_{axis}", coef.shape[1])
    L.check(L.lib().pd_image_preprocess_bands16(C.byref(a), torch.cuda.current_stream().cuda_stream), "pd_image_preprocess_bands16")
    torch.cuda.synchronize()


def histogram(x, n, strides, c, H, W, counts):
    """pd_band_histogram16 through ctypes; `counts` int32 [c][65536] on the device (read as unsigned), accumulated into."""
    import phendiff_amd._lib as L
    a = L.BandHistogram16Args(N=n, H=H, W=W, C=c, image_stride=strides[0], row_stride=strides[1], pixel_stride=strides[2], x=x.data_ptr(),
                              counts=counts.data_ptr())
    L.check(L.lib().pd_band_histogram16(C.byref(a), torch.cuda.current_stream().cuda_stream), "pd_band_histogram16")
    torch.cuda.synchronize()


def bincounts(a):
    """(..., C) uint16 -> int64 [C][65536]"""
    return np.stack([np.bincount(a[..., c].ravel(), minlength=65536) for c in range(a.shape[-1])])


def default_vecs(c):
    return (torch.zeros(c, device=DEV), torch.full((c,), 65535.0, device=DEV), torch.full((c,), 0.5, device=DEV), torch.full((c,), 0.5, device=DEV))


def as_i16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16))


@pytest.mark.parametrize("pad", [14, 63], ids=["odd-sample-stride", "dword-stride"])
def test_p1_row_gaps_and_ends_never_reach_the_output(pad):
    """Rows `pad` samples apart more than their width (14: 279 samples a row, every other row starts off a dword), the gap columns and both ends of the
    allocation filled with 0xFFFF, then with 0: identical output bits and histogram, equal to the references."""
    from guard_bands import guarded_rows
    H, W, OH, OW, c = 37, 53, 9, 33, 5
    src = stack16("full", N, H, W, c)
    rs = W * c + pad
    view, h = guarded_rows(as_i16(src).view(N * H, W * c), rs, device=DEV, name="source rows")
    vecs = default_vecs(c)
    results = []
    for fill in (h.poison, h.clear):
        fill()
        y = torch.full((N, c, OH, OW), float("nan"), device=DEV)
        raw = torch.full((N, OH, OW, c), 0x2B2B, dtype=torch.int16, device=DEV)
        launch16(view, N, (H * rs * 2, rs * 2, c * 2), c, H, W, OH, OW, y, raw, N, vecs)
        check(y, raw.view(torch.uint16), reference16("full", N, H, W, c, OH, OW), 0.0, 65535.0, 0.5, 0.5)
        counts = torch.zeros((c, 65536), dtype=torch.int32, device=DEV)
        histogram(view, N, (H * rs * 2, rs * 2, c * 2), c, H, W, counts)
        assert np.array_equal(counts.cpu().numpy(), bincounts(src))
        results.append((y, raw))
    assert torch.equal(results[0][0].view(torch.int32), results[1][0].view(torch.int32)) and torch.equal(results[0][1], results[1][1])


def test_p2_outputs_are_written_completely_and_nothing_else():
    """y_u16, y_f32 and counts sit between canaries; every element is written, the canaries survive.  Flipped and out_index-scattered."""
    from guard_bands import guarded
    H, W, OH, OW, c = 37, 53, 9, 33, 5
    src = stack16("full", N, H, W, c)
    x = as_i16(src).to(DEV)
    y, hy = guarded(torch.full((N, c, OH, OW), float("nan")), device=DEV, name="y_f32")
    raw, hr = guarded(torch.full((N, OH, OW, c), 0x2B2B, dtype=torch.int16), device=DEV, name="y_u16")
    counts, hc = guarded(torch.zeros((c, 65536), dtype=torch.int32), device=DEV, name="counts")
    for h in (hy, hr, hc):
        h.canary()
    slots = torch.tensor([2, 0, 1], dtype=torch.int32, device=DEV)
    flips = torch.tensor([3, 1, 2], dtype=torch.uint8, device=DEV)
    launch16(x, N, (H * W * c * 2, W * c * 2, c * 2), c, H, W, OH, OW, y, raw, N, default_vecs(c), out_index=slots, flips=flips)
    histogram(x, N, (H * W * c * 2, W * c * 2, c * 2), c, H, W, counts)
    assert hy.intact() and hr.intact() and hc.intact()
    assert not torch.isnan(y).any()
    order = [1, 2, 0]                        # slot s holds image order[s]
    want = np.asarray(reference16("full", N, H, W, c, OH, OW))[order]
    check(y, raw.view(torch.uint16), want, 0.0, 65535.0, 0.5, 0.5, flips.cpu()[order])
    assert np.array_equal(counts.cpu().numpy(), bincounts(src))


def test_p3_images_do_not_leak_into_other_slots():
    import phendiff_amd as P
    H, W, OH, OW, c = 37, 53, 9, 33, 5
    a = stack16("full", N, H, W, c)
    pre = P.ImagePreprocessor((OH, OW), device=DEV, channels=c)
    y0, raw0 = pre(a, return_raw=True)
    b = a.copy()
    b[1] = 0xFFFF
    y1, raw1 = pre(b, return_raw=True)
    torch.cuda.synchronize()
    for s in (0, 2):
        assert torch.equal(y0[s].view(torch.int32), y1[s].view(torch.int32)) and torch.equal(as_int(raw0[s]), as_int(raw1[s]))
    assert bool((as_int(raw1[1]) == 65535).all()) and not torch.equal(y0[1], y1[1])


# ---- histogram and percentiles ------------------------------------------------------------------------------------------------------
def test_histogram_equals_bincount_accumulates_and_reads_strided_views():
    a, b = contents("full", (2, 64, 64, 5), 31), contents("12bit", (1, 1, 1, 5), 32)
    counts = torch.zeros((5, 65536), dtype=torch.int32, device=DEV)
    histogram(as_i16(a).to(DEV), 2, (64 * 64 * 10, 64 * 10, 10), 5, 64, 64, counts)
    assert np.array_equal(counts.cpu().numpy(), bincounts(a))
    histogram(as_i16(b).to(DEV), 1, (10, 10, 10), 5, 1, 1, counts)                   # a 1 x 1 image, into the same counts: the sum
    assert np.array_equal(counts.cpu().numpy(), bincounts(a) + bincounts(b))
    histogram(as_i16(a).to(DEV), 2, (64 * 64 * 10, 64 * 10, 10), 5, 64, 64, counts)
    assert np.array_equal(counts.cpu().numpy(), 2 * bincounts(a) + bincounts(b))
    # bands 2..4 of an eight-band tensor, rows with a gap, the second image alone: pointer offset + strides
    wide = contents("full", (2, 40, 70, 8), 33)
    dev = as_i16(wide).to(DEV)
    counts.zero_()
    histogram(dev[1, :, 3:, 2:5], 1, (0, 70 * 16, 16), 3, 40, 67, counts[:3])
    assert np.array_equal(counts[:3].cpu().numpy(), bincounts(wide[1, :, 3:, 2:5])) and int(counts[3:].abs().sum()) == 0


def test_histogram_of_all_equal_bands_is_exact():
    """The contention worst case (a microscopy background): every sample of a band holds one value, one band in each half of a counter word."""
    a = np.empty((1, 256, 256, 2), np.uint16)
    a[..., 0], a[..., 1] = 777, 40000
    counts = torch.zeros((2, 65536), dtype=torch.int32, device=DEV)
    histogram(as_i16(a).to(DEV), 1, (256 * 256 * 4, 256 * 4, 4), 2, 256, 256, counts)
    got = counts.cpu().numpy()
    assert got[0, 777] == 65536 and got[1, 40000] == 65536 and int(got.sum()) == 2 * 65536
    a[0, 100, 100, 0] = 33545                              # 777 + 32768: the other half of the same counter word
    counts.zero_()
    histogram(as_i16(a).to(DEV), 1, (256 * 256 * 4, 256 * 4, 4), 2, 256, 256, counts)
    assert np.array_equal(counts.cpu().numpy(), bincounts(a))


@pytest.mark.parametrize("q", [(0.1, 99.9), (0, 100)])
def test_band_percentiles_equal_the_sort_rank_rule(q):
    import phendiff_amd as P
    from phendiff_amd.data import percentile_rank
    a = contents("12bit", (2, 64, 64, 5), 41)
    a[..., 3] = 1234                                         # a constant band: hi = lo + 1
    b = contents("full", (1, 20, 30, 5), 42)
    b[..., 3] = 1234
    lo, hi = P.band_percentiles([a[0], b[0], a[1]], q=q, channels=5, device=DEV)
    assert lo.dtype == hi.dtype == torch.float32 and lo.is_cuda and tuple(lo.shape) == tuple(hi.shape) == (5,)
    for c in range(5):
        band = np.sort(np.concatenate([a[..., c].ravel(), b[..., c].ravel()]))
        want_lo, want_hi = (float(band[percentile_rank(band.size, v) - 1]) for v in q)
        if c == 3:
            assert (want_lo, want_hi) == (1234.0, 1234.0)
            want_hi = 1235.0
        assert (float(lo[c]), float(hi[c])) == (want_lo, want_hi), c
    # the device tensors are a window as they are
    mean, std = norms(5)
    pre = P.ImagePreprocessor((9, 33), mean=mean, std=std, device=DEV, channels=5, window=(lo, hi))
    assert pre._window_vectors()[0].data_ptr() == lo.data_ptr() and pre._window_vectors()[1].data_ptr() == hi.data_ptr()
    check(pre(a), None, np.stack([pil_bands16(x, 9, 33) for x in a]), lo.cpu(), hi.cpu(), mean, std)


# ---- the way back -------------------------------------------------------------------------------------------------------------------
def test_round_trip_restores_the_resized_samples():
    import phendiff_amd as P
    H, W, OH, OW, c = 37, 53, 9, 33, 5
    mean, std = norms(c)
    x = stack16("full", N, H, W, c)
    pre = P.ImagePreprocessor((OH, OW), mean=mean, std=std, device=DEV, channels=c)
    y, raw = pre(x, return_raw=True)
    back = pre.restore(y)
    torch.cuda.synchronize()
    assert back.dtype == torch.uint16 and tuple(back.shape) == (N, OH, OW, c)
    # v / 65535 is rounded to fp32, and so are the four operations back: at most one count off
    assert int((as_int(back) - as_int(raw)).abs().max()) <= 1
    assert torch.equal(as_int(back), postproc16(y.cpu(), 0.0, 65535.0, mean, std))
    # a clipping window, values outside [0, 1] after de-normalisation, NaN and infinities
    lo, hi = clipping_window("full", c)
    z = torch.randn(2, c, 16, 40, generator=torch.Generator().manual_seed(3)) * 1.5
    z[0, 0, 0, :6] = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, 1e30, -1e30])
    got = P.restore_bands16(z.to(DEV), (lo, hi), mean, std)
    torch.cuda.synchronize()
    want = postproc16(z, lo, hi, mean, std)
    assert torch.equal(as_int(got), want)
    assert int(want[0, 0, 0, 0]) == int(lo[0]) and int(want.min()) >= 8000 and int(want.max()) <= 50000 + 911 * 4
