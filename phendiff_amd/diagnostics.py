"""Diagnostics.

Over a launch plan's activation buffers (every activation of a plan owns its buffer, so after one evaluation the
whole forward can be inspected): the per-block max |activation| that makes an fp16 overflow a NAMED failure instead of a NaN at
the output (fp16 is BASELINE configs[4]'s dtype: `--mixed_precision fp16`, img2img_comparison.py:56-59).

Over an inverted or regenerated batch that stays on the device (``pd_sample_stats``, csrc/sample_stats.hip): ``check_gaussianity`` -- the
reference's ``check_Gaussianity`` (utils_Img2Img.py:79-93: per-sample mean, std, the 100-bin histogram on (-3, 3) and the p-value of
D'Agostino-Pearson's K^2 test) -- and ``sample_distances`` (``Lp_loss``, :245-270, for p = 1, 2, inf, plus MSE and PSNR).  Only
B x (10 + bins) numbers cross to the host; ``normaltest_from_moments`` turns the moments into the test there.

Between a source batch and its transfer (``pd_ssim``, csrc/ssim.hip): ``sample_ssim`` -- SSIM and multi-scale SSIM per sample in fp64, what
image-to-image work reports for "everything but the phenotype stayed"; ``ssim_maps_means`` is the device-side call under it."""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L

FP16_MAX = 65504.0


def activation_absmax(plan) -> dict:
    """{"<index>.<kind>.<block name>.<tensor>": max |x|} over every floating-point buffer on the plan's tape (block inputs /
    intermediates / outputs as the block emitters recorded them), in forward order.  Synchronises the device."""
    out = {}
    for i, rec in enumerate(plan.tape):
        for k, v in vars(rec).items():
            if torch.is_tensor(v) and v.is_floating_point() and v.numel() > 0:
                out[f"{i:03d}.{rec.kind}.{getattr(rec, 'name', '')}.{k}"] = float(v.float().abs().max())
    return out


def assert_finite_activations(plans, limit: float = FP16_MAX, what: str = "") -> dict:
    """Raise naming the FIRST buffer (forward order) that holds a NaN / Inf or exceeds ``limit``; returns the merged report plus
    ``"__max__": (name, value)`` of the largest entry."""
    report = {}
    for pi, plan in enumerate(plans if isinstance(plans, (list, tuple)) else [plans]):
        for k, v in activation_absmax(plan).items():
            report[f"p{pi}.{k}"] = v
    for k, v in report.items():
        if not math.isfinite(v) or v > limit:
            top = sorted(((x, n) for n, x in report.items() if math.isfinite(x)), reverse=True)[:5]
            raise AssertionError(f"{what}: activation overflow at {k}: max |x| = {v} (limit {limit}); largest finite before it: {top}")
    name = max(report, key=report.get) if report else None
    report["__max__"] = (name, report.get(name))
    return report


# ------------------------------------------------------------------------------------------------ pd_sample_stats
CHUNK = L.SAMPLE_STATS_CHUNK            # elements of a sample per workgroup
MAX_BINS = L.SAMPLE_STATS_MAX_BINS      # what the LDS histogram holds
STATS_FIELDS = L.SAMPLE_STATS_FIELDS    # the columns of the stats row
_DTYPES = {torch.float32: L.PD_F32, torch.bfloat16: L.PD_BF16, torch.float16: L.PD_F16}


def _as_rows(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.PhenDiffHipError(f"{what} must live on an MI355X device (no CPU fallback)")
    if t.dtype not in _DTYPES:
        raise TypeError(f"{what}: dtype {t.dtype} (float32, bfloat16 or float16)")
    if t.dim() < 1 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous (B, ...) tensor")


def sample_stats(x, y=None, edges=None, stream=None):
    """One ``pd_sample_stats`` call on ``x`` (B, ...): returns ``(stats, hist)`` ON THE DEVICE -- ``stats`` float64 [B, 10] (columns
    ``STATS_FIELDS``), ``hist`` int32 [B, bins] holding the uint32 counts (None without ``edges``).  ``y``: ``x.shape`` or ``x.shape[1:]``;
    ``edges``: bins + 1 ascending values (any sequence; float64 on the device).  ``stream``: a ``torch.cuda.Stream`` (default: the current
    one); nothing synchronises."""
    _as_rows(x, "x")
    dev = x.device
    B = x.shape[0]
    n = x.numel() // B if B else 0
    stride = 0
    if y is not None:
        _as_rows(y, "y")
        if y.device != dev or y.dtype != x.dtype:
            raise ValueError(f"y ({y.dtype} on {y.device}) must share x's dtype and device ({x.dtype} on {dev})")
        if tuple(y.shape) == tuple(x.shape):
            stride = n
        elif tuple(y.shape) != tuple(x.shape[1:]):
            raise ValueError(f"y.shape={tuple(y.shape)} should be equal to either x.shape or x.shape[1:] (x.shape={tuple(x.shape)})")
    bins = 0
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        if edges is not None:
            e = torch.as_tensor(np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1)))
            bins = e.numel() - 1
            if bins < 1:
                raise ValueError("edges: at least two values")
            edges_dev = e.to(dev)
        lib = L.lib()
        ws_bytes = lib.pd_sample_stats_workspace(B, n, bins)
        ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.float64, device=dev)
        stats = torch.empty((B, len(STATS_FIELDS)), dtype=torch.float64, device=dev)
        hist = torch.empty((B, bins), dtype=torch.int32, device=dev) if bins else None
        a = L.SampleStatsArgs(dtype=_DTYPES[x.dtype], bins=bins, B=B, n=n, y_sample_stride=stride, x=x.data_ptr(), y=L.ptr(y),
                              edges=edges_dev.data_ptr() if bins else None, stats=stats.data_ptr(), hist=L.ptr(hist),
                              workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
        L.check(lib.pd_sample_stats(C.byref(a), torch.cuda.current_stream(dev).cuda_stream), "pd_sample_stats")
    return stats, hist


def normaltest_from_moments(n, m2, m3, m4):
    """D'Agostino-Pearson's omnibus test of normality from the sample size and the central moments sum(d^k) / n: ``(K2, pvalue)`` as
    ``scipy.stats.normaltest`` returns them from the raw data.  K2 = Z1^2 + Z2^2 with Z1 the skewness test's statistic (D'Agostino 1970: the
    sample skewness through Johnson's S_U transform) and Z2 the kurtosis test's (Anscombe & Glynn 1983: the sample kurtosis through a
    Wilson-Hilferty cube root); under normality K2 ~ chi^2 with 2 degrees of freedom, whose survival function is exp(-K2 / 2).
    Plain float64 Python.  n < 8 raises ValueError (the skewness test is not defined there); m2 == 0 gives (nan, nan)."""
    n = int(n)
    if n < 8:
        raise ValueError(f"normaltest needs at least 8 observations; n = {n}")
    m2, m3, m4 = float(m2), float(m3), float(m4)
    if not (m2 > 0.0) or not math.isfinite(m2) or not math.isfinite(m3) or not math.isfinite(m4):
        return float("nan"), float("nan")
    n = float(n)
    # skewness: Z1
    g1 = m3 / m2 ** 1.5
    y = g1 * math.sqrt(((n + 1.0) * (n + 3.0)) / (6.0 * (n - 2.0)))
    beta2 = 3.0 * (n * n + 27.0 * n - 70.0) * (n + 1.0) * (n + 3.0) / ((n - 2.0) * (n + 5.0) * (n + 7.0) * (n + 9.0))
    w2 = -1.0 + math.sqrt(2.0 * (beta2 - 1.0))
    delta = 1.0 / math.sqrt(0.5 * math.log(w2))
    alpha = math.sqrt(2.0 / (w2 - 1.0))
    if y == 0.0:
        y = 1.0      # (SciPy's convention for an exactly symmetric sample)
    z1 = delta * math.log(y / alpha + math.sqrt((y / alpha) ** 2 + 1.0))
    # kurtosis: Z2
    b2 = m4 / (m2 * m2)
    mean_b2 = 3.0 * (n - 1.0) / (n + 1.0)
    var_b2 = 24.0 * n * (n - 2.0) * (n - 3.0) / ((n + 1.0) * (n + 1.0) * (n + 3.0) * (n + 5.0))
    x = (b2 - mean_b2) / math.sqrt(var_b2)
    sqrt_beta1 = 6.0 * (n * n - 5.0 * n + 2.0) / ((n + 7.0) * (n + 9.0)) * math.sqrt((6.0 * (n + 3.0) * (n + 5.0)) / (n * (n - 2.0) * (n - 3.0)))
    a = 6.0 + 8.0 / sqrt_beta1 * (2.0 / sqrt_beta1 + math.sqrt(1.0 + 4.0 / (sqrt_beta1 ** 2)))
    term1 = 1.0 - 2.0 / (9.0 * a)
    denom = 1.0 + x * math.sqrt(2.0 / (a - 4.0))
    if denom == 0.0:
        return float("nan"), float("nan")
    term2 = math.copysign(((1.0 - 2.0 / a) / abs(denom)) ** (1.0 / 3.0), denom)
    z2 = (term1 - term2) / math.sqrt(2.0 / (9.0 * a))
    k2 = z1 * z1 + z2 * z2
    return k2, math.exp(-0.5 * k2)


@dataclass
class GaussianityReport:
    """Per-sample arrays (numpy, length B): ``mean``, ``std`` (unbiased, n - 1: torch's ``.std()``), ``skewness`` m3 / m2^1.5, ``kurtosis``
    m4 / m2^2 - 3 (excess), ``statistic`` / ``pvalue`` of the K^2 normality test, ``minimum``, ``maximum``, ``nonfinite`` (int64), ``hist``
    int64 [B, bins] over ``edges`` (float64, bins + 1: np.histogram's), and ``n`` / ``shape`` of the input."""
    n: int
    shape: tuple
    mean: np.ndarray
    std: np.ndarray
    skewness: np.ndarray
    kurtosis: np.ndarray
    statistic: np.ndarray
    pvalue: np.ndarray
    minimum: np.ndarray
    maximum: np.ndarray
    nonfinite: np.ndarray
    hist: np.ndarray
    edges: np.ndarray

    def __str__(self):
        lines = [f"Checking Gausianity of components of tensor of shape {tuple(self.shape)}..."]
        for i in range(len(self.mean)):
            lines.append(f"Gaussian(?) {i}: mean={self.mean[i]}, std={self.std[i]}; "
                         f"2-sided Χ² probability for the normality hypothesis: {self.pvalue[i]}")
        return "\n".join(lines)


@torch.no_grad()
def check_gaussianity(gauss, bins: int = 100, range=(-3.0, 3.0), stream=None) -> GaussianityReport:
    """``check_Gaussianity`` (utils_Img2Img.py:79-93) of a (B, ...) batch on the device, e.g. ``DDIBGraph.inverted``: per sample the mean,
    the standard deviation, the ``bins``-bin histogram on ``range`` (the counts ``plt.hist`` / ``np.histogram`` would draw; no figure is
    made) and the normality test's p-value.  ``str(report)`` gives the reference's printed lines.  Synchronises ``stream``."""
    bins = int(bins)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins = {bins}: 1 .. {MAX_BINS}")
    lo, hi = float(range[0]), float(range[1])
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"range = {range}: finite, lower < upper")
    edges = np.linspace(lo, hi, bins + 1)
    stats_dev, hist_dev = sample_stats(gauss, edges=edges, stream=stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(gauss.device)):
        st = stats_dev.cpu().numpy()
        hist = hist_dev.cpu().numpy().view(np.uint32).astype(np.int64)
    n = gauss.numel() // gauss.shape[0]
    col = {k: st[:, i] for i, k in enumerate(STATS_FIELDS)}
    m2 = col["m2"]
    with np.errstate(divide="ignore", invalid="ignore"):
        std = np.sqrt(m2 * (n / (n - 1.0))) if n > 1 else np.full_like(m2, np.nan)
        skew = col["m3"] / m2 ** 1.5
        kurt = col["m4"] / (m2 * m2) - 3.0
    if n >= 8:
        k2p = np.array([normaltest_from_moments(n, a, b, c) for a, b, c in zip(m2, col["m3"], col["m4"])], dtype=np.float64).reshape(-1, 2)
    else:
        k2p = np.full((len(m2), 2), np.nan)
    return GaussianityReport(n=n, shape=tuple(gauss.shape), mean=col["sum"] / n, std=std, skewness=skew, kurtosis=kurt, statistic=k2p[:, 0],
                             pvalue=k2p[:, 1], minimum=col["min"].copy(), maximum=col["max"].copy(),
                             nonfinite=col["nonfinite"].astype(np.int64), hist=hist, edges=edges)


@torch.no_grad()
def sample_distances(x, y, data_range: float = 2.0, stream=None) -> dict:
    """Per-sample distances between ``x`` (B, ...) and ``y`` (``x.shape`` or ``x.shape[1:]``: ``Lp_loss``'s assertion, utils_Img2Img.py:245-270)
    on the device, accumulated in fp64: ``{"l1", "l2", "linf"}`` = ``torch.linalg.vector_norm(x - y, ord=1 / 2 / inf)`` over each sample,
    ``"mse"`` and ``"psnr"`` = 10 log10(data_range^2 / mse) (data_range 2.0: images in [-1, 1]; inf where mse is 0).  numpy float64 [B].
    Synchronises ``stream``."""
    if y is None:
        raise ValueError("sample_distances needs y")
    stats_dev, _ = sample_stats(x, y=y, stream=stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(x.device)):
        st = stats_dev.cpu().numpy()
    n = x.numel() // x.shape[0]
    i1, i2, im = (STATS_FIELDS.index(k) for k in ("err_l1", "err_sq", "err_max"))
    mse = st[:, i2] / n
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(float(data_range) ** 2 / mse)
    return {"l1": st[:, i1].copy(), "l2": np.sqrt(st[:, i2]), "linf": st[:, im].copy(), "mse": mse, "psnr": psnr}


# ------------------------------------------------------------------------------------------------ pd_ssim
SSIM_MAX_WIN = L.CONSTANTS["PD_SSIM_MAX_WIN"]
SSIM_MAX_LEVELS = L.CONSTANTS["PD_SSIM_MAX_LEVELS"]
SSIM_K1, SSIM_K2 = 0.01, 0.03
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli & Bovik 2003


def gaussian_window(win_size: int = 11, sigma: float = 1.5) -> np.ndarray:
    """The ``win_size`` taps g[i] = exp(-(i - (win_size - 1) / 2)^2 / (2 sigma^2)) divided by their sum, numpy float64: the separable window
    of SSIM (11, 1.5: Wang et al. 2004).  ``win_size`` odd, 3 .. 33; ``sigma`` finite and positive."""
    win_size, sigma = int(win_size), float(sigma)
    if win_size % 2 != 1 or not 3 <= win_size <= SSIM_MAX_WIN:
        raise ValueError(f"win_size = {win_size}: odd, 3 .. {SSIM_MAX_WIN}")
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma = {sigma}: finite and positive")
    d = np.arange(win_size, dtype=np.float64) - (win_size - 1) / 2.0
    g = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return g / g.sum()


def _ssim_operands(x, y, levels, win_size):
    """The checks of ``ssim_maps_means``, what the tensors ARE before where they live (so each is reported on any box): returns y's sample
    stride (C * H * W, or 0 for one shared y)."""
    for t, what in ((x, "x"), (y, "y")):
        if not torch.is_tensor(t):
            raise L.PhenDiffHipError(f"{what} must be a tensor on an MI355X device (no CPU fallback)")
        if t.dtype not in _DTYPES:
            raise TypeError(f"{what}: dtype {t.dtype} (float32, bfloat16 or float16)")
    if x.dim() != 4 or not x.is_contiguous() or not y.is_contiguous():
        raise ValueError(f"x must be a contiguous (B, C, H, W) tensor and y a contiguous one; x.shape={tuple(x.shape)}")
    if y.dtype != x.dtype:
        raise ValueError(f"y ({y.dtype}) must share x's dtype ({x.dtype})")
    B, Cc, H, W = x.shape
    if tuple(y.shape) == tuple(x.shape):
        stride = Cc * H * W
    elif tuple(y.shape) == tuple(x.shape[1:]):
        stride = 0
    else:
        raise ValueError(f"y.shape={tuple(y.shape)} should be equal to either x.shape or x.shape[1:] (x.shape={tuple(x.shape)})")
    if not 1 <= levels <= SSIM_MAX_LEVELS:
        raise ValueError(f"levels = {levels}: 1 .. {SSIM_MAX_LEVELS}")
    if min(B, Cc, H, W) < 1:
        raise ValueError(f"x.shape={tuple(x.shape)}: every dimension must be positive")
    if min(H, W) >> (levels - 1) < win_size:
        raise ValueError(f"images of {H} x {W} are too small for win_size = {win_size} at levels = {levels}: "
                         f"min(H, W) must be at least {win_size << (levels - 1)}")
    if not x.is_cuda or not y.is_cuda:
        raise L.PhenDiffHipError("x and y must live on an MI355X device (no CPU fallback)")
    if y.device != x.device:
        raise ValueError(f"y (on {y.device}) must share x's device ({x.device})")
    return stride


def ssim_maps_means(x, y, data_range: float = 2.0, levels: int = 1, win_size: int = 11, sigma: float = 1.5, stream=None):
    """One ``pd_ssim`` call on ``x`` (B, C, H, W) and ``y`` (``x.shape`` or ``x.shape[1:]``): returns float64 [B, C, levels, 2] ON THE
    DEVICE -- per sample, channel and scale the mean of the SSIM map ([..., 0]) and of its contrast-structure factor ([..., 1]) over the
    valid positions of a ``win_size``-tap Gaussian window (no padding); scale s is the 2x2 mean of scale s - 1.  All arithmetic is fp64.
    ``stream``: a ``torch.cuda.Stream`` (default: the current one); nothing synchronises, so the call can be captured."""
    levels, win_size, data_range = int(levels), int(win_size), float(data_range)
    taps = gaussian_window(win_size, sigma)
    if not (math.isfinite(data_range) and data_range > 0.0):
        raise ValueError(f"data_range = {data_range}: finite and positive")
    stride = _ssim_operands(x, y, levels, win_size)
    dev = x.device
    B, Cc, H, W = x.shape
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        lib = L.lib()
        ws_bytes = lib.pd_ssim_workspace(B, Cc, H, W, levels)
        ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.float64, device=dev)
        out = torch.empty((B, Cc, levels, 2), dtype=torch.float64, device=dev)
        a = L.SsimArgs(dtype=_DTYPES[x.dtype], C=Cc, H=H, W=W, win=win_size, levels=levels, B=B, y_sample_stride=stride,
                       c1=(SSIM_K1 * data_range) ** 2, c2=(SSIM_K2 * data_range) ** 2, x=x.data_ptr(), y=y.data_ptr(), out=out.data_ptr(),
                       workspace=ws.data_ptr(), workspace_bytes=ws_bytes, **{f"w{i}": float(g) for i, g in enumerate(taps)})
        L.check(lib.pd_ssim(C.byref(a), torch.cuda.current_stream(dev).cuda_stream), "pd_ssim")
    return out


def ms_ssim_weights(levels: int, weights=None) -> np.ndarray:
    """The ``levels`` exponents of MS-SSIM, float64: the first ``levels`` of ``MS_SSIM_WEIGHTS`` renormalised to sum 1, or ``weights`` as given
    (``levels`` positive finite numbers)."""
    if weights is None:
        w = np.asarray(MS_SSIM_WEIGHTS[:levels], dtype=np.float64)
        return w / w.sum() if levels < len(MS_SSIM_WEIGHTS) else w
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size != levels or not np.all(np.isfinite(w)) or not np.all(w > 0.0):
        raise ValueError(f"weights: {levels} positive numbers, one per level; got {weights!r}")
    return w


@torch.no_grad()
def sample_ssim(x, y, data_range: float = 2.0, levels: int = 1, win_size: int = 11, sigma: float = 1.5, weights=None, stream=None) -> dict:
    """Structural similarity between ``x`` (B, C, H, W) and ``y`` (``x.shape`` or ``x.shape[1:]``) on the device, in fp64 (``pd_ssim``):
    ``"ssim"`` [B] the channel mean of ``"ssim_per_channel"`` [B, C] (the mean SSIM map at full resolution: Wang et al. 2004, Gaussian
    window of ``win_size`` taps and ``sigma``, valid positions only, C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2; data_range 2.0:
    images in [-1, 1]), ``"cs_per_channel"`` [B, C, levels] the mean contrast-structure factor per scale.  With ``levels`` > 1 also
    ``"ms_ssim"`` [B] and ``"ms_ssim_per_channel"`` [B, C]: prod_{s < levels - 1} max(cs_s, 0)^w_s * max(ssim_{levels - 1}, 0)^w_{levels - 1}
    over the 2x2-mean pyramid, ``weights`` defaulting to the first ``levels`` of (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) renormalised to
    sum 1.  min(H, W) must be at least win_size * 2^(levels - 1).  numpy float64.  Synchronises ``stream``."""
    levels = int(levels)
    w = ms_ssim_weights(levels, weights) if 1 <= levels <= SSIM_MAX_LEVELS else None
    means_dev = ssim_maps_means(x, y, data_range=data_range, levels=levels, win_size=win_size, sigma=sigma, stream=stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(x.device)):
        m = means_dev.cpu().numpy()
    out = {"ssim": m[:, :, 0, 0].mean(axis=1), "ssim_per_channel": m[:, :, 0, 0].copy(), "cs_per_channel": m[:, :, :, 1].copy()}
    if levels > 1:
        factors = np.concatenate([m[:, :, :levels - 1, 1], m[:, :, levels - 1:, 0]], axis=2)      # cs of every scale but the last, ssim of the last
        # (np.maximum passes a NaN on: a sample with a NaN stays NaN)
        out["ms_ssim_per_channel"] = np.prod(np.maximum(factors, 0.0) ** w, axis=2)
        out["ms_ssim"] = out["ms_ssim_per_channel"].mean(axis=1)
    return out
