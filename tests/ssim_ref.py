"""SSIM and multi-scale SSIM restated in torch float64 on the CPU -- the reference the pd_ssim tests compare with.  Self-contained: imports
nothing from phendiff_amd.

Definition (Wang, Bovik, Sheikh & Simoncelli 2004; Wang, Simoncelli & Bovik 2003; the conventions of pytorch_msssim):
  * window: win odd taps g[i] = exp(-(i - (win - 1) / 2)^2 / (2 sigma^2)) / sum, float64; the 2-D window is their outer product
  * VALID filtering (no padding) of x, y, x^2, y^2, xy per channel: mx, my, exx, eyy, exy on (H - win + 1) x (W - win + 1) positions
  * vx = exx - mx^2, vy = eyy - my^2, vxy = exy - mx my;  C1 = (0.01 R)^2, C2 = (0.03 R)^2
  * cs = (2 vxy + C2) / (vx + vy + C2),  ssim = cs (2 mx my + C1) / (mx^2 + my^2 + C1)
  * per (sample, channel, scale) the means of ssim and cs over the valid positions; scale s + 1 = F.avg_pool2d(scale s, 2)
  * SSIM of a sample: channel mean of the scale-0 ssim mean
  * MS-SSIM per channel: prod_{s < L - 1} max(cs_s, 0)^w_s * max(ssim_{L - 1}, 0)^w_{L - 1}; of a sample: the channel mean"""
import numpy as np
import torch
import torch.nn.functional as F

K1, K2 = 0.01, 0.03
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(win=11, sigma=1.5):
    """The taps, numpy float64."""
    d = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    g = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return g / g.sum()


def _filter(t, g):
    """Valid depthwise filtering of [B, C, H, W] float64 with the outer product of the taps."""
    C = t.shape[1]
    k = torch.outer(g, g).expand(C, 1, -1, -1).contiguous()
    return F.conv2d(t, k, groups=C)


def ssim_cs_maps(x, y, data_range=2.0, win=11, sigma=1.5):
    """(ssim, cs) maps, float64 [B, C, H - win + 1, W - win + 1], of float64 x and y [B, C, H, W]."""
    assert x.dtype == torch.float64 and y.dtype == torch.float64 and x.shape == y.shape and x.dim() == 4
    g = torch.from_numpy(window(win, sigma))
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    mx, my = _filter(x, g), _filter(y, g)
    vx = _filter(x * x, g) - mx * mx
    vy = _filter(y * y, g) - my * my
    vxy = _filter(x * y, g) - mx * my
    cs = (2.0 * vxy + c2) / (vx + vy + c2)
    return cs * (2.0 * mx * my + c1) / (mx * mx + my * my + c1), cs


def maps_means(x, y, data_range=2.0, levels=1, win=11, sigma=1.5):
    """float64 numpy [B, C, levels, 2]: mean ssim, mean cs per scale.  x: [B, C, H, W] of any float dtype (widened exactly); y: x's shape or
    one sample [C, H, W] shared by all."""
    x = x.detach().cpu().to(torch.float64)
    y = y.detach().cpu().to(torch.float64)
    if y.dim() == 3:
        y = y.unsqueeze(0).expand_as(x)
    assert min(x.shape[2], x.shape[3]) >> (levels - 1) >= win
    out = []
    for s in range(levels):
        if s:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        ssim, cs = ssim_cs_maps(x.contiguous(), y.contiguous(), data_range, win, sigma)
        out.append(torch.stack([ssim.mean(dim=(2, 3)), cs.mean(dim=(2, 3))], dim=-1))
    return torch.stack(out, dim=2).numpy()


def weights_of(levels, weights=None):
    if weights is None:
        w = np.asarray(WEIGHTS[:levels], dtype=np.float64)
        return w / w.sum() if levels < 5 else w
    return np.asarray(weights, dtype=np.float64)


def scores(means, weights=None):
    """From maps_means' array: {"ssim" [B], "ssim_per_channel" [B, C], "cs_per_channel" [B, C, L]} and, for L > 1, "ms_ssim" [B] and
    "ms_ssim_per_channel" [B, C]."""
    L = means.shape[2]
    out = {"ssim_per_channel": means[:, :, 0, 0], "ssim": means[:, :, 0, 0].mean(axis=1), "cs_per_channel": means[:, :, :, 1]}
    if L > 1:
        w = weights_of(L, weights)
        ms = np.ones(means.shape[:2])
        for s in range(L):
            factor = means[:, :, s, 1] if s < L - 1 else means[:, :, s, 0]
            ms = ms * np.maximum(factor, 0.0) ** w[s]
        out["ms_ssim_per_channel"] = ms
        out["ms_ssim"] = ms.mean(axis=1)
    return out
