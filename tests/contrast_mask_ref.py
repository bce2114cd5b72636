"""float64 numpy restatement of the three mask kernels (include/phendiff_hip.h: pd_class_contrast, pd_contrast_mask, pd_mask_blend), with
the roundings the header names: the mean of a sample is summed and divided in float64 and rounded to fp32 once, ``limit = ratio * mean``
is an fp32 product; everything else stays in float64.  A plain module: imported by the host and the GPU tests."""
import math

import numpy as np


def class_contrast_ref(a, b, acc=None):
    """``(acc or 0) + sum_c |a - b| / C`` in float64.  a, b: (B, C, H, W); acc: (B, H, W) or None (the first draw)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.abs(a - b).sum(axis=1) / a.shape[1]
    return m if acc is None else np.asarray(acc, dtype=np.float64) + m


def contrast_mask_ref(acc, ratio):
    """(mask uint8 (B, H, W), map float64 (B, H, W), stats float32 (B, 3)) of an accumulated contrast ``acc`` (B, H, W)."""
    acc = np.asarray(acc, dtype=np.float64)
    B = acc.shape[0]
    n = acc[0].size
    mask, cmap, stats = np.zeros(acc.shape, np.uint8), np.zeros(acc.shape, np.float64), np.zeros((B, 3), np.float32)
    with np.errstate(all="ignore"):
        for s in range(B):
            flat = acc[s].ravel()
            total = math.fsum(flat) if np.isfinite(flat).all() else float(flat.sum())
            mean = np.float32(total / n)
            limit = np.float32(np.float64(np.float32(ratio)) * np.float64(mean))      # (exact in float64: the fp32 product's rounding)
            if np.isfinite(limit) and limit > 0:
                cmap[s] = np.minimum(acc[s], np.float64(limit)) / np.float64(limit)
                mask[s] = cmap[s] > 0.5
            stats[s] = (mean, limit, np.float32(int(mask[s].sum()) / n))
    return mask, cmap, stats


def mask_blend_ref(x, keep, mask):
    """``where(mask, x, keep)``, the mask (B, H, W) broadcast over the channels."""
    return np.where(np.asarray(mask)[:, None] != 0, x, keep)
