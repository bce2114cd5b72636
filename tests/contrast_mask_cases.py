"""The seeded inputs the host and the GPU tests of the mask kernels share, and their float64 reference (computed once per case).

A case is (B, C, H, W, num_maps).  Per noise draw the two "noise predictions" a and b are small Gaussians; a also carries a per-sample
"hot" disc (a plateau of height 1 with a soft edge, its centre and radius different for every sample, the same in every draw and channel):
the accumulated contrast is ~ num_maps inside the disc and ~ 0.05 num_maps outside, so no mask is empty or full and few pixels lie near
the threshold (tests/test_host_contrast_mask.py asserts the margin; if a seed violates it, change SEED here)."""
import functools

import numpy as np

from contrast_mask_ref import class_contrast_ref, contrast_mask_ref

SEED = 20251
RATIO = 3.0
NOISE_STD = 0.03
EDGE = 0.35      # width of the disc's edge in pixels

# 4087 pixels: more than one chunk of PD_CONTRAST_MASK_CHUNK = 2048 pixels per sample and not a multiple of it
CASES = [(1, 1, 5, 7, 1),          # 35 pixels: a quad tail
         (3, 1, 5, 7, 2),          # sample boundaries fall inside a quad
         (3, 3, 8, 8, 3),
         (2, 5, 16, 16, 10),
         (2, 32, 4, 4, 2),
         (3, 1, 67, 61, 2)]
GUARD_CASES = [CASES[0], CASES[5]]      # the 35-pixel case and the 67 x 61 one


def case_id(case):
    return "B{}-C{}-{}x{}-maps{}".format(*case)


def hot_region(B, H, W, rng):
    """(B, H, W) float64 in [0, 1]: per sample a disc with a soft edge."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((B, H, W))
    for s in range(B):
        cy, cx = rng.uniform(0.3, 0.7) * (H - 1), rng.uniform(0.3, 0.7) * (W - 1)
        r0 = rng.uniform(0.22, 0.33) * min(H, W) + 0.5
        r = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
        out[s] = 1.0 / (1.0 + np.exp((r - r0) / EDGE))
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(a, b): two lists of ``num_maps`` float32 (B, C, H, W) arrays.  Read-only: shared between tests."""
    B, C, H, W, M = case
    rng = np.random.default_rng([SEED, B, C, H, W, M])
    hot = hot_region(B, H, W, rng)[:, None]
    a, b = [], []
    for _ in range(M):
        ak = (NOISE_STD * rng.standard_normal((B, C, H, W)) + hot).astype(np.float32)
        bk = (NOISE_STD * rng.standard_normal((B, C, H, W))).astype(np.float32)
        ak.setflags(write=False)
        bk.setflags(write=False)
        a.append(ak)
        b.append(bk)
    return a, b


@functools.lru_cache(maxsize=None)
def reference(case):
    """dict: ``acc`` (float64 (B, H, W), over all draws), ``acc32`` (its fp32 rounding: what pd_contrast_mask is given), and ``mask``,
    ``map``, ``stats`` of ``acc32`` at RATIO.  Read-only."""
    a, b = inputs(case)
    acc = None
    for ak, bk in zip(a, b):
        acc = class_contrast_ref(ak, bk, acc)
    acc32 = acc.astype(np.float32)
    mask, cmap, stats = contrast_mask_ref(acc32, RATIO)
    out = dict(acc=acc, acc32=acc32, mask=mask, map=cmap, stats=stats)
    for v in out.values():
        v.setflags(write=False)
    return out
