"""References for the 16-bit image path, shared by tests/test_host_image16.py and tests/test_gpu_image16.py (a plain module: no fixtures,
no pytest hooks).

    contents(kind, shape, seed)        uint16 test data: "full" range, "12bit" (0..4095), "saturated" ({0, 255, 256, 32768, 65535})
    pil_bands16(a, OH, OW)             every band through PIL.Image.resize of a mode I;16 image -- THE reference of the resize
    emulate_resize16(a, OH, OW)        the arithmetic pd_image_preprocess_bands16 restates, in numpy over resample_tables_f64
    window_normalize(raw, ...)         the float tail, the same five fp32 torch operations on the CPU
    postproc16(x, ...)                 pd_postproc_bands16 restated in fp32 torch operations on the CPU
"""
import functools

import numpy as np
import torch

KINDS = ("full", "12bit", "saturated")
SATURATED = np.array([0, 255, 256, 32768, 65535], dtype=np.uint16)


def contents(kind, shape, seed=0):
    rng = np.random.default_rng(seed + 7919 * KINDS.index(kind) + sum(int(s) * (31 ** i) for i, s in enumerate(shape)))
    if kind == "full":
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    if kind == "12bit":
        return rng.integers(0, 4096, shape, dtype=np.uint16)
    return SATURATED[rng.integers(0, len(SATURATED), shape)]


def pil_bands16(a, OH, OW):
    """One stack (H, W, C) or band (H, W) uint16 -> the same rank at (OH, OW): every band resized as a mode I;16 image."""
    from PIL import Image

    def one(band):
        im = Image.fromarray(np.ascontiguousarray(band))
        assert im.mode == "I;16"
        out = np.array(im.resize((OW, OH), Image.BILINEAR))
        assert out.dtype == np.uint16 and out.shape == (OH, OW)
        return out
    if a.ndim == 2:
        return one(a)
    return np.stack([one(a[..., c]) for c in range(a.shape[-1])], axis=-1)


def _resample_axis(a, out_size, axis):
    """One pass over `axis` of a uint16 array: per output ONE float64 accumulator, ss = 0.0; ss = ss + (double)src * coef for k in order
    (numpy rounds the product and the sum separately); (int)(ss + 0.5) clamped to 0..65535.  An unchanged axis is skipped."""
    from phendiff_amd.data import resample_tables_f64
    in_size = a.shape[axis]
    if in_size == out_size:
        return a
    coef, bounds = resample_tables_f64(in_size, out_size)
    src = np.moveaxis(a, axis, -1)
    res = np.empty(src.shape[:-1] + (out_size,), dtype=np.uint16)
    for o in range(out_size):
        first, count = int(bounds[o, 0]), int(bounds[o, 1])
        ss = np.zeros(src.shape[:-1], dtype=np.float64)
        for k in range(count):
            ss = ss + src[..., first + k].astype(np.float64) * coef[o, k]
        res[..., o] = np.clip((ss + 0.5).astype(np.int64), 0, 65535).astype(np.uint16)
    return np.moveaxis(res, -1, axis)


def emulate_resize16(a, OH, OW):
    """(H, W[, C]) uint16 -> (OH, OW[, C]): the horizontal pass first, into uint16, then the vertical pass."""
    return np.ascontiguousarray(_resample_axis(_resample_axis(a, OW, 1), OH, 0))


@functools.lru_cache(maxsize=None)
def stack16(kind, n, H, W, c, seed=0):
    a = contents(kind, (n, H, W, c), seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference16(kind, n, H, W, c, OH, OW, seed=0):
    """PIL's samples for stack16(kind, n, H, W, c, seed): computed once per case, shared, read-only."""
    r = np.stack([pil_bands16(a, OH, OW) for a in stack16(kind, n, H, W, c, seed)])
    r.setflags(write=False)
    return r


def _vec(v, c):
    t = torch.as_tensor(v, dtype=torch.float32).flatten()
    return (t.expand(c) if t.numel() == 1 else t).contiguous()


def window_normalize(raw, lo, hi, mean, std, flips=None):
    """uint16 (N, OH, OW, C) -> float32 (N, C, OH, OW): ((v - lo) / (hi - lo)).clamp(0, 1), then (f - mean) / std, then the flips."""
    raw = np.asarray(raw)
    c = raw.shape[-1]
    lo, hi, mean, std = (_vec(v, c).view(1, c, 1, 1) for v in (lo, hi, mean, std))
    t = torch.from_numpy(raw.astype(np.int32)).permute(0, 3, 1, 2).to(torch.float32)      # (float)v: exact
    f = t.sub(lo).div(hi.sub(lo)).clamp(0.0, 1.0)
    y = f.sub(mean).div(std)
    if flips is not None:
        out = []
        for i, code in enumerate(int(k) for k in flips):
            img = y[i]
            if code & 1:
                img = torch.flip(img, [2])
            if code & 2:
                img = torch.flip(img, [1])
            out.append(img)
        y = torch.stack(out)
    return y.contiguous()


def postproc16(x, lo, hi, mean, std):
    """float32 (N, C, H, W) on the CPU -> int32 (N, H, W, C) holding the uint16 values pd_postproc_bands16 writes."""
    c = x.shape[1]
    lo, hi, mean, std = (_vec(v, c).view(1, c, 1, 1) for v in (lo, hi, mean, std))
    f = x.mul(std).add(mean)
    f = torch.where(f >= 0, f.clamp(max=1.0), torch.zeros_like(f))       # NaN -> 0
    r = f.mul(hi.sub(lo)).add(lo)
    u = torch.where(r >= 0, r.round().clamp(max=65535.0), torch.zeros_like(r))
    return u.to(torch.int32).permute(0, 2, 3, 1).contiguous()


def as_int(t):
    """A uint16 tensor as int32 on the CPU (torch compares few uint16 tensors itself)."""
    return torch.from_numpy(t.cpu().view(torch.int16).numpy().view(np.uint16).astype(np.int32))
