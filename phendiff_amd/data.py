"""Image preprocessing on the GPU: decoded uint8 images -> the float32 NCHW tensor in [-1, 1] every entry point of the engine takes.

The reference builds that tensor on the host, per image, in PIL / torchvision, in two places:

    src/utils_dataset.py:104-118   Resize((h, w), BILINEAR) -> ToTensor -> Normalize([0.5], [0.5])
                                   [-> RandomHorizontalFlip -> RandomVerticalFlip]            (--data_aug_on_the_fly)
    src/utils_dataset.py:120-127   Resize -> PILToTensor (uint8): the "raw" twin behind the FID / IS / KID reference sets
    src/utils_Img2Img.py:197-206   Resize(definition, BILINEAR) -> ToTensor -> Normalize([m], [s])

Here one launch of ``pd_image_preprocess`` (``csrc/data_kernels.hip``) does it for a batch.  The resize is Pillow's 8-bit bilinear resample
in its own integer arithmetic -- the output equals ``PIL.Image.resize(..., Image.BILINEAR)`` byte for byte, and the float tail is the same
three IEEE operations -- so a model trained behind the reference's transform stack sees identical tensors.  The coefficient tables are built
on the host in float64 (:func:`resample_tables`), exactly as Pillow's ``precompute_coeffs`` / ``normalize_coeffs_8bpc`` build them.

Decoding (PNG / TIFF -> bytes) and file I/O stay with the caller.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L

PRECISION_BITS = 32 - 8 - 2          # Pillow's 8-bit resample: 22-bit fixed-point coefficients
MAX_DOWNSCALE = 32                   # per axis; pd_image_preprocess refuses more (ksize <= 65)
MAX_BANDS = 32                       # pd_image_preprocess_bands: bands per pixel (what the pixel UNet's conv_in takes)
MAX_BAND_PIXEL_STRIDE = 64           # ... and the widest pixel stride it reads in place


def resample_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's bilinear (triangle filter) resampling tables of one axis: ``coef`` int32 [out][ksize] (22-bit fixed point, zero past each
    row's count) and ``bounds`` int32 [out][2] = (first source index, count).  All arithmetic is float64 and ``int()`` truncates toward
    zero, as in ``precompute_coeffs``; the weights of a row are summed first to last (``cumsum``: numpy's ``sum`` is pairwise)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample_tables: sizes must be positive (got {in_size} -> {out_size})")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # astype truncates toward zero, like C's (int)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    valid = x < n[:, None]
    arg = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fs))
    w = np.where(valid & (arg < 1.0), 1.0 - arg, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    coef = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
    coef = np.where(valid, coef, 0).astype(np.int32)
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    return np.ascontiguousarray(coef), np.ascontiguousarray(bounds)


def resized_output_size(h: int, w: int, size: Union[int, Sequence[int]]) -> Tuple[int, int]:
    """Output (height, width) of ``Resize(size)``: a pair passes through; an ``int`` is the new SHORT edge, the long edge becomes
    ``int(size * long / short)`` (torchvision 0.15.2 ``_compute_resized_output_size``, what ``Resize(definition)`` of ``load_datasets`` does)."""
    if not isinstance(size, (int, np.integer)):
        size = tuple(int(s) for s in size)
        if len(size) == 1:
            size = size[0]
        elif len(size) == 2:
            return size
        else:
            raise ValueError(f"size must be an int or (h, w), got {size}")
    size = int(size)
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w


def draw_flips(n: int, generator: Optional[torch.Generator] = None, p: float = 0.5) -> torch.Tensor:
    """Flip codes (uint8 [n]: bit 0 horizontal, bit 1 vertical) drawn the way the reference's composed transform consumes the RNG for one
    image after the other: ``torch.rand(1) < p`` for RandomHorizontalFlip, then again for RandomVerticalFlip."""
    codes = torch.zeros(n, dtype=torch.uint8)
    for i in range(n):
        h = bool(torch.rand(1, generator=generator) < p)
        v = bool(torch.rand(1, generator=generator) < p)
        codes[i] = int(h) | (int(v) << 1)
    return codes


class _Plan:
    """Device tables of one (H, W) -> (OH, OW) resize and the argument struct that carries them."""

    def __init__(self, H, W, OH, OW, device, bands=False):
        self.args = (L.ImagePreprocessBandsArgs if bands else L.ImagePreprocessArgs)(H=H, W=W, OH=OH, OW=OW)
        self.keep = []
        for axis, (i, o) in (("x", (W, OW)), ("y", (H, OH))):
            if i == o:
                continue      # an unchanged axis is skipped (as in PIL): no table
            coef, bounds = resample_tables(i, o)
            coef, bounds = torch.from_numpy(coef).to(device), torch.from_numpy(bounds).to(device)
            self.keep += [coef, bounds]
            setattr(self.args, f"coef_{axis}", coef.data_ptr())
            setattr(self.args, f"bounds_{axis}", bounds.data_ptr())
            setattr(self.args, f"ksize_{axis}", coef.shape[1])


def _as_uint8_array(img, channels=None):
    """One image of a list -> a uint8 torch tensor (H, W) or (H, W, 1 | 3 | 4); PIL images of other modes go through convert("RGB").
    ``channels``: a band stack instead, (H, W, channels) (or (H, W) for one band); PIL holds no such image and is refused."""
    if channels is not None and hasattr(img, "mode") and hasattr(img, "convert"):
        raise TypeError(f"images: a {channels}-band stack is a uint8 tensor or array (H, W, {channels}), not a PIL image")
    if isinstance(img, torch.Tensor):
        t = img
    elif isinstance(img, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(img))
    elif hasattr(img, "mode") and hasattr(img, "convert"):         # PIL.Image.Image, without importing PIL here
        if img.mode not in ("L", "RGB", "RGBA"):
            img = img.convert("RGB")
        t = torch.from_numpy(np.array(img))
    else:
        raise TypeError(f"images: expected uint8 tensors, arrays or PIL images, got {type(img).__name__}")
    if t.dtype != torch.uint8:
        raise TypeError(f"images must be uint8, got {t.dtype}")
    if channels is not None:
        if not ((t.dim() == 3 and t.shape[2] == channels) or (t.dim() == 2 and channels == 1)):
            raise ValueError(f"an image must have shape (H, W, {channels}), got {tuple(t.shape)}")
        return t
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] not in (1, 3, 4)):
        raise ValueError(f"an image must have shape (H, W) or (H, W, 1 | 3 | 4), got {tuple(t.shape)}")
    return t


class ImagePreprocessor:
    """``Resize(definition, BILINEAR) -> ToTensor -> Normalize(mean, std) [-> random flips]`` for a batch, on the GPU.

    definition            ``(h, w)``, or an ``int``: the short edge, aspect ratio kept (:func:`resized_output_size`)
    mean, std             a float or three floats (per channel)
    data_aug_on_the_fly   draw flip codes with :func:`draw_flips` when ``__call__`` gets none
    channels              None: RGB output as described below.  ``C`` in 1..32: a stack of C independent bands (Cell Painting stains,
                          multiplexed immunofluorescence) through ``pd_image_preprocess_bands`` -- C bands in, C bands out, each resampled
                          as a mode-L image.  ``images`` is then a uint8 ``(N, H, W, C)`` tensor / array (``(N, H, W)`` for C = 1) or a
                          list of ``(H, W, C)`` items (no PIL images), ``mean`` / ``std`` take one value or C, and the outputs are
                          ``(n, C, OH, OW)`` and, with ``return_raw``, ``(n, OH, OW, C)``.  Flips, slots, strided device views and
                          capture work as without it.

    ``__call__(images, flips=None, generator=None, return_raw=False)`` returns the float32 NCHW tensor, or with ``return_raw`` the pair
    ``(tensor, raw)`` where ``raw`` is the resized uint8 NHWC batch (never flipped: the reference's raw twin has no flips) in the layout
    ``metrics.InceptionV3Features`` takes.  ``images``: a uint8 tensor / array ``(N, H, W)`` or ``(N, H, W, 1 | 3 | 4)`` on the CPU or the
    device (one channel is replicated to three, a fourth is dropped), or a list of ``(H, W[, C])`` arrays / tensors / PIL images of
    possibly different sizes -- grouped by size, one launch per group, slots in list order.  Outputs are fresh tensors; the tables are
    cached per (H, W, OH, OW).  A device tensor whose channel stride is 1 is read in place through its strides (no copy), and with
    device-resident ``images`` and ``flips`` the call enqueues nothing but the kernel, so it can be captured in a graph once the plan of its
    shape exists (call once before capturing)."""

    def __init__(self, definition, mean=0.5, std=0.5, data_aug_on_the_fly: bool = False, device="cuda:0", channels: Optional[int] = None):
        if isinstance(definition, (int, np.integer)):
            self.definition = int(definition)
        else:
            self.definition = tuple(int(s) for s in definition)
            if len(self.definition) == 1:
                self.definition = self.definition[0]
            elif len(self.definition) != 2:
                raise ValueError(f"definition must be an int or (h, w), got {definition}")
        if channels is not None and not (isinstance(channels, (int, np.integer)) and 1 <= channels <= MAX_BANDS):
            raise ValueError(f"channels must be None or an int in 1..{MAX_BANDS}, got {channels}")
        self.channels = None if channels is None else int(channels)
        k = self.channels or 3
        self.mean, self.std = self._per_channel(mean, "mean", k), self._per_channel(std, "std", k)
        self._mean_std = None      # (device fp32 [C], device fp32 [C]) of the band entry, built on first use
        if any(s == 0.0 for s in self.std):
            raise ValueError("std must be non-zero")
        self.data_aug_on_the_fly = bool(data_aug_on_the_fly)
        self.device = torch.device(device)
        self._plans = {}

    @staticmethod
    def _per_channel(v, what, k):
        if isinstance(v, torch.Tensor):
            v = v.flatten().tolist()
        if isinstance(v, (int, float)):
            v = [v]
        v = [float(x) for x in v]
        if len(v) == 1:
            v = v * k
        if len(v) != k:
            raise ValueError(f"{what}: one value or {'three' if k == 3 else k}, got {len(v)}")
        return v

    # ---- input handling --------------------------------------------------------------------------------------------------------------
    def _groups(self, images):
        """-> (number of images, [(batch tensor (n, H, W[, C]), slots or None)])"""
        if isinstance(images, (torch.Tensor, np.ndarray)):
            t = torch.from_numpy(images) if isinstance(images, np.ndarray) else images
            if t.dtype != torch.uint8:
                raise TypeError(f"images must be uint8, got {t.dtype}")
            ch = self.channels
            if ch is not None:
                if not ((t.dim() == 4 and t.shape[3] == ch) or (t.dim() == 3 and ch == 1)):
                    raise ValueError(f"images must have shape (N, H, W, {ch}) with channels={ch}, got {tuple(t.shape)}")
            elif t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[3] not in (1, 3, 4)):
                raise ValueError(f"images must have shape (N, H, W) or (N, H, W, 1 | 3 | 4), got {tuple(t.shape)}")
            if t.shape[0] == 0:
                raise ValueError("images: empty batch")
            return t.shape[0], [(t, None)]
        items = [_as_uint8_array(i, self.channels) for i in images]
        if not items:
            raise ValueError("images: empty list")
        by_shape = {}
        for slot, t in enumerate(items):
            by_shape.setdefault(tuple(t.shape), []).append(slot)
        groups = []
        for shape, slots in by_shape.items():
            members = [items[s] for s in slots]
            if any(m.is_cuda for m in members):
                members = [m.to(self.device) for m in members]
            batch = torch.stack(members)
            groups.append((batch, None if len(by_shape) == 1 else slots))
        return len(items), groups

    def _plan(self, H, W, OH, OW):
        key = (H, W, OH, OW)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = _Plan(H, W, OH, OW, self.device, bands=self.channels is not None)
        return plan

    def _strided(self, t):
        """The batch as the kernel reads it: (device tensor, image / row / pixel byte strides, Cin)."""
        if t.device != self.device:
            t = t.contiguous().to(self.device)
        if t.dim() == 3:
            t = t.unsqueeze(3)
        n, h, w, c = t.shape
        cin = self.channels or (1 if c == 1 else 3)
        s = t.stride()
        ok = (c == 1 or s[3] == 1) and cin <= s[2] <= (8 if self.channels is None else MAX_BAND_PIXEL_STRIDE) and s[1] >= w * s[2] and (n == 1 or s[0] >= (h - 1) * s[1] + w * s[2])
        if not ok:
            t = t.contiguous()
            s = t.stride()
        return t, s[0], s[1], s[2], cin

    # ---- the call ----------------------------------------------------------------------------------------------------------------------
    def __call__(self, images, flips=None, generator: Optional[torch.Generator] = None, return_raw: bool = False):
        n, groups = self._groups(images)
        sizes = {resized_output_size(b.shape[1], b.shape[2], self.definition) for b, _ in groups}
        if len(sizes) != 1:
            raise ValueError(f"definition={self.definition} resolves to different output sizes for this call's images: {sorted(sizes)}; "
                             "pass an (h, w) definition or batch images of one aspect ratio")
        OH, OW = sizes.pop()
        for b, _ in groups:
            if b.shape[1] > MAX_DOWNSCALE * OH or b.shape[2] > MAX_DOWNSCALE * OW:
                raise ValueError(f"down-scale factor above {MAX_DOWNSCALE}: {tuple(b.shape[1:3])} -> {(OH, OW)}")
        if flips is None and self.data_aug_on_the_fly:
            flips = draw_flips(n, generator)
        if flips is not None:
            if not isinstance(flips, torch.Tensor):
                flips = torch.as_tensor(np.asarray(flips, dtype=np.uint8))
            if flips.dtype != torch.uint8 or flips.shape != (n,):
                raise ValueError(f"flips: uint8 codes of shape ({n},), got {flips.dtype} {tuple(flips.shape)}")
        if not torch.cuda.is_available():
            raise L.PhenDiffHipError("ImagePreprocessor needs a HIP device: phendiff_amd has no CPU fallback")
        lib = L.lib()
        dev = self.device
        if flips is not None:
            flips = flips.to(dev).contiguous()
        bands = self.channels is not None
        cout = self.channels or 3
        if bands and self._mean_std is None:
            self._mean_std = (torch.tensor(self.mean, dtype=torch.float32, device=dev), torch.tensor(self.std, dtype=torch.float32, device=dev))
        fn, what = (lib.pd_image_preprocess_bands, "pd_image_preprocess_bands") if bands else (lib.pd_image_preprocess, "pd_image_preprocess")
        y = torch.empty((n, cout, OH, OW), dtype=torch.float32, device=dev)
        raw = torch.empty((n, OH, OW, cout), dtype=torch.uint8, device=dev) if return_raw else None
        keep = []
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            for batch, slots in groups:
                t, s_img, s_row, s_pix, cin = self._strided(batch)
                plan = self._plan(t.shape[1], t.shape[2], OH, OW)
                a = plan.args
                a.N, a.out_slots = t.shape[0], n
                if bands:
                    a.C, a.mean, a.std = cin, self._mean_std[0].data_ptr(), self._mean_std[1].data_ptr()
                else:
                    a.Cin = cin
                    (a.mean0, a.mean1, a.mean2), (a.std0, a.std1, a.std2) = self.mean, self.std
                a.image_stride, a.row_stride, a.pixel_stride = s_img, s_row, s_pix
                a.x = t.data_ptr()
                a.out_index = a.flips = None
                if slots is not None:
                    idx = torch.tensor(slots, dtype=torch.int32).to(dev)
                    a.out_index = idx.data_ptr()
                    keep.append(idx)
                if flips is not None:
                    f = flips if slots is None else flips[torch.tensor(slots, device=dev)]
                    a.flips = f.data_ptr()
                    keep.append(f)
                a.y_f32, a.y_u8 = y.data_ptr(), L.ptr(raw)
                rc = fn(C.byref(a), st)
                if rc == L.PD_ERR_SHAPE and bands and s_pix > cin:
                    # a view into wider pixels stages whole source rows at ITS pixel stride; under a steep horizontal down-scale such a
                    # row may not fit the LDS budget where the same bands, dense, do (refused before launch): read a dense copy instead
                    t = t.contiguous()
                    a.image_stride, a.row_stride, a.pixel_stride = t.stride()[:3]
                    a.x = t.data_ptr()
                    rc = fn(C.byref(a), st)
                L.check(rc, what)
                keep.append(t)
        del keep            # temporaries were allocated on the launch stream: the allocator reuses them only behind the kernel
        return (y, raw) if return_raw else y
