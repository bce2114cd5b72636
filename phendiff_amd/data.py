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

16-bit band stacks (plate-reader / sCMOS TIFFs) take ``pd_image_preprocess_bands16`` (``csrc/data16_kernels.hip``): Pillow's mode ``I;16``
resample in ITS arithmetic -- float64 weights (:func:`resample_tables_f64`), one product and one sum per tap, each rounded on its own -- then
an intensity window instead of ``/ 255``.  :func:`band_percentiles` reads such a window off the data (``pd_band_histogram16``), and
:func:`restore_bands16` is the way back to uint16 (``pd_postproc_bands16``).

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
MAX_BAND16_PIXEL_STRIDE = 128        # pd_image_preprocess_bands16: the same 64 samples, in bytes


def _triangle_weights(in_size: int, out_size: int, who: str):
    """``precompute_coeffs`` of one axis before any rounding: (w float64 [out][ksize] normalised by the row sum, valid bool [out][ksize],
    xmin int64 [out], n int64 [out]).  All arithmetic is float64 and ``int()`` truncates toward zero; the weights of a row are summed
    first to last (``cumsum``: numpy's ``sum`` is pairwise)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"{who}: sizes must be positive (got {in_size} -> {out_size})")
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
    return w, valid, xmin, n


def resample_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's bilinear (triangle filter) resampling tables of one axis: ``coef`` int32 [out][ksize] (22-bit fixed point, zero past each
    row's count) and ``bounds`` int32 [out][2] = (first source index, count).  All arithmetic is float64 and ``int()`` truncates toward
    zero, as in ``precompute_coeffs``; the weights of a row are summed first to last (``cumsum``: numpy's ``sum`` is pairwise)."""
    w, valid, xmin, n = _triangle_weights(in_size, out_size, "resample_tables")
    coef = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
    coef = np.where(valid, coef, 0).astype(np.int32)
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    return np.ascontiguousarray(coef), np.ascontiguousarray(bounds)


def resample_tables_f64(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """The tables of Pillow's 16-bit (mode ``I;16``) resample: ``coef`` float64 [out][ksize], the triangle-filter weights of
    ``precompute_coeffs`` normalised by the row sum and NOT rounded to fixed point (there is no ``normalize_coeffs_8bpc`` on that path; zero
    past each row's count), and the same ``bounds`` and ksize as :func:`resample_tables`."""
    w, valid, xmin, n = _triangle_weights(in_size, out_size, "resample_tables_f64")
    coef = np.where(valid, w, 0.0).astype(np.float64)
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    return np.ascontiguousarray(coef), np.ascontiguousarray(bounds)


def percentile_rank(n: int, q: float) -> int:
    """The rank of the ``q``-th percentile among ``n`` samples as :func:`band_percentiles` defines it: ``k = max(1, ceil(n * q / 100))`` in
    Python float64 -- the percentile is the k-th smallest sample (``np.sort(band.ravel())[k - 1]``)."""
    n, q = int(n), float(q)
    if n < 1:
        raise ValueError(f"percentile_rank: n must be positive (got {n})")
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"percentile_rank: q must be in [0, 100] (got {q})")
    return min(n, max(1, int(math.ceil(n * q / 100))))


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

    def __init__(self, H, W, OH, OW, device, bands=False, bits=8):
        struct = L.ImagePreprocessBands16Args if bits == 16 else (L.ImagePreprocessBandsArgs if bands else L.ImagePreprocessArgs)
        self.args = struct(H=H, W=W, OH=OH, OW=OW)
        self.keep = []
        for axis, (i, o) in (("x", (W, OW)), ("y", (H, OH))):
            if i == o:
                continue      # an unchanged axis is skipped (as in PIL): no table
            coef, bounds = (resample_tables_f64 if bits == 16 else resample_tables)(i, o)
            coef, bounds = torch.from_numpy(coef).to(device), torch.from_numpy(bounds).to(device)
            self.keep += [coef, bounds]
            setattr(self.args, f"coef_{axis}", coef.data_ptr())
            setattr(self.args, f"bounds_{axis}", bounds.data_ptr())
            setattr(self.args, f"ksize_{axis}", coef.shape[1])


def _check_dtype(dtype, channels):
    """uint8 always; uint16 for band stacks (``channels=C``); anything else -- int16, int32, floats -- is refused."""
    if dtype == torch.uint16:
        if channels is None:
            raise TypeError("uint16 images are band stacks: pass channels=C (16-bit RGB without channels is not supported)")
    elif dtype != torch.uint8:
        raise TypeError(f"images must be uint8{'' if channels is None else ' or uint16'}, got {dtype}")


def _band_vector(v, k, device, what):
    """One float, ``k`` floats or a float32 [k] tensor -> a device float32 [k] tensor.  A tensor is used as it is (moved to the device if
    it is not there): its values are never read on the host."""
    if isinstance(v, torch.Tensor):
        if v.dtype != torch.float32 or tuple(v.shape) != (k,):
            raise ValueError(f"{what}: a tensor must be float32 of shape ({k},), got {v.dtype} {tuple(v.shape)}")
        return v.to(device).contiguous()
    return torch.tensor(ImagePreprocessor._per_channel(v, what, k), dtype=torch.float32, device=device)


def _strided_view(t, device, channels, bits):
    """The batch as the kernels read it: (device tensor, image / row / pixel BYTE strides, channels read per pixel).  A device tensor
    whose channel stride is 1 and whose strides the entry reads in place is passed as it is; anything else as a dense copy."""
    if t.device != device:
        t = t.contiguous().to(device)
    if t.dim() == 3:
        t = t.unsqueeze(3)
    n, h, w, c = t.shape
    cin = channels or (1 if c == 1 else 3)
    esz = bits // 8
    limit = 8 if channels is None else (MAX_BAND_PIXEL_STRIDE if bits == 8 else MAX_BAND16_PIXEL_STRIDE // 2)      # in elements
    s = t.stride()
    ok = (c == 1 or s[3] == 1) and cin <= s[2] <= limit and s[1] >= w * s[2] and (n == 1 or s[0] >= (h - 1) * s[1] + w * s[2])
    if not ok:
        t = t.contiguous()
        s = t.stride()
    return t, s[0] * esz, s[1] * esz, s[2] * esz, cin


def _group_images(images, channels, device):
    """-> (number of images, [(batch tensor (n, H, W[, C]), slots or None)], 8 | 16).  A uint16 batch comes back viewed as int16 (the
    same bytes: torch has few uint16 kernels, and the batch is only stacked, copied and pointed at)."""
    if isinstance(images, (torch.Tensor, np.ndarray)):
        t = torch.from_numpy(images) if isinstance(images, np.ndarray) else images
        _check_dtype(t.dtype, channels)
        ch = channels
        if ch is not None:
            if not ((t.dim() == 4 and t.shape[3] == ch) or (t.dim() == 3 and ch == 1)):
                raise ValueError(f"images must have shape (N, H, W, {ch}) with channels={ch}, got {tuple(t.shape)}")
        elif t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[3] not in (1, 3, 4)):
            raise ValueError(f"images must have shape (N, H, W) or (N, H, W, 1 | 3 | 4), got {tuple(t.shape)}")
        if t.shape[0] == 0:
            raise ValueError("images: empty batch")
        if t.dtype == torch.uint16:
            return t.shape[0], [(t.view(torch.int16), None)], 16
        return t.shape[0], [(t, None)], 8
    items = [_as_uint8_array(i, channels) for i in images]
    if not items:
        raise ValueError("images: empty list")
    dtypes = {t.dtype for t in items}
    if len(dtypes) != 1:
        raise TypeError(f"images: one list holds uint8 and uint16 items ({sorted(str(d) for d in dtypes)})")
    bits = 16 if dtypes.pop() == torch.uint16 else 8
    if bits == 16:
        items = [t.view(torch.int16) for t in items]
    by_shape = {}
    for slot, t in enumerate(items):
        by_shape.setdefault(tuple(t.shape), []).append(slot)
    groups = []
    for shape, slots in by_shape.items():
        members = [items[s] for s in slots]
        if any(m.is_cuda for m in members):
            members = [m.to(device) for m in members]
        batch = torch.stack(members)
        groups.append((batch, None if len(by_shape) == 1 else slots))
    return len(items), groups, bits


def _as_uint8_array(img, channels=None):
    """One image of a list -> a uint8 torch tensor (H, W) or (H, W, 1 | 3 | 4); PIL images of other modes go through convert("RGB").
    ``channels``: a band stack instead, uint8 or uint16, (H, W, channels) (or (H, W) for one band); PIL holds no such image and is refused."""
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
    _check_dtype(t.dtype, channels)
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
                          uint16 stacks (``torch.uint16`` tensors, ``np.uint16`` arrays: 16-bit TIFFs as they are decoded) take
                          ``pd_image_preprocess_bands16``: every band resampled as Pillow resamples a mode ``I;16`` image, bit for bit;
                          ``return_raw`` gives the resized uint16 NHWC batch.
    window                ``(lo, hi)`` for uint16 stacks, each one float, C floats or a device float32 ``[C]`` tensor (used as it is, no
                          host read -- e.g. what :func:`band_percentiles` returns): the tensor is
                          ``(clamp((v - lo) / (hi - lo), 0, 1) - mean) / std``.  Default (0, 65535), the analogue of ``ToTensor``.
                          :meth:`restore` is the way back to uint16.

    ``__call__(images, flips=None, generator=None, return_raw=False)`` returns the float32 NCHW tensor, or with ``return_raw`` the pair
    ``(tensor, raw)`` where ``raw`` is the resized uint8 NHWC batch (never flipped: the reference's raw twin has no flips) in the layout
    ``metrics.InceptionV3Features`` takes.  ``images``: a uint8 tensor / array ``(N, H, W)`` or ``(N, H, W, 1 | 3 | 4)`` on the CPU or the
    device (one channel is replicated to three, a fourth is dropped), or a list of ``(H, W[, C])`` arrays / tensors / PIL images of
    possibly different sizes -- grouped by size, one launch per group, slots in list order.  Outputs are fresh tensors; the tables are
    cached per (H, W, OH, OW).  A device tensor whose channel stride is 1 is read in place through its strides (no copy), and with
    device-resident ``images`` and ``flips`` the call enqueues nothing but the kernel, so it can be captured in a graph once the plan of its
    shape exists (call once before capturing)."""

    def __init__(self, definition, mean=0.5, std=0.5, data_aug_on_the_fly: bool = False, device="cuda:0", channels: Optional[int] = None,
                 window=None):
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
        self.window, self._window_dev = None, None
        if window is not None:
            if self.channels is None:
                raise ValueError("window: an intensity window belongs to uint16 band stacks (channels=C)")
            if len(window) != 2:
                raise ValueError(f"window must be (lo, hi), got {window}")
            sides = []
            for v, what in zip(window, ("window lo", "window hi")):
                if isinstance(v, torch.Tensor):          # used as it is: never read on the host
                    if v.dtype != torch.float32 or tuple(v.shape) != (self.channels,):
                        raise ValueError(f"{what}: a tensor must be float32 of shape ({self.channels},), got {v.dtype} {tuple(v.shape)}")
                    sides.append(v)
                else:
                    sides.append(self._per_channel(v, what, self.channels))
            if all(isinstance(s, list) for s in sides) and any(h <= l for l, h in zip(*sides)):
                raise ValueError(f"window: hi must be above lo in every band, got lo={sides[0]} hi={sides[1]}")
            self.window = tuple(sides)

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
        """-> (number of images, [(batch tensor (n, H, W[, C]), slots or None)], 8 | 16 bits a sample)"""
        return _group_images(images, self.channels, self.device)

    def _plan(self, H, W, OH, OW, bits=8):
        key = (H, W, OH, OW) if bits == 8 else (H, W, OH, OW, bits)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = _Plan(H, W, OH, OW, self.device, bands=self.channels is not None, bits=bits)
        return plan

    def _strided(self, t):
        """The batch as the kernel reads it: (device tensor, image / row / pixel byte strides, Cin)."""
        if t.dtype == torch.uint16:
            t = t.view(torch.int16)
        return _strided_view(t, self.device, self.channels, 16 if t.dtype == torch.int16 else 8)

    def _window_vectors(self):
        """The intensity window of the 16-bit path as device float32 [C] tensors (built on first use)."""
        if self._window_dev is None:
            lo, hi = self.window if self.window is not None else (0.0, 65535.0)
            self._window_dev = (_band_vector(lo, self.channels, self.device, "window lo"), _band_vector(hi, self.channels, self.device, "window hi"))
        return self._window_dev

    def _mean_std_vectors(self):
        if self._mean_std is None:
            dev = self.device
            self._mean_std = (torch.tensor(self.mean, dtype=torch.float32, device=dev), torch.tensor(self.std, dtype=torch.float32, device=dev))
        return self._mean_std

    def restore(self, x):
        """The way back for a 16-bit band stack: float32 ``(N, C, H, W)`` in this instance's normalised range -> uint16 ``(N, H, W, C)`` in
        the source's range, through the instance's own window, mean and std (:func:`restore_bands16`)."""
        if self.channels is None:
            raise ValueError("restore: only band stacks (channels=C) have a 16-bit way back")
        if not torch.cuda.is_available():
            raise L.PhenDiffHipError("ImagePreprocessor.restore needs a HIP device: phendiff_amd has no CPU fallback")
        mean, std = self._mean_std_vectors()
        return restore_bands16(x, self._window_vectors(), mean, std)

    # ---- the call ----------------------------------------------------------------------------------------------------------------------
    def __call__(self, images, flips=None, generator: Optional[torch.Generator] = None, return_raw: bool = False):
        n, groups, bits = self._groups(images)
        if bits == 8 and self.window is not None:
            raise ValueError("window: an intensity window belongs to uint16 sources; uint8 images go through ToTensor's / 255")
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
        # the path of this call, chosen once: its entry point, the struct fields that name the channel count and the raw output, and the
        # fields of the float tail, which are the same for every group
        if not bands:
            what, chan_field, raw_field = "pd_image_preprocess", "Cin", "y_u8"
            tail = dict(zip(("mean0", "mean1", "mean2", "std0", "std1", "std2"), self.mean + self.std))
        else:
            what, chan_field, raw_field = ("pd_image_preprocess_bands16", "C", "y_u16") if bits == 16 else ("pd_image_preprocess_bands", "C", "y_u8")
            tail = dict(zip(("mean", "std"), (v.data_ptr() for v in self._mean_std_vectors())))
            if bits == 16:
                tail.update(zip(("lo", "hi"), (v.data_ptr() for v in self._window_vectors())))
        fn = getattr(lib, what)
        esz = bits // 8
        y = torch.empty((n, cout, OH, OW), dtype=torch.float32, device=dev)
        raw = torch.empty((n, OH, OW, cout), dtype=torch.uint16 if bits == 16 else torch.uint8, device=dev) if return_raw else None
        keep = []
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            for batch, slots in groups:
                t, s_img, s_row, s_pix, cin = _strided_view(batch, dev, self.channels, bits)
                plan = self._plan(t.shape[1], t.shape[2], OH, OW, bits)
                a = plan.args
                a.N, a.out_slots = t.shape[0], n
                for field, value in ((chan_field, cin), (raw_field, L.ptr(raw)), *tail.items()):
                    setattr(a, field, value)
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
                a.y_f32 = y.data_ptr()
                rc = fn(C.byref(a), st)
                if rc == L.PD_ERR_SHAPE and bands and s_pix > cin * esz:
                    # a view into wider pixels stages whole source rows at ITS pixel stride; under a steep horizontal down-scale such a
                    # row may not fit the LDS budget where the same bands, dense, do (refused before launch): read a dense copy instead
                    t = t.contiguous()
                    a.image_stride, a.row_stride, a.pixel_stride = (s * esz for s in t.stride()[:3])
                    a.x = t.data_ptr()
                    rc = fn(C.byref(a), st)
                L.check(rc, what)
                keep.append(t)
        del keep            # temporaries were allocated on the launch stream: the allocator reuses them only behind the kernel
        return (y, raw) if return_raw else y


def band_percentiles(images, q=(0.1, 99.9), channels: Optional[int] = None, device="cuda:0"):
    """An intensity window from the data: per-band percentiles ``(lo, hi)`` of uint16 stacks, device float32 ``[C]`` each, ready for
    ``ImagePreprocessor(..., window=(lo, hi))``.  ``images`` as the 16-bit path of :class:`ImagePreprocessor` takes them (a tensor / array
    ``(N, H, W, C)``, ``(N, H, W)`` for C = 1, or a list of ``(H, W, C)`` items of mixed sizes).

    Exact, not interpolated: ``pd_band_histogram16`` counts every value (one launch per source size, all into one histogram), a device
    cumulative sum follows, and with n samples per band the q-th percentile is the k-th smallest one, ``k = percentile_rank(n, q)``
    (``np.sort(band.ravel())[k - 1]``).  A constant band (``hi == lo``) gets ``hi = lo + 1``.  Nothing is read back to the host."""
    if not (isinstance(channels, (int, np.integer)) and 1 <= channels <= MAX_BANDS):
        raise ValueError(f"band_percentiles: channels must be an int in 1..{MAX_BANDS}, got {channels}")
    channels = int(channels)
    if len(q) != 2 or not 0.0 <= float(q[0]) <= float(q[1]) <= 100.0:
        raise ValueError(f"band_percentiles: q must be (low, high) with 0 <= low <= high <= 100, got {q}")
    dev = torch.device(device)
    _, groups, bits = _group_images(images, channels, dev)
    if bits != 16:
        raise TypeError("band_percentiles: images must be uint16")
    samples = sum(b.shape[0] * b.shape[1] * b.shape[2] for b, _ in groups)
    ranks = [percentile_rank(samples, v) for v in q]
    if not torch.cuda.is_available():
        raise L.PhenDiffHipError("band_percentiles needs a HIP device: phendiff_amd has no CPU fallback")
    lib = L.lib()
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        counts = torch.zeros((channels, 65536), dtype=torch.int32, device=dev)        # (read as unsigned below)
        keep = []
        for batch, _ in groups:
            t, s_img, s_row, s_pix, cin = _strided_view(batch, dev, channels, 16)
            a = L.BandHistogram16Args(N=t.shape[0], H=t.shape[1], W=t.shape[2], C=cin, image_stride=s_img, row_stride=s_row, pixel_stride=s_pix,
                                      x=t.data_ptr(), counts=counts.data_ptr())
            L.check(lib.pd_band_histogram16(C.byref(a), st), "pd_band_histogram16")
            keep.append(t)
        del keep
        below = torch.cumsum(counts.to(torch.int64) & 0xFFFFFFFF, dim=1)
        lo, hi = ((below < k).sum(dim=1).to(torch.float32) for k in ranks)          # the first value whose cumulative count reaches k
        hi = torch.where(hi == lo, lo + 1.0, hi)
    return lo, hi


def restore_bands16(x, window, mean, std):
    """Float32 ``(N, C, H, W)`` on the device -> uint16 ``(N, H, W, C)`` in the source's range: the inverse of the 16-bit path's float tail,
    for saving transferred stacks beside their sources.  ``window = (lo, hi)``, ``mean``, ``std``: one float, C floats or a device float32
    ``[C]`` tensor each.  One element-wise kernel (``pd_postproc_bands16``): ``f = clamp(x * std + mean, 0, 1)``,
    ``u = clamp(rint(f * (hi - lo) + lo), 0, 65535)``, every product and sum rounded on its own, NaN -> 0."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 4:
        raise TypeError("restore_bands16: x must be a float32 tensor (N, C, H, W)")
    if not x.is_cuda:
        raise L.PhenDiffHipError("restore_bands16 needs a tensor on a HIP device: phendiff_amd has no CPU fallback")
    n, c, h, w = x.shape
    if not 1 <= c <= MAX_BANDS or n < 1:
        raise ValueError(f"restore_bands16: 1..{MAX_BANDS} bands and a non-empty batch, got {tuple(x.shape)}")
    dev = x.device
    lo, hi = (_band_vector(v, c, dev, what) for v, what in zip(window, ("window lo", "window hi")))
    mean, std = _band_vector(mean, c, dev, "mean"), _band_vector(std, c, dev, "std")
    x = x.contiguous()
    with torch.cuda.device(dev):
        y = torch.empty((n, h, w, c), dtype=torch.uint16, device=dev)
        a = L.PostprocBands16Args(N=n, C=c, H=h, W=w, x=x.data_ptr(), lo=lo.data_ptr(), hi=hi.data_ptr(), mean=mean.data_ptr(), std=std.data_ptr(),
                                  y=y.data_ptr())
        L.check(L.lib().pd_postproc_bands16(C.byref(a), torch.cuda.current_stream(dev).cuda_stream), "pd_postproc_bands16")
    return y
