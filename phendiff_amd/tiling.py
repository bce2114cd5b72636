"""Tiled trajectories (MultiDiffusion-style): a field of view larger than the size the UNet was trained at is a *canvas*; at every step
overlapping tiles of the training size are evaluated and their outputs blended into one canvas-sized model output, on which the ordinary
scheduler step runs.  This module is the host side: the grid, its blending weights, and the two launches (``pd_tile_gather``,
``pd_tile_blend``; ``csrc/tile_kernels.hip``).  The trajectories are ``img2img.tiled_inversion`` / ``tiled_ddib`` /
``tiled_inverted_regeneration`` (eager) and ``trajectories.TiledDDIBGraph`` (captured).

Per axis with canvas extent ``L``, tile extent ``t`` and overlap ``ov``: stride ``s = t - ov``, ``n = ceil((L - t) / s) + 1`` tiles
(1 when ``L == t``), tile ``k`` starts at ``min(k * s, L - t)`` -- the last tile is flush with the edge, so near it more than two tiles
may cover a position.  The raw window of a tile is ``r(i) = min(i + 1, t - i, ov + 1)`` (a ramp over the overlap, flat inside); the
weight of tile ``k`` at position ``p`` is ``r(p - o_k) / sum_j r(p - o_j)`` over the tiles of the axis that cover ``p``, computed in
float64 and kept as an fp32 table ``[n][t]``.  The grid is the tensor product of its two axes: the 2-D weight of tile ``(ky, kx)`` is
the product of the two axis weights, and the weights of a position sum to one.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _pair(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what}: an int or a (y, x) pair, got {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def axis_origins(extent: int, tile: int, overlap: int):
    """The tile origins of one axis (ascending; the last one is ``extent - tile``)."""
    if overlap < 0:
        raise ValueError(f"overlap {overlap} is negative")
    if overlap >= tile:
        raise ValueError(f"overlap {overlap} must be smaller than the tile extent {tile}")
    if extent < tile:
        raise ValueError(f"tile extent {tile} exceeds the canvas extent {extent}")
    stride = tile - overlap
    n = 1 if extent == tile else -(-(extent - tile) // stride) + 1
    return tuple(min(k * stride, extent - tile) for k in range(n))


def axis_weights(extent: int, tile: int, overlap: int) -> np.ndarray:
    """float64 ``[n][tile]``: the normalised weight of tile ``k`` at its local position ``i``."""
    origins = axis_origins(extent, tile, overlap)
    i = np.arange(tile)
    window = np.minimum(np.minimum(i + 1, tile - i), overlap + 1).astype(np.float64)
    total = np.zeros(extent, dtype=np.float64)
    for o in origins:
        total[o:o + tile] += window
    return np.stack([window / total[o:o + tile] for o in origins])


class TileGrid:
    """The tiles of a ``height x width`` canvas: ``tile`` and ``overlap`` are ints or ``(y, x)`` pairs.  ``origins_y`` / ``origins_x``,
    ``weights_y`` / ``weights_x`` (fp32 ``[n][t]`` host tensors), ``tiles_per_image``; tile order is ``ky`` then ``kx``."""

    def __init__(self, height: int, width: int, tile, overlap=0):
        self.height, self.width = int(height), int(width)
        (self.th, self.tw), (self.ovy, self.ovx) = _pair(tile, "tile"), _pair(overlap, "overlap")
        self.origins_y = axis_origins(self.height, self.th, self.ovy)
        self.origins_x = axis_origins(self.width, self.tw, self.ovx)
        self.sy, self.sx = self.th - self.ovy, self.tw - self.ovx
        self.nty, self.ntx = len(self.origins_y), len(self.origins_x)
        self.tiles_per_image = self.nty * self.ntx
        self.weights_y = torch.from_numpy(axis_weights(self.height, self.th, self.ovy).astype(np.float32))
        self.weights_x = torch.from_numpy(axis_weights(self.width, self.tw, self.ovx).astype(np.float32))
        self._device_weights = {}

    def __repr__(self):
        return (f"TileGrid({self.height}x{self.width}, tile {self.th}x{self.tw}, overlap ({self.ovy}, {self.ovx}): "
                f"{self.nty} x {self.ntx} tiles)")

    def origins(self):
        """``[(y0, x0)]`` of a canvas's tiles, in tile order."""
        return [(y0, x0) for y0 in self.origins_y for x0 in self.origins_x]

    def device_weights(self, device):
        """``(weights_y, weights_x)`` on ``device`` (made once per device)."""
        key = str(torch.device(device))
        if key not in self._device_weights:
            self._device_weights[key] = (self.weights_y.to(device).contiguous(), self.weights_x.to(device).contiguous())
        return self._device_weights[key]

    def _geometry(self, B: int, C_: int):
        return dict(B=B, C=C_, Hc=self.height, Wc=self.width, th=self.th, tw=self.tw, nty=self.nty, ntx=self.ntx, sy=self.sy, sx=self.sx)

    def gather_args(self, canvas: torch.Tensor, tiles: torch.Tensor, first: int = 0, count: int = None) -> "L.TileGatherArgs":
        """``pd_tile_gather``'s arguments: tiles ``[first, first + count)`` of ``canvas`` (B, C, H, W) into ``tiles`` (count, C, th, tw)."""
        B, C_ = canvas.shape[:2]
        count = B * self.tiles_per_image - first if count is None else count
        return L.TileGatherArgs(first=first, count=count, canvas=canvas.data_ptr(), tiles=tiles.data_ptr(), **self._geometry(B, C_))

    def blend_args(self, tiles: torch.Tensor, out: torch.Tensor) -> "L.TileBlendArgs":
        """``pd_tile_blend``'s arguments: all tile outputs (T, C, th, tw) into ``out`` (B, C, H, W)."""
        B, C_ = out.shape[:2]
        wy, wx = self.device_weights(out.device)
        return L.TileBlendArgs(tiles=tiles.data_ptr(), wy=wy.data_ptr(), wx=wx.data_ptr(), out=out.data_ptr(), **self._geometry(B, C_))

    def _check_canvas(self, canvas):
        if canvas.ndim != 4 or tuple(canvas.shape[2:]) != (self.height, self.width):
            raise ValueError(f"expected a (B, C, {self.height}, {self.width}) canvas, got {tuple(canvas.shape)}")
        if not canvas.is_cuda:
            raise L.PhenDiffHipError("phendiff_amd runs on MI355X only (no CPU fallback): move the canvas to 'cuda'")
        if canvas.dtype != torch.float32 or not canvas.is_contiguous():
            raise ValueError("the canvas and the tile batch are dense fp32 NCHW tensors")

    def gather(self, canvas: torch.Tensor, first: int = 0, count: int = None, out: torch.Tensor = None, stream: int = None):
        """Tiles ``[first, first + count)`` of ``canvas`` as a (count, C, th, tw) batch (one launch on ``stream``, default: the current one)."""
        self._check_canvas(canvas)
        B, C_ = canvas.shape[:2]
        count = B * self.tiles_per_image - first if count is None else count
        if out is None:
            out = torch.empty((max(count, 0), C_, self.th, self.tw), dtype=torch.float32, device=canvas.device)
        st = stream if stream is not None else torch.cuda.current_stream(canvas.device).cuda_stream
        L.check(L.lib().pd_tile_gather(C.byref(self.gather_args(canvas, out, first, count)), st), "pd_tile_gather")
        return out

    def blend(self, tiles: torch.Tensor, out: torch.Tensor, stream: int = None):
        """All tile outputs (T, C, th, tw) blended into the canvas ``out`` (B, C, H, W), every element written (one launch)."""
        self._check_canvas(out)
        want = (out.shape[0] * self.tiles_per_image, out.shape[1], self.th, self.tw)
        if tuple(tiles.shape) != want or tiles.dtype != torch.float32 or not tiles.is_contiguous() or tiles.device != out.device:
            raise ValueError(f"expected a dense fp32 tile batch of shape {want} on {out.device}, got {tuple(tiles.shape)}")
        st = stream if stream is not None else torch.cuda.current_stream(out.device).cuda_stream
        L.check(L.lib().pd_tile_blend(C.byref(self.blend_args(tiles, out)), st), "pd_tile_blend")
        return out
