"""References for the tiled trajectories, in plain torch on the CPU: the grid, the blending weights, gather, blend in the stated operation
order, and the tiled inversion / DDIB loop over the oracle's UNet and schedulers.  Nothing here comes from phendiff_amd.tiling: the grid
and the weights are written down a second time, from the definition.  A plain module: tests/test_host_tiling.py and
tests/test_gpu_tiling.py import the same builders and case lists."""
import math

import numpy as np
import torch

# (B, C, Hc, Wc, tile, overlap): the general case | triple coverage along y, zero overlap with a flush tile at x0 = 8 | unaligned origins 1
# and 3 (the element path) | one tile, 32 channels
KERNEL_CASES = ((2, 3, 72, 88, 32, 8), (1, 5, 72, 40, 32, (16, 0)), (1, 1, 33, 35, 32, 4), (3, 32, 32, 32, 32, 0))
KNOWN_ORIGINS = (((72, 32, 8), (0, 24, 40)), ((88, 32, 8), (0, 24, 48, 56)), ((72, 32, 16), (0, 16, 32, 40)), ((32, 32, 0), (0,)),
                 ((40, 32, 0), (0, 8)), ((33, 32, 4), (0, 1)), ((35, 32, 4), (0, 3)))


def pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def origins_1d(L, t, ov):
    assert 0 <= ov < t <= L
    s = t - ov
    n = 1 if L == t else math.ceil((L - t) / s) + 1
    return [min(k * s, L - t) for k in range(n)]


def window_1d(t, ov):
    return [min(i + 1, t - i, ov + 1) for i in range(t)]


def weights_1d(L, t, ov):
    """float64 [n][t]: n_k(p) = r(p - o_k) / sum_j r(p - o_j), position by position from the definition."""
    orig, r = origins_1d(L, t, ov), window_1d(t, ov)
    w = np.zeros((len(orig), t), dtype=np.float64)
    for p in range(L):
        cover = [(k, p - o) for k, o in enumerate(orig) if 0 <= p - o < t]
        total = float(sum(r[i] for _, i in cover))
        for k, i in cover:
            w[k, i] = r[i] / total
    return w


def coverage_1d(L, t, ov):
    c = np.zeros(L, dtype=np.int64)
    for o in origins_1d(L, t, ov):
        c[o:o + t] += 1
    return c


class GridRef:
    def __init__(self, H, W, tile, overlap):
        (self.th, self.tw), (self.ovy, self.ovx) = pair(tile), pair(overlap)
        self.H, self.W = H, W
        self.oy, self.ox = origins_1d(H, self.th, self.ovy), origins_1d(W, self.tw, self.ovx)
        self.wy64, self.wx64 = weights_1d(H, self.th, self.ovy), weights_1d(W, self.tw, self.ovx)
        self.wy, self.wx = torch.from_numpy(self.wy64.astype(np.float32)), torch.from_numpy(self.wx64.astype(np.float32))
        self.per_image = len(self.oy) * len(self.ox)

    def tiles(self, B):
        """[(b, ky, kx, y0, x0)] in tile order: b, then ky, then kx."""
        return [(b, ky, kx, y0, x0) for b in range(B) for ky, y0 in enumerate(self.oy) for kx, x0 in enumerate(self.ox)]


def gather_ref(canvas, g, first=0, count=None):
    tl = g.tiles(canvas.shape[0])
    count = len(tl) - first if count is None else count
    return torch.stack([canvas[b, :, y0:y0 + g.th, x0:x0 + g.tw] for b, _, _, y0, x0 in tl[first:first + count]]).contiguous()


def blend_ref(tiles, g, B):
    """out = sum (wy * wx) * m over the covering tiles, ky ascending then kx ascending; the weight product, each term and each addition are
    separate fp32 operations (torch on fp32 tensors), the first term of a position is taken as it is."""
    Cc = tiles.shape[1]
    out = torch.full((B, Cc, g.H, g.W), float("nan"), dtype=torch.float32)
    started = torch.zeros((B, g.H, g.W), dtype=torch.bool)
    for i, (b, ky, kx, y0, x0) in enumerate(g.tiles(B)):
        w = g.wy[ky][:, None] * g.wx[kx][None, :]
        term = w[None] * tiles[i]
        ys, xs = slice(y0, y0 + g.th), slice(x0, x0 + g.tw)
        seen = started[b, ys, xs][None]
        out[b, :, ys, xs] = torch.where(seen, out[b, :, ys, xs] + term, term)
        started[b, ys, xs] = True
    assert bool(started.all())
    return out


def covered_by(g, B, tile_index):
    """bool [B][H][W]: the positions tile `tile_index` covers."""
    b, _, _, y0, x0 = g.tiles(B)[tile_index]
    m = torch.zeros((B, g.H, g.W), dtype=torch.bool)
    m[b, y0:y0 + g.th, x0:x0 + g.tw] = True
    return m


# ================================================================================================ trajectories
def _sample(out):
    """The oracle's UNet returns an object with `.sample`; the closed-form stand-ins of the self-check return the tensor."""
    return out.sample if hasattr(out, "sample") else out


def tiled_model_out(unet, x, t, labels, g):
    """One tiled evaluation: gather, the model over all tiles (a tile carries its image's class and the step's timestep), blend."""
    tiles = gather_ref(x, g)
    lab = labels.repeat_interleave(g.per_image, dim=0)
    return blend_ref(_sample(unet(tiles, t, lab)), g, x.shape[0])


@torch.no_grad()
def tiled_inversion_ref(unet, sched_config, x, labels, S, g, variant="0.18.2"):
    from oracle import DDIMInverseSchedulerRef
    inv = DDIMInverseSchedulerRef.from_config(sched_config, variant=variant)
    inv.set_timesteps(S)
    x = x.clone()
    for t in inv.timesteps:
        x = inv.step(tiled_model_out(unet, x, t, labels, g), t, x).prev_sample
    return x


@torch.no_grad()
def tiled_ddib_ref(unet, fwd, x, orig, target, S, g, variant="0.18.2"):
    """(images NHWC in [0, 1] as a numpy array, the inverted canvas).  `fwd`: the oracle's forward scheduler (DDIMSchedulerRef, or
    threshold_refs.make_threshold_ref's)."""
    inverted = tiled_inversion_ref(unet, fwd.config, x, orig, S, g, variant)
    fwd.set_timesteps(S)
    img = inverted.clone()
    for t in fwd.timesteps:
        img = fwd.step(tiled_model_out(unet, img, t, target, g), t, img).prev_sample
    return (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy(), inverted


@torch.no_grad()
def untiled_ddib_ref(unet, fwd, x, orig, target, S, variant="0.18.2"):
    """The same loop with the model on the whole canvas (what oracle.ddib_ref computes), for the reference's self-check."""
    from oracle import DDIMInverseSchedulerRef
    inv = DDIMInverseSchedulerRef.from_config(fwd.config, variant=variant)
    inv.set_timesteps(S)
    x = x.clone()
    for t in inv.timesteps:
        x = inv.step(_sample(unet(x, t, orig)), t, x).prev_sample
    inverted = x.clone()
    fwd.set_timesteps(S)
    for t in fwd.timesteps:
        x = fwd.step(_sample(unet(x, t, target)), t, x).prev_sample
    return (x / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy(), inverted


def canvas_batch(B, Cc, H, W, seed=1234):
    """Images in [-1, 1] with a class-dependent offset, and their binary labels (tests/test_gpu_unet_ddib.synth_batch on a canvas)."""
    gen = torch.Generator().manual_seed(seed)
    labels = torch.arange(B) % 2
    x = torch.rand(B, Cc, H, W, generator=gen) * 2 - 1
    return (x + 0.25 * (2 * labels.float() - 1).view(B, 1, 1, 1)).clamp(-1, 1), labels
