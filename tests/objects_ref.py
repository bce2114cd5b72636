"""Plain numpy references of the per-object measurements (phendiff_amd.objects / csrc/object_stats.hip), written from the definitions:
loops over pixels and objects, no SciPy.

    index_ref        dense labels 1..count in raster order of each component's first pixel (on mask_ops_ref.label_ref), count, status
    geometry_ref     the int64 table [B][K][12]: area, y0, y1, x0, x1, sum_y, sum_x, sum_yy, sum_xx, sum_yx, edges, border
    intensity_ref    per object and channel: math.fsum of the values and of their squares (squares formed in float64), min, max, and the
                     two sums of absolute values the error bound needs
    shape_ref        the derived shape numbers, the formulas of phendiff_amd.objects.shape_tables in numpy

and the shared inputs of the GPU tests: ``images(name, kind)`` (seeded stacks over the cases of tests/mask_ops_cases.py) and
``reference(name, connectivity, K, kind)``, computed once per request and read-only.  A plain module (no fixtures)."""
import functools
import math

import numpy as np

import mask_ops_ref as R
from mask_ops_cases import CASES

GEOM_FIELDS = ("area", "y0", "y1", "x0", "x1", "sum_y", "sum_x", "sum_yy", "sum_xx", "sum_yx", "edges", "border")
OVERFLOW = 1
K_DEFAULT = 1024


def index_ref(mask, connectivity=8, max_objects=K_DEFAULT):
    """(index int32 [B][H][W], count int32 [B], status int32 [B])."""
    label, _, _, count = R.label_ref(mask, connectivity, 1)
    B, H, W = label.shape
    index, status = np.zeros((B, H, W), np.int32), np.zeros((B,), np.int32)
    for s in range(B):
        rank = 0
        for y in range(H):
            for x in range(W):
                if label[s, y, x] == y * W + x + 1:      # a root: the component's first pixel in raster order
                    rank += 1
                    if rank <= max_objects:
                        index[s][label[s] == label[s, y, x]] = rank
        assert rank == count[s]
        status[s] = OVERFLOW if rank > max_objects else 0
    return index, count.astype(np.int32), status


def geometry_ref(index, max_objects=K_DEFAULT):
    """int64 [B][K][12], by a loop over the pixels; rows without an object are zero."""
    B, H, W = index.shape
    g = np.zeros((B, max_objects, len(GEOM_FIELDS)), np.int64)
    seen = np.zeros((B, max_objects), bool)
    for s in range(B):
        ix = index[s].tolist()
        for y in range(H):
            for x in range(W):
                k = ix[y][x]
                if k == 0:
                    continue
                row = g[s, k - 1]
                if not seen[s, k - 1]:
                    seen[s, k - 1] = True
                    row[1], row[2], row[3], row[4] = y, y, x, x
                row[0] += 1
                row[1], row[2], row[3], row[4] = min(row[1], y), max(row[2], y), min(row[3], x), max(row[4], x)
                row[5] += y
                row[6] += x
                row[7] += y * y
                row[8] += x * x
                row[9] += y * x
                for v, u in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):      # a unit edge to anything that is not this object
                    if not (0 <= v < H and 0 <= u < W) or ix[v][u] != k:
                        row[10] += 1
                if y == 0 or y == H - 1 or x == 0 or x == W - 1:
                    row[11] = 1
    return g


def intensity_ref(index, images, max_objects=K_DEFAULT):
    """(table float64 [B][K][C][4]: fsum, fsum of squares, min, max; bound float64 [B][K][C][2]: n * 2^-52 * sum|v| and the same for the
    squares -- the worst-case error of an fp64 sum of n terms in any order, with a factor 2 of margin)."""
    B, Cn, H, W = images.shape
    table = np.zeros((B, max_objects, Cn, 4), np.float64)
    bound = np.zeros((B, max_objects, Cn, 2), np.float64)
    for s in range(B):
        flat = index[s].reshape(-1)
        order = np.argsort(flat, kind="stable")
        ks, starts = np.unique(flat[order], return_index=True)
        ends = list(starts[1:]) + [flat.size]
        for k, a, b in zip(ks.tolist(), starts.tolist(), ends):
            if k == 0:
                continue
            pix = order[a:b]
            for c in range(Cn):
                v = images[s, c].reshape(-1)[pix].astype(np.float64)
                sq = v * v
                table[s, k - 1, c] = (math.fsum(v.tolist()), math.fsum(sq.tolist()), v.min(), v.max())
                bound[s, k - 1, c] = (v.size * 2.0 ** -52 * math.fsum(np.abs(v).tolist()), v.size * 2.0 ** -52 * math.fsum(sq.tolist()))
    return table, bound


def shape_ref(geometry):
    """dict of float64 arrays: area, centroid, bbox, edges, border, orientation, major_axis_length, minor_axis_length, eccentricity."""
    g = geometry.astype(np.float64)
    col = {n: g[..., i] for i, n in enumerate(GEOM_FIELDS)}
    A = col["area"]
    valid = geometry[..., 0] > 0
    safe = np.where(valid, A, 1.0)
    cy, cx = col["sum_y"] / safe, col["sum_x"] / safe
    myy = col["sum_yy"] / safe - cy * cy + 1.0 / 12.0
    mxx = col["sum_xx"] / safe - cx * cx + 1.0 / 12.0
    myx = col["sum_yx"] / safe - cy * cx
    d = np.sqrt((myy - mxx) * (myy - mxx) + 4.0 * (myx * myx))
    l1 = (myy + mxx + d) / 2.0
    l2 = np.maximum((myy + mxx - d) / 2.0, 0.0)

    def keep(t):
        return np.where(valid, t, 0.0)

    return dict(area=A, centroid=np.stack([keep(cy), keep(cx)], -1),
                bbox=np.stack([col["y0"], col["x0"], keep(col["y1"] + 1.0), keep(col["x1"] + 1.0)], -1), edges=col["edges"], border=col["border"],
                orientation=keep(0.5 * np.arctan2(2.0 * myx, myy - mxx)), major_axis_length=keep(4.0 * np.sqrt(l1)),
                minor_axis_length=keep(4.0 * np.sqrt(l2)), eccentricity=keep(np.sqrt(np.maximum(1.0 - l2 / l1, 0.0))))


# ---- the shared inputs of the GPU tests --------------------------------------------------------------------------------------------------
KINDS = {"f32": (np.float32, 3), "u8": (np.uint8, 1), "u16": (np.uint16, 5)}


@functools.lru_cache(maxsize=None)
def images(name, kind):
    """A seeded (B, C, H, W) stack over case `name`: float32 with C = 3 (channel 1 carries an offset of 1000: the sum of squares has to
    hold it), uint8 with C = 1, uint16 with C = 5."""
    B, H, W = CASES[name].shape
    dtype, Cn = KINDS[kind]
    rng = np.random.default_rng(7919 * H + 104729 * W + len(kind))
    if kind == "f32":
        out = rng.standard_normal((B, Cn, H, W)).astype(np.float32)
        out[:, 1] += np.float32(1000.0)
    else:
        out = rng.integers(0, np.iinfo(dtype).max + 1, (B, Cn, H, W)).astype(dtype)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, connectivity, max_objects=K_DEFAULT, kind=None):
    """kind None: (index, count, status, geometry) of case `name`; else (table, bound) of images(name, kind) under that index."""
    if kind is None:
        index, count, status = index_ref(CASES[name], connectivity, max_objects)
        out = (index, count, status, geometry_ref(index, max_objects))
    else:
        out = intensity_ref(reference(name, connectivity, max_objects)[0], images(name, kind), max_objects)
    for a in out:
        a.setflags(write=False)
    return out
