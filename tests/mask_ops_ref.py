"""Plain numpy references of the mask refinement (phendiff_amd.mask_ops / csrc/mask_morph.hip), written from the definitions:

    d2_all_pairs         the squared Euclidean distance transform by brute force over all pixel pairs
    d2_ref               the same numbers factored by rows (min over y' of (y - y')^2 + min over x' in row y' of (x - x')^2): still a
                         brute-force minimum, H W (H + W) terms instead of (H W)^2 -- tests/test_host_mask_ops.py proves the two equal
    dilate_ref, erode_ref, open_ref, close_ref      the disc {dy^2 + dx^2 <= r2} by its definition (a threshold of the distance)
    label_ref            flood fill; label = 1 + the smallest linear index of the component
    drop_small_ref, fill_holes_ref, refine_ref       the two filters (with their stats rows) and the recipe

Masks: (B, H, W) arrays, nonzero = set.  Everything is integers; every comparison against these is exact.  A plain module (no fixtures)."""
import math

import numpy as np

FAR = 1 << 30
STAGES = ("close", "open", "fill_holes", "min_area", "dilate")


def r2_of(radius):
    return int(math.floor(float(radius) ** 2))


def _saturate(d2, limit):
    return d2 if not limit else np.where(d2 > limit, limit + 1, d2).astype(np.int32)


def d2_all_pairs(mask, to_set=False, limit=None):
    mask = np.asarray(mask) != 0
    B, H, W = mask.shape
    yy, xx = np.mgrid[0:H, 0:W]
    yy, xx = yy.reshape(-1).astype(np.int64), xx.reshape(-1).astype(np.int64)
    out = np.full((B, H * W), FAR, np.int64)
    for s in range(B):
        sel = np.flatnonzero(mask[s].reshape(-1) == bool(to_set))
        if sel.size:
            d = (yy[:, None] - yy[sel][None, :]) ** 2 + (xx[:, None] - xx[sel][None, :]) ** 2
            out[s] = d.min(axis=1)
    return _saturate(out.reshape(B, H, W).astype(np.int32), limit)


def d2_ref(mask, to_set=False, limit=None):
    mask = np.asarray(mask) != 0
    B, H, W = mask.shape
    assert H <= 4096 and W <= 4096      # (int32 below: every true distance stays under `big`)
    want = mask == bool(to_set)
    dx2 = (np.arange(W)[:, None] - np.arange(W)[None, :]).astype(np.int32) ** 2      # [x][x']
    dy2 = (np.arange(H)[:, None] - np.arange(H)[None, :]).astype(np.int32) ** 2      # [y][y']
    big = np.int32(1 << 29)
    out = np.empty((B, H, W), np.int32)
    for s in range(B):
        # per row y': the squared distance along the row to its nearest wanted pixel (big where the row holds none)
        rowd = np.where(want[s][:, None, :], dx2[None, :, :], big).min(axis=2)      # [y'][x]
        out[s] = (dy2[:, :, None] + rowd[None, :, :]).min(axis=1)                    # [y][x]
    return _saturate(np.where(out >= big, FAR, out).astype(np.int32), limit)


def dilate_ref(mask, r2):
    return (d2_ref(mask, True) <= r2).astype(np.uint8)


def erode_ref(mask, r2):
    return ((np.asarray(mask) != 0) & (d2_ref(mask, False) > r2)).astype(np.uint8)


def open_ref(mask, r2):
    return dilate_ref(erode_ref(mask, r2), r2)


def close_ref(mask, r2):
    return erode_ref(dilate_ref(mask, r2), r2)


def label_ref(mask, connectivity=8, phase=1):
    """(label, area, border, count): int32 [B][H][W] twice, uint8 [B][H][W], int32 [B]."""
    mask = np.asarray(mask) != 0
    B, H, W = mask.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    label, area = np.zeros((B, H, W), np.int32), np.zeros((B, H, W), np.int32)
    border, count = np.zeros((B, H, W), np.uint8), np.zeros((B,), np.int32)
    for s in range(B):
        want = (mask[s] == bool(phase)).tolist()
        seen = [[False] * W for _ in range(H)]
        for y0 in range(H):
            for x0 in range(W):
                if not want[y0][x0] or seen[y0][x0]:
                    continue
                seen[y0][x0] = True      # raster order: (y0, x0) is the component's smallest linear index
                stack, pix, onb = [(y0, x0)], [], False
                while stack:
                    y, x = stack.pop()
                    pix.append((y, x))
                    onb = onb or y == 0 or y == H - 1 or x == 0 or x == W - 1
                    for dy, dx in steps:
                        v, u = y + dy, x + dx
                        if 0 <= v < H and 0 <= u < W and want[v][u] and not seen[v][u]:
                            seen[v][u] = True
                            stack.append((v, u))
                ys, xs = zip(*pix)
                label[s, ys, xs] = y0 * W + x0 + 1
                area[s, ys, xs] = len(pix)
                border[s, ys, xs] = int(onb)
                count[s] += 1
    return label, area, border, count


def _stats(mask, out, label, selected_roots):
    B = mask.shape[0]
    idx = np.arange(mask[0].size, dtype=np.int64).reshape(mask[0].shape) + 1
    root = label == idx[None]
    st = np.zeros((B, 5), np.int32)
    st[:, 0] = (mask != 0).reshape(B, -1).sum(1)
    st[:, 1] = (out != 0).reshape(B, -1).sum(1)
    st[:, 2] = root.reshape(B, -1).sum(1)
    st[:, 3] = (root & selected_roots).reshape(B, -1).sum(1)
    return st


def drop_small_ref(mask, min_area, connectivity=8):
    """(out, stats): the set pixels whose component has at least min_area pixels."""
    mask = np.asarray(mask)
    label, area, _, _ = label_ref(mask, connectivity, 1)
    keep = (mask != 0) & (area >= min_area)
    return keep.astype(np.uint8), _stats(mask, keep, label, keep)


def fill_holes_ref(mask, max_area=None, connectivity=8):
    """(out, stats): holes are components of clear pixels, under the connectivity DUAL to the foreground's, that do not touch the border."""
    mask = np.asarray(mask)
    label, area, border, _ = label_ref(mask, {8: 4, 4: 8}[connectivity], 0)
    limit = -1 if max_area is None else max_area
    fill = (mask == 0) & (border == 0) & ((area <= limit) if limit >= 0 else True)
    out = (mask != 0) | fill
    return out.astype(np.uint8), _stats(mask, out, label, fill)


def refine_ref(mask, close=0.0, open=0.0, fill_holes=0, min_area=0, dilate=0.0, connectivity=8):
    """(out, stats [B][enabled stages][5]): close -> open -> fill holes -> drop small -> dilate; a stage whose parameter is 0 is skipped."""
    cur = (np.asarray(mask) != 0).astype(np.uint8)
    B = cur.shape[0]
    rows = []

    def morph_row(a, b):
        st = np.zeros((B, 5), np.int32)
        st[:, 0], st[:, 1] = a.reshape(B, -1).sum(1), b.reshape(B, -1).sum(1)
        return st

    if close:
        nxt = close_ref(cur, r2_of(close))
        rows.append(morph_row(cur, nxt))
        cur = nxt
    if open:
        nxt = open_ref(cur, r2_of(open))
        rows.append(morph_row(cur, nxt))
        cur = nxt
    if fill_holes:
        cur, st = fill_holes_ref(cur, None if fill_holes < 0 else fill_holes, connectivity)
        rows.append(st)
    if min_area:
        cur, st = drop_small_ref(cur, min_area, connectivity)
        rows.append(st)
    if dilate:
        nxt = dilate_ref(cur, r2_of(dilate))
        rows.append(morph_row(cur, nxt))
        cur = nxt
    return cur, np.stack(rows, axis=1)
