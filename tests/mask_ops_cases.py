"""The shared inputs of the mask-refinement tests: (B = 3, H, W) uint8 masks, every sample's content different, built from a seeded numpy
generator or drawn by rule.  Set pixels carry arbitrary nonzero bytes (nonzero = set).  ``reference(name, key)`` computes a reference
once per (case, request) and keeps it; the arrays are read-only.

Sizes: 1 x 1, 1 x W, H x 1, 5 x 7, 37 x 53 (odd, no multiple of any tile, more than one workgroup per sample), 64 x 64 and one 256 x 256."""
import functools

import numpy as np

import mask_ops_ref as R

B = 3
SEED = 20241


def _bytes(rng, m):
    """Set pixels as arbitrary nonzero bytes."""
    return (m.astype(np.uint8) * rng.integers(1, 256, m.shape).astype(np.uint8)).astype(np.uint8)


def _random(rng, H, W, densities):
    return np.stack([rng.random((H, W)) < d for d in densities])


def spiral(H, W):
    """A one-pixel-wide rectangular spiral that fills the image (one clear pixel between the turns): one long component."""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True

    def free(dy, dx):      # the next cell is inside and clear, and the one after it is not a turn already drawn
        v, u = y + dy, x + dx
        if not (0 <= v < H and 0 <= u < W) or m[v, u]:
            return False
        v, u = v + dy, u + dx
        return not (0 <= v < H and 0 <= u < W and m[v, u])

    while True:
        if not free(dy, dx):
            dy, dx = dx, -dy      # turn right
            if not free(dy, dx):
                return m
        y, x = y + dy, x + dx
        m[y, x] = True


def serpentine(H, W):
    """Every other row set, joined at alternating ends: one long component that fills the image."""
    m = np.zeros((H, W), bool)
    m[0::2, :] = True
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def comb(H, W):
    """A spine along the top row with a tooth in every other column."""
    m = np.zeros((H, W), bool)
    m[0, :] = True
    m[:, 0::2] = True
    if H > 2:
        m[H - 1, :] = False      # the teeth end above the last row
    return m


def checkerboard(H, W):
    """One component under 8-connectivity, all singletons under 4."""
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy + xx) % 2 == 0


def nested_rings(H, W):
    """A hole inside an island inside a hole: rings 2 pixels wide, 3 pixels apart, around the centre, clear of the border."""
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.maximum(np.abs(yy - H // 2), np.abs(xx - W // 2))
    return (d % 5 < 2) & (d < min(H, W) // 2 - 1)


def border_hole(H, W):
    """A set frame-like blob with one hole inside and one 'hole' that touches the image border (which must not be filled)."""
    m = np.zeros((H, W), bool)
    m[2:H - 2, 0:W - 3] = True
    m[H // 2 - 3:H // 2 + 3, 0:5] = False          # open to column 0: touches the border
    m[5:9, W // 2:W // 2 + 6] = False              # a true hole
    m[H - 8, W - 10] = False                       # a pin-hole
    return m


def row_wrap(H, W):
    """Components that would touch only across a row's end and the next row's start: (y, W - 1) and (y + 1, 0) are not neighbours."""
    m = np.zeros((H, W), bool)
    for y in range(0, H - 1, 3):
        m[y, W - 2:] = True
        m[y + 1, :2] = True
    return m


def sample_seam(H, W):
    """Sample s: objects on the LAST row; sample s + 1: objects on the FIRST row in the same columns (not neighbours across samples)."""
    out = np.zeros((B, H, W), bool)
    for s in range(B):
        out[s, H - 1, s::2] = True
        out[s, 0, (s + 1) % 2::2] = True
        out[s, H // 2, W // 3:W // 3 + 2 + s] = True
    return out


def speckled(rng, H, W):
    """What a contrast mask looks like: a few blobs ('cells') with pin-holes and ragged rims, specks on the background."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W), bool)
    for s in range(B):
        m = np.zeros((H, W), bool)
        for _ in range(4 + s):
            cy, cx = rng.integers(0, H), rng.integers(0, W)
            ry, rx = rng.integers(max(2, H // 10), max(3, H // 4)), rng.integers(max(2, W // 10), max(3, W // 4))
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        m &= rng.random((H, W)) > 0.03      # pin-holes
        m |= rng.random((H, W)) < 0.02      # specks
        out[s] = m
    return out


def _build():
    rng = np.random.default_rng(SEED)
    cases = {}
    for H, W in ((1, 1), (1, 53), (37, 1), (5, 7), (37, 53), (64, 64)):
        cases[f"random_{H}x{W}"] = _bytes(rng, _random(rng, H, W, (0.02, 0.5, 0.98)))
    for H, W in ((1, 53), (37, 53), (64, 64)):      # all clear, all set (the PD_MASK_FAR paths) beside a half-dense sample
        cases[f"extremes_{H}x{W}"] = _bytes(rng, np.stack([np.zeros((H, W), bool), np.ones((H, W), bool), rng.random((H, W)) < 0.5]))
    for H, W in ((37, 53), (64, 64)):
        cases[f"long_{H}x{W}"] = _bytes(rng, np.stack([spiral(H, W), serpentine(H, W), comb(H, W)]))
    cases["shapes_37x53"] = _bytes(rng, np.stack([checkerboard(37, 53), nested_rings(37, 53), border_hole(37, 53)]))
    cases["wrap_37x53"] = _bytes(rng, np.stack([row_wrap(37, 53), row_wrap(37, 53)[::-1].copy(), row_wrap(37, 53)[:, ::-1].copy()]))
    cases["seam_5x7"] = _bytes(rng, sample_seam(5, 7))
    cases["seam_37x53"] = _bytes(rng, sample_seam(37, 53))
    cases["speckled_64x64"] = _bytes(rng, speckled(rng, 64, 64))
    cases["speckled_256x256"] = _bytes(rng, speckled(rng, 256, 256))
    for v in cases.values():
        assert v.dtype == np.uint8 and v.ndim == 3 and v.shape[0] == B
        v.setflags(write=False)
    return cases


CASES = _build()
NAMES = list(CASES)
SMALL = [n for n in NAMES if CASES[n][0].size <= 64 * 64]      # everything but the 256 x 256 case
BIG = "speckled_256x256"
RADII = (1, 1.5, 2.9)
RECIPES = (dict(close=1.5, open=1.5, fill_holes=-1, min_area=6, dilate=3), dict(open=1, fill_holes=5, connectivity=4),
           dict(close=2, min_area=3, connectivity=4))


@functools.lru_cache(maxsize=None)
def reference(name, what, *args):
    """One reference result of case `name`, computed once: what in d2 / dilate / erode / open / close / label / drop_small / fill_holes /
    refine; args as the reference takes them (refine: the index into RECIPES)."""
    m = CASES[name]
    if what == "refine":
        out = R.refine_ref(m, **RECIPES[args[0]])
    else:
        out = {"d2": R.d2_ref, "dilate": R.dilate_ref, "erode": R.erode_ref, "open": R.open_ref, "close": R.close_ref, "label": R.label_ref,
               "drop_small": R.drop_small_ref, "fill_holes": R.fill_holes_ref}[what](m, *args)
    for a in (out if isinstance(out, tuple) else (out,)):
        a.setflags(write=False)
    return out
