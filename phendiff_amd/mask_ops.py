"""Mask refinement on the GPU: disc morphology, connected components, hole filling, removal of small components -- what makes a
per-pixel contrast mask (:func:`~phendiff_amd.masked.class_contrast_mask`) usable: the binarised ``|eps_target - eps_source|`` is a
thresholded noise difference, so it carries specks on the background, pin-holes inside cells and ragged outlines.

Kernels: ``csrc/mask_morph.hip`` (contract: ``include/phendiff_hip.h``) -- an exact squared Euclidean distance transform in int32
(``pd_mask_distance``), disc dilation / erosion by thresholding it (``pd_mask_morph``), label-equivalence union-find
(``pd_mask_components``) and the two filters over a labelled phase (``pd_mask_filter``).  All arithmetic is in integers: the results are
exact, equal to the plain definitions (``tests/mask_ops_ref.py``) and to SciPy's ``distance_transform_edt`` (squared),
``binary_dilation(border_value=0)`` / ``binary_erosion(border_value=1)`` under the disc ``{dy^2 + dx^2 <= floor(radius^2)}``, ``label``
(after canonicalising) and ``binary_fill_holes``.  The product imports neither SciPy nor OpenCV.

  * single calls on the current stream: :func:`mask_distance`, :func:`mask_dilate`, :func:`mask_erode`, :func:`mask_open`,
    :func:`mask_close`, :func:`mask_components`, :func:`remove_small_components`, :func:`fill_holes`;
  * :class:`MaskRefine`: the recipe close -> open -> fill holes -> drop small -> dilate as one object that owns every buffer and
    argument struct (capturable: a fixed list of launches, nothing read back), and :func:`refine_mask`, its one-call form.

Masks: (B, 1, H, W) or (B, H, W), bool or uint8 (nonzero = set), on an MI355X; H, W <= 16384.  The outside of the image is neither set nor
clear: an object the image edge cuts is not eroded from the edge, and a closing does not pull the border in.  A sample's result is a
function of that sample alone."""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import torch

from . import _lib as L

MASK_FAR = L.CONSTANTS["PD_MASK_FAR"]                  # the squared distance where a sample holds no pixel to measure to
MASK_MAX_SIDE = L.CONSTANTS["PD_MASK_MAX_SIDE"]
MASK_STATS_FIELDS = ("pixels_in", "pixels_out", "components", "selected", "status")
DILATE, ERODE = L.CONSTANTS["PD_MORPH_DILATE"], L.CONSTANTS["PD_MORPH_ERODE"]
STATS_IN, STATS_OUT = L.CONSTANTS["PD_MORPH_STATS_IN"], L.CONSTANTS["PD_MORPH_STATS_OUT"]
DROP_SMALL, FILL_HOLES = L.CONSTANTS["PD_FILTER_DROP_SMALL"], L.CONSTANTS["PD_FILTER_FILL_HOLES"]
STAGES = ("close", "open", "fill_holes", "min_area", "dilate")      # the recipe's fixed order
if len(MASK_STATS_FIELDS) != L.CONSTANTS["PD_MASK_STATS_FIELDS"]:
    raise L.PhenDiffHipError(f"{L.HEADER_PATH}: PD_MASK_STATS_FIELDS = {L.CONSTANTS['PD_MASK_STATS_FIELDS']}, {len(MASK_STATS_FIELDS)} names here")


# ---- host rules ------------------------------------------------------------------------------------------------------------------------------
def disc_r2(radius) -> int:
    """``floor(radius^2)`` in float64: the disc of ``radius`` is ``{dy^2 + dx^2 <= r2}``.  Radius 1 is the 4-neighbour cross (r2 = 1), 1.5
    the 3 x 3 square (2), 2 the 13-pixel disc (4), 2.9 gives 8."""
    try:
        r = float(radius)
    except (TypeError, ValueError):
        r = math.nan
    if isinstance(radius, bool) or not (math.isfinite(r) and r >= 0.0):
        raise ValueError(f"radius must be a finite number >= 0, got {radius!r}")
    r2 = math.floor(r * r)
    if r2 >= MASK_FAR:
        raise ValueError(f"radius = {r}: floor(radius^2) = {r2} reaches PD_MASK_FAR = {MASK_FAR}")
    return int(r2)


def dual_connectivity(connectivity: int) -> int:
    """The connectivity holes are labelled with: dual to the foreground's (8 -> 4, 4 -> 8; what ``binary_fill_holes`` implies)."""
    return {8: 4, 4: 8}[connectivity]


def _check_connectivity(connectivity, who):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"{who}: connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _check_area(value, name, who, least=0):
    if isinstance(value, bool) or not isinstance(value, int) or value < least:
        raise ValueError(f"{who}: {name} must be an integer >= {least}, got {value!r}")
    return int(value)


def _checked(mask, who):
    """(dense uint8 (B, H * W)-addressable view, B, H, W, the input's shape) of a mask given to a single-call function."""
    from .masked import _as_bytes, _require_cuda, check_mask      # (masked imports MaskRefine from here: resolved at call time)
    if not torch.is_tensor(mask) or mask.dim() not in (3, 4):
        raise ValueError(f"{who}: the mask must be a (B, 1, H, W) or (B, H, W) tensor, got {type(mask).__name__}"
                         + (f" of shape {tuple(mask.shape)}" if torch.is_tensor(mask) else ""))
    shape = tuple(mask.shape)
    B, H, W = shape[0], shape[-2], shape[-1]
    m = check_mask(mask, B, H, W, mask.device, who)
    if B < 1 or not (1 <= H <= MASK_MAX_SIDE and 1 <= W <= MASK_MAX_SIDE):
        raise ValueError(f"{who}: a ({B}, {H}, {W}) mask (B >= 1, each side 1 to {MASK_MAX_SIDE})")
    _require_cuda(mask, who)
    return _as_bytes(m), B, H, W, shape


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


# ---- argument structs --------------------------------------------------------------------------------------------------------------------
def mask_distance_args(mask: torch.Tensor, d2: torch.Tensor, to_set: bool, limit: int, B: int, H: int, W: int) -> "L.MaskDistanceArgs":
    """``pd_mask_distance`` over a dense uint8 mask of B * H * W bytes into the dense int32 ``d2``."""
    return L.MaskDistanceArgs(B=B, H=H, W=W, mask=mask.data_ptr(), to_set=int(bool(to_set)), limit=int(limit), d2=d2.data_ptr())


def mask_morph_args(mask, out: torch.Tensor, op: int, r2: int, workspace: torch.Tensor, B: int, H: int, W: int, stats=None, stats_stride: int = 0,
                    stats_mode: int = 0) -> "L.MaskMorphArgs":
    """``pd_mask_morph``.  ``mask``: a tensor, or ``None`` for a source that is set at enqueue time; ``stats``: an int32 view whose first
    five elements are sample 0's row (``stats_stride`` words between samples), or ``None``; ``stats_mode``: ``STATS_IN | STATS_OUT``."""
    return L.MaskMorphArgs(B=B, H=H, W=W, mask=L.ptr(mask), op=op, r2=int(r2), out=out.data_ptr(), workspace=workspace.data_ptr(),
                           stats=L.ptr(stats), stats_stride=int(stats_stride), stats_mode=int(stats_mode))


def mask_components_args(mask, phase: int, connectivity: int, workspace: torch.Tensor, B: int, H: int, W: int, label=None, area=None, border=None,
                         count=None, status=None) -> "L.MaskComponentsArgs":
    """``pd_mask_components``: ``label`` / ``area`` int32 and ``border`` uint8 of the mask's size, ``count`` / ``status`` int32 (B,)."""
    return L.MaskComponentsArgs(B=B, H=H, W=W, mask=L.ptr(mask), phase=int(phase), connectivity=int(connectivity), label=L.ptr(label),
                                area=L.ptr(area), border=L.ptr(border), count=L.ptr(count), status=L.ptr(status), workspace=workspace.data_ptr())


def mask_filter_args(mask, label, area, border, rule: int, area_limit: int, out: torch.Tensor, B: int, H: int, W: int, status=None, stats=None,
                     stats_stride: int = 0) -> "L.MaskFilterArgs":
    """``pd_mask_filter``: ``stats`` is an int32 view whose first five elements are sample 0's row (``stats_stride`` words between samples)."""
    return L.MaskFilterArgs(B=B, H=H, W=W, mask=L.ptr(mask), label=label.data_ptr(), area=area.data_ptr(), border=border.data_ptr(),
                            status=L.ptr(status), rule=int(rule), area_limit=int(area_limit), out=out.data_ptr(), stats=L.ptr(stats),
                            stats_stride=int(stats_stride))


def _morph_workspace(B, H, W, dev):
    size = L.lib().pd_mask_morph_workspace(B, H, W)
    if size == 0:
        raise ValueError(f"mask morphology: no launch over a ({B}, {H}, {W}) mask")
    return torch.empty((size // 4,), dtype=torch.int32, device=dev)


def _components_workspace(B, H, W, dev):
    size = L.lib().pd_mask_components_workspace(B, H, W)
    if size == 0:
        raise ValueError(f"mask components: no launch over a ({B}, {H}, {W}) mask")
    return torch.empty((size // 4,), dtype=torch.int32, device=dev)


# ---- single calls on the current stream --------------------------------------------------------------------------------------------------
def mask_distance(mask: torch.Tensor, to_set: bool = False, limit: int = None) -> torch.Tensor:
    """The exact squared Euclidean distance, int32 in the mask's shape, from every pixel to the nearest clear pixel of its sample
    (``to_set=True``: to the nearest set pixel) -- 0 on such a pixel, ``MASK_FAR`` (2^30) everywhere in a sample that holds none.
    ``limit`` (an integer > 0): every value above it is returned as ``limit + 1`` and the cost per pixel is O(sqrt(limit)).
    ``scipy.ndimage.distance_transform_edt(mask) ** 2`` is ``to_set=False``."""
    who = "mask_distance"
    limit = 0 if limit is None else _check_area(limit, "limit", who, least=1)
    if limit >= MASK_FAR:
        raise ValueError(f"{who}: limit = {limit} reaches PD_MASK_FAR = {MASK_FAR}")
    m, B, H, W, shape = _checked(mask, who)
    d2 = torch.empty(shape, dtype=torch.int32, device=m.device)
    L.check(L.lib().pd_mask_distance(C.byref(mask_distance_args(m, d2, to_set, limit, B, H, W)), _stream(m)), "pd_mask_distance")
    return d2


def _morph_chain(mask, ops, radius, who):
    r2 = disc_r2(radius)
    m, B, H, W, shape = _checked(mask, who)
    ws = _morph_workspace(B, H, W, m.device)
    cur = m
    for op in ops:
        out = torch.empty(shape, dtype=torch.uint8, device=m.device)
        L.check(L.lib().pd_mask_morph(C.byref(mask_morph_args(cur, out, op, r2, ws, B, H, W)), _stream(m)), "pd_mask_morph")
        cur = out
    return cur


def mask_dilate(mask: torch.Tensor, radius: float) -> torch.Tensor:
    """Dilation by the disc ``{dy^2 + dx^2 <= floor(radius^2)}``: uint8 0 / 1 in the mask's shape."""
    return _morph_chain(mask, (DILATE,), radius, "mask_dilate")


def mask_erode(mask: torch.Tensor, radius: float) -> torch.Tensor:
    """Erosion by the disc; the outside of the image counts as set (an object the edge cuts is not eroded from the edge)."""
    return _morph_chain(mask, (ERODE,), radius, "mask_erode")


def mask_open(mask: torch.Tensor, radius: float) -> torch.Tensor:
    """Erosion, then dilation: removes what the disc does not fit into.  Idempotent."""
    return _morph_chain(mask, (ERODE, DILATE), radius, "mask_open")


def mask_close(mask: torch.Tensor, radius: float) -> torch.Tensor:
    """Dilation, then erosion: fills what the disc does not fit into.  Idempotent."""
    return _morph_chain(mask, (DILATE, ERODE), radius, "mask_close")


def _label(m, B, H, W, shape, phase, connectivity, want_label=True):
    dev = m.device
    out = SimpleNamespace(label=torch.empty(shape, dtype=torch.int32, device=dev) if want_label else None,
                          area=torch.empty(shape, dtype=torch.int32, device=dev), border=torch.empty(shape, dtype=torch.uint8, device=dev),
                          count=torch.empty((B,), dtype=torch.int32, device=dev), status=torch.empty((B,), dtype=torch.int32, device=dev))
    ws = _components_workspace(B, H, W, dev)
    a = mask_components_args(m, phase, connectivity, ws, B, H, W, out.label, out.area, out.border, out.count, out.status)
    L.check(L.lib().pd_mask_components(C.byref(a), _stream(m)), "pd_mask_components")
    return out


def mask_components(mask: torch.Tensor, connectivity: int = 8, phase: int = 1) -> SimpleNamespace:
    """Connected components of the set pixels (``phase=0``: of the clear pixels) under 4- or 8-connectivity.  Returns a namespace, all on
    the device: ``.label`` (int32, the mask's shape: 1 + the smallest linear index ``y * W + x`` of the component, 0 on the other phase),
    ``.area`` (int32: the pixel count of the pixel's component), ``.border`` (uint8: the component touches the image border), ``.count``
    (int32 (B,)) and ``.status`` (int32 (B,): 0)."""
    who = "mask_components"
    connectivity = _check_connectivity(connectivity, who)
    if isinstance(phase, bool) or phase not in (0, 1):
        raise ValueError(f"{who}: phase must be 1 (the set pixels) or 0 (the clear pixels), got {phase!r}")
    m, B, H, W, shape = _checked(mask, who)
    return _label(m, B, H, W, shape, phase, connectivity)


def _filter(mask, who, rule, phase, connectivity, area_limit):
    m, B, H, W, shape = _checked(mask, who)
    lab = _label(m, B, H, W, shape, phase, connectivity)
    out = torch.empty(shape, dtype=torch.uint8, device=m.device)
    a = mask_filter_args(m, lab.label, lab.area, lab.border, rule, area_limit, out, B, H, W, status=lab.status)
    L.check(L.lib().pd_mask_filter(C.byref(a), _stream(m)), "pd_mask_filter")
    return out


def remove_small_components(mask: torch.Tensor, min_area: int, connectivity: int = 8) -> torch.Tensor:
    """The mask without the components of fewer than ``min_area`` pixels (uint8 0 / 1 in the mask's shape)."""
    who = "remove_small_components"
    return _filter(mask, who, DROP_SMALL, 1, _check_connectivity(connectivity, who), _check_area(min_area, "min_area", who))


def fill_holes(mask: torch.Tensor, max_area: int = None, connectivity: int = 8) -> torch.Tensor:
    """The mask with its holes set: the components of clear pixels -- under the connectivity dual to the foreground's ``connectivity`` --
    that do not touch the image border and have at most ``max_area`` pixels (``None``: any size, ``scipy.ndimage.binary_fill_holes``)."""
    who = "fill_holes"
    limit = -1 if max_area is None else _check_area(max_area, "max_area", who)
    return _filter(mask, who, FILL_HOLES, 0, dual_connectivity(_check_connectivity(connectivity, who)), limit)


# ---- the recipe ------------------------------------------------------------------------------------------------------------------------------
class MaskRefine:
    """The refinement recipe as one object, for a (B, H, W) batch on ``device``:

        close (radius)  ->  open (radius)  ->  fill holes (max area; -1: any size)  ->  drop components below ``min_area``  ->  dilate (radius)

    in this fixed order; a stage whose parameter is 0 is skipped.  ``connectivity`` (4 or 8) is the foreground's; holes are labelled with
    its dual.  The object owns every buffer and argument struct, so whoever keeps it (a runner's captured graph) keeps the memory it
    launches into.  :meth:`enqueue` ``(st, src)`` enqueues the launches of :meth:`plan` on stream ``st`` -- 2 per dilation or erosion, 6
    per labelled stage -- and leaves the result in ``.mask`` ((B, 1, H, W) uint8, 0 / 1).  The buffers ping-pong; ``src`` is never written.
    ``.stats``: (B, stages, 5) int32, one row per ENABLED stage (``.stages`` names them, in order): set pixels in, set pixels out,
    components seen, components kept (``min_area``) or filled (``fill_holes``) -- both 0 for a morphological stage -- and status (0)."""

    DEFAULTS = dict(close=0.0, open=0.0, fill_holes=0, min_area=0, dilate=0.0, connectivity=8)

    @staticmethod
    def check_params(**params) -> dict:
        """The normalised parameters (every key of ``DEFAULTS``), or ``ValueError``: unknown keys, negative or non-finite radii, a radius in
        (0, 1) (its disc is the pixel itself), a radius whose ``floor(radius^2)`` reaches ``PD_MASK_FAR``, ``fill_holes`` below -1 or
        ``min_area`` below 0 or not integers, ``connectivity`` not in (4, 8), and parameters that are all zero (nothing to do).  Touches no
        device and allocates nothing."""
        who = "MaskRefine"
        unknown = sorted(set(params) - set(MaskRefine.DEFAULTS))
        if unknown:
            raise ValueError(f"{who}: unknown parameters {unknown} (known: {sorted(MaskRefine.DEFAULTS)})")
        p = dict(MaskRefine.DEFAULTS, **params)
        for name in ("close", "open", "dilate"):
            try:
                r2 = disc_r2(p[name])
            except ValueError as e:
                raise ValueError(f"{who}: {name}: {e}") from None
            p[name] = float(p[name])
            if p[name] > 0.0 and r2 == 0:
                raise ValueError(f"{who}: {name} = {p[name]}: the disc of a radius below 1 is the pixel itself (0 skips the stage)")
        p["fill_holes"] = _check_area(p["fill_holes"], "fill_holes", who, least=-1)
        p["min_area"] = _check_area(p["min_area"], "min_area", who)
        p["connectivity"] = _check_connectivity(p["connectivity"], who)
        if not any(p[name] for name in STAGES):
            raise ValueError(f"{who}: every stage's parameter is 0: nothing to refine")
        return p

    @staticmethod
    def plan(**params) -> list:
        """The launches of the recipe, in order, as (stage, entry point, details) -- host arithmetic only."""
        p = MaskRefine.check_params(**params)
        conn, out = p["connectivity"], []
        for stage in STAGES:
            if not p[stage]:
                continue
            if stage in ("close", "open", "dilate"):
                r2 = disc_r2(p[stage])
                for op in {"close": ("dilate", "erode"), "open": ("erode", "dilate"), "dilate": ("dilate",)}[stage]:
                    out.append((stage, "pd_mask_morph", dict(op=op, r2=r2)))
            elif stage == "fill_holes":
                out.append((stage, "pd_mask_components", dict(phase=0, connectivity=dual_connectivity(conn))))
                out.append((stage, "pd_mask_filter", dict(rule="fill_holes", area_limit=p[stage])))
            else:
                out.append((stage, "pd_mask_components", dict(phase=1, connectivity=conn)))
                out.append((stage, "pd_mask_filter", dict(rule="drop_small", area_limit=p[stage])))
        return out

    def __init__(self, B: int, H: int, W: int, device, **params):
        self.params = MaskRefine.check_params(**params)
        B, H, W = int(B), int(H), int(W)
        if B < 1 or not (1 <= H <= MASK_MAX_SIDE and 1 <= W <= MASK_MAX_SIDE):
            raise ValueError(f"MaskRefine: a ({B}, {H}, {W}) batch (B >= 1, each side 1 to {MASK_MAX_SIDE})")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.PhenDiffHipError("MaskRefine: phendiff_amd runs on MI355X only (no CPU fallback): device must be 'cuda'")
        self.B, self.H, self.W, self.device = B, H, W, dev
        steps = MaskRefine.plan(**self.params)
        self.stages = tuple(s for s in STAGES if self.params[s])
        n = len(self.stages)
        self.stats = torch.empty((B, n, len(MASK_STATS_FIELDS)), dtype=torch.int32, device=dev)      # (every enqueue writes every word)
        stride = n * len(MASK_STATS_FIELDS)
        self._bufs = [torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev) for _ in range(2 if len(steps) > 1 else 1)]
        self._morph_ws = _morph_workspace(B, H, W, dev) if any(fn == "pd_mask_morph" for _, fn, _ in steps) else None
        if any(fn == "pd_mask_components" for _, fn, _ in steps):
            self._comp_ws = _components_workspace(B, H, W, dev)
            self._label = torch.empty((B, H, W), dtype=torch.int32, device=dev)
            self._area = torch.empty((B, H, W), dtype=torch.int32, device=dev)
            self._border = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
            self._status = torch.empty((B,), dtype=torch.int32, device=dev)
        lib = L.lib()
        self.ops, self._src_args = [], []      # (name, function, struct); the structs whose .mask is the source, set by enqueue
        cur, free = None, 0                    # the tensor the next launch reads (None: the source) and the buffer it may write

        def reads(a):
            if cur is None:
                self._src_args.append(a)
            return a

        for i, (stage, fn, d) in enumerate(steps):
            row = self.stats[0, self.stages.index(stage)]
            if fn == "pd_mask_morph":
                first = i == 0 or steps[i - 1][0] != stage
                last = i + 1 == len(steps) or steps[i + 1][0] != stage
                out = self._bufs[free]
                a = reads(mask_morph_args(cur, out, DILATE if d["op"] == "dilate" else ERODE, d["r2"], self._morph_ws, B, H, W,
                                          stats=row, stats_stride=stride, stats_mode=(STATS_IN if first else 0) | (STATS_OUT if last else 0)))
                cur, free = out, 1 - free
            elif fn == "pd_mask_components":
                a = reads(mask_components_args(cur, d["phase"], d["connectivity"], self._comp_ws, B, H, W, self._label, self._area, self._border,
                                               None, self._status))
            else:
                out = self._bufs[free]
                a = reads(mask_filter_args(cur, self._label, self._area, self._border, FILL_HOLES if d["rule"] == "fill_holes" else DROP_SMALL,
                                           d["area_limit"], out, B, H, W, status=self._status, stats=row, stats_stride=stride))
                cur, free = out, 1 - free
            self.ops.append((fn, getattr(lib, fn), a))
        self.mask = cur

    def enqueue(self, st: int, src: torch.Tensor):
        """Enqueue the recipe over ``src`` (dense uint8, B * H * W elements, on the object's device; read, never written) on stream ``st``."""
        if not (torch.is_tensor(src) and src.dtype == torch.uint8 and src.is_contiguous() and src.numel() == self.B * self.H * self.W
                and src.device == self.device):
            raise ValueError(f"MaskRefine.enqueue: src must be a dense uint8 mask of {self.B} x {self.H} x {self.W} elements on {self.device}")
        for a in self._src_args:
            a.mask = src.data_ptr()
        for name, fn, a in self.ops:
            L.check(fn(C.byref(a), st), name)
        return self


def refine_mask(mask: torch.Tensor, **params) -> torch.Tensor:
    """The recipe of :class:`MaskRefine` over ``mask`` on the current stream: uint8 0 / 1 in the mask's shape.  ``refine_mask(m, close=1.5,
    open=1.5, fill_holes=-1, min_area=64, dilate=3)``."""
    params = MaskRefine.check_params(**params)
    m, B, H, W, shape = _checked(mask, "refine_mask")
    r = MaskRefine(B, H, W, m.device, **params)
    r.enqueue(_stream(m), m)
    return r.mask.view(shape)
