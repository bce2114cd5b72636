"""Per-object measurements on the GPU: from a mask to a table with one row per object -- dense labels, shape, intensity -- without a
copy to the host and without ``scipy.ndimage`` / ``skimage.regionprops`` (the product imports neither).

Kernels: ``csrc/object_stats.hip`` (contract: ``include/phendiff_hip.h``), after ``pd_mask_components`` (``csrc/mask_morph.hip``):
``pd_object_index`` (dense labels ``1..count`` in ``scipy.ndimage.label``'s numbering), ``pd_object_geometry`` (one int64 row per object:
area, bounding box, raw moments, edges, border) and ``pd_object_intensity`` (fp64 sum, sum of squares, min, max of an image stack under the
labels, per channel).  Integers are exact; floating-point sums are fp64 in a fixed order, bitwise reproducible; a sample's rows are a
function of that sample alone; nothing is read back by the host.

  * :func:`label_objects` (mask -> :class:`ObjectLabels`) and :func:`measure_intensity` (labels, images -> sums and moments): single
    calls on the current stream;
  * :class:`ObjectMeasure`: both as one object that owns every buffer and argument struct (capturable: 12 launches, nothing read back);
  * :func:`object_change` (two stacks under one set of labels) and :func:`measure_transfer` (the same over the output of
    :func:`~phendiff_amd.masked.masked_ddib`).

Tables have ``K = max_objects`` rows per sample; row ``k - 1`` belongs to index ``k``; rows past ``min(count, K)`` are zero."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import torch

from . import _lib as L
from .mask_ops import MASK_MAX_SIDE, _check_area, _check_connectivity, _checked, _components_workspace, _stream, mask_components_args

GEOM_FIELDS = ("area", "y0", "y1", "x0", "x1", "sum_y", "sum_x", "sum_yy", "sum_xx", "sum_yx", "edges", "border")
INTENSITY_FIELDS = ("sum", "sumsq", "min", "max")
OBJ_OVERFLOW, OBJ_BAD_LABEL, OBJ_LABEL_STATUS = (L.CONSTANTS[n] for n in ("PD_OBJ_OVERFLOW", "PD_OBJ_BAD_LABEL", "PD_OBJ_LABEL_STATUS"))
MAX_OBJECTS = L.CONSTANTS["PD_OBJ_MAX_OBJECTS"]
IMAGE_DTYPES = {torch.float32: L.CONSTANTS["PD_OBJ_F32"], torch.uint8: L.CONSTANTS["PD_OBJ_U8"], torch.uint16: L.CONSTANTS["PD_OBJ_U16"]}
for _names, _prefix, _total in ((GEOM_FIELDS, "PD_OG_", "PD_OBJ_GEOM_FIELDS"), (INTENSITY_FIELDS, "PD_OI_", "PD_OBJ_INTENSITY_FIELDS")):
    if [L.CONSTANTS[_prefix + n.upper()] for n in _names] != list(range(L.CONSTANTS[_total])):
        raise L.PhenDiffHipError(f"{L.HEADER_PATH}: the {_prefix}* enumerators are not {_names} in this order")


class ObjectLabels(SimpleNamespace):
    """What :func:`label_objects` returns, all on the device; ``K = max_objects``:

    ``.index`` (int32, the mask's shape: 0 on clear pixels, else ``k`` in ``1..count`` -- ``scipy.ndimage.label``'s numbering),
    ``.count`` (int32 (B,): the true number of components), ``.status`` (int32 (B,): 0, or ``OBJ_OVERFLOW`` where ``count > K`` --
    components past ``K`` then have index 0 and no row), ``.geometry`` (int64 (B, K, 12), columns ``GEOM_FIELDS``), ``.valid``
    ((B, K) bool: the row holds an object) and the float64 tables of :func:`shape_tables`."""


# ---- host rules ------------------------------------------------------------------------------------------------------------------------------
def _check_max_objects(value, who):
    value = _check_area(value, "max_objects", who, least=1)
    if value > MAX_OBJECTS:
        raise ValueError(f"{who}: max_objects = {value} above PD_OBJ_MAX_OBJECTS = {MAX_OBJECTS}")
    return value


def _check_images(images, B, H, W, device, who, channels=None, dtype=None):
    """A dense (B, C, H, W) float32 / uint8 / uint16 stack on ``device`` (``channels`` / ``dtype``: what it must be), or ``ValueError``."""
    if not torch.is_tensor(images) or images.dim() != 4:
        raise ValueError(f"{who}: the images must be a (B, C, H, W) tensor, got {type(images).__name__}"
                         + (f" of shape {tuple(images.shape)}" if torch.is_tensor(images) else ""))
    if images.dtype not in IMAGE_DTYPES or (dtype is not None and images.dtype != dtype):
        raise ValueError(f"{who}: the images must be {dtype if dtype is not None else 'float32, uint8 or uint16'}, got {images.dtype}")
    Bi, Cc, Hi, Wi = images.shape
    if (Bi, Hi, Wi) != (B, H, W) or Cc < 1 or (channels is not None and Cc != channels):
        raise ValueError(f"{who}: the images have shape {tuple(images.shape)}, the labels are ({B}, {H}, {W})"
                         + (f" and C = {channels}" if channels is not None else ""))
    if images.device != torch.device(device):
        raise ValueError(f"{who}: the images live on {images.device}, the labels on {torch.device(device)}")
    return images.contiguous()


def _check_labels(labels, who):
    if not (isinstance(labels, SimpleNamespace) and all(torch.is_tensor(getattr(labels, n, None)) for n in ("index", "geometry"))):
        raise ValueError(f"{who}: labels must be what label_objects returns, got {type(labels).__name__}")
    index, geometry = labels.index, labels.geometry
    if index.dtype != torch.int32 or index.dim() not in (3, 4) or geometry.dtype != torch.int64 or geometry.dim() != 3 \
            or geometry.shape[0] != index.shape[0] or geometry.shape[2] != len(GEOM_FIELDS) or geometry.device != index.device:
        raise ValueError(f"{who}: labels.index must be int32 (B, H, W) and labels.geometry int64 (B, K, {len(GEOM_FIELDS)}) on one device")
    B, H, W = index.shape[0], index.shape[-2], index.shape[-1]
    if index.numel() != B * H * W:
        raise ValueError(f"{who}: labels.index has shape {tuple(index.shape)}")
    return index.contiguous(), geometry.contiguous(), B, H, W, geometry.shape[1]


# ---- argument structs --------------------------------------------------------------------------------------------------------------------
def object_index_args(label, index, count, status, workspace, max_objects: int, B: int, H: int, W: int, label_status=None) -> "L.ObjectIndexArgs":
    """``pd_object_index``: ``label`` / ``index`` dense int32 of B * H * W elements, ``count`` / ``status`` / ``label_status`` int32 (B,)."""
    return L.ObjectIndexArgs(B=B, H=H, W=W, max_objects=int(max_objects), label=label.data_ptr(), label_status=L.ptr(label_status),
                             index=index.data_ptr(), count=count.data_ptr(), status=status.data_ptr(), workspace=workspace.data_ptr())


def object_geometry_args(index, geometry, max_objects: int, B: int, H: int, W: int) -> "L.ObjectGeometryArgs":
    """``pd_object_geometry``: ``geometry`` dense int64 (B, K, 12)."""
    return L.ObjectGeometryArgs(B=B, H=H, W=W, max_objects=int(max_objects), index=index.data_ptr(), geometry=geometry.data_ptr())


def object_intensity_args(index, geometry, images, out, max_objects: int, B: int, H: int, W: int, channels: int, dtype) -> "L.ObjectIntensityArgs":
    """``pd_object_intensity``: ``images`` a tensor (dense (B, C, H, W) of ``dtype``) or ``None`` for a stack set at enqueue time; ``out``
    dense float64 (B, K, C, 4)."""
    return L.ObjectIntensityArgs(B=B, H=H, W=W, max_objects=int(max_objects), C=int(channels), dtype=IMAGE_DTYPES[dtype], index=index.data_ptr(),
                                 geometry=geometry.data_ptr(), images=L.ptr(images), out=out.data_ptr())


def _index_workspace(B, H, W, dev):
    size = L.lib().pd_object_index_workspace(B, H, W)
    if size == 0:
        raise ValueError(f"object index: no launch over a ({B}, {H}, {W}) batch")
    return torch.empty((size // 4,), dtype=torch.int32, device=dev)


# ---- derived tables: ordinary torch arithmetic on (B, K) -----------------------------------------------------------------------------------
def shape_tables(geometry: torch.Tensor) -> dict:
    """The float64 shape numbers of an int64 (B, K, 12) geometry table (plumbing: elementwise torch arithmetic on (B, K) tensors, on the
    table's device).  With ``A = area`` and the raw sums over the object's pixel centres ``(y, x)``:

        centroid            (cy, cx) = (sum_y / A, sum_x / A)
        bbox                (y0, x0, y1 + 1, x1 + 1)                        half open, as ``skimage.measure.regionprops``
        central moments     myy = sum_yy / A - cy^2 + 1/12,   mxx = sum_xx / A - cx^2 + 1/12,   myx = sum_yx / A - cy cx
                            (the 1/12 is the second moment of a unit pixel about its centre: a single pixel has a nonzero extent)
        eigenvalues         d = sqrt((myy - mxx)^2 + 4 myx^2);   l1 = (myy + mxx + d) / 2,   l2 = max((myy + mxx - d) / 2, 0)
        major / minor_axis_length   4 sqrt(l1), 4 sqrt(l2)                  (the ellipse with the object's second moments)
        eccentricity        sqrt(1 - l2 / l1)
        orientation         atan2(2 myx, myy - mxx) / 2                     the angle from the row axis to the major axis, in (-pi/2, pi/2]
        edges, border       as counted (float64)

    Rows without an object (``A == 0``) hold 0 everywhere.  An a x b rectangle: axis lengths ``4 max(a, b) / sqrt(12)`` and
    ``4 min(a, b) / sqrt(12)``."""
    g = geometry.to(torch.float64)
    col = {n: g[..., i] for i, n in enumerate(GEOM_FIELDS)}
    A = col["area"]
    valid = geometry[..., 0] > 0
    safe = torch.where(valid, A, torch.ones_like(A))
    cy, cx = col["sum_y"] / safe, col["sum_x"] / safe
    myy = col["sum_yy"] / safe - cy * cy + 1.0 / 12.0
    mxx = col["sum_xx"] / safe - cx * cx + 1.0 / 12.0
    myx = col["sum_yx"] / safe - cy * cx
    d = torch.sqrt((myy - mxx) * (myy - mxx) + 4.0 * (myx * myx))
    l1 = (myy + mxx + d) / 2.0
    l2 = torch.clamp((myy + mxx - d) / 2.0, min=0.0)
    zero = torch.zeros_like(A)

    def keep(t):
        return torch.where(valid, t, zero)

    return dict(valid=valid, area=A, centroid=torch.stack([keep(cy), keep(cx)], dim=-1),
                bbox=torch.stack([col["y0"], col["x0"], keep(col["y1"] + 1.0), keep(col["x1"] + 1.0)], dim=-1),
                edges=col["edges"], border=col["border"], orientation=keep(0.5 * torch.atan2(2.0 * myx, myy - mxx)),
                major_axis_length=keep(4.0 * torch.sqrt(l1)), minor_axis_length=keep(4.0 * torch.sqrt(l2)),
                eccentricity=keep(torch.sqrt(torch.clamp(1.0 - l2 / l1, min=0.0))))


def intensity_tables(raw: torch.Tensor, area: torch.Tensor) -> SimpleNamespace:
    """``.sum, .mean, .std`` (population: ``sqrt(max(sumsq / n - mean^2, 0))``), ``.min, .max`` -- (B, K, C) float64 -- and ``.valid``
    ((B, K) bool) of a raw (B, K, C, 4) table and the (B, K) areas; rows without an object hold 0."""
    valid = area > 0
    n = torch.where(valid, area, torch.ones_like(area)).to(torch.float64)[..., None]
    mean = raw[..., 0] / n
    var = torch.clamp(raw[..., 1] / n - mean * mean, min=0.0)
    std = torch.where(torch.isnan(raw[..., 1]), raw[..., 1], torch.sqrt(var))      # (clamp turns a NaN into 0: a NaN inside an object stays one)
    return SimpleNamespace(sum=raw[..., 0], mean=mean, std=std, min=raw[..., 2], max=raw[..., 3], valid=valid, raw=raw)


# ---- single calls on the current stream --------------------------------------------------------------------------------------------------
def label_objects(mask: torch.Tensor, connectivity: int = 8, max_objects: int = 1024) -> ObjectLabels:
    """The objects of a mask ((B, 1, H, W) or (B, H, W), bool or uint8, on an MI355X): the connected components of its set pixels under
    4- or 8-connectivity, numbered ``1..count`` in raster order of their first pixel, and one geometry row each for the first
    ``max_objects`` of them.  ``pd_mask_components`` -> ``pd_object_index`` -> ``pd_object_geometry`` on the current stream, 11 launches;
    returns an :class:`ObjectLabels`."""
    who = "label_objects"
    connectivity = _check_connectivity(connectivity, who)
    K = _check_max_objects(max_objects, who)
    m, B, H, W, shape = _checked(mask, who)
    dev, st, lib = m.device, _stream(m), L.lib()
    index = torch.empty(shape, dtype=torch.int32, device=dev)
    count, status, comp_status = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(3))
    geometry = torch.empty((B, K, len(GEOM_FIELDS)), dtype=torch.int64, device=dev)
    a = mask_components_args(m, 1, connectivity, _components_workspace(B, H, W, dev), B, H, W, label=index, status=comp_status)
    L.check(lib.pd_mask_components(C.byref(a), st), "pd_mask_components")
    a = object_index_args(index, index, count, status, _index_workspace(B, H, W, dev), K, B, H, W, label_status=comp_status)      # in place
    L.check(lib.pd_object_index(C.byref(a), st), "pd_object_index")
    L.check(lib.pd_object_geometry(C.byref(object_geometry_args(index, geometry, K, B, H, W)), st), "pd_object_geometry")
    return ObjectLabels(index=index, count=count, status=status, geometry=geometry, connectivity=connectivity, max_objects=K,
                        **shape_tables(geometry))


def _measure_raw(index, geometry, images, B, H, W, K):
    out = torch.empty((B, K, images.shape[1], len(INTENSITY_FIELDS)), dtype=torch.float64, device=index.device)
    a = object_intensity_args(index, geometry, images, out, K, B, H, W, images.shape[1], images.dtype)
    L.check(L.lib().pd_object_intensity(C.byref(a), _stream(index)), "pd_object_intensity")
    return out


def measure_intensity(labels: ObjectLabels, images: torch.Tensor) -> SimpleNamespace:
    """The intensity of ``images`` ((B, C, H, W), float32 / uint8 / uint16, on the labels' device) under ``labels``: ``.sum, .mean, .std``
    (population), ``.min, .max``, each (B, K, C) float64, ``.valid`` (B, K) bool and ``.raw`` (B, K, C, 4); rows without an object hold
    0.  One launch on the current stream.  The sums are exact for the integer types (below 2^53) and bitwise reproducible for float32."""
    who = "measure_intensity"
    index, geometry, B, H, W, K = _check_labels(labels, who)
    from .masked import _require_cuda
    images = _check_images(images, B, H, W, index.device, who)
    _require_cuda(index, who)
    return intensity_tables(_measure_raw(index, geometry, images, B, H, W, K), geometry[..., 0])


# ---- the capturable form -------------------------------------------------------------------------------------------------------------------
class ObjectMeasure:
    """Labels, geometry and intensity of a (B, H, W) mask and a (B, C, H, W) image stack of ``dtype`` as one object that owns every
    buffer, workspace and argument struct, so whoever keeps it (a captured graph) keeps the memory it launches into.  :meth:`enqueue`
    ``(st, mask, images)`` enqueues 12 launches on stream ``st`` (``pd_mask_components`` 4, ``pd_object_index`` 4, ``pd_object_geometry``
    3, ``pd_object_intensity`` 1) and reads nothing back; the results are ``.index`` (int32 (B, H, W)), ``.count`` / ``.status`` (int32
    (B,)), ``.geometry`` (int64 (B, K, 12)) and ``.intensity`` (float64 (B, K, C, 4): sum, sum of squares, min, max).  Neither input is
    written.  :meth:`tables` derives the float64 tables of :func:`label_objects` and :func:`measure_intensity` from them."""

    def __init__(self, B: int, H: int, W: int, C: int, device, connectivity: int = 8, max_objects: int = 1024, dtype=torch.float32):
        who = "ObjectMeasure"
        self.connectivity = _check_connectivity(connectivity, who)
        K = self.max_objects = _check_max_objects(max_objects, who)
        if dtype not in IMAGE_DTYPES:
            raise ValueError(f"{who}: dtype must be float32, uint8 or uint16, got {dtype!r}")
        if any(isinstance(v, bool) or not isinstance(v, int) for v in (B, H, W, C)) or B < 1 or C < 1 \
                or not (1 <= H <= MASK_MAX_SIDE and 1 <= W <= MASK_MAX_SIDE):
            raise ValueError(f"{who}: a ({B!r}, {C!r}, {H!r}, {W!r}) stack (integers; B, C >= 1, each side 1 to {MASK_MAX_SIDE})")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.PhenDiffHipError(f"{who}: phendiff_amd runs on MI355X only (no CPU fallback): device must be 'cuda'")
        self.B, self.H, self.W, self.C, self.device, self.dtype = B, H, W, C, dev, dtype
        self.index = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        self.count, self.status, self._comp_status = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(3))
        self.geometry = torch.empty((B, K, len(GEOM_FIELDS)), dtype=torch.int64, device=dev)
        self.intensity = torch.empty((B, K, C, len(INTENSITY_FIELDS)), dtype=torch.float64, device=dev)
        self._comp_ws, self._index_ws = _components_workspace(B, H, W, dev), _index_workspace(B, H, W, dev)
        lib = L.lib()
        self._components = mask_components_args(None, 1, self.connectivity, self._comp_ws, B, H, W, label=self.index, status=self._comp_status)
        self._intensity = object_intensity_args(self.index, self.geometry, None, self.intensity, K, B, H, W, C, dtype)
        self.ops = [("pd_mask_components", lib.pd_mask_components, self._components),
                    ("pd_object_index", lib.pd_object_index,
                     object_index_args(self.index, self.index, self.count, self.status, self._index_ws, K, B, H, W, label_status=self._comp_status)),
                    ("pd_object_geometry", lib.pd_object_geometry, object_geometry_args(self.index, self.geometry, K, B, H, W)),
                    ("pd_object_intensity", lib.pd_object_intensity, self._intensity)]

    def enqueue(self, st: int, mask: torch.Tensor, images: torch.Tensor):
        """Enqueue the measurement of ``mask`` (dense uint8, B * H * W elements) and ``images`` (dense (B, C, H, W) of the object's dtype),
        both on the object's device, on stream ``st``."""
        if not (torch.is_tensor(mask) and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == self.B * self.H * self.W
                and mask.device == self.device):
            raise ValueError(f"ObjectMeasure.enqueue: mask must be a dense uint8 mask of {self.B} x {self.H} x {self.W} elements on {self.device}")
        if not (torch.is_tensor(images) and images.dtype == self.dtype and images.is_contiguous()
                and tuple(images.shape) == (self.B, self.C, self.H, self.W) and images.device == self.device):
            raise ValueError(f"ObjectMeasure.enqueue: images must be a dense {self.dtype} stack of shape {(self.B, self.C, self.H, self.W)} on {self.device}")
        self._components.mask = mask.data_ptr()
        self._intensity.images = images.data_ptr()
        for name, fn, a in self.ops:
            L.check(fn(C.byref(a), st), name)
        return self

    def tables(self) -> SimpleNamespace:
        """The derived float64 tables of the last enqueue (torch arithmetic on the current stream)."""
        return SimpleNamespace(labels=ObjectLabels(index=self.index, count=self.count, status=self.status, geometry=self.geometry,
                                                   connectivity=self.connectivity, max_objects=self.max_objects, **shape_tables(self.geometry)),
                               intensity=intensity_tables(self.intensity, self.geometry[..., 0]))


# ---- what changed, per object --------------------------------------------------------------------------------------------------------------
def object_change(labels: ObjectLabels, source: torch.Tensor, result: torch.Tensor) -> SimpleNamespace:
    """Two stacks of one shape and dtype under the same labels, per object and channel ((B, K, C) float64): ``.mean_source``,
    ``.mean_result``, ``.delta_mean`` and ``.delta_std`` (result minus source) and ``.changed_fraction`` -- the share of the object's
    pixels whose values differ (``source != result`` as a uint8 stack through the same kernel: an exact count over the area) --
    with ``.valid`` (B, K), ``.source`` and ``.result`` (what :func:`measure_intensity` returns for each)."""
    who = "object_change"
    index, geometry, B, H, W, K = _check_labels(labels, who)
    from .masked import _require_cuda
    source = _check_images(source, B, H, W, index.device, who)
    result = _check_images(result, B, H, W, index.device, who, channels=source.shape[1], dtype=source.dtype)
    _require_cuda(index, who)
    area = geometry[..., 0]
    src, res = (intensity_tables(_measure_raw(index, geometry, t, B, H, W, K), area) for t in (source, result))
    bits = {torch.float32: torch.int32, torch.uint16: torch.int16, torch.uint8: torch.uint8}[source.dtype]      # bit-wise: -0.0 differs from 0.0, a NaN from
    differs = (source.view(bits) != result.view(bits)).to(torch.uint8)                                         # itself only where its bits do
    n = torch.where(src.valid, area, torch.ones_like(area)).to(torch.float64)[..., None]
    changed = _measure_raw(index, geometry, differs, B, H, W, K)[..., 0] / n
    return SimpleNamespace(mean_source=src.mean, mean_result=res.mean, delta_mean=res.mean - src.mean, delta_std=res.std - src.std,
                           changed_fraction=changed, valid=src.valid, source=src, result=res)


def measure_transfer(out, source: torch.Tensor, connectivity: int = 8, max_objects: int = 1024) -> SimpleNamespace:
    """:func:`object_change` over the output of :func:`~phendiff_amd.masked.masked_ddib` -- the one call after a masked transfer: the
    objects of ``out.mask``, ``source`` against ``out.images`` (a device tensor: ``output_type="pt"``; (B, H, W, C) as the transfer
    returns it, or (B, C, H, W)).  ``source``: the same stack before the transfer, in the images' layout or (B, C, H, W), and in their
    range (for a model-range input ``x``: ``(x / 2 + 0.5).clamp(0, 1)``).  Returns what :func:`object_change` returns, with ``.labels``."""
    who = "measure_transfer"
    mask, images = getattr(out, "mask", None), getattr(out, "images", None)
    if not torch.is_tensor(mask) or not torch.is_tensor(images) or images.dim() != 4:
        raise ValueError(f"{who}: out must carry a tensor .mask and a 4-d tensor .images (masked_ddib with output_type='pt')")
    if not torch.is_tensor(source) or source.dim() != 4:
        raise ValueError(f"{who}: source must be a 4-d tensor")
    connectivity = _check_connectivity(connectivity, who)
    max_objects = _check_max_objects(max_objects, who)
    H, W = mask.shape[-2], mask.shape[-1]

    def nchw(t):      # (B, H, W, C) -> (B, C, H, W); a stack that already is (B, C, H, W) stays
        return t if tuple(t.shape[-2:]) == (H, W) else t.permute(0, 3, 1, 2)

    images, source = nchw(images), nchw(source)
    for name, t in (("out.images", images), ("source", source)):
        if tuple(t.shape[-2:]) != (H, W) or t.shape[0] != mask.shape[0]:
            raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, the mask {tuple(mask.shape)}")
    labels = label_objects(mask, connectivity=connectivity, max_objects=max_objects)
    change = object_change(labels, source, images)
    change.labels = labels
    return change
