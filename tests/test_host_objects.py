"""The per-object measurements without a GPU: the numpy references of tests/objects_ref.py against closed forms (a rectangle, a single
pixel) and against SciPy (where SciPy is installed; the product never imports it), the host-side refusals of ``phendiff_amd.objects`` on
CPU tensors and the C ABI of the three entry points (struct layout, exports, constants, validation before any launch)."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import objects_ref as O
from abi_header import define, header_fields
from mask_ops_cases import BIG, CASES, SMALL
from test_host_contrast_mask import _aligned_buffer

F = {n: i for i, n in enumerate(O.GEOM_FIELDS)}


# ---- the references ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b,top,left", [(3, 5, 2, 4), (6, 2, 0, 0), (1, 7, 3, 1), (4, 4, 5, 9)])
def test_rectangle_closed_forms(a, b, top, left):
    H, W = 11, 14
    m = np.zeros((1, H, W), np.uint8)
    m[0, top:top + a, left:left + b] = 1
    index, count, status = O.index_ref(m, 8, 4)
    assert count.tolist() == [1] and status.tolist() == [0] and np.array_equal(index, m.astype(np.int32))
    g = O.geometry_ref(index, 4)
    ys, xs = np.arange(top, top + a), np.arange(left, left + b)
    want = dict(area=a * b, y0=top, y1=top + a - 1, x0=left, x1=left + b - 1, sum_y=b * ys.sum(), sum_x=a * xs.sum(), sum_yy=b * (ys ** 2).sum(),
                sum_xx=a * (xs ** 2).sum(), sum_yx=ys.sum() * xs.sum(), edges=2 * (a + b), border=int(top == 0 or left == 0))
    assert g[0, 0].tolist() == [want[n] for n in O.GEOM_FIELDS]
    assert not g[0, 1:].any()
    sh = O.shape_ref(g)
    assert sh["area"][0, 0] == a * b and sh["bbox"][0, 0].tolist() == [top, left, top + a, left + b]
    assert np.allclose(sh["centroid"][0, 0], [top + (a - 1) / 2, left + (b - 1) / 2], rtol=0, atol=1e-12)
    # second moments of an a x b block of unit pixels: a^2 / 12 and b^2 / 12 (the pixel-extent term included), no cross term
    assert math.isclose(sh["major_axis_length"][0, 0], 4 * max(a, b) / math.sqrt(12), rel_tol=1e-12)
    assert math.isclose(sh["minor_axis_length"][0, 0], 4 * min(a, b) / math.sqrt(12), rel_tol=1e-10)
    assert math.isclose(sh["eccentricity"][0, 0], math.sqrt(1 - (min(a, b) / max(a, b)) ** 2), rel_tol=1e-9, abs_tol=1e-7)
    if a != b:      # the major axis lies along the rows' axis (0) for a tall rectangle, across it (pi / 2) for a wide one
        assert math.isclose(abs(sh["orientation"][0, 0]), 0.0 if a > b else math.pi / 2, abs_tol=1e-12)
    assert all(not v[0, 1:].any() for v in sh.values())


def test_single_pixel_and_numbering():
    m = np.zeros((2, 5, 6), np.uint8)
    m[0, 2, 3] = 9
    m[1, 0, 5] = m[1, 0, 0] = m[1, 4, 2] = 1
    m[1, 1, 1] = 1      # 8-connected to (0, 0); its own object under 4
    index, count, status = O.index_ref(m, 8, 3)
    assert count.tolist() == [1, 3] and status.tolist() == [0, 0]
    assert index[1, 0, 0] == index[1, 1, 1] == 1 and index[1, 0, 5] == 2 and index[1, 4, 2] == 3
    g = O.geometry_ref(index, 3)
    assert g[0, 0].tolist() == [1, 2, 2, 3, 3, 2, 3, 4, 9, 6, 4, 0]
    sh = O.shape_ref(g)
    assert sh["centroid"][0, 0].tolist() == [2.0, 3.0] and sh["eccentricity"][0, 0] == 0.0
    assert math.isclose(sh["major_axis_length"][0, 0], 4 / math.sqrt(12), rel_tol=1e-15) and sh["major_axis_length"][0, 0] == sh["minor_axis_length"][0, 0]
    assert g[1, 0, F["edges"]] == 8 and g[1, 0, F["border"]] == 1 and g[1, 0, F["sum_yx"]] == 1      # the diagonal pair: 8 unit edges
    # rank past max_objects: index 0, the true count, the flag; the kept objects unchanged
    i4, c4, s4 = O.index_ref(m, 4, 2)
    assert c4.tolist() == [1, 4] and s4.tolist() == [0, O.OVERFLOW]
    assert i4[1, 0, 0] == 1 and i4[1, 0, 5] == 2 and i4[1, 1, 1] == 0 and i4[1, 4, 2] == 0
    assert np.array_equal(O.geometry_ref(i4, 2)[1], O.geometry_ref(O.index_ref(m, 4, 9)[0], 9)[1, :2])
    img = np.arange(2 * 2 * 5 * 6, dtype=np.float32).reshape(2, 2, 5, 6)
    t, bound = O.intensity_ref(index, img, 3)
    v = np.array([img[1, 1, 0, 0], img[1, 1, 1, 1]], np.float64)
    assert t[1, 0, 1].tolist() == [v.sum(), (v * v).sum(), v.min(), v.max()] and not t[0, 1:].any()
    assert bound[1, 0, 1, 0] == 2 * 2.0 ** -52 * v.sum()


@pytest.mark.parametrize("name", SMALL + [BIG])
def test_references_against_scipy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    m = CASES[name] != 0
    B = m.shape[0]
    for conn in (8, 4):
        index, count, status, g = O.reference(name, conn)
        for s in range(B):
            lab, n = ndi.label(m[s], structure=np.ones((3, 3)) if conn == 8 else None)
            assert n == count[s] and n <= O.K_DEFAULT and status[s] == 0
            assert np.array_equal(lab, index[s]), (s, conn)
            ids = np.arange(1, n + 1)
            if n:
                assert np.array_equal(ndi.sum(m[s], lab, ids).astype(np.int64), g[s, :n, F["area"]])
                com = np.array(ndi.center_of_mass(m[s], lab, ids))
                assert np.allclose(com, O.shape_ref(g)["centroid"][s, :n], rtol=1e-12, atol=1e-9)
                for k, sl in enumerate(ndi.find_objects(lab)):
                    assert (sl[0].start, sl[0].stop - 1, sl[1].start, sl[1].stop - 1) == tuple(g[s, k, 1:5])
            assert not g[s, n:].any()
        for kind in ("f32", "u16") if name != BIG else ("f32",):
            img = O.images(name, kind)
            table, bound = O.reference(name, conn, O.K_DEFAULT, kind)
            for s in range(B):
                n = int(count[s])
                if not n:
                    continue
                ids = np.arange(1, n + 1)
                for c in range(img.shape[1]):
                    v = img[s, c].astype(np.float64)
                    assert np.array_equal(ndi.minimum(v, index[s], ids), table[s, :n, c, 2]) and np.array_equal(ndi.maximum(v, index[s], ids), table[s, :n, c, 3])
                    assert (np.abs(ndi.sum(v, index[s], ids) - table[s, :n, c, 0]) <= bound[s, :n, c, 0]).all()
                    assert (np.abs(ndi.sum(v * v, index[s], ids) - table[s, :n, c, 1]) <= bound[s, :n, c, 1]).all()


# ---- host rules --------------------------------------------------------------------------------------------------------------------------
def test_host_refusals_on_cpu_tensors():
    import phendiff_amd as P
    ok = torch.ones(2, 6, 7, dtype=torch.uint8)
    for bad in (torch.ones(2, 6, 7), torch.ones(6, 7, dtype=torch.bool), torch.ones(2, 2, 6, 7, dtype=torch.uint8), "mask", None,
                torch.ones(2, 6, 0, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="label_objects"):
            P.label_objects(bad)
    for conn in (6, 0, True, None, "8"):
        with pytest.raises(ValueError, match="connectivity"):
            P.label_objects(ok, connectivity=conn)
    for K in (0, -1, 2.5, True, None, "9", (1 << 28) + 1):
        with pytest.raises(ValueError, match="max_objects"):
            P.label_objects(ok, max_objects=K)
        with pytest.raises(ValueError, match="max_objects"):
            P.ObjectMeasure(2, 6, 7, 3, "cuda", max_objects=K)
    with pytest.raises(P.PhenDiffHipError):      # a valid request on a CPU mask: what is left is the device (no CPU fallback)
        P.label_objects(ok)
    for kw in (dict(connectivity=5), dict(dtype=torch.float64), dict(dtype=torch.int32)):
        with pytest.raises(ValueError, match="ObjectMeasure"):
            P.ObjectMeasure(2, 6, 7, 3, "cuda", **kw)
    for B, H, W, Cn in ((0, 6, 7, 3), (2, 0, 7, 3), (2, 6, 16385, 3), (2, 6, 7, 0), (2.0, 6, 7, 3)):
        with pytest.raises(ValueError, match="ObjectMeasure"):
            P.ObjectMeasure(B, H, W, Cn, "cuda")
    with pytest.raises(P.PhenDiffHipError):
        P.ObjectMeasure(2, 6, 7, 3, "cpu")
    # labels as label_objects returns them, on the CPU: the images are checked against them before any device is asked for
    labels = SimpleNamespace(index=torch.zeros(2, 6, 7, dtype=torch.int32), geometry=torch.zeros(2, 4, 12, dtype=torch.int64))
    good = torch.zeros(2, 3, 6, 7)
    bad_images = [torch.zeros(2, 3, 6, 8), torch.zeros(3, 3, 6, 7), torch.zeros(2, 6, 7), torch.zeros(2, 3, 6, 7, dtype=torch.float64),
                  torch.zeros(2, 3, 6, 7, dtype=torch.int16), torch.zeros(2, 0, 6, 7), "images", torch.zeros(2, 3, 6, 7, device="meta")]
    for bad in bad_images:
        with pytest.raises(ValueError, match="measure_intensity"):
            P.measure_intensity(labels, bad)
        with pytest.raises(ValueError, match="object_change"):
            P.object_change(labels, bad, good)
        with pytest.raises(ValueError, match="object_change"):
            P.object_change(labels, good, bad)
    with pytest.raises(ValueError, match="object_change"):      # the two stacks must agree in channels and dtype
        P.object_change(labels, good, torch.zeros(2, 2, 6, 7))
    with pytest.raises(ValueError, match="object_change"):
        P.object_change(labels, good, torch.zeros(2, 3, 6, 7, dtype=torch.uint8))
    for bad in (None, SimpleNamespace(index=labels.index), SimpleNamespace(index=labels.index.long(), geometry=labels.geometry),
                SimpleNamespace(index=labels.index, geometry=torch.zeros(2, 4, 11, dtype=torch.int64)),
                SimpleNamespace(index=labels.index, geometry=torch.zeros(3, 4, 12, dtype=torch.int64))):
        with pytest.raises(ValueError, match="measure_intensity"):
            P.measure_intensity(bad, good)
    with pytest.raises(P.PhenDiffHipError):
        P.measure_intensity(labels, good)
    with pytest.raises(P.PhenDiffHipError):
        P.object_change(labels, good, good)
    out = P.MaskedTransferOutput(images=torch.zeros(2, 6, 7, 3), mask=torch.ones(2, 1, 6, 7, dtype=torch.uint8))
    for bad_out, src in ((SimpleNamespace(images=None, mask=out.mask), good), (SimpleNamespace(images=out.images, mask=None), good), (out, None),
                         (out, torch.zeros(2, 3, 6, 9)), (P.MaskedTransferOutput(images=torch.zeros(2, 6, 9, 3), mask=out.mask), good)):
        with pytest.raises(ValueError, match="measure_transfer"):
            P.measure_transfer(bad_out, src)
    with pytest.raises(ValueError, match="max_objects"):
        P.measure_transfer(out, good, max_objects=0)
    with pytest.raises(P.PhenDiffHipError):
        P.measure_transfer(out, good)


def test_derived_tables_on_the_cpu():
    """shape_tables / intensity_tables are torch arithmetic: on a CPU table they give the reference's numbers."""
    from phendiff_amd import objects as M
    name = "speckled_64x64"
    index, count, _, g = O.reference(name, 8)
    got, want = M.shape_tables(torch.from_numpy(g.copy())), O.shape_ref(g)
    for k, ref in want.items():
        assert got[k].dtype == torch.float64 and np.allclose(got[k].numpy(), ref, rtol=1e-12, atol=1e-9), k
    assert np.array_equal(got["valid"].numpy(), g[..., 0] > 0) and int(got["valid"].sum()) == int(count.sum())
    table, _ = O.reference(name, 8, O.K_DEFAULT, "f32")
    t = M.intensity_tables(torch.from_numpy(table.copy()), torch.from_numpy(g[..., 0].copy()))
    n = np.maximum(g[..., 0], 1)[..., None]
    assert np.allclose(t.mean.numpy(), table[..., 0] / n, rtol=1e-15) and np.array_equal(t.sum.numpy(), table[..., 0])
    assert np.allclose(t.std.numpy() ** 2, np.maximum(table[..., 1] / n - (table[..., 0] / n) ** 2, 0), rtol=1e-12, atol=1e-12)
    assert not t.mean.numpy()[g[..., 0] == 0].any() and not t.std.numpy()[g[..., 0] == 0].any()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
INDEX_FIELDS = ["B", "H", "W", "max_objects", "label", "label_status", "index", "count", "status", "workspace"]
GEOMETRY_FIELDS = ["B", "H", "W", "max_objects", "index", "geometry"]
INTENSITY_FIELDS = ["B", "H", "W", "max_objects", "C", "dtype", "index", "geometry", "images", "out"]


def test_structs_exports_and_constants():
    import phendiff_amd._lib as L
    from phendiff_amd import objects as M
    for cname, fields, cls in (("pd_object_index_args", INDEX_FIELDS, L.ObjectIndexArgs), ("pd_object_geometry_args", GEOMETRY_FIELDS, L.ObjectGeometryArgs),
                               ("pd_object_intensity_args", INTENSITY_FIELDS, L.ObjectIntensityArgs)):
        assert header_fields(cname) == fields == [f[0] for f in cls._fields_]
    lib = L.lib()
    for name in ("pd_object_index", "pd_object_index_workspace", "pd_object_geometry", "pd_object_intensity"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == define("PD_ABI_VERSION")
    # ranks for every pixel, then one offset per tile of 1024 pixels
    assert lib.pd_object_index_workspace(3, 37, 53) == 3 * (37 * 53 + 2) * 4 and lib.pd_object_index_workspace(2, 32, 32) == 2 * (1024 + 1) * 4
    assert lib.pd_object_index_workspace(1, 1, 1) == 8
    for bad in ((0, 4, 4), (-1, 4, 4), (2, 0, 4), (2, 4, 0), (2, 16385, 4), (2, 4, 16385)):
        assert lib.pd_object_index_workspace(*bad) == 0
    # the header and the module agree on every PD_OBJ_* / PD_OG_* / PD_OI_* constant
    assert M.GEOM_FIELDS == O.GEOM_FIELDS and len(M.GEOM_FIELDS) == define("PD_OBJ_GEOM_FIELDS") == L.CONSTANTS["PD_OBJ_GEOM_FIELDS"] == 12
    assert [L.CONSTANTS["PD_OG_" + n.upper()] for n in M.GEOM_FIELDS] == list(range(12))
    assert len(M.INTENSITY_FIELDS) == define("PD_OBJ_INTENSITY_FIELDS") == 4
    assert [L.CONSTANTS["PD_OI_" + n.upper()] for n in M.INTENSITY_FIELDS] == [0, 1, 2, 3]
    assert (M.OBJ_OVERFLOW, M.OBJ_BAD_LABEL, M.OBJ_LABEL_STATUS) == (1, 2, 4) == tuple(L.CONSTANTS[n] for n in ("PD_OBJ_OVERFLOW", "PD_OBJ_BAD_LABEL", "PD_OBJ_LABEL_STATUS"))
    assert M.OBJ_OVERFLOW == O.OVERFLOW and M.MAX_OBJECTS == define("PD_OBJ_MAX_OBJECTS") == 1 << 28 == define("PD_MASK_MAX_SIDE") ** 2
    assert M.IMAGE_DTYPES == {torch.float32: L.CONSTANTS["PD_OBJ_F32"], torch.uint8: L.CONSTANTS["PD_OBJ_U8"], torch.uint16: L.CONSTANTS["PD_OBJ_U16"]}
    assert sorted(M.IMAGE_DTYPES.values()) == [0, 1, 2]
    names = [n for n in L.CONSTANTS if n.startswith(("PD_OBJ_", "PD_OG_", "PD_OI_"))]
    assert len(names) == 3 + 3 + 3 + 12 + 4


def test_entry_points_validate_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    _keep, p = _aligned_buffer(1 << 16)
    q = p + 8192
    sizes = [dict(B=0), dict(B=-2), dict(H=0), dict(W=0), dict(H=-3), dict(H=16385), dict(W=16385), dict(H=1 << 20, W=1 << 20),
             dict(max_objects=0), dict(max_objects=-5), dict(max_objects=(1 << 28) + 1)]
    table = [
        ("pd_object_index", L.ObjectIndexArgs,
         dict(B=2, H=5, W=7, max_objects=13, label=p, label_status=None, index=q, count=q + 1024, status=q + 2048, workspace=q + 4096),
         sizes, [{n: None} for n in ("label", "index", "count", "status", "workspace")]
         + [dict(label=p + 2), dict(index=q + 1), dict(count=q + 1026), dict(status=q + 2051), dict(workspace=q + 4098), dict(label_status=q + 3073)]),
        ("pd_object_geometry", L.ObjectGeometryArgs, dict(B=2, H=5, W=7, max_objects=13, index=p, geometry=q),
         sizes, [dict(index=None), dict(geometry=None), dict(index=p + 2), dict(geometry=q + 4), dict(geometry=q + 1)]),
        ("pd_object_intensity", L.ObjectIntensityArgs, dict(B=2, H=5, W=7, max_objects=13, C=3, dtype=0, index=p, geometry=p + 1024, images=q, out=q + 4096),
         sizes + [dict(C=0), dict(C=-1), dict(dtype=3), dict(dtype=-1), dict(B=1 << 20, max_objects=1 << 10, C=3)],
         [{n: None} for n in ("index", "geometry", "images", "out")]
         + [dict(index=p + 2), dict(geometry=p + 1028), dict(out=q + 4100), dict(images=q + 2), dict(dtype=2, images=q + 1)]),
    ]
    for name, struct, ok, shapes, args in table:
        fn = getattr(lib, name)
        for change, code in [(c, L.PD_ERR_SHAPE) for c in shapes] + [(c, L.CONSTANTS["PD_ERR_ARG"]) for c in args]:
            rc = fn(C.byref(struct(**dict(ok, **change))), None)
            assert rc == code, (name, change, rc, lib.pd_last_error())
            assert name.encode() in lib.pd_last_error(), (name, change, lib.pd_last_error())
        assert fn(None, None) == L.CONSTANTS["PD_ERR_ARG"] and name.encode() in lib.pd_last_error() and b"null args" in lib.pd_last_error()
    # images need the alignment of their element only: a uint8 stack at an odd address passes the pointer checks (and fails on nothing else
    # before the launch, which this test must not reach: so a size is wrong as well, and the answer is the size's)
    a = L.ObjectIntensityArgs(**dict(table[2][2], dtype=1, images=q + 1, C=0))
    assert lib.pd_object_intensity(C.byref(a), None) == L.PD_ERR_SHAPE and b"C = 0" in lib.pd_last_error()
