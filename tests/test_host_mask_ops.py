"""The mask refinement without a GPU: the numpy references against SciPy (where SciPy is installed; the product never imports it) and
against the brute force over all pixel pairs, the host rules of ``phendiff_amd.mask_ops`` (``disc_r2``, ``MaskRefine.check_params``, the
stage order), the ``refine=`` validation of the three masked-transfer entry points (on meta / CPU objects, with nothing packed) and the C
ABI of the four entry points (struct layout, exports, validation before any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_ops_ref as R
from abi_header import define, header_fields
from mask_ops_cases import BIG, CASES, NAMES, RADII, RECIPES, SMALL, reference
from test_host_contrast_mask import _aligned_buffer, _meta_pipe, _nothing_packed


def disc(r2):
    k = int(np.floor(np.sqrt(r2)))
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    return yy ** 2 + xx ** 2 <= r2


# ---- the references ------------------------------------------------------------------------------------------------------------------------
def test_disc_sizes():
    assert [R.r2_of(r) for r in (1, 1.5, 2, 2.9)] == [1, 2, 4, 8]
    assert int(disc(1).sum()) == 5 and int(disc(2).sum()) == 9 and disc(2).shape == (3, 3) and int(disc(4).sum()) == 13


@pytest.mark.parametrize("name", [n for n in SMALL if CASES[n][0].size <= 37 * 53])
def test_factored_distance_is_the_all_pairs_distance(name):
    m = CASES[name]
    for to_set in (False, True):
        assert np.array_equal(reference(name, "d2", to_set), R.d2_all_pairs(m, to_set))
        assert np.array_equal(R.d2_ref(m, to_set, 5), R.d2_all_pairs(m, to_set, 5))
    d = reference(name, "d2", True)
    for s in range(m.shape[0]):
        assert (d[s] == R.FAR).all() == (not m[s].any())
    assert int(R.d2_ref(m, True, 5).max()) <= 6


@pytest.mark.parametrize("name", NAMES)
def test_references_against_scipy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    m = CASES[name] != 0
    B, H, W = m.shape
    for to_set in (False, True):
        ours = reference(name, "d2", to_set)
        for s in range(B):
            target = m[s] if to_set else ~m[s]
            if target.any():      # (SciPy leaves an image without any target pixel undefined; here it is PD_MASK_FAR)
                edt = ndi.distance_transform_edt(~target)
                assert np.array_equal(np.rint(edt ** 2).astype(np.int64), ours[s]), (s, to_set)
            else:
                assert (ours[s] == R.FAR).all()
    for radius in RADII if name != BIG else RADII[1:2]:
        r2 = R.r2_of(radius)
        dil, ero = reference(name, "dilate", r2), reference(name, "erode", r2)
        for s in range(B):
            assert np.array_equal(ndi.binary_dilation(m[s], structure=disc(r2), border_value=0), dil[s] != 0), (s, radius)
            assert np.array_equal(ndi.binary_erosion(m[s], structure=disc(r2), border_value=1), ero[s] != 0), (s, radius)
    for conn, phase in ((8, 1), (4, 1), (4, 0), (8, 0)):
        label, area, border, count = reference(name, "label", conn, phase)
        for s in range(B):
            lab, n = ndi.label(m[s] == bool(phase), structure=np.ones((3, 3)) if conn == 8 else None)
            assert n == count[s]
            canon, ar, bd = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
            for k in range(1, n + 1):
                ys, xs = np.nonzero(lab == k)
                canon[ys, xs] = (ys * W + xs).min() + 1
                ar[ys, xs] = ys.size
                bd[ys, xs] = int((ys == 0).any() or (ys == H - 1).any() or (xs == 0).any() or (xs == W - 1).any())
            assert np.array_equal(canon, label[s]) and np.array_equal(ar, area[s]) and np.array_equal(bd, border[s]), (s, conn, phase)
    for conn in (8, 4):
        filled, stats = reference(name, "fill_holes", None, conn)
        for s in range(B):
            want = ndi.binary_fill_holes(m[s], structure=None if conn == 8 else np.ones((3, 3)))
            assert np.array_equal(want, filled[s] != 0), (s, conn)
        assert np.array_equal(stats[:, 1] - stats[:, 0], (filled != 0).reshape(B, -1).sum(1) - m.reshape(B, -1).sum(1))


def test_reference_filters_and_recipe_by_hand():
    m = np.zeros((1, 7, 9), np.uint8)
    m[0, 1:6, 1:6] = 1
    m[0, 3, 3] = 0               # a pin-hole
    m[0, 0, 8] = 1               # a speck
    out, st = R.fill_holes_ref(m)
    assert out[0, 3, 3] == 1 and int(out.sum()) == 26 and st.tolist() == [[25, 26, 2, 1, 0]]      # the background and the hole; one filled
    out, st = R.fill_holes_ref(m, 0)
    assert out[0, 3, 3] == 0 and st.tolist() == [[25, 25, 2, 0, 0]]
    out, st = R.drop_small_ref(m, 2)
    assert out[0, 0, 8] == 0 and int(out.sum()) == 24 and st.tolist() == [[25, 24, 2, 1, 0]]
    out, st = R.refine_ref(m, fill_holes=-1, min_area=2, dilate=1)
    assert st.shape == (1, 3, 5) and st[0].tolist() == [[25, 26, 2, 1, 0], [26, 25, 2, 1, 0], [25, 45, 0, 0, 0]]
    # a diagonal pair: one component under 8, two under 4; the hole of a diagonal ring leaks under 8-connected background (foreground 4)
    d = np.array([[[1, 0], [0, 1]]], np.uint8)
    assert R.label_ref(d, 8)[3].tolist() == [1] and R.label_ref(d, 4)[3].tolist() == [2]
    ring = np.array([[[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 0, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]], np.uint8)
    assert R.fill_holes_ref(ring, None, 8)[0][0, 2, 2] == 1 and R.fill_holes_ref(ring, None, 4)[0][0, 2, 2] == 0
    # an object the image edge cuts is not eroded from the edge; a closing does not pull the border in
    edge = np.zeros((1, 5, 6), np.uint8)
    edge[0, :, :3] = 1
    assert R.erode_ref(edge, 1)[0].tolist() == [[1, 1, 0, 0, 0, 0]] * 5
    assert np.array_equal(R.close_ref(np.ones((1, 4, 4), np.uint8), 4), np.ones((1, 4, 4), np.uint8))


# ---- host rules --------------------------------------------------------------------------------------------------------------------------
def test_disc_r2():
    import phendiff_amd as P
    assert [P.disc_r2(r) for r in (1, 1.5, 2, 2.9)] == [1, 2, 4, 8]
    assert P.disc_r2(0) == 0 and P.disc_r2(3) == 9 and isinstance(P.disc_r2(1.5), int)
    far = P.mask_ops.MASK_FAR
    assert far == 1 << 30 == define("PD_MASK_FAR") and define("PD_MASK_MAX_SIDE") == 16384
    assert P.disc_r2(32767.9) < far
    for bad in (-1, float("nan"), float("inf"), 32768, None, "x", True):
        with pytest.raises(ValueError):
            P.disc_r2(bad)


def test_check_params_refusals():
    import phendiff_amd as P
    check = P.MaskRefine.check_params
    full = check(close=1.5, open=1.5, fill_holes=-1, min_area=64, dilate=3)
    assert full == dict(close=1.5, open=1.5, fill_holes=-1, min_area=64, dilate=3.0, connectivity=8)
    assert check(min_area=1, connectivity=4)["connectivity"] == 4
    bad = [dict(close=-1), dict(open=-0.5), dict(dilate=-2), dict(dilate=float("nan")), dict(close=float("inf")), dict(dilate="3px"),
           dict(min_area=-1), dict(fill_holes=-2), dict(min_area=2.5), dict(fill_holes=True), dict(min_area=None),
           dict(min_area=4, connectivity=6), dict(min_area=4, connectivity=True), dict(min_area=4, connectivity=None),
           dict(dilate=32768), dict(close=1e9),                        # floor(radius^2) reaches PD_MASK_FAR
           dict(dilate=0.5),                                           # a disc that is the pixel itself
           dict(erode=1), dict(min_area=4, radius=2), dict(min_area=4, threshold=0.5),      # unknown keys
           dict(), dict(close=0, open=0.0, fill_holes=0, min_area=0, dilate=0), dict(connectivity=4)]      # all zero
    for params in bad:
        with pytest.raises(ValueError, match="MaskRefine"):
            check(**params)
    with pytest.raises(ValueError, match="MaskRefine"):      # ... before anything is allocated: no device is ever touched
        P.MaskRefine(2, 8, 8, "cuda", dilate=-1)
    with pytest.raises(ValueError):
        P.refine_mask(torch.ones(1, 4, 4, dtype=torch.uint8), bogus=1)
    with pytest.raises(P.PhenDiffHipError):                  # valid parameters, a CPU mask: no CPU fallback
        P.refine_mask(torch.ones(1, 4, 4, dtype=torch.uint8), dilate=1)
    for fn in (P.mask_dilate, P.mask_erode, P.mask_open, P.mask_close):
        with pytest.raises(ValueError):
            fn(torch.ones(1, 4, 4), 1)                       # a float mask
        with pytest.raises(ValueError):
            fn(torch.ones(4, 4, dtype=torch.bool), 1)        # no batch dimension
    with pytest.raises(ValueError, match="connectivity"):
        P.mask_components(torch.ones(1, 4, 4, dtype=torch.bool), connectivity=6)


def test_stage_order():
    import phendiff_amd as P
    plan = P.MaskRefine.plan(dilate=3, min_area=64, fill_holes=-1, open=1.5, close=1.5)      # whatever order the keys come in
    assert [(s, f) for s, f, _ in plan] == [("close", "pd_mask_morph"), ("close", "pd_mask_morph"), ("open", "pd_mask_morph"),
                                            ("open", "pd_mask_morph"), ("fill_holes", "pd_mask_components"), ("fill_holes", "pd_mask_filter"),
                                            ("min_area", "pd_mask_components"), ("min_area", "pd_mask_filter"), ("dilate", "pd_mask_morph")]
    assert [d.get("op") for _, f, d in plan if f == "pd_mask_morph"] == ["dilate", "erode", "erode", "dilate", "dilate"]
    assert [d["r2"] for _, f, d in plan if f == "pd_mask_morph"] == [2, 2, 2, 2, 9]
    # holes are labelled with the dual connectivity, the foreground with its own
    assert [(d["phase"], d["connectivity"]) for _, f, d in plan if f == "pd_mask_components"] == [(0, 4), (1, 8)]
    plan4 = P.MaskRefine.plan(fill_holes=9, min_area=2, connectivity=4)
    assert [(d["phase"], d["connectivity"]) for _, f, d in plan4 if f == "pd_mask_components"] == [(0, 8), (1, 4)]
    assert [d["area_limit"] for _, f, d in plan4 if f == "pd_mask_filter"] == [9, 2]
    # a stage whose parameter is 0 is skipped
    assert [s for s, _, _ in P.MaskRefine.plan(open=2, dilate=1)] == ["open", "open", "dilate"]
    assert P.mask_ops.STAGES == R.STAGES == ("close", "open", "fill_holes", "min_area", "dilate")
    assert all(set(r) <= set(P.MaskRefine.DEFAULTS) for r in RECIPES)


def test_refine_is_validated_before_anything_touches_the_device():
    import phendiff_amd as P
    pipe = _meta_pipe()
    x, labels = torch.zeros(2, 3, 32, 32), torch.tensor([0, 1])
    ones = torch.ones(2, 1, 32, 32, dtype=torch.uint8)
    entries = {
        "masked_ddib": lambda **kw: P.masked_ddib(pipe, x, labels, 1 - labels, 4, **kw),
        "masked_ddib (given)": lambda **kw: P.masked_ddib(pipe, x, labels, 1 - labels, 4, mask=ones, **kw),
        "class_contrast_mask": lambda **kw: P.class_contrast_mask(pipe, x, labels, 1 - labels, 4, **kw),
        "MaskedDDIBGraph": lambda **kw: P.MaskedDDIBGraph(pipe, 2, 4, mask="given", **kw),
        "MaskedDDIBGraph (contrast)": lambda **kw: P.MaskedDDIBGraph(pipe, 2, 4, noise=object.__new__(P.DeviceNoise), **kw),
    }
    for name, call in entries.items():
        for bad in (dict(dilate=-1), dict(bogus=1), dict(), dict(min_area=4, connectivity=5), dict(close=1e9), [("dilate", 1)], "dilate", 3):
            with pytest.raises(ValueError, match=name.split(" ")[0] + ".*refine"):
                call(refine=bad)
        with pytest.raises(P.PhenDiffHipError):      # a valid request on CPU tensors: what is left is the device
            call(refine=dict(close=1.5, min_area=4))
    assert _nothing_packed(pipe)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
DISTANCE_FIELDS = ["B", "H", "W", "mask", "to_set", "limit", "d2"]
MORPH_FIELDS = ["B", "H", "W", "mask", "op", "r2", "out", "workspace", "stats", "stats_stride", "stats_mode"]
COMPONENTS_FIELDS = ["B", "H", "W", "mask", "phase", "connectivity", "label", "area", "border", "count", "status", "workspace"]
FILTER_FIELDS = ["B", "H", "W", "mask", "label", "area", "border", "status", "rule", "area_limit", "out", "stats", "stats_stride"]


def test_structs_and_exports():
    import phendiff_amd._lib as L
    for cname, fields, cls in (("pd_mask_distance_args", DISTANCE_FIELDS, L.MaskDistanceArgs), ("pd_mask_morph_args", MORPH_FIELDS, L.MaskMorphArgs),
                               ("pd_mask_components_args", COMPONENTS_FIELDS, L.MaskComponentsArgs), ("pd_mask_filter_args", FILTER_FIELDS, L.MaskFilterArgs)):
        assert header_fields(cname) == fields == [f[0] for f in cls._fields_]
    lib = L.lib()
    for name in ("pd_mask_distance", "pd_mask_morph", "pd_mask_morph_workspace", "pd_mask_components", "pd_mask_components_workspace", "pd_mask_filter"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.pd_mask_morph_workspace(3, 37, 53) == 3 * 37 * 53 * 4 and lib.pd_mask_components_workspace(3, 37, 53) == 2 * 3 * 37 * 53 * 4
    for bad in ((0, 4, 4), (-1, 4, 4), (2, 0, 4), (2, 4, 0), (2, 16385, 4), (2, 4, 16385)):
        assert lib.pd_mask_morph_workspace(*bad) == lib.pd_mask_components_workspace(*bad) == 0
    assert lib.pd_mask_morph_workspace(1, 16384, 16384) == 4 << 28
    assert L.CONSTANTS["PD_MORPH_DILATE"] != L.CONSTANTS["PD_MORPH_ERODE"] and L.CONSTANTS["PD_FILTER_DROP_SMALL"] != L.CONSTANTS["PD_FILTER_FILL_HOLES"]
    assert [L.CONSTANTS[n] for n in ("PD_MS_PIXELS_IN", "PD_MS_PIXELS_OUT", "PD_MS_COMPONENTS", "PD_MS_SELECTED", "PD_MS_STATUS")] == [0, 1, 2, 3, 4]


def test_entry_points_validate_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    _keep, p = _aligned_buffer(1 << 16)
    q = p + 8192      # a second, disjoint region (2 * 5 * 7 bytes each)
    sizes = [dict(B=0), dict(B=-2), dict(H=0), dict(W=0), dict(H=-3), dict(H=16385), dict(W=16385), dict(H=1 << 20, W=1 << 20)]
    far = 1 << 30
    table = [
        ("pd_mask_distance", L.MaskDistanceArgs, dict(B=2, H=5, W=7, mask=p, to_set=0, limit=0, d2=q),
         sizes + [dict(mask=None), dict(d2=None), dict(d2=q + 2), dict(limit=-1), dict(limit=far)]),
        ("pd_mask_morph", L.MaskMorphArgs, dict(B=2, H=5, W=7, mask=p, op=0, r2=2, out=q, workspace=q + 4096, stats=q + 2048, stats_stride=5, stats_mode=3),
         sizes + [dict(mask=None), dict(out=None), dict(workspace=None), dict(workspace=q + 4098), dict(op=2), dict(op=-1), dict(r2=-1), dict(r2=far),
                  dict(out=p), dict(out=p + 69), dict(out=p + 1),      # out aliases mask: the same bytes, its last byte, one byte in
                  dict(stats_stride=4), dict(stats=q + 2050), dict(stats_mode=4), dict(stats_mode=-1)]),
        ("pd_mask_components", L.MaskComponentsArgs,
         dict(B=2, H=5, W=7, mask=p, phase=1, connectivity=8, label=q, area=q + 1024, border=q + 2048, count=q + 3072, status=q + 3200, workspace=q + 4096),
         sizes + [dict(mask=None), dict(workspace=None), dict(label=None, area=None, border=None, count=None), dict(label=q + 2), dict(area=q + 1025),
                  dict(count=q + 3073), dict(status=q + 3202), dict(workspace=q + 4097)]
         + [dict(connectivity=c) for c in (0, 6, 9, -4)] + [dict(phase=2), dict(phase=-1)]),
        ("pd_mask_filter", L.MaskFilterArgs,
         dict(B=2, H=5, W=7, mask=p, label=q, area=q + 1024, border=q + 2048, status=None, rule=0, area_limit=4, out=p, stats=q + 3072, stats_stride=5),
         sizes + [{n: None} for n in ("mask", "label", "area", "border", "out")] + [dict(label=q + 1), dict(area=q + 1026), dict(stats=q + 3074), dict(status=q + 3)]
         + [dict(rule=2), dict(rule=-1), dict(rule=0, area_limit=-1), dict(stats_stride=4), dict(stats_stride=0)]),
    ]
    for name, struct, ok, bad in table:
        fn = getattr(lib, name)
        for change in bad:
            rc = fn(C.byref(struct(**dict(ok, **change))), None)
            assert rc < 0, (name, change)
            assert name.encode() in lib.pd_last_error(), (name, change, lib.pd_last_error())
        assert fn(None, None) < 0 and name.encode() in lib.pd_last_error() and b"null args" in lib.pd_last_error()
    # sizes and parameters answer PD_ERR_SHAPE, pointers, ops and aliasing PD_ERR_ARG
    assert lib.pd_mask_distance(C.byref(L.MaskDistanceArgs(**dict(table[0][2], H=16385))), None) == L.PD_ERR_SHAPE
    assert lib.pd_mask_components(C.byref(L.MaskComponentsArgs(**dict(table[2][2], connectivity=6))), None) == L.PD_ERR_SHAPE
    assert lib.pd_mask_morph(C.byref(L.MaskMorphArgs(**dict(table[1][2], out=p + 1))), None) == -1
    assert b"alias" in lib.pd_last_error()
    assert lib.pd_mask_filter(C.byref(L.MaskFilterArgs(**dict(table[3][2], rule=7))), None) == -1
