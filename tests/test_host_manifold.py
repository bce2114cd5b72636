"""``pd_knn_radii`` / ``pd_manifold_query`` without a GPU: the C ABI (struct layout, exports, workspace queries, every refusal before a
launch) and the host side of precision / recall / density / coverage in ``phendiff_amd.metrics`` (the numpy twins against
``prdc_ref`` and scikit-learn; no CPU fallback of the device functions; the new switches default to off and cost nothing)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import prdc_ref as R
from abi_header import define, header_fields

CASES = sorted(R.TABLE)


def radii_default_splits(lib, n, k, cap):
    """The S behind pd_knn_radii_workspace(n, k, 0): documented as some S in 1 .. min(column tiles, cap) for which the query returns the
    same size (a tuning value of the library: nothing here pins it)."""
    ws0 = lib.pd_knn_radii_workspace(n, k, 0)
    s, rest = divmod(ws0 // 8 - n, n * (k + 1))
    assert ws0 % 8 == 0 and rest == 0 and 1 <= s <= min(-(-n // 64), cap), (n, k, ws0, s)
    assert lib.pd_knn_radii_workspace(n, k, s) == ws0
    return s


def query_default_splits(lib, nq, nr, cap):
    ws0 = lib.pd_manifold_query_workspace(nq, nr, 0)
    hits = [s for s in range(1, min(-(-nr // 64), cap) + 1) if lib.pd_manifold_query_workspace(nq, nr, s) == ws0]
    assert len(hits) == 1, (nq, nr, ws0, hits)
    return hits[0]


def test_structs_and_constants_match_header():
    import phendiff_amd._lib as L
    want = ["D", "k", "splits", "N", "f_stride", "f", "rad2", "workspace", "workspace_bytes"]
    assert header_fields("pd_knn_radii_args") == want == [f[0] for f in L.KnnRadiiArgs._fields_]
    assert [getattr(L.KnnRadiiArgs, f).offset for f in want] == [0, 4, 8] + list(range(16, 64, 8))
    assert C.sizeof(L.KnnRadiiArgs) == 64
    want = ["D", "splits", "Nq", "Nr", "q_stride", "r_stride", "q", "r", "rad2", "count", "dmin2", "workspace", "workspace_bytes"]
    assert header_fields("pd_manifold_query_args") == want == [f[0] for f in L.ManifoldQueryArgs._fields_]
    assert [getattr(L.ManifoldQueryArgs, f).offset for f in want] == [0, 4] + list(range(8, 96, 8))
    assert C.sizeof(L.ManifoldQueryArgs) == 96
    assert define("PD_MANIFOLD_MAX_K") == L.CONSTANTS["PD_MANIFOLD_MAX_K"] == 16
    assert define("PD_MANIFOLD_MAX_SPLITS") == L.CONSTANTS["PD_MANIFOLD_MAX_SPLITS"]


def test_symbols_are_exported_and_abi_stays_8():
    import phendiff_amd._lib as L
    lib = L.lib()
    for name in ("pd_knn_radii", "pd_knn_radii_workspace", "pd_manifold_query", "pd_manifold_query_workspace"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == define("PD_ABI_VERSION") == 8
    with open(L.HEADER_PATH) as f:
        head = f.read().split("#define PD_ABI_VERSION")[0]
    assert "pd_knn_radii" in head and "pd_manifold_query" in head      # the list of entry points added under ABI 8


def test_workspace_queries():
    """8 (N + N S (k + 1)) and 8 (Nq + Nr + Nq S) + 4 Nq S rounded up to 8, S the splits in effect; 0 for refused sizes."""
    import phendiff_amd._lib as L
    lib, cap = L.lib(), L.CONSTANTS["PD_MANIFOLD_MAX_SPLITS"]
    assert lib.pd_knn_radii_workspace(70, 3, 1) == 8 * (70 + 70 * 4)
    assert lib.pd_knn_radii_workspace(70, 3, 3) == 8 * (70 + 70 * 3 * 4)
    assert lib.pd_knn_radii_workspace(17, 16, 2) == 8 * (17 + 17 * 2 * 17)
    for n in (4, 70, 2000, 10000, 50000, 1 << 20):
        for k in (1, 3):
            assert radii_default_splits(lib, n, k, cap) == radii_default_splits(lib, n, 3, cap)      # of the shapes only, not of k
    assert radii_default_splits(lib, 4, 3, cap) == 1 and radii_default_splits(lib, 2000, 3, cap) > 1      # a few thousand rows are split
    for bad in ((0, 3, 0), (-5, 3, 0), (1 << 31, 3, 0), (70, 0, 0), (70, 17, 0), (70, -1, 0), (3, 3, 0), (70, 3, -1), (70, 3, cap + 1)):
        assert lib.pd_knn_radii_workspace(*bad) == 0, bad
    assert lib.pd_manifold_query_workspace(77, 150, 1) == 8 * (77 + 150 + 77) + 4 * 78
    assert lib.pd_manifold_query_workspace(1, 5, 3) == 8 * (1 + 5 + 3) + 16
    assert lib.pd_manifold_query_workspace(130, 260, 2) == 8 * (130 + 260 + 260) + 4 * 260
    for nq, nr in ((1, 5), (77, 150), (10000, 10000), (50000, 20000)):
        s = query_default_splits(lib, nq, nr, cap)
        assert lib.pd_manifold_query_workspace(nq, nr, 0) == 8 * (nq + nr + nq * s) + (4 * nq * s + 7) // 8 * 8, (nq, nr)
    assert query_default_splits(lib, 1, 5, cap) == 1
    for bad in ((0, 5, 0), (5, 0, 0), (-1, 5, 0), (1 << 31, 5, 0), (5, 1 << 31, 0), (5, 5, -1), (5, 5, cap + 1)):
        assert lib.pd_manifold_query_workspace(*bad) == 0, bad


def test_knn_radii_refusals_before_any_launch():
    """Every refusal returns its status code and names what it refuses; the stream is null and no pointer is dereferenced."""
    import phendiff_amd._lib as L
    lib, cap = L.lib(), L.CONSTANTS["PD_MANIFOLD_MAX_SPLITS"]
    ARG, SHAPE = L.CONSTANTS["PD_ERR_ARG"], L.CONSTANTS["PD_ERR_SHAPE"]
    ok = dict(D=64, k=3, splits=2, N=70, f_stride=128, f=0x10000, rad2=0x20000, workspace=0x30000, workspace_bytes=8 * (70 + 70 * 2 * 4))

    def refused(code, word, **change):
        rc = lib.pd_knn_radii(C.byref(L.KnnRadiiArgs(**dict(ok, **change))), None)
        msg = lib.pd_last_error()
        assert rc == code, (change, rc, msg)
        assert word in msg, (change, msg)

    assert lib.pd_knn_radii(None, None) == ARG and b"null args" in lib.pd_last_error()
    for name in ("f", "rad2", "workspace"):
        refused(ARG, b"null", **{name: None})
    refused(ARG, b"aligned", f=0x10004)
    refused(ARG, b"aligned", rad2=0x20004)
    refused(ARG, b"workspace_bytes", workspace_bytes=8 * (70 + 70 * 2 * 4) - 1)
    refused(ARG, b"workspace_bytes", splits=3)
    for D in (0, 32, 100, 4160, -64):
        refused(SHAPE, b"D = ", D=D)
    refused(SHAPE, b"stride", f_stride=60)
    refused(SHAPE, b"stride", f_stride=66)
    refused(SHAPE, b"k = 0", k=0)
    refused(SHAPE, b"k = 17", k=17)
    refused(SHAPE, b"k = -1", k=-1)
    refused(SHAPE, b"k + 1", N=3)
    refused(SHAPE, b"k + 1", N=16, k=16)
    refused(SHAPE, b"N = 0", N=0)
    refused(SHAPE, b"N = -4", N=-4)
    refused(SHAPE, b"N = ", N=1 << 31, workspace_bytes=1 << 62)
    refused(SHAPE, b"splits", splits=-1)
    refused(SHAPE, b"splits", splits=cap + 1, workspace_bytes=1 << 62)
    # 2^25 row blocks x 64 splits = 2^31 workgroups, one more than a grid holds; one split fewer passes that check and stops at the workspace
    assert cap == 64
    refused(SHAPE, b"grid too large", N=(1 << 31) - 1, splits=64, workspace_bytes=1 << 62)
    refused(ARG, b"workspace_bytes", N=(1 << 31) - 1, splits=63, workspace_bytes=8)


def test_manifold_query_refusals_before_any_launch():
    import phendiff_amd._lib as L
    lib, cap = L.lib(), L.CONSTANTS["PD_MANIFOLD_MAX_SPLITS"]
    ARG, SHAPE = L.CONSTANTS["PD_ERR_ARG"], L.CONSTANTS["PD_ERR_SHAPE"]
    need = 8 * (77 + 150 + 77 * 2) + 4 * 77 * 2
    ok = dict(D=64, splits=2, Nq=77, Nr=150, q_stride=64, r_stride=128, q=0x10000, r=0x20000, rad2=0x30000, count=0x40000, dmin2=0x50000,
              workspace=0x60000, workspace_bytes=need)

    def refused(code, word, **change):
        rc = lib.pd_manifold_query(C.byref(L.ManifoldQueryArgs(**dict(ok, **change))), None)
        msg = lib.pd_last_error()
        assert rc == code, (change, rc, msg)
        assert word in msg, (change, msg)

    assert lib.pd_manifold_query(None, None) == ARG and b"null args" in lib.pd_last_error()
    for name in ("q", "r", "workspace"):
        refused(ARG, b"null", **{name: None})
    refused(ARG, b"rad2 is null", rad2=None)                      # count without radii
    refused(ARG, b"null outputs", count=None, dmin2=None)
    refused(ARG, b"null outputs", count=None, dmin2=None, rad2=None)
    refused(ARG, b"aligned", q=0x10008)
    refused(ARG, b"aligned", r=0x20004)
    refused(ARG, b"aligned", dmin2=0x50004)
    refused(ARG, b"aligned", count=0x40002)
    refused(ARG, b"workspace_bytes", workspace_bytes=need - 1)
    refused(ARG, b"workspace_bytes", splits=3)
    for D in (0, 32, 100, 4160, -64):
        refused(SHAPE, b"D = ", D=D)
    refused(SHAPE, b"stride", q_stride=60)
    refused(SHAPE, b"stride", r_stride=32)
    refused(SHAPE, b"stride", q_stride=66)
    refused(SHAPE, b"stride", r_stride=130)
    refused(SHAPE, b"Nq = 0", Nq=0)
    refused(SHAPE, b"Nr = 0", Nr=0)
    refused(SHAPE, b"Nq = -1", Nq=-1)
    refused(SHAPE, b"Nq = ", Nq=1 << 31, workspace_bytes=1 << 62)
    refused(SHAPE, b"Nr = ", Nr=1 << 31, workspace_bytes=1 << 62)
    refused(SHAPE, b"splits", splits=-2)
    refused(SHAPE, b"splits", splits=cap + 1, workspace_bytes=1 << 62)
    assert cap == 64
    refused(SHAPE, b"grid too large", Nq=(1 << 31) - 1, splits=64, workspace_bytes=1 << 62)
    refused(SHAPE, b"grid too large", Nq=(1 << 31) - 1, Nr=(1 << 31) - 1, splits=64, workspace_bytes=1 << 62)
    refused(ARG, b"workspace_bytes", Nq=(1 << 31) - 1, splits=63, workspace_bytes=8)


def test_device_functions_have_no_cpu_fallback():
    import phendiff_amd._lib as L
    import phendiff_amd.metrics as M
    f = torch.rand(40, 64)
    with pytest.raises(L.PhenDiffHipError):
        M.knn_radii_device(f, 3)
    with pytest.raises(L.PhenDiffHipError):
        M.manifold_query_device(f, f)
    with pytest.raises(L.PhenDiffHipError):
        M.precision_recall_device(f, f)
    with pytest.raises(L.PhenDiffHipError):
        M.density_coverage_device(f, f)
    with pytest.raises(L.PhenDiffHipError):
        M.density_coverage_device(f.numpy(), f.numpy())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_numpy_twins_equal_the_reference(case):
    """The Gram-form twins against direct differences: decisions (hence the five metrics and the counts) exactly, values within TOL."""
    import phendiff_amd.metrics as M
    real, gen, _ = R.fixture(*case)
    ref = R.check_fixture(case)
    k = case[3]
    pr, dc = M.precision_recall(gen, real, k), M.density_coverage(gen, real, k)
    assert set(pr) == {M.KEY_PRECISION, M.KEY_RECALL, M.KEY_F_SCORE} and set(dc) == {M.KEY_DENSITY, M.KEY_COVERAGE}
    for key, v in list(pr.items()) + list(dc.items()):
        assert v == ref[key], (key, v, ref[key])
    rad2, want = M.knn_radii(real, k), R.radii(real, k)
    e_r = float((np.abs(rad2 - want) / R.radii_scale(real, k)).max())
    count, dmin2 = M.manifold_query(gen, real, rad2)
    want_count, want_min = R.query(gen, real, want)
    e_m = float((np.abs(dmin2 - want_min) / R.query_scale(gen, real)).max())
    print(f"numpy twins {case}: max |d rad2| / norms = {e_r:.3e}, max |d dmin2| / norms = {e_m:.3e} (bound {R.TOL:g})")
    assert e_r <= R.TOL and e_m <= R.TOL and np.array_equal(count, want_count)
    assert M.manifold_query(gen, real)[0] is None


def test_numpy_radii_agree_with_sklearn():
    neighbors = pytest.importorskip("sklearn.neighbors")
    import phendiff_amd.metrics as M
    for case in ((300, 280, 64, 5), (210, 200, 2048, 3)):
        real, _, _ = R.fixture(*case)
        k = case[3]
        f = real.astype(np.float64)
        dist, _ = neighbors.NearestNeighbors(n_neighbors=k + 1, algorithm="brute", metric="euclidean").fit(f).kneighbors(f)
        want = dist[:, k] ** 2
        got = M.knn_radii(real, k)
        # sklearn's brute force is itself a Gram form followed by a square root: its own error is a few ulps of the norms, not of d2
        err = float((np.abs(got - want) / R.radii_scale(real, k)).max())
        print(f"knn_radii vs sklearn {case}: max |d rad2| / norms = {err:.3e} (bound {R.TOL:g})")
        assert err <= R.TOL


def test_blocked_path_equals_the_unblocked_one():
    import phendiff_amd.metrics as M
    case = (260, 130, 192, 5)
    real, gen, _ = R.fixture(*case)
    k = case[3]
    whole = (M.precision_recall(gen, real, k, block_rows=1 << 20), M.density_coverage(gen, real, k, block_rows=1 << 20))
    for rows in (1, 7, 64, 129):
        assert (M.precision_recall(gen, real, k, block_rows=rows), M.density_coverage(gen, real, k, block_rows=rows)) == whole, rows
    r_whole = M.knn_radii(real, k, block_rows=1 << 20)
    c_whole, m_whole = M.manifold_query(gen, real, r_whole, block_rows=1 << 20)
    for rows in (1, 7, 64, 129):
        r_b = M.knn_radii(real, k, block_rows=rows)
        c_b, m_b = M.manifold_query(gen, real, r_whole, block_rows=rows)
        assert np.array_equal(c_b, c_whole), rows
        assert (np.abs(r_b - r_whole) <= R.TOL * R.radii_scale(real, k)).all() and (np.abs(m_b - m_whole) <= R.TOL * R.query_scale(gen, real)).all(), rows


def test_numpy_twins_edge_cases():
    import phendiff_amd.metrics as M
    real, gen, _ = R.fixture(70, 70, 64, 1)
    twice = np.concatenate([real, real])
    # every row has a twin: distance 0 up to the rounding of BLAS's Gram form (the exact 0.0 is the KERNEL's property: its norms are Gram
    # entries; numpy's are not)
    scale = 2 * R.norms(twice)
    assert (M.knn_radii(twice, 1) <= R.TOL * scale).all()
    count, dmin2 = M.manifold_query(twice, twice, R.TOL * scale)
    assert (count >= 2).all() and (dmin2 <= R.TOL * scale).all()
    bad = real.copy()
    bad[5] = np.nan
    count, dmin2 = M.manifold_query(gen, bad, M.knn_radii(bad, 3))           # a NaN reference row is never near anything
    keep = np.arange(len(real)) != 5
    c0, m0 = M.manifold_query(gen, real[keep], M.knn_radii(bad, 3)[keep])
    assert np.array_equal(count, c0) and np.array_equal(dmin2, m0) and np.isinf(M.knn_radii(bad, 3)[5])
    with pytest.raises(ValueError):
        M.knn_radii(real, 0)
    with pytest.raises(ValueError):
        M.knn_radii(real[:3], 3)
    assert M._f_score(0.0, 0.0) == 0.0


def test_new_switches_default_to_off_and_cost_nothing(monkeypatch):
    """calculate_metrics with the new switches off returns exactly the old keys and calls none of the new functions."""
    import phendiff_amd.metrics as M
    for fn in (M.calculate_metrics, M.class_metrics_hook):
        par = inspect.signature(fn).parameters
        assert par["prc"].default is False and par["dc"].default is False
        assert par["prc_neighborhood"].default == 3 and par["dc_nearest_k"].default == 5
    assert inspect.signature(M.precision_recall_device).parameters["neighborhood"].default == 3
    assert inspect.signature(M.density_coverage_device).parameters["nearest_k"].default == 5
    real, gen, ref = R.fixture(150, 77, 64, 3)
    feats = {id(gen): {"2048": gen.astype(np.float64), "logits_unbiased": gen.astype(np.float64)[:, :10]},
             id(real): {"2048": real.astype(np.float64), "logits_unbiased": real.astype(np.float64)[:, :10]}}
    monkeypatch.setattr(M, "extract_features", lambda net, images, batch_size=64: feats[id(images)])
    on = M.calculate_metrics(None, gen, real, isc=True, fid=False, kid=True, kid_subset_size=20, prc=True, dc=True, dc_nearest_k=3)
    assert {k: on[k] for k in ("precision", "recall", "f_score", "density", "coverage")} == {k: ref[k] for k in ref if k != "margin"}
    only = M.calculate_metrics(None, gen, real, isc=False, fid=False, kid=False, prc=True)      # needs the real features without fid / kid
    assert only == {k: ref[k] for k in ("precision", "recall", "f_score")}

    def boom(*a, **k):
        raise AssertionError("a precision / recall / density / coverage function ran with its switch off")
    for name in ("precision_recall", "density_coverage", "precision_recall_device", "density_coverage_device", "manifold_metrics_device",
                 "knn_radii", "manifold_query", "knn_radii_device", "manifold_query_device"):
        monkeypatch.setattr(M, name, boom)
    off = M.calculate_metrics(None, gen, real, isc=True, fid=False, kid=True, kid_subset_size=20)
    assert set(off) == {M.KEY_ISC_MEAN, M.KEY_ISC_STD, M.KEY_KID_MEAN, M.KEY_KID_STD}
    assert off == {k: on[k] for k in off}
    with pytest.raises(AssertionError):
        M.calculate_metrics(None, gen, real, isc=False, fid=False, kid=False, dc=True)
