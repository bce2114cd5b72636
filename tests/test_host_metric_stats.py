"""``pd_kid_mmd`` / ``pd_feature_moments`` without a GPU: the C ABI (struct layout, exports, workspace queries, every refusal before a
launch) and the Python surface of the device statistics in ``phendiff_amd.metrics`` (the subset tables reproduce the host loop's draws;
no CPU fallback; the new switch defaults to off)."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

from abi_header import define, header_fields


def test_structs_and_constants_match_header():
    import phendiff_amd._lib as L
    want = ["D", "S", "m", "degree", "N1", "N2", "f1_stride", "f2_stride", "idx_stride", "gamma", "coef0", "f1", "f2", "idx1", "idx2", "sums",
            "mmd", "workspace", "workspace_bytes"]
    assert header_fields("pd_kid_mmd_args") == want == [f[0] for f in L.KidMmdArgs._fields_]
    assert [getattr(L.KidMmdArgs, f).offset for f in want] == [0, 4, 8, 12] + list(range(16, 136, 8))
    assert C.sizeof(L.KidMmdArgs) == 136
    want = ["D", "N", "f_stride", "cov_stride", "f", "mean", "cov", "workspace", "workspace_bytes"]
    assert header_fields("pd_feature_moments_args") == want == [f[0] for f in L.FeatureMomentsArgs._fields_]
    assert [getattr(L.FeatureMomentsArgs, f).offset for f in want] == list(range(0, 72, 8))
    assert C.sizeof(L.FeatureMomentsArgs) == 72
    assert define("PD_METRIC_STATS_TILE") == L.METRIC_STATS_TILE
    assert define("PD_FEATURE_MOMENTS_CHUNK") == L.FEATURE_MOMENTS_CHUNK


def test_symbols_are_exported_and_abi_stays_8():
    import phendiff_amd._lib as L
    lib = L.lib()
    for name in ("pd_kid_mmd", "pd_kid_mmd_workspace", "pd_feature_moments", "pd_feature_moments_workspace"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == 8


def test_workspace_queries():
    import phendiff_amd._lib as L
    lib = L.lib()
    tiles = lambda m: (lambda nt: nt * (nt + 1) + nt * nt)((m + L.METRIC_STATS_TILE - 1) // L.METRIC_STATS_TILE)      # noqa: E731
    assert lib.pd_kid_mmd_workspace(1, 2) == 3 * 8
    assert lib.pd_kid_mmd_workspace(4, 64) == 4 * 3 * 8
    assert lib.pd_kid_mmd_workspace(3, 77) == 3 * 10 * 8 == 3 * tiles(77) * 8
    assert lib.pd_kid_mmd_workspace(100, 1000) == 100 * 528 * 8 == 100 * tiles(1000) * 8
    for bad in ((0, 50), (-1, 50), (3, 1), (3, 0), (3, -5), (1 << 20, 1 << 20), (1, 1 << 31)):
        assert lib.pd_kid_mmd_workspace(*bad) == 0, bad
    ck = L.FEATURE_MOMENTS_CHUNK
    assert lib.pd_feature_moments_workspace(2, 64) == 64 * 8
    assert lib.pd_feature_moments_workspace(ck, 192) == 192 * 8
    assert lib.pd_feature_moments_workspace(ck + 1, 192) == 2 * 192 * 8
    assert lib.pd_feature_moments_workspace(5000, 2048) == ((5000 + ck - 1) // ck) * 2048 * 8
    for bad in ((1, 64), (0, 64), (-3, 64), (300, 0), (300, 32), (300, 100), (300, 4160), (300, -64), (1 << 31, 64)):
        assert lib.pd_feature_moments_workspace(*bad) == 0, bad


def test_kid_mmd_refusals_before_any_launch():
    """Every refusal returns a negative code and names what it refuses; the stream is null and no pointer is dereferenced."""
    import phendiff_amd._lib as L
    lib = L.lib()
    ok = dict(D=64, S=3, m=77, degree=3, N1=150, N2=131, f1_stride=64, f2_stride=128, idx_stride=77, gamma=1 / 64, coef0=1.0, f1=0x10000,
              f2=0x20000, idx1=0x30000, idx2=0x40000, sums=0x50000, mmd=0x60000, workspace=0x70000, workspace_bytes=3 * 10 * 8)

    def refused(word, **change):
        rc = lib.pd_kid_mmd(C.byref(L.KidMmdArgs(**dict(ok, **change))), None)
        msg = lib.pd_last_error()
        assert rc < 0, (change, rc, msg)
        assert word in msg, (change, msg)

    assert lib.pd_kid_mmd(None, None) == -1 and b"null args" in lib.pd_last_error()
    for name in ("f1", "f2", "idx1", "idx2", "sums", "mmd", "workspace"):
        refused(b"null", **{name: None})
    for D in (0, 32, 100, 4160, -64):
        refused(b"D = ", D=D)
    refused(b"stride", f1_stride=60)
    refused(b"stride", f2_stride=32)
    refused(b"stride", f1_stride=66)
    refused(b"stride", f2_stride=130)
    refused(b"aligned", f1=0x10004)
    refused(b"S = 0", S=0)
    refused(b"S = -2", S=-2)
    refused(b"m = 1", m=1)
    refused(b"m = 0", m=0)
    refused(b"exceeds", m=132, idx_stride=132)
    refused(b"exceeds", N1=76)
    refused(b"idx_stride", idx_stride=76)
    refused(b"degree", degree=0)
    refused(b"degree", degree=9)
    for v in (math.nan, math.inf, -math.inf):
        refused(b"gamma", gamma=v)
        refused(b"coef0", coef0=v)
    refused(b"workspace_bytes", workspace_bytes=3 * 10 * 8 - 1)
    refused(b"grid too large", S=1 << 30, N1=1 << 22, N2=1 << 22, m=1 << 20, idx_stride=1 << 20, workspace_bytes=1 << 62)


def test_feature_moments_refusals_before_any_launch():
    import phendiff_amd._lib as L
    lib = L.lib()
    ok = dict(D=128, N=129, f_stride=192, cov_stride=192, f=0x10000, mean=0x20000, cov=0x30000, workspace=0x40000, workspace_bytes=3 * 128 * 8)

    def refused(word, **change):
        rc = lib.pd_feature_moments(C.byref(L.FeatureMomentsArgs(**dict(ok, **change))), None)
        msg = lib.pd_last_error()
        assert rc < 0, (change, rc, msg)
        assert word in msg, (change, msg)

    assert lib.pd_feature_moments(None, None) == -1 and b"null args" in lib.pd_last_error()
    for name in ("f", "mean", "cov", "workspace"):
        refused(b"null", **{name: None})
    for D in (0, 32, 100, 4160, -64):
        refused(b"D = ", D=D)
    refused(b"stride f", f_stride=64)
    refused(b"stride f", f_stride=130)
    refused(b"stride cov", cov_stride=127)
    refused(b"aligned", f=0x10008)
    refused(b"N = 1", N=1)
    refused(b"N = 0", N=0)
    refused(b"workspace_bytes", workspace_bytes=3 * 128 * 8 - 1)
    refused(b"grid too large", N=1 << 31, workspace_bytes=1 << 62)


def test_kid_subset_indices_reproduce_the_host_loop():
    """The tables hold exactly the host loop's draws: MMD^2 recomputed in numpy from them, with the host function's own expressions,
    gives kernel_inception_distance's mean and std bit for bit."""
    import phendiff_amd.metrics as M
    n1, n2, S, m = 300, 260, 10, 50
    rng = np.random.default_rng(5)
    f1 = np.abs(rng.standard_normal((n1, 64))).astype(np.float32).astype(np.float64)
    f2 = (np.abs(rng.standard_normal((n2, 64))) + 0.3).astype(np.float32).astype(np.float64)
    i1, i2 = M.kid_subset_indices(n1, n2, S, m)
    assert i1.dtype == i2.dtype == np.int32 and i1.shape == i2.shape == (S, m)
    assert all(len(set(r)) == m for r in i1) and all(len(set(r)) == m for r in i2)
    assert 0 <= i1.min() and i1.max() < n1 and 0 <= i2.min() and i2.max() < n2
    gam, mmds = 1.0 / 64, np.zeros(S)
    for s in range(S):
        a, b = f1[i1[s]], f2[i2[s]]
        kxx, kxy, kyy = (a @ a.T * gam + 1) ** 3, (a @ b.T * gam + 1) ** 3, (b @ b.T * gam + 1) ** 3
        mmds[s] = ((kxx.sum() - np.trace(kxx)) + (kyy.sum() - np.trace(kyy))) / (m * (m - 1)) - 2 * kxy.sum() / (m * m)
    want = M.kernel_inception_distance(f1, f2, kid_subsets=S, kid_subset_size=m)
    assert want[M.KEY_KID_MEAN] == float(np.mean(mmds)) and want[M.KEY_KID_STD] == float(np.std(mmds))
    j1, j2 = M.kid_subset_indices(n1, n2, S, m, rng_seed=7)
    assert not np.array_equal(i1, j1)
    with pytest.raises(ValueError):
        M.kid_subset_indices(n1, n2, S, 261)


def test_device_functions_have_no_cpu_fallback():
    import phendiff_amd._lib as L
    import phendiff_amd.metrics as M
    f = torch.rand(40, 64)
    with pytest.raises(L.PhenDiffHipError):
        M.kernel_inception_distance_device(f, f, kid_subsets=2, kid_subset_size=8)
    with pytest.raises(L.PhenDiffHipError):
        M.fid_statistics_device(f)
    with pytest.raises(L.PhenDiffHipError):
        M.kid_mmd_device(f, f, np.zeros((1, 2), np.int32), np.zeros((1, 2), np.int32))
    with pytest.raises(L.PhenDiffHipError):
        M.fid_statistics_device(f.double().numpy())


def test_device_statistics_switch_defaults_to_off():
    import phendiff_amd.metrics as M
    assert inspect.signature(M.calculate_metrics).parameters["device_statistics"].default is False
    assert inspect.signature(M.class_metrics_hook).parameters["device_statistics"].default is False
    assert callable(M.extract_features_device)
