"""The inversion diagnostics without a GPU: the numpy restatement (tests/gaussianity_ref.py) and ``normaltest_from_moments`` against
``scipy.stats.normaltest``, the C ABI of ``pd_sample_stats`` (struct layout, constants, exports, every refusal before a launch) and the
Python surface's refusals.

Tolerances.  K^2 is a smooth function of (n, m2, m3, m4) evaluated in float64 by all three parties from the same rounded data; the
restatement and SciPy were found to agree to <= 4e-15 relative on the inputs below, so 1e-12 is asserted.  p = exp(-K^2 / 2), so
dp / p = dK^2 / 2 <= 1e-12 * K^2 / 2 < 3.5e-10 wherever p > 1e-300 (K^2 < 1382): 1e-9 relative is asserted there, and nothing below
(SciPy's own chi^2 survival function is not accurate to a relative bound in the subnormal tail)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gaussianity_ref as R
from abi_header import ROOT, define, header_fields, source

SIZES = (8, 20, 105, 3072, 4099, 196608)


def draws(n, seed=0):
    rng = np.random.default_rng(seed + n)
    for name, x in (("normal", rng.standard_normal(n)), ("uniform", rng.uniform(-2, 2, n)), ("student-t5", rng.standard_t(5, n))):
        yield name, x.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("n", SIZES)
def test_normaltest_matches_scipy(n):
    stats = pytest.importorskip("scipy.stats")
    import warnings
    from phendiff_amd import normaltest_from_moments
    for name, x in draws(n):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # (SciPy warns that the kurtosis test is inaccurate below n = 20)
            want = stats.normaltest(x)
        m = R.moments(x)
        for who, (k2, p) in (("restatement", R.normaltest(x)), ("product", normaltest_from_moments(n, m["m2"], m["m3"], m["m4"]))):
            rel = abs(k2 - want.statistic) / want.statistic
            print(f"normaltest n={n} {name} {who}: K2 = {k2:.6g}, rel. difference from scipy {rel:.2e}")
            assert rel <= 1e-12, (who, name, k2, want.statistic)
            if want.pvalue > 1e-300:
                assert abs(p - want.pvalue) <= 1e-9 * want.pvalue, (who, name, p, want.pvalue)
            else:
                assert p <= 1e-299


def test_normaltest_small_and_degenerate_samples():
    from phendiff_amd import normaltest_from_moments
    with pytest.raises(ValueError):
        normaltest_from_moments(7, 1.0, 0.0, 3.0)
    with pytest.raises(ValueError):
        R.normaltest(np.arange(7.0))
    k2, p = normaltest_from_moments(100, 0.0, 0.0, 0.0)      # a constant sample: no skewness, no kurtosis
    assert np.isnan(k2) and np.isnan(p)
    k2, p = normaltest_from_moments(8, 1.0, 0.0, 3.0)        # an exactly symmetric sample takes SciPy's y = 1 branch: finite
    assert np.isfinite(k2) and 0 <= p <= 1


def test_product_has_no_scipy_import():
    src = open(os.path.join(ROOT, "phendiff_amd", "diagnostics.py")).read()
    assert not re.search(r"^\s*(import|from)\s+scipy", src, flags=re.M)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_struct_and_constants_match_header():
    import phendiff_amd._lib as L
    want = ["dtype", "bins", "B", "n", "y_sample_stride", "x", "y", "edges", "stats", "hist", "workspace", "workspace_bytes"]
    assert header_fields("pd_sample_stats_args") == want == [f[0] for f in L.SampleStatsArgs._fields_]
    T = L.SampleStatsArgs
    assert [getattr(T, f).offset for f in want] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80]
    assert C.sizeof(T) == 88
    src = source()
    assert define("PD_SAMPLE_STATS_FIELDS") == len(L.SAMPLE_STATS_FIELDS) == 10
    assert define("PD_SAMPLE_STATS_CHUNK") == L.SAMPLE_STATS_CHUNK
    assert define("PD_SAMPLE_STATS_MAX_BINS") == L.SAMPLE_STATS_MAX_BINS
    enum = dict((k.lower(), int(v)) for k, v in re.findall(r"PD_SS_(\w+)\s*=\s*(\d+)", src))
    assert [enum[k] for k in L.SAMPLE_STATS_FIELDS] == list(range(10))
    from phendiff_amd import diagnostics as D
    assert (D.CHUNK, D.MAX_BINS) == (L.SAMPLE_STATS_CHUNK, L.SAMPLE_STATS_MAX_BINS)
    assert L.SAMPLE_STATS_CHUNK % (256 * 8) == 0      # whole 16-byte slots per thread for either element width


def test_symbols_are_exported_and_abi_stays_8():
    import phendiff_amd._lib as L
    lib = L.lib()
    for name in ("pd_sample_stats", "pd_sample_stats_workspace"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == 8


def test_workspace_query():
    import phendiff_amd._lib as L
    lib = L.lib()
    ck = L.SAMPLE_STATS_CHUNK
    assert lib.pd_sample_stats_workspace(1, 1, 0) == 80
    assert lib.pd_sample_stats_workspace(3, ck, 100) == 3 * 80
    assert lib.pd_sample_stats_workspace(3, ck + 1, 100) == 3 * 2 * 80
    assert lib.pd_sample_stats_workspace(32, 3 * 256 * 256, 100) == 32 * 24 * 80
    for bad in ((0, 8, 0), (2, 0, 0), (-1, 8, 0), (2, 8, -1), (2, 8, L.SAMPLE_STATS_MAX_BINS + 1), (1 << 20, 1 << 50, 0)):
        assert lib.pd_sample_stats_workspace(*bad) == 0, bad


def test_refusals_before_any_launch():
    """Every refusal returns its code and names the field; the stream is null and no pointer is dereferenced."""
    import phendiff_amd._lib as L
    lib = L.lib()
    ok = dict(dtype=L.PD_F32, bins=100, B=3, n=105, y_sample_stride=105, x=0x10000, y=0x20000, edges=0x30000, stats=0x40000, hist=0x50000,
              workspace=0x60000, workspace_bytes=3 * 80)

    def refused(code, word, **change):
        rc = lib.pd_sample_stats(C.byref(L.SampleStatsArgs(**dict(ok, **change))), None)
        msg = lib.pd_last_error()
        assert rc == code, (change, rc, msg)
        assert word in msg, (change, msg)

    assert lib.pd_sample_stats(None, None) == -1 and b"null args" in lib.pd_last_error()
    refused(-1, b"null x", x=None)
    refused(-1, b"null stats", stats=None)
    refused(-1, b"null workspace", workspace=None)
    refused(-1, b"dtype", dtype=3)
    refused(-1, b"dtype", dtype=-1)
    refused(-1, b"bins = -1", bins=-1)
    refused(-1, b"without edges", edges=None)
    refused(-1, b"without a hist", hist=None)
    refused(-1, b"workspace_bytes", workspace_bytes=3 * 80 - 8)
    refused(-2, b"B and n", B=0)
    refused(-2, b"B and n", n=-5, y_sample_stride=-5)
    refused(-2, b"bins = 4097", bins=L.SAMPLE_STATS_MAX_BINS + 1)
    refused(-2, b"y_sample_stride", y_sample_stride=104)
    refused(-2, b"y_sample_stride", y_sample_stride=-105)
    refused(-2, b"2^62", B=1 << 20, n=1 << 50, y_sample_stride=0, bins=0)
    refused(-2, b"2^62", B=1 << 31, n=8, y_sample_stride=0)
    refused(-2, b"2^32", B=1, n=1 << 32, y_sample_stride=0)
    refused(-2, b"grid too large", B=1 << 20, n=1 << 30, y_sample_stride=0)      # 2^20 * 2^17 blocks


# ---------------------------------------------------------------------------------------------------------------- Python surface
def test_surface_is_exported_and_needs_a_device():
    import phendiff_amd as P
    from phendiff_amd import diagnostics as D
    assert P.check_gaussianity is D.check_gaussianity and P.sample_distances is D.sample_distances
    assert P.normaltest_from_moments is D.normaltest_from_moments and P.GaussianityReport is D.GaussianityReport
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(P.PhenDiffHipError):
        P.check_gaussianity(x)
    with pytest.raises(P.PhenDiffHipError):
        P.sample_distances(x, x)
    with pytest.raises(ValueError):
        P.check_gaussianity(x, bins=0)
    with pytest.raises(ValueError):
        P.check_gaussianity(x, bins=D.MAX_BINS + 1)
    with pytest.raises(ValueError):
        P.check_gaussianity(x, range=(1.0, 1.0))


def test_report_prints_the_reference_line():
    from phendiff_amd import GaussianityReport
    z = np.zeros(2)
    rep = GaussianityReport(n=48, shape=(2, 3, 4, 4), mean=np.array([0.25, -1.5]), std=np.array([1.0, 2.0]), skewness=z, kurtosis=z,
                            statistic=z, pvalue=np.array([0.5, 1e-3]), minimum=z, maximum=z, nonfinite=np.zeros(2, dtype=np.int64),
                            hist=np.zeros((2, 4), dtype=np.int64), edges=np.linspace(-3, 3, 5))
    lines = str(rep).splitlines()
    assert lines[0] == "Checking Gausianity of components of tensor of shape (2, 3, 4, 4)..."
    assert lines[1] == "Gaussian(?) 0: mean=0.25, std=1.0; 2-sided Χ² probability for the normality hypothesis: 0.5"
    assert lines[2] == "Gaussian(?) 1: mean=-1.5, std=2.0; 2-sided Χ² probability for the normality hypothesis: 0.001"


def test_restatement_histogram_rule():
    """np.histogram's rule, which the kernel's contract restates: left-closed bins, the last one closed on both sides."""
    x = np.array([-3.0, 3.0, 0.0, np.nextafter(3.0, 4.0), np.nextafter(-3.0, -4.0), np.nan, np.inf, -np.inf, 2.999])
    counts, edges = R.histogram(x, 4, (-3.0, 3.0))
    assert counts.tolist() == [1, 0, 1, 2] and R.outside(x, (-3.0, 3.0)) == 5 and counts.sum() + 5 == x.size
