"""pd_sample_stats / check_gaussianity / sample_distances on the MI355X against the numpy float64 restatement (tests/gaussianity_ref.py),
computed on the rounded values widened to float64.

Bounds (each figure is printed before it is asserted; run with -s):
  * moments: |m_k(gpu) - m_k(ref)| <= 1e-9 * mean(|d|^k), |mean(gpu) - mean(ref)| <= 1e-9 * mean|x|.  A float64 sum of n terms in any
    order is off by at most n * 2^-53 times the sum of the magnitudes, i.e. n * 2^-53 = 4.7e-10 of mean(|d|^k) at n = 2^22; the shapes here
    stay below 2^15 and the kernel sums in a tree, so the expected figure is near 1e-15.  min, max and the non-finite count are exact.
  * K^2: |K2(gpu) - K2(ref)| <= 1e-6 * (1 + K2).  Z1 ~ b1 * sqrt(n / 6) with b1 = m3 / m2^1.5: a relative moment error of 1e-9 moves b1 by
    at most 2.5e-9 * (|b1| + mean|d|^3 / m2^1.5), times sqrt(n / 6) <= 74 at n <= 2^15, so Z1 (and likewise Z2) by < 1e-6 (1 + |Z|).
  * distances: 1e-9 relative (the same summation bound); max |e| exact.
  * histogram: equal to np.histogram count for count.
  * invariances: torch.equal."""
import ctypes as C

import numpy as np
import pytest
import torch

import gaussianity_ref as R
from guard_bands import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
RANGE = (-3.0, 3.0)


def chunk():
    from phendiff_amd import diagnostics as D
    return D.CHUNK


def shapes():
    ck = chunk()
    return [(1, 8), (3, 105), (2, ck), (2, ck + 1), (3, 2 * ck + 5), (5, 4099), (2, 3 * 32 * 32)]


def draw(B, n, dtype, seed=0):
    """Rows cycle through normal, uniform(-2, 2) and Student-t(5) draws; returned as the rounded CPU tensor of `dtype`."""
    rng = np.random.default_rng(seed * 1000003 + B * 7919 + n)
    rows = []
    for b in range(B):
        rows.append((rng.standard_normal(n), rng.uniform(-2, 2, n), rng.standard_t(5, n))[b % 3])
    return torch.from_numpy(np.stack(rows)).to(dtype)


def f64(t):
    return t.detach().cpu().to(torch.float64).numpy()


def run(x, y=None, edges=None):
    """The product's thin wrapper over one pd_sample_stats call; returns (stats float64 [B, 10], hist int64 [B, bins] or None) on the host."""
    from phendiff_amd import diagnostics as D
    stats, hist = D.sample_stats(x, y=y, edges=edges)
    torch.cuda.synchronize()
    return stats.cpu().numpy(), (None if hist is None else hist.cpu().numpy().view(np.uint32).astype(np.int64))


def col(stats, name):
    from phendiff_amd import diagnostics as D
    return stats[:, D.STATS_FIELDS.index(name)]


def check_moments(x_cpu, stats, what):
    """Asserts the moment, K^2 and exact-field bounds of every row; returns the largest (error / scale) seen."""
    worst_m, worst_k = 0.0, 0.0
    n = x_cpu.shape[1]
    for b in range(x_cpu.shape[0]):
        m = R.moments(f64(x_cpu[b]))
        mean = col(stats, "sum")[b] / n
        errs = [abs(mean - m["mean"]) / m["abs1"] if m["abs1"] > 0 else abs(mean - m["mean"])]
        for k in (2, 3, 4):
            scale = m["abs_d"][k]
            e = abs(col(stats, f"m{k}")[b] - m[f"m{k}"])
            errs.append(e / scale if scale > 0 else e)
        worst_m = max(worst_m, max(errs))
        assert max(errs) <= 1e-9, (what, b, errs)
        assert col(stats, "min")[b] == m["min"] and col(stats, "max")[b] == m["max"] and col(stats, "nonfinite")[b] == 0, (what, b)
        if n >= 8 and m["m2"] > 0:
            k2_ref, _ = R.normaltest_of_moments(n, m["m2"], m["m3"], m["m4"])
            k2, _ = R.normaltest_of_moments(n, col(stats, "m2")[b], col(stats, "m3")[b], col(stats, "m4")[b])
            ek = abs(k2 - k2_ref) / (1 + k2_ref)
            worst_k = max(worst_k, ek)
            assert ek <= 1e-6, (what, b, k2, k2_ref)
    print(f"pd_sample_stats {what}: max moment error / mean|d|^k = {worst_m:.3e} (bound 1e-9), max |dK2| / (1 + K2) = {worst_k:.3e} (bound 1e-6)")
    return worst_m, worst_k


# ---------------------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("mode", list(DTYPES))
def test_moments_and_k2_match_the_restatement(mode):
    for B, n in shapes():
        x = draw(B, n, DTYPES[mode])
        stats, _ = run(x.to(DEV))
        check_moments(x, stats, f"{mode} ({B}, {n})")
        assert np.all(col(stats, "err_l1") == 0) and np.all(col(stats, "err_sq") == 0) and np.all(col(stats, "err_max") == 0)


@pytest.mark.parametrize("mode", list(DTYPES))
def test_shifted_and_outlier_samples(mode):
    """Row 0: N(1000, 1) -- the mean cancels nine digits, where a one-pass sum of squares would fail.  Row 1: a constant and one outlier."""
    n = 4099
    rng = np.random.default_rng(5)
    x = np.stack([1000.0 + rng.standard_normal(n), np.full(n, 0.5)])
    x[1, 1234] = 7.0
    x = torch.from_numpy(x).to(DTYPES[mode])
    stats, _ = run(x.to(DEV))
    check_moments(x, stats, f"{mode} shifted / outlier")


# ---------------------------------------------------------------------------------------------------------------- histogram
def neighbours(t):
    """The representable values just below and just above each (finite, non-zero) element of `t`, in t's own format."""
    it = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    away = torch.where(it < 0, -1, 1).to(it.dtype)      # bits + 1 grows the magnitude: upward for a positive value, downward for a negative one
    return (it - away).view(t.dtype), (it + away).view(t.dtype)


def edge_case_batch(bins, dtype, n_fill):
    edges = np.linspace(RANGE[0], RANGE[1], bins + 1)
    e = torch.from_numpy(edges).to(dtype)      # every edge value, rounded to the format
    picks = sorted({k for k in (1, bins // 6 + 1, bins // 2 - 1, bins // 2 + 1, bins) if 1 <= k <= bins})      # five edges (fewer for bins = 1)
    near = e[[k for k in picks if float(e[k]) != 0.0]]
    below, above = neighbours(near)
    special = torch.tensor([-3.0, 3.0, 0.0, -3.5, 4.0, 100.0, -100.0, float("nan"), float("inf"), float("-inf")]).to(dtype)
    rng = np.random.default_rng(bins)
    row0 = torch.cat([special, e, below, above, torch.from_numpy(rng.standard_normal(n_fill) * 1.5).to(dtype)])
    row0 = row0[torch.from_numpy(rng.permutation(row0.numel()))]
    row1 = torch.from_numpy(rng.uniform(-4, 4, row0.numel())).to(dtype)
    return torch.stack([row0, row1]), edges


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("bins", [1, 100, 4096])
def test_histogram_equals_numpy(bins, mode):
    from phendiff_amd import diagnostics as D
    assert D.MAX_BINS == 4096
    x, edges = edge_case_batch(bins, DTYPES[mode], n_fill=3000 + chunk())      # more than one chunk: the flush adds across workgroups
    stats, hist = run(x.to(DEV), edges=edges)
    n = x.shape[1]
    for b in range(2):
        want, ref_edges = R.histogram(f64(x[b]), bins, RANGE)
        assert np.array_equal(ref_edges, edges)
        diff = np.nonzero(hist[b] != want)[0]
        assert diff.size == 0, (b, diff[:8], hist[b][diff[:8]], want[diff[:8]])
        assert hist[b].sum() + R.outside(f64(x[b]), RANGE) == n
    assert col(stats, "nonfinite").tolist() == [3.0, 0.0]
    assert col(stats, "min")[1] == f64(x[1]).min() and col(stats, "max")[1] == f64(x[1]).max()
    assert col(stats, "min")[0] == -np.inf and col(stats, "max")[0] == np.inf      # (the NaN is passed over)


# ---------------------------------------------------------------------------------------------------------------- distances
@pytest.mark.parametrize("mode", list(DTYPES))
def test_distances_match_vector_norm(mode):
    worst = 0.0
    for B, n in ((3, 105), (3, 2 * chunk() + 5)):
        x, y = draw(B, n, DTYPES[mode], seed=1), draw(B, n, DTYPES[mode], seed=2)
        for yy in (y, y[1].contiguous()):
            stats, _ = run(x.to(DEV), y=yy.to(DEV))
            want = R.distances(f64(x), f64(yy))
            got = {"l1": col(stats, "err_l1"), "l2": np.sqrt(col(stats, "err_sq")), "linf": col(stats, "err_max")}
            for k in ("l1", "l2"):
                rel = np.abs(got[k] - want[k]) / want[k]
                worst = max(worst, rel.max())
                assert rel.max() <= 1e-9, (k, B, n, rel)
            assert np.array_equal(got["linf"], want["linf"])
    print(f"pd_sample_stats {mode} distances: max relative error {worst:.3e} (bound 1e-9)")


# ---------------------------------------------------------------------------------------------------------------- invariances
class Call:
    """One pd_sample_stats call through ctypes on caller-held buffers (so a test can guard them, poison them or capture the launches)."""

    def __init__(self, x, y=None, edges=None, guard=False):
        import phendiff_amd._lib as L
        self.L, self.guards = L, {}
        B = x.shape[0]
        n = x.numel() // B
        bins = 0 if edges is None else len(edges) - 1

        def place(t, name):
            if not guard:
                return t.to(DEV)
            view, h = guarded(t, device=DEV, name=name)
            self.guards[name] = h
            return view

        self.x = place(x, "x")
        self.y = None if y is None else place(y, "y")
        self.edges = None if edges is None else place(torch.from_numpy(np.asarray(edges, dtype=np.float64)), "edges")
        ws_bytes = L.lib().pd_sample_stats_workspace(B, n, bins)
        assert ws_bytes > 0 and ws_bytes % 8 == 0
        self.stats = place(torch.zeros(B, len(L.SAMPLE_STATS_FIELDS), dtype=torch.float64), "stats")
        self.hist = None if edges is None else place(torch.zeros(B, bins, dtype=torch.int32), "hist")
        self.ws = place(torch.zeros(ws_bytes // 8, dtype=torch.float64), "workspace")
        stride = 0 if y is None or y.dim() == 1 else n
        dt = {torch.float32: L.PD_F32, torch.bfloat16: L.PD_BF16, torch.float16: L.PD_F16}[x.dtype]
        self.args = L.SampleStatsArgs(dtype=dt, bins=bins, B=B, n=n, y_sample_stride=stride, x=self.x.data_ptr(), y=L.ptr(self.y),
                                      edges=L.ptr(self.edges), stats=self.stats.data_ptr(), hist=L.ptr(self.hist),
                                      workspace=self.ws.data_ptr(), workspace_bytes=ws_bytes)

    def launch(self):
        L = self.L
        L.check(L.lib().pd_sample_stats(C.byref(self.args), torch.cuda.current_stream().cuda_stream), "pd_sample_stats")

    def scribble(self):
        """Outputs and workspace filled with values no run produces: -1.25e300 in stats / workspace, 0xFFFFFFFF in hist."""
        self.stats.fill_(-1.25e300)
        self.ws.fill_(-1.25e300)
        if self.hist is not None:
            self.hist.fill_(-1)

    def outputs(self):
        torch.cuda.synchronize()
        return self.stats.clone(), (None if self.hist is None else self.hist.clone())


EDGES100 = np.linspace(RANGE[0], RANGE[1], 101)


def shapes_inv():
    return [105, 2 * chunk() + 5]


@pytest.mark.parametrize("mode", list(DTYPES))
def test_a_sample_does_not_depend_on_its_batch(mode):
    for n in shapes_inv():
        x, y = draw(3, n, DTYPES[mode], seed=3), draw(3, n, DTYPES[mode], seed=4)
        whole = Call(x, y, EDGES100)
        whole.launch()
        s3, h3 = whole.outputs()
        alone = Call(x[2:3].contiguous(), y[2:3].contiguous(), EDGES100)      # (its start is aligned; row 2 of the batch starts at 2 n elements)
        alone.launch()
        s1, h1 = alone.outputs()
        assert torch.equal(s1[0], s3[2]) and torch.equal(h1[0], h3[2]), n
        assert not torch.isnan(s3).any()


def test_two_calls_give_the_same_bits():
    x, y = draw(3, 2 * chunk() + 5, torch.float32, seed=5), draw(3, 2 * chunk() + 5, torch.float32, seed=6)
    c = Call(x, y, EDGES100)
    c.launch()
    first = c.outputs()
    c.scribble()
    c.launch()
    second = c.outputs()
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    other = Call(x, y, EDGES100)      # other buffers, other addresses
    other.launch()
    third = other.outputs()
    assert torch.equal(first[0], third[0]) and torch.equal(first[1], third[1])


def test_graph_replay_equals_eager():
    x, y = draw(3, 2 * chunk() + 5, torch.float32, seed=7), draw(3, 2 * chunk() + 5, torch.float32, seed=8)[0].contiguous()      # (one y for all)
    c = Call(x, y, EDGES100)
    c.launch()
    eager = c.outputs()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.launch()
    c.scribble()
    g.replay()
    replay = c.outputs()
    assert torch.equal(eager[0], replay[0]) and torch.equal(eager[1], replay[1])
    c.x.copy_(draw(3, 2 * chunk() + 5, torch.float32, seed=9))      # the captured launches read the buffers, not a snapshot
    g.replay()
    changed = c.outputs()
    assert not torch.equal(eager[0], changed[0])


# ---------------------------------------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("mode", list(DTYPES))
def test_guard_bands(mode):
    for n in shapes_inv():
        x, y = draw(3, n, DTYPES[mode], seed=10), draw(3, n, DTYPES[mode], seed=11)
        c = Call(x, y, EDGES100, guard=True)
        for name in ("x", "y", "edges"):
            c.guards[name].clear()
        for name in ("stats", "hist", "workspace"):
            c.guards[name].canary()
        c.scribble()
        c.launch()
        clean = c.outputs()
        for name in ("stats", "hist", "workspace"):
            assert c.guards[name].intact()
        # every output element was written
        assert not (clean[0] == -1.25e300).any() and not (clean[1] == -1).any() and not (c.ws == -1.25e300).any()
        assert int(clean[1].sum()) <= 3 * n
        for name in ("x", "y", "edges"):      # NaN all around the inputs: not one output bit moves
            c.guards[name].poison()
        c.scribble()
        c.launch()
        poisoned = c.outputs()
        assert torch.equal(clean[0], poisoned[0]) and torch.equal(clean[1], poisoned[1]), n
        for name in ("stats", "hist", "workspace"):
            assert c.guards[name].intact()
        want = Call(x, y, EDGES100)      # and the guarded placement gives what the plain one gives
        want.launch()
        plain = want.outputs()
        assert torch.equal(clean[0], plain[0]) and torch.equal(clean[1], plain[1])


# ---------------------------------------------------------------------------------------------------------------- public surface
def test_check_gaussianity_matches_the_restatement():
    import phendiff_amd as P
    x = draw(4, 3 * 32 * 32, torch.float32, seed=12).reshape(4, 3, 32, 32)
    rep = P.check_gaussianity(x.to(DEV))
    n = 3 * 32 * 32
    assert rep.n == n and rep.hist.shape == (4, 100) and rep.hist.dtype == np.int64 and np.array_equal(rep.edges, EDGES100)
    for b in range(4):
        v = f64(x[b]).reshape(-1)
        m = R.moments(v)
        k2, p = R.normaltest(v)
        assert abs(rep.mean[b] - m["mean"]) <= 1e-9 * m["abs1"]
        std = np.sqrt(m["m2"] * n / (n - 1))
        assert abs(rep.std[b] - std) <= 1e-9 * std
        assert abs(rep.std[b] - float(x[b].double().std())) <= 1e-9 * std      # torch's unbiased .std(), what the reference prints
        assert abs(rep.statistic[b] - k2) <= 1e-6 * (1 + k2)
        assert abs(rep.pvalue[b] - p) <= p * 1e-6 * (1 + k2)                    # dp / p = dK2 / 2
        assert np.array_equal(rep.hist[b], R.histogram(v, 100, RANGE)[0])
        assert rep.minimum[b] == m["min"] and rep.maximum[b] == m["max"] and rep.nonfinite[b] == 0
        assert abs(rep.skewness[b] - m["m3"] / m["m2"] ** 1.5) <= 1e-8 and abs(rep.kurtosis[b] - (m["m4"] / m["m2"] ** 2 - 3)) <= 1e-8
    lines = str(rep).splitlines()
    assert len(lines) == 5 and lines[1].startswith(f"Gaussian(?) 0: mean={rep.mean[0]}, std={rep.std[0]}; 2-sided")
    assert rep.pvalue[0] > rep.pvalue[1] and rep.pvalue[1] < 1e-10      # row 0 is a normal draw, row 1 a uniform one
    few = P.check_gaussianity(x.to(DEV), bins=7, range=(-1.0, 2.0))
    assert np.array_equal(few.hist[2], R.histogram(f64(x[2]).reshape(-1), 7, (-1.0, 2.0))[0])


def test_sample_distances_both_shapes_of_y():
    import phendiff_amd as P
    x = draw(4, 3 * 32 * 32, torch.float32, seed=13).reshape(4, 3, 32, 32).clamp(-1, 1)
    y = draw(4, 3 * 32 * 32, torch.float32, seed=14).reshape(4, 3, 32, 32).clamp(-1, 1)
    for yy in (y, y[0].contiguous()):
        got = P.sample_distances(x.to(DEV), yy.to(DEV))
        want = R.distances(f64(x).reshape(4, -1), f64(yy).reshape(-1, 3 * 32 * 32) if yy.dim() == 4 else f64(yy).reshape(-1))
        assert set(got) == {"l1", "l2", "linf", "mse", "psnr"}
        for k in ("l1", "l2", "mse", "psnr"):
            assert np.all(np.abs(got[k] - want[k]) <= 1e-9 * np.abs(want[k])), k
        assert np.array_equal(got["linf"], want["linf"])
    same = P.sample_distances(x.to(DEV), x.to(DEV))
    assert np.all(same["l2"] == 0) and np.all(np.isinf(same["psnr"]))
    with pytest.raises(ValueError):
        P.sample_distances(x.to(DEV), y[:2].to(DEV))


def test_diagnostics_accept_the_graph_runners_buffers():
    """DDIBGraph(super_small, 32 x 32, 2 steps): `.inverted` goes straight into both functions."""
    import phendiff_amd as P
    from oracle import CondUNet2DRef
    torch.manual_seed(0)
    cfg = dict(P.UNET_CONFIGS["super_small"], sample_size=32)
    keys = CondUNet2DRef.__init__.__code__.co_varnames
    ref_unet = CondUNet2DRef(**{k: v for k, v in cfg.items() if k in keys}).eval()
    unet = P.CustomCondUNet2DModel(compute_dtype="f32", **cfg)
    unet.load_state_dict(ref_unet.state_dict())
    pipe = P.ConditionalDDIMPipeline(unet.to(DEV), P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
    labels = torch.arange(2) % 2
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1234)) * 2 - 1
    g = P.DDIBGraph(pipe, batch_size=2, num_inference_steps=2)
    g.run(x.to(DEV), labels.to(DEV), (1 - labels).to(DEV))
    rep = P.check_gaussianity(g.inverted)
    n = 3 * 32 * 32
    assert rep.n == n and rep.hist.shape == (2, 100)
    for a in (rep.mean, rep.std, rep.skewness, rep.kurtosis, rep.statistic, rep.pvalue, rep.minimum, rep.maximum):
        assert np.isfinite(a).all()
    assert (rep.nonfinite == 0).all() and (rep.hist.sum(axis=1) <= n).all() and (rep.hist >= 0).all()
    want = R.moments(f64(g.inverted[1]).reshape(-1))
    assert abs(rep.mean[1] - want["mean"]) <= 1e-9 * want["abs1"]
    d = P.sample_distances(g.inverted, x.to(DEV))
    assert all(np.isfinite(d[k]).all() for k in ("l1", "l2", "linf", "mse", "psnr"))
    d1 = P.sample_distances(g.inverted, x[0].to(DEV).contiguous())
    assert np.isfinite(d1["l2"]).all() and d1["l2"][0] == d["l2"][0]
