"""pd_ssim / ssim_maps_means / sample_ssim on the MI355X against the torch float64 restatement on the CPU (tests/ssim_ref.py), both fed the
same values: rounded to the engine's dtype on the host, then widened exactly.

Bounds (each figure is printed before it is asserted; run with -s):
  * every mean ssim / cs (magnitude <= 1): |got - ref| <= 1e-9; the final scalars: <= 1e-9 * (1 + |ref|) -- the project's bound for its fp64
    diagnostics (tests/test_gpu_sample_stats.py).  With |x| <= 4 and R = 2 a filtered map is an fp64 sum of <= 1089 products of magnitude
    <= 16, off by about 1e-14, divided by a denominator >= C2 = 3.6e-3: three orders inside the bound.
  * invariances (batch, alignment, repetition, stream, graph replay, guard bands): torch.equal.

The tile of the pass is 16 x 32 valid positions: (2, 2, 70, 133) with win 11 has 60 x 123 of them, 4 x 4 tiles, ragged in both axes."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssim_ref as R
from guard_bands import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
BOUND = 1e-9

# (B, C, H, W, win, levels)
SINGLE = [(2, 3, 11, 11, 11, 1), (1, 1, 12, 47, 11, 1), (3, 5, 45, 67, 11, 1), (2, 2, 70, 133, 11, 1), (1, 32, 40, 40, 7, 1),
          (2, 3, 33, 40, 33, 1), (2, 3, 3, 3, 3, 1)]
MULTI = [(2, 3, 45, 51, 11, 3), (1, 2, 176, 176, 11, 5), (1, 1, 177, 190, 11, 5)]
SHARED_Y = [(3, 5, 45, 67, 11, 1), (2, 3, 45, 51, 11, 3)]
SIGMA = {3: 0.5, 7: 1.0, 11: 1.5, 33: 5.0}


def smooth(B, Cc, H, W, rng):
    yy, xx = np.meshgrid(np.linspace(0, 3, H), np.linspace(0, 4, W), indexing="ij")
    phase = rng.uniform(0, 6, (B, Cc, 1, 1))
    return 0.6 * np.sin(2.1 * xx + phase) * np.cos(1.7 * yy + 0.5 * phase) + 0.1


def pair(shape, dtype, kind="perturbed", seed=0):
    """(x, y) on the CPU in `dtype`.  perturbed: a smooth image plus noise against a differently perturbed copy; same: y = x; flat: a
    background of 0.9 + 1e-4 noise, twice; anti: y = -x plus a little noise."""
    B, Cc, H, W = shape
    rng = np.random.default_rng(seed * 7919 + B * 1000003 + Cc * 10007 + H * 131 + W)
    noise = lambda s: s * rng.standard_normal((B, Cc, H, W))      # noqa: E731
    if kind == "flat":
        x, y = 0.9 + noise(1e-4), 0.9 + noise(1e-4)
    else:
        base = smooth(B, Cc, H, W, rng)
        x = base + noise(0.2 if kind == "anti" else 0.05)
        y = {"perturbed": lambda: base + noise(0.15), "same": lambda: x, "anti": lambda: -x + noise(0.02)}[kind]()
    return torch.from_numpy(x).to(dtype), torch.from_numpy(y).to(dtype)


def run(x, y, win, levels, **kw):
    """ssim_maps_means on the device; the [B, C, levels, 2] array on the host."""
    from phendiff_amd import diagnostics as D
    out = D.ssim_maps_means(x.to(DEV), y.to(DEV), levels=levels, win_size=win, sigma=SIGMA[win], **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_REF = {}


def ref(case, mode, kind, shared=False):
    """(x, y, maps_means of the reference) of a case, computed once."""
    key = (case, mode, kind, shared)
    if key not in _REF:
        B, Cc, H, W, win, levels = case
        x, y = pair((B, Cc, H, W), DTYPES[mode], kind)
        if shared:
            y = y[B - 1].contiguous()
        _REF[key] = (x, y, R.maps_means(x, y, levels=levels, win=win, sigma=SIGMA[win]))
    return _REF[key]


def check(got, want, what):
    """Asserts the bound on every mean and on the final scalars; returns the worst |got - ref| over the means."""
    assert got.shape == want.shape and np.isfinite(want).all(), what
    worst = np.abs(got - want).max()
    gs, ws = R.scores(got), R.scores(want)
    worst_s = max(np.abs(gs[k] - ws[k]).max() / (1 + np.abs(ws[k]).max()) for k in ws)
    print(f"pd_ssim {what}: max |mean - ref| = {worst:.3e}, final scalars {worst_s:.3e} (bound {BOUND:g})")
    assert worst <= BOUND, what
    for k in ws:
        assert np.all(np.abs(gs[k] - ws[k]) <= BOUND * (1 + np.abs(ws[k]))), (what, k)
    return worst


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("mode", list(DTYPES))
def test_parity_with_the_reference(mode):
    worst = 0.0
    for case in SINGLE + MULTI:
        x, y, want = ref(case, mode, "perturbed")
        worst = max(worst, check(run(x, y, case[4], case[5]), want, f"{mode} {case}"))
        if case[4] == 11 and case[2] > 11:
            assert 0.05 < want[..., 0].mean() < 0.95, case      # neither noise against noise nor a copy
    for case in SHARED_Y:
        x, y, want = ref(case, mode, "perturbed", shared=True)
        assert y.dim() == 3
        worst = max(worst, check(run(x, y, case[4], case[5]), want, f"{mode} {case} shared y"))
    print(f"pd_ssim {mode}: worst |mean - ref| over all shapes = {worst:.3e} (bound {BOUND:g})")


@pytest.mark.parametrize("mode", list(DTYPES))
def test_identical_flat_and_anticorrelated_images(mode):
    for case in ((3, 5, 45, 67, 11, 1), (2, 3, 45, 51, 11, 3)):
        x, y, want = ref(case, mode, "same")
        got = run(x, y, case[4], case[5])
        check(got, want, f"{mode} {case} y = x")
        assert np.abs(got - 1.0).max() <= BOUND
        # a flat background: E[x^2] - mu^2 cancels eight digits, what fp32 arithmetic would lose
        x, y, want = ref(case, mode, "flat")
        check(run(x, y, case[4], case[5]), want, f"{mode} {case} flat background")
        # anti-correlated: cs < 0 at every scale, so the clamp of MS-SSIM is what keeps the power real
        x, y, want = ref(case, mode, "anti")
        assert (want[..., 1] < -0.25).all(), want[..., 1]
        got = run(x, y, case[4], case[5])
        check(got, want, f"{mode} {case} anti-correlated")
        assert (got[..., 1] < 0).all()
        if case[5] > 1:
            assert np.all(R.scores(got)["ms_ssim"] == 0.0)


# ---------------------------------------------------------------------------------------------------------------- the API
def test_sample_ssim_keys_shapes_and_weights():
    import phendiff_amd as P
    case = (2, 3, 45, 51, 11, 3)
    x, y, want = ref(case, "f32", "perturbed")
    xd, yd = x.to(DEV), y.to(DEV)
    one = P.sample_ssim(xd, yd)
    assert set(one) == {"ssim", "ssim_per_channel", "cs_per_channel"}
    assert one["ssim"].shape == (2,) and one["ssim_per_channel"].shape == (2, 3) and one["cs_per_channel"].shape == (2, 3, 1)
    assert all(v.dtype == np.float64 for v in one.values())
    assert np.array_equal(one["ssim"], one["ssim_per_channel"].mean(axis=1))
    ws = R.scores(want)
    assert np.abs(one["ssim"] - ws["ssim"]).max() <= BOUND
    ms = P.sample_ssim(xd, yd, levels=3)
    assert set(ms) == {"ssim", "ssim_per_channel", "cs_per_channel", "ms_ssim", "ms_ssim_per_channel"}
    assert ms["ms_ssim"].shape == (2,) and ms["ms_ssim_per_channel"].shape == (2, 3) and ms["cs_per_channel"].shape == (2, 3, 3)
    assert np.array_equal(ms["ssim"], one["ssim"]) and np.array_equal(ms["ms_ssim"], ms["ms_ssim_per_channel"].mean(axis=1))
    for k in ws:
        assert np.all(np.abs(ms[k] - ws[k]) <= BOUND * (1 + np.abs(ws[k]))), k
    default = np.array([0.0448, 0.2856, 0.3001]) / (0.0448 + 0.2856 + 0.3001)
    explicit = P.sample_ssim(xd, yd, levels=3, weights=tuple(default))
    assert np.array_equal(explicit["ms_ssim"], ms["ms_ssim"])
    other = P.sample_ssim(xd, yd, levels=3, weights=(0.2, 0.3, 0.5))
    assert np.all(np.abs(other["ms_ssim"] - R.scores(want, (0.2, 0.3, 0.5))["ms_ssim"]) <= 2 * BOUND)
    assert not np.array_equal(other["ms_ssim"], ms["ms_ssim"])
    shared = P.sample_ssim(xd, yd[1].contiguous(), levels=3)
    assert np.array_equal(shared["ms_ssim"][1], ms["ms_ssim"][1]) and shared["ms_ssim"][0] != ms["ms_ssim"][0]
    # a data range: C1 and C2 scale with its square
    x8 = P.sample_ssim(xd * 4, yd * 4, data_range=8.0)
    assert np.abs(x8["ssim"] - one["ssim"]).max() <= 1e-6
    with pytest.raises(ValueError, match="at least 44"):
        P.sample_ssim(xd[:, :, :43].contiguous(), yd[:, :, :43].contiguous(), levels=3)
    with pytest.raises(ValueError, match="x.shape or x.shape"):
        P.sample_ssim(xd, yd[:1])


# ---------------------------------------------------------------------------------------------------------------- independence, determinism
def maps(x, y, levels, **kw):
    from phendiff_amd import diagnostics as D
    out = D.ssim_maps_means(x, y, levels=levels, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", list(DTYPES))
def test_a_sample_does_not_depend_on_its_batch_or_alignment(mode):
    for case in ((3, 5, 45, 67, 11, 1), (3, 3, 45, 51, 11, 3)):
        x, y = pair(case[:4], DTYPES[mode], seed=3)
        x, y = x.to(DEV), y.to(DEV)
        n = x[0].numel()
        assert n % 2 == 1                                           # row 1 of a 16-bit batch starts at 2-byte alignment, row 2 at 4-byte
        whole = maps(x, y, case[5])
        alone = maps(x[2:3].contiguous(), y[2:3].contiguous(), case[5])
        assert torch.equal(alone[0], whole[2]), case
        alone1 = maps(x[1:2].contiguous(), y[1:2].contiguous(), case[5])
        assert torch.equal(alone1[0], whole[1]), case
        # the same tensors one element further inside a larger allocation
        bx, by = torch.zeros(x.numel() + 8, dtype=x.dtype, device=DEV), torch.zeros(y.numel() + 8, dtype=y.dtype, device=DEV)
        ox, oy = bx[1:1 + x.numel()].view(x.shape), by[3:3 + y.numel()].view(y.shape)
        ox.copy_(x)
        oy.copy_(y)
        assert ox.data_ptr() == bx.data_ptr() + x.element_size() and ox.is_contiguous()
        assert torch.equal(maps(ox, oy, case[5]), whole), case
        # one shared y
        shared = maps(x, y[2].contiguous(), case[5])
        assert torch.equal(shared[2], whole[2]) and not torch.equal(shared[0], whole[0])
        assert not torch.isnan(whole).any()


def test_two_calls_and_a_side_stream_give_the_same_bits():
    x, y = pair((2, 2, 70, 133), torch.float32, seed=5)
    x, y = x.to(DEV), y.to(DEV)
    first = maps(x, y, 2)
    second = maps(x, y, 2)
    assert torch.equal(first, second)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    third = maps(x, y, 2, stream=side)
    assert torch.equal(first, third)


def test_graph_replay_equals_eager():
    from phendiff_amd import diagnostics as D
    x, y = pair((2, 3, 45, 51), torch.float32, seed=7)
    x, y = x.to(DEV), y[1].contiguous().to(DEV)      # (one y for all)
    eager = maps(x, y, 3)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = D.ssim_maps_means(x, y, levels=3)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(pair((2, 3, 45, 51), torch.float32, seed=9)[0])      # the captured launches read the buffers, not a snapshot
    g.replay()
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and not torch.equal(out, eager)
    assert torch.equal(out, maps(x, y, 3))


def test_offsets_past_2_to_31_elements():
    """2049 planes of 1024 x 1024 bf16: the last sample starts at element 2^31.  Its numbers equal, bit for bit, those of a call on it alone."""
    x = torch.randn(2049, 1, 1024, 1024, dtype=torch.bfloat16, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    y = (x[7] * 0.9).contiguous()
    whole = maps(x, y, 1)
    for b in (0, 7, 2048):
        assert torch.equal(maps(x[b:b + 1], y, 1)[0], whole[b]), b
    assert abs(float(whole[7, 0, 0, 0]) - 1.0) < 0.05 and abs(float(whole[2048, 0, 0, 0])) < 0.05 and torch.isfinite(whole).all()


# ---------------------------------------------------------------------------------------------------------------- guard bands
class Call:
    """One pd_ssim call through ctypes on caller-held buffers, every one of them inside guard bands."""

    def __init__(self, x, y, win=11, levels=1, guard=True, short_by=0):
        import phendiff_amd._lib as L
        from phendiff_amd import diagnostics as D
        self.L, self.guards = L, {}
        B, Cc, H, W = x.shape

        def place(t, name):
            if not guard:
                return t.to(DEV)
            view, h = guarded(t, device=DEV, name=name)
            self.guards[name] = h
            return view

        self.x, self.y = place(x, "x"), place(y, "y")
        self.ws_bytes = L.lib().pd_ssim_workspace(B, Cc, H, W, levels)
        assert self.ws_bytes > 0 and self.ws_bytes % 8 == 0
        self.out = place(torch.zeros(B, Cc, levels, 2, dtype=torch.float64), "out")
        self.ws = place(torch.zeros(self.ws_bytes // 8, dtype=torch.float64), "workspace")      # exactly what the query asks for
        dt = {torch.float32: L.PD_F32, torch.bfloat16: L.PD_BF16, torch.float16: L.PD_F16}[x.dtype]
        taps = {f"w{i}": float(g) for i, g in enumerate(D.gaussian_window(win, SIGMA[win]))}
        self.args = L.SsimArgs(dtype=dt, C=Cc, H=H, W=W, win=win, levels=levels, B=B, y_sample_stride=0 if y.dim() == 3 else Cc * H * W,
                               c1=0.02 ** 2, c2=0.06 ** 2, x=self.x.data_ptr(), y=self.y.data_ptr(), out=self.out.data_ptr(),
                               workspace=self.ws.data_ptr(), workspace_bytes=self.ws_bytes - short_by, **taps)

    def rc(self):
        return self.L.lib().pd_ssim(C.byref(self.args), torch.cuda.current_stream().cuda_stream)

    def launch(self):
        self.L.check(self.rc(), "pd_ssim")

    def scribble(self):
        self.out.fill_(-1.25e300)
        self.ws.fill_(-1.25e300)

    def output(self):
        torch.cuda.synchronize()
        return self.out.clone()


GUARD_CASES = [((3, 5, 45, 67), 11, 2), ((3, 1, 33, 41), 33, 1)]      # C * H * W odd; the last tile ragged in both axes


@pytest.mark.parametrize("mode", list(DTYPES))
def test_guard_bands(mode):
    for shape, win, levels in GUARD_CASES:
        x, y = pair(shape, DTYPES[mode], seed=10)
        assert x.numel() % 2 == 1
        for yy in (y, y[1].contiguous()):
            c = Call(x, yy, win, levels)
            for name in ("out", "workspace"):
                c.guards[name].canary()
            c.scribble()
            c.launch()
            clean = c.output()
            for name in ("out", "workspace"):
                assert c.guards[name].intact()
            assert not (clean == -1.25e300).any() and torch.isfinite(clean).all()      # every element of out was written
            want = R.maps_means(x, yy, levels=levels, win=win, sigma=SIGMA[win])
            assert np.abs(clean.cpu().numpy() - want).max() <= BOUND
            for name in ("x", "y"):      # P1: NaN all around the inputs: not one output bit moves
                c.guards[name].poison()
            c.scribble()
            c.launch()
            poisoned = c.output()
            assert torch.equal(clean, poisoned), (shape, win)
            for name in ("out", "workspace"):      # P2
                assert c.guards[name].intact()
            plain = Call(x, yy, win, levels, guard=False)      # and the guarded placement gives what the plain one gives
            plain.launch()
            assert torch.equal(clean, plain.output())
            # P3: a NaN in sample 1 of x is sample 1's alone
            c.x[1, 0, shape[2] // 2, shape[3] // 2] = float("nan")
            c.scribble()
            c.launch()
            bad = c.output()
            assert torch.equal(bad[0], clean[0]) and torch.equal(bad[2], clean[2])
            assert torch.isnan(bad[1, 0]).all() and torch.equal(bad[1, 1:], clean[1, 1:])
            for name in ("out", "workspace"):
                assert c.guards[name].intact()


def test_workspace_one_byte_short_is_refused():
    import phendiff_amd._lib as L
    x, y = pair((2, 3, 45, 51), torch.float32, seed=11)
    c = Call(x, y, 11, 3, short_by=1)
    c.guards["out"].canary()
    c.scribble()
    assert c.rc() == L.CONSTANTS["PD_ERR_ARG"] and b"workspace_bytes" in L.lib().pd_last_error()
    torch.cuda.synchronize()
    assert (c.out == -1.25e300).all() and c.guards["out"].intact()      # nothing was launched
    ok = Call(x, y, 11, 3)
    ok.launch()
    assert np.abs(ok.output().cpu().numpy() - R.maps_means(x, y, levels=3)).max() <= BOUND
