"""pd_knn_radii / pd_manifold_query and precision / recall / density / coverage of phendiff_amd.metrics on the MI355X, against the float64
numpy reference of prdc_ref.py (squared distances by direct differences -- another formula than the kernels' Gram form).

Bounds (derived in prdc_ref, not measured): |d rad2|, |d dmin2| <= 1e-11 (|a|^2 + |b|^2) of the pair behind the value; every fixture's
margin (the smallest |d2 - rad2| / (|a|^2 + |b|^2) over the comparisons made) is asserted above 1e-9 on the reference itself, so every <=
decision is unambiguous and counts and the five metrics must be EXACT.  Everything else is bitwise: torch.equal.
Every test prints the figures it asserts on."""
import ctypes as C

import numpy as np
import pytest
import torch

import prdc_ref as R
from guard_bands import MIN_GUARD_BYTES
from test_gpu_guard_bands import Case, Op, out_op, p1_poisoned_surroundings, p2_canaried_outputs
from test_gpu_kernels import env, stream  # noqa: F401

pytestmark = pytest.mark.gpu
INT_PATTERN = -1234567


def real_rows(n, d):
    return R.cloud(n, d, 21, axis=1, part=0.4)


def gen_rows(n, d):
    return R.cloud(n, d, 22, axis=0, part=0.5)


def strided(f, stride, dev):
    """The rows of f at a pitch of `stride` elements, NaN in between."""
    buf = torch.full((f.shape[0], stride), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :f.shape[1]] = torch.from_numpy(np.ascontiguousarray(f)).to(dev)
    return buf[:, :f.shape[1]]


def radii_raw(env_, F, k, splits=0, rad2=None, ws=None):
    """One pd_knn_radii call through ctypes on caller-held device buffers; output and workspace pre-filled with NaN."""
    L, lib, _, dev = env_
    N, D = F.shape
    rad2 = torch.full((N,), float("nan"), dtype=torch.float64, device=dev) if rad2 is None else rad2
    ws_bytes = lib.pd_knn_radii_workspace(N, k, splits)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device=dev) if ws is None else ws
    assert ws.numel() * 8 >= ws_bytes
    a = L.KnnRadiiArgs(D=D, k=k, splits=splits, N=N, f_stride=F.stride(0), f=F.data_ptr(), rad2=rad2.data_ptr(), workspace=ws.data_ptr(),
                       workspace_bytes=ws_bytes)
    L.check(lib.pd_knn_radii(C.byref(a), stream()), "pd_knn_radii")
    return rad2


def query_raw(env_, Q, Rf, rad2=None, want_count=True, want_dmin2=True, splits=0, count=None, dmin2=None, ws=None):
    """One pd_manifold_query call; count pre-filled with a pattern, dmin2 and the workspace with NaN."""
    L, lib, _, dev = env_
    (Nq, D), Nr = Q.shape, Rf.shape[0]
    if want_count and count is None:
        count = torch.full((Nq,), INT_PATTERN, dtype=torch.int32, device=dev)
    if want_dmin2 and dmin2 is None:
        dmin2 = torch.full((Nq,), float("nan"), dtype=torch.float64, device=dev)
    ws_bytes = lib.pd_manifold_query_workspace(Nq, Nr, splits)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device=dev) if ws is None else ws
    assert ws.numel() * 8 >= ws_bytes
    a = L.ManifoldQueryArgs(D=D, splits=splits, Nq=Nq, Nr=Nr, q_stride=Q.stride(0), r_stride=Rf.stride(0), q=Q.data_ptr(), r=Rf.data_ptr(),
                            rad2=L.ptr(rad2), count=L.ptr(count), dmin2=L.ptr(dmin2), workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
    L.check(lib.pd_manifold_query(C.byref(a), stream()), "pd_manifold_query")
    return count, dmin2


def dev_f32(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)      # (a copy: the shared fixtures are read-only)


def check_radii(what, f, k, rad2):
    want, scale = R.radii(f, k), R.radii_scale(f, k)
    err = float((np.abs(rad2 - want) / scale).max())
    print(f"pd_knn_radii {what}: max |d rad2| / (|a|^2 + |b|^2) = {err:.3e} (bound {R.TOL:g})")
    assert np.isfinite(rad2).all()      # (every element written: the buffer was NaN)
    assert (np.abs(rad2 - want) <= R.TOL * scale).all(), err


def query_margin(q, r, rad2):
    d = R.d2(q, r)
    return float((np.abs(d - rad2[None, :]) / (R.norms(q)[:, None] + R.norms(r)[None, :])).min())


def check_query(what, q, r, rad2, count, dmin2):
    """rad2: the float64 radii the kernel was given (None: no counts)."""
    want_count, want_min = R.query(q, r, rad2)
    if dmin2 is not None:
        err = float((np.abs(dmin2 - want_min) / R.query_scale(q, r)).max())
        print(f"pd_manifold_query {what}: max |d dmin2| / (|a|^2 + |b|^2) = {err:.3e} (bound {R.TOL:g})")
        assert np.isfinite(dmin2).all() and (np.abs(dmin2 - want_min) <= R.TOL * R.query_scale(q, r)).all(), err
    if count is not None:
        margin = query_margin(q, r, rad2)
        print(f"pd_manifold_query {what}: margin of the fixture {margin:.2e} (must exceed {R.MIN_MARGIN:g}); counts exact")
        assert margin > R.MIN_MARGIN
        assert np.array_equal(count, want_count), int((count != want_count).sum())


# ---------------------------------------------------------------------------------------------------------------- parity
RADII_CASES = [  # N, D, k, stride
    (70, 64, 3, None),        # a ragged tile
    (64, 64, 1, None),        # one exact tile
    (130, 192, 5, None),      # several ragged tiles
    (200, 2048, 3, None),     # the real width
    (4, 64, 3, None),         # k + 1 = N
    (17, 64, 16, None),       # the largest k
    (130, 64, 5, 64 + 36),    # f_stride > D
]


@pytest.mark.parametrize("cfg", RADII_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_knn_radii_parity(env, cfg):
    N, D, k, stride = cfg
    dev = env[3]
    f = real_rows(N, D)
    F = strided(f, stride, dev) if stride else dev_f32(f, dev)
    assert F.stride(0) == (stride or D)
    check_radii(str(cfg), f, k, radii_raw(env, F, k).cpu().numpy())


QUERY_CASES = [  # Nq, Nr, D, k of the radii, count, dmin2, strides (q, r)
    (77, 150, 64, 3, True, True, None),
    (130, 260, 192, 5, True, True, None),
    (200, 210, 2048, 3, True, True, None),
    (1, 5, 64, 3, True, True, None),
    (77, 150, 64, 3, True, False, None),          # count only
    (77, 150, 64, 3, False, True, None),          # dmin2 only (no radii)
    (130, 260, 192, 5, True, True, (192 + 4, 192 + 64)),
]


@pytest.mark.parametrize("cfg", QUERY_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_manifold_query_parity(env, cfg):
    Nq, Nr, D, k, want_count, want_dmin2, strides = cfg
    dev = env[3]
    q, r = gen_rows(Nq, D), real_rows(Nr, D)
    rad2 = R.radii(r, k) if want_count else None
    Q = strided(q, strides[0], dev) if strides else dev_f32(q, dev)
    Rf = strided(r, strides[1], dev) if strides else dev_f32(r, dev)
    count, dmin2 = query_raw(env, Q, Rf, None if rad2 is None else torch.from_numpy(rad2).to(dev), want_count, want_dmin2)
    assert (count is None) == (not want_count) and (dmin2 is None) == (not want_dmin2)
    check_query(str(cfg), q, r, rad2, None if count is None else count.cpu().numpy(), None if dmin2 is None else dmin2.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- bitwise properties
def test_outputs_are_bitwise_independent_of_calls_splits_order_and_batch(env):
    dev = env[3]
    q, r = gen_rows(130, 192), real_rows(260, 192)
    Q, Rf = dev_f32(q, dev), dev_f32(r, dev)
    rad2 = radii_raw(env, Rf, 5)
    assert torch.equal(rad2, radii_raw(env, Rf, 5)) and bool(torch.isfinite(rad2).all())
    count, dmin2 = query_raw(env, Q, Rf, rad2)
    again = query_raw(env, Q, Rf, rad2)
    assert torch.equal(count, again[0]) and torch.equal(dmin2, again[1])
    for splits in (1, 2, 3, 5, 64):      # (260 rows are 5 column tiles: 64 splits leave most of them empty)
        assert torch.equal(radii_raw(env, Rf, 5, splits), rad2), splits
        c, m = query_raw(env, Q, Rf, rad2, splits=splits)
        assert torch.equal(c, count) and torch.equal(m, dmin2), splits
    perm = torch.from_numpy(np.random.default_rng(3).permutation(260)).to(dev)
    assert torch.equal(radii_raw(env, Rf[perm].contiguous(), 5), rad2[perm])
    c, m = query_raw(env, Q, Rf[perm].contiguous(), rad2[perm].contiguous())
    assert torch.equal(c, count) and torch.equal(m, dmin2)
    rows = torch.tensor([129, 3, 64, 65, 0, 77], device=dev)
    c, m = query_raw(env, Q[rows].contiguous(), Rf, rad2)
    assert torch.equal(c, count[rows]) and torch.equal(m, dmin2[rows])
    for k in (1, 3, 16):                 # the three list lengths of the selection agree with one another through the reference
        check_radii(f"k = {k}", r, k, radii_raw(env, Rf, k).cpu().numpy())


def test_equal_rows_are_at_distance_exactly_zero(env):
    dev = env[3]
    f = real_rows(70, 64)
    F = dev_f32(np.concatenate([f, f[::-1]]), dev)      # every row appears twice, at unrelated positions of two tiles
    rad2 = radii_raw(env, F, 1)
    assert torch.equal(rad2, torch.zeros_like(rad2))
    count, dmin2 = query_raw(env, F, F, rad2)
    assert bool((count >= 2).all()) and torch.equal(dmin2, torch.zeros_like(dmin2))


def test_nan_isolation(env):
    dev = env[3]
    q, r = gen_rows(77, 64), real_rows(150, 64)
    Q, Rf = dev_f32(q, dev), dev_f32(r, dev)
    rad2 = radii_raw(env, Rf, 3)
    count, dmin2 = query_raw(env, Q, Rf, rad2)
    j = int(torch.nonzero(count > 0)[-1])      # a row that has neighbours to lose
    # (1) a NaN in one query row changes that row's outputs alone
    Qn = Q.clone()
    Qn[j, 13] = float("nan")
    c, m = query_raw(env, Qn, Rf, rad2)
    keep = torch.arange(77, device=dev) != j
    assert torch.equal(c[keep], count[keep]) and torch.equal(m[keep], dmin2[keep])
    assert int(c[j]) == 0 and float(m[j]) == float("inf")
    # (2) a NaN reference row: every count and dmin2 as without that row; no radius gets smaller (none changes), its own is +inf
    Rn = Rf.clone()
    Rn[64, 5] = float("nan")
    others = torch.arange(150, device=dev) != 64
    without = Rf[others].contiguous()
    rad2_n, rad2_w = radii_raw(env, Rn, 3), radii_raw(env, without, 3)
    assert torch.equal(rad2_n[others], rad2_w) and float(rad2_n[64]) == float("inf") and bool((rad2_n[others] >= rad2[others]).all())
    c, m = query_raw(env, Q, Rn, rad2_n)
    c_w, m_w = query_raw(env, Q, without, rad2_w)
    assert torch.equal(c, c_w) and torch.equal(m, m_w) and bool(torch.isfinite(m).all())


# ---------------------------------------------------------------------------------------------------------------- guard bands
# Feature rows are 64 elements wider than D (NaN in P1); guards of 64 KiB (two 64-row tiles of these rows stay below it) around every operand.
PAD = 64


def radii_guard_case(env_):
    N, D, k = 130, 64, 5
    f = real_rows(N, D)
    ws = env_[1].pd_knn_radii_workspace(N, k, 0) // 8
    ins = {"f": Op(torch.from_numpy(f), stride=D + PAD)}
    outs = {"rad2": out_op((N,), torch.float64),
            "ws": out_op((ws,), torch.float64, whole=False)}      # (a split with fewer than k + 1 columns leaves +inf candidates: by design)

    def launch(T):
        assert T["f"].stride(0) == D + PAD
        radii_raw(env_, T["f"], k, rad2=T["rad2"], ws=T["ws"])

    return Case(ins, outs, launch, lambda O: check_radii("guarded", f, k, O["rad2"].numpy()))


def query_guard_case(env_):
    Nq, Nr, D, k = 77, 150, 64, 3
    q, r = gen_rows(Nq, D), real_rows(Nr, D)
    rad2 = R.radii(r, k)
    ws = env_[1].pd_manifold_query_workspace(Nq, Nr, 0) // 8
    ins = {"q": Op(torch.from_numpy(q), stride=D + PAD), "r": Op(torch.from_numpy(r), stride=D + PAD), "rad2": Op(torch.from_numpy(rad2))}
    outs = {"count": Op(torch.full((Nq,), INT_PATTERN, dtype=torch.int32)), "dmin2": out_op((Nq,), torch.float64),
            "ws": out_op((ws,), torch.float64, whole=False)}      # (the counts' half of the workspace holds integers)

    def launch(T):
        assert T["q"].stride(0) == D + PAD and T["r"].stride(0) == D + PAD
        query_raw(env_, T["q"], T["r"], T["rad2"], count=T["count"], dmin2=T["dmin2"], ws=T["ws"])

    return Case(ins, outs, launch, lambda O: check_query("guarded", q, r, rad2, O["count"].numpy(), O["dmin2"].numpy()))


GUARD_CASES = {"pd_knn_radii": radii_guard_case, "pd_manifold_query": query_guard_case}
assert MIN_GUARD_BYTES >= 64 * 1024


@pytest.mark.parametrize("entry", sorted(GUARD_CASES))
def test_p1_poisoned_surroundings(env, monkeypatch, entry):
    p1_poisoned_surroundings(GUARD_CASES[entry](env), env[3], monkeypatch)


@pytest.mark.parametrize("entry", sorted(GUARD_CASES))
def test_p2_canaried_outputs(env, monkeypatch, entry):
    p2_canaried_outputs(GUARD_CASES[entry](env), env[3], monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("case", sorted(R.TABLE), ids=lambda c: "-".join(str(v) for v in c))
def test_the_five_metrics_equal_the_reference(env, case):
    import phendiff_amd.metrics as M
    dev = env[3]
    real, gen, _ = R.fixture(*case)
    ref = R.check_fixture(case)
    k = case[3]
    G, X = dev_f32(gen, dev), dev_f32(real, dev)
    got = dict(M.precision_recall_device(G, X, k), **M.density_coverage_device(G, X, k))
    print(f"device {case}: {got}")
    assert set(got) == {M.KEY_PRECISION, M.KEY_RECALL, M.KEY_F_SCORE, M.KEY_DENSITY, M.KEY_COVERAGE}
    for key, v in got.items():
        assert v == ref[key], (key, v, ref[key])
    rad2 = M.knn_radii_device(X, k)
    count, dmin2 = M.manifold_query_device(G, X, rad2)
    assert rad2.is_cuda and rad2.dtype == torch.float64 and count.dtype == torch.int32 and dmin2.dtype == torch.float64
    assert torch.equal(rad2, radii_raw(env, X, k)) and M.manifold_query_device(G, X)[0] is None
    check_radii(f"{case} through metrics", real, k, rad2.cpu().numpy())
    assert np.array_equal(count.cpu().numpy(), R.query(gen, real, R.radii(real, k))[0])


NEW_KEYS = ("precision", "recall", "f_score", "density", "coverage")


def _random_inception(seed, mode):
    import phendiff_amd.metrics as M
    from oracle import InceptionV3FeaturesRef, randomize_inception_
    net = M.InceptionV3Features(mode)
    net.load_state_dict(randomize_inception_(InceptionV3FeaturesRef(), seed=seed).state_dict())
    return net.to("cuda:0")


def test_calculate_metrics_with_precision_recall_density_coverage(env):
    """24 + 24 synthetic images through the f32 InceptionV3 (random-init: structure): the five new keys on the device path equal the device
    functions applied to the host path's features, and the host path's own numpy values (the margin of these features' decisions is
    asserted first, on the direct-difference reference, as for every fixture)."""
    import phendiff_amd.metrics as M
    from test_gpu_metrics import _synthetic_sets
    net = _random_inception(3, "f32")
    gen, real = _synthetic_sets(24, 32, 7)
    kw = dict(isc=False, fid=False, kid=False, batch_size=24, prc=True, prc_neighborhood=3, dc=True, dc_nearest_k=5)
    got = M.calculate_metrics(net, gen, real, device_statistics=True, **kw)
    assert set(got) == set(NEW_KEYS)
    assert all(np.isfinite(v) and v >= 0 for v in got.values()) and all(got[k] <= 1 for k in ("precision", "recall", "f_score", "coverage"))
    h1, h2 = M.extract_features(net, gen, 24)["2048"], M.extract_features(net, real, 24)["2048"]
    G, X = dev_f32(h1.astype(np.float32), env[3]), dev_f32(h2.astype(np.float32), env[3])
    assert np.array_equal(h1.astype(np.float32).astype(np.float64), h1)      # (fp32 features widened: the way back is exact)
    want = dict(M.precision_recall_device(G, X, 3), **M.density_coverage_device(G, X, 5))
    print(f"product path: {got}")
    assert got == want
    # cached real-image features, host arrays or device tensors; the other metrics beside the new ones
    d2_ = M.extract_features_device(net, real, 24)
    again = M.calculate_metrics(net, gen, device_statistics=True, input2_features=d2_, **dict(kw, kid=True, kid_subset_size=12))
    assert {k: again[k] for k in NEW_KEYS} == got and M.KEY_KID_MEAN in again
    host = M.calculate_metrics(net, gen, real, **kw)
    ref3, ref5 = R.prdc(h2, h1, 3), R.prdc(h2, h1, 5)
    print(f"product path: margins of the 24 + 24 features {ref3['margin']:.2e} (k = 3), {ref5['margin']:.2e} (k = 5); host path: {host}")
    assert ref3["margin"] > R.MIN_MARGIN and ref5["margin"] > R.MIN_MARGIN
    assert host == got == {**{k: ref3[k] for k in ("precision", "recall", "f_score")}, **{k: ref5[k] for k in ("density", "coverage")}}
    old = M.calculate_metrics(net, gen, real, isc=True, fid=False, kid=False, batch_size=24, device_statistics=True)
    assert set(old) == {M.KEY_ISC_MEAN, M.KEY_ISC_STD}


def test_class_metrics_hook_stores_them_per_class():
    import phendiff_amd as P
    import phendiff_amd.metrics as M
    from phendiff_amd.eval_generation import generate_samples
    from test_gpu_metrics import _synthetic_sets
    net = _random_inception(4, "bf16")
    torch.manual_seed(0)
    unet = P.CustomCondUNet2DModel(compute_dtype="bf16", **dict(P.UNET_CONFIGS["super_small"], sample_size=32)).to("cuda:0")
    pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
    real0, real1 = _synthetic_sets(12, 32, 9)
    results = {}
    hook = M.class_metrics_hook(net, {0: real0, 1: real1}, results, isc=False, fid=False, kid=False, batch_size=16, device_statistics=True,
                                prc=True, dc=True)
    generate_samples(pipe, nb_classes=2, nb_generated_images=12, eval_batch_size=8, num_inference_steps=2, class_names=["a", "b"], on_class_done=hook)
    assert set(results) == {f"{m}/{c}" for c in "ab" for m in NEW_KEYS}
    assert all(np.isfinite(v) and v >= 0 for v in results.values())
