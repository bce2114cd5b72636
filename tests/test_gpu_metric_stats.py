"""pd_kid_mmd / pd_feature_moments and the device statistics of phendiff_amd.metrics on the MI355X, against float64 numpy.

Test data: fp32, non-negative features (pool3 features are averages of ReLU outputs), |randn| * U(0.2, 1.2) + U(0, 0.5) per column, so
mean / std per column stays below 10 and every KID sum is a sum of positive terms (no cancellation).  Bounds (worst-case rounding, not
measured from the kernels):
  KID      |d sums_k| <= 1e-11 sums_k and |d mmd| <= 1e-11 (mean kxx + mean kyy + 2 mean kxy): (m^2 + 3 D) 2^-53 ~ 5e-12 for m <= 200,
           D <= 2048 on either side
  moments  |d mean_i| <= 1e-12 (|mean_i| + sd_i), |d cov_ij| <= 1e-12 sqrt(v_i v_j): N 2^-53 (1 + mean / sd) < 1e-12 for these N
  FID      sqrtm's conditioning cannot be derived: calibrated on the host alone -- d_host = |FID from np.cov - FID from a covariance summed
           in blocks of 16 rows in numpy|, and |FID_dev - FID_host| <= max(100 d_host, 1e-12 FID_host)
Every test prints the figures it asserts on."""
import ctypes as C

import numpy as np
import pytest
import torch

from guard_bands import MIN_GUARD_BYTES
from test_gpu_guard_bands import Case, Op, out_op, p1_poisoned_surroundings, p2_canaried_outputs
from test_gpu_kernels import env, stream  # noqa: F401

pytestmark = pytest.mark.gpu
POISON_INDEX = 0x7FFFFFFF


def features(n, d, seed, dead=None):
    rng = np.random.default_rng(seed)
    f = np.abs(rng.standard_normal((n, d))) * rng.uniform(0.2, 1.2, d) + rng.uniform(0.0, 0.5, d)
    if dead is not None:
        f[:, dead] = 0.0
    return f.astype(np.float32)


def tables(n1, n2, S, m, seed, avoid=None):
    """[S][m] rows without replacement; `avoid` = (row of f1, row of f2) no subset may select."""
    rng = np.random.default_rng(seed)

    def draw(n, skip):
        pool = np.array([i for i in range(n) if i != skip])
        return np.stack([rng.permutation(pool)[:m] for _ in range(S)]).astype(np.int32)
    return draw(n1, None if avoid is None else avoid[0]), draw(n2, None if avoid is None else avoid[1])


def kid_numpy(f1, f2, i1, i2, degree, gamma, coef0):
    """The formula of oracle.inception_ref._mmd2_ref / kid_ref on given index tables: (sums [S][3], mmd [S], scale [S])."""
    f1, f2 = f1.astype(np.float64), f2.astype(np.float64)
    gam = gamma if gamma is not None else 1.0 / f1.shape[1]
    S, m = i1.shape
    sums, mmd = np.zeros((S, 3)), np.zeros(S)
    for s in range(S):
        a, b = f1[i1[s]], f2[i2[s]]
        k = lambda X, Y: (X @ Y.T * gam + coef0) ** degree      # noqa: E731
        kxx, kxy, kyy = k(a, a), k(a, b), k(b, b)
        sums[s] = ((kxx.sum(axis=1) - np.diagonal(kxx)).sum(), (kyy.sum(axis=1) - np.diagonal(kyy)).sum(), kxy.sum())
        mmd[s] = (sums[s, 0] + sums[s, 1]) / (m * (m - 1)) - 2 * sums[s, 2] / (m * m)
    scale = (sums[:, 0] + sums[:, 1]) / (m * (m - 1)) + 2 * sums[:, 2] / (m * m)
    return sums, mmd, scale


def kid_raw(env_, F1, F2, I1, I2, m, degree=3, gamma=None, coef0=1, sums=None, mmd=None, ws=None):
    """One pd_kid_mmd call through ctypes on caller-held device buffers (rows of F / I may be strided views); outputs pre-filled with NaN."""
    L, lib, _, dev = env_
    S, D = I1.shape[0], F1.shape[1]
    sums = torch.full((S, 3), float("nan"), dtype=torch.float64, device=dev) if sums is None else sums
    mmd = torch.full((S,), float("nan"), dtype=torch.float64, device=dev) if mmd is None else mmd
    ws_bytes = lib.pd_kid_mmd_workspace(S, m)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device=dev) if ws is None else ws
    assert I1.stride(1) == 1 and I2.stride(1) == 1 and I1.stride(0) == I2.stride(0) and ws.numel() * 8 >= ws_bytes
    a = L.KidMmdArgs(D=D, S=S, m=m, degree=degree, N1=F1.shape[0], N2=F2.shape[0], f1_stride=F1.stride(0), f2_stride=F2.stride(0),
                     idx_stride=I1.stride(0), gamma=float(gamma if gamma is not None else 1.0 / D), coef0=float(coef0), f1=F1.data_ptr(),
                     f2=F2.data_ptr(), idx1=I1.data_ptr(), idx2=I2.data_ptr(), sums=sums.data_ptr(), mmd=mmd.data_ptr(), workspace=ws.data_ptr(),
                     workspace_bytes=ws_bytes)
    L.check(lib.pd_kid_mmd(C.byref(a), stream()), "pd_kid_mmd")
    return sums, mmd


def check_kid(what, sums, mmd, ref):
    want_sums, want_mmd, scale = ref
    e_s = float((np.abs(sums - want_sums) / want_sums).max())
    e_m = float((np.abs(mmd - want_mmd) / scale).max())
    print(f"pd_kid_mmd {what}: max |d sums| / sums = {e_s:.3e}, max |d mmd| / scale = {e_m:.3e} (bounds 1e-11)")
    assert np.isfinite(sums).all() and np.isfinite(mmd).all()
    assert (np.abs(sums - want_sums) <= 1e-11 * want_sums).all(), e_s
    assert (np.abs(mmd - want_mmd) <= 1e-11 * scale).all(), e_m


KID_CASES = [  # N1, N2, m, D, S, degree, gamma, coef0
    (150, 131, 77, 64, 3, 3, None, 1),        # a ragged tile
    (260, 300, 130, 192, 3, 3, None, 1),      # several tiles, ragged
    (210, 220, 200, 2048, 2, 3, None, 1),     # the real width
    (70, 70, 64, 64, 1, 3, None, 1),          # one exact tile; the subset is a permutation of almost all rows
    (40, 33, 2, 64, 4, 3, None, 1),           # minimum m
    (90, 90, 65, 128, 2, 1, 0.5, 0),          # degree 1
    (90, 90, 65, 128, 2, 2, 0.01, 2),         # degree 2
]


@pytest.mark.parametrize("cfg", KID_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_kid_mmd_parity(env, cfg):
    n1, n2, m, D, S, degree, gamma, coef0 = cfg
    dev = env[3]
    f1, f2 = features(n1, D, 11), features(n2, D, 12) + np.float32(0.05)
    i1, i2 = tables(n1, n2, S, m, 13)
    sums, mmd = kid_raw(env, torch.from_numpy(f1).to(dev), torch.from_numpy(f2).to(dev), torch.from_numpy(i1).to(dev), torch.from_numpy(i2).to(dev),
                        m, degree, gamma, coef0)
    check_kid(str(cfg), sums.cpu().numpy(), mmd.cpu().numpy(), kid_numpy(f1, f2, i1, i2, degree, gamma, coef0))


def test_kid_end_to_end_against_the_oracle(env):
    import phendiff_amd.metrics as M
    from oracle import kid_ref
    dev = env[3]
    f1, f2 = features(300, 64, 21), features(260, 64, 22) + np.float32(0.05)
    got = M.kernel_inception_distance_device(torch.from_numpy(f1).to(dev), torch.from_numpy(f2).to(dev), kid_subsets=5, kid_subset_size=50)
    want = kid_ref(f1, f2, kid_subsets=5, kid_subset_size=50)
    i1, i2 = M.kid_subset_indices(300, 260, 5, 50)
    scale = float(kid_numpy(f1, f2, i1, i2, 3, None, 1)[2].min())
    d_mean = abs(got[M.KEY_KID_MEAN] - want["kernel_inception_distance_mean"])
    d_std = abs(got[M.KEY_KID_STD] - want["kernel_inception_distance_std"])
    print(f"KID end to end: mean {got[M.KEY_KID_MEAN]:.17g} vs {want['kernel_inception_distance_mean']:.17g}: |d| / scale = {d_mean / scale:.3e}; "
          f"std |d| / scale = {d_std / scale:.3e} (bounds 1e-11)")
    assert set(got) == set(want)
    assert d_mean <= 1e-11 * scale and d_std <= 1e-11 * scale
    with pytest.raises(ValueError):
        M.kernel_inception_distance_device(torch.from_numpy(f1).to(dev), torch.from_numpy(f2).to(dev), kid_subsets=2, kid_subset_size=261)


def test_kid_is_deterministic_and_subsets_are_independent(env):
    dev = env[3]
    F1, F2 = torch.from_numpy(features(150, 64, 31)).to(dev), torch.from_numpy(features(131, 64, 32)).to(dev)
    i1, i2 = tables(150, 131, 3, 77, 33)
    I1, I2 = torch.from_numpy(i1).to(dev), torch.from_numpy(i2).to(dev)
    s_a, m_a = kid_raw(env, F1, F2, I1, I2, 77)
    s_b, m_b = kid_raw(env, F1, F2, I1, I2, 77)
    assert torch.equal(s_a, s_b) and torch.equal(m_a, m_b) and bool(torch.isfinite(m_a).all())
    for s in range(3):
        s_1, m_1 = kid_raw(env, F1, F2, I1[s:s + 1].contiguous(), I2[s:s + 1].contiguous(), 77)
        assert torch.equal(s_1[0], s_a[s]) and torch.equal(m_1[0], m_a[s]), s


def test_kid_nan_isolation(env):
    dev = env[3]
    n1, n2, S, m = 150, 131, 3, 77
    f1, f2 = features(n1, 64, 41), features(n2, 64, 42)
    # (1) a NaN row that no subset selects changes no output bit
    i1, i2 = tables(n1, n2, S, m, 43, avoid=(17, 130))
    I1, I2 = torch.from_numpy(i1).to(dev), torch.from_numpy(i2).to(dev)
    F1, F2 = torch.from_numpy(f1).to(dev), torch.from_numpy(f2).to(dev)
    base = kid_raw(env, F1, F2, I1, I2, m)
    G1, G2 = F1.clone(), F2.clone()
    G1[17], G2[130] = float("nan"), float("nan")
    got = kid_raw(env, G1, G2, I1, I2, m)
    assert bool(torch.isfinite(base[1]).all()) and torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    # (2) a NaN row selected by subset 0 alone leaves the other subsets' bits alone
    j1 = i1.copy()
    j1[0, 5] = 17
    J1 = torch.from_numpy(j1).to(dev)
    clean = kid_raw(env, F1, F2, J1, I2, m)
    got = kid_raw(env, G1, F2, J1, I2, m)
    assert bool(torch.isnan(got[1][0])) and bool(torch.isnan(got[0][0, 0])) and bool(torch.isnan(got[0][0, 2]))
    assert torch.equal(got[0][0, 1], clean[0][0, 1])      # (YY of subset 0 does not touch f1)
    assert torch.equal(got[0][1:], clean[0][1:]) and torch.equal(got[1][1:], clean[1][1:])
    # (3) table rows at a pitch above m, poison indices in between: never read
    pitch = m + 19
    P1 = torch.full((S, pitch), POISON_INDEX, dtype=torch.int32, device=dev)
    P2 = torch.full((S, pitch), POISON_INDEX, dtype=torch.int32, device=dev)
    P1[:, :m], P2[:, :m] = I1, I2
    got = kid_raw(env, F1, F2, P1[:, :m], P2[:, :m], m)
    torch.cuda.synchronize()
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


# ---------------------------------------------------------------------------------------------------------------- moments
def moments_raw(env_, F, cov_stride=None, mean=None, cov=None, ws=None):
    L, lib, _, dev = env_
    N, D = F.shape
    cs = cov_stride or D
    mean = torch.full((D,), float("nan"), dtype=torch.float64, device=dev) if mean is None else mean
    cov = torch.full((D, cs), float("nan"), dtype=torch.float64, device=dev)[:, :D] if cov is None else cov
    ws_bytes = lib.pd_feature_moments_workspace(N, D)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device=dev) if ws is None else ws
    a = L.FeatureMomentsArgs(D=D, N=N, f_stride=F.stride(0), cov_stride=cov.stride(0), f=F.data_ptr(), mean=mean.data_ptr(), cov=cov.data_ptr(),
                             workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
    L.check(lib.pd_feature_moments(C.byref(a), stream()), "pd_feature_moments")
    return mean, cov


def check_moments(what, f, mean, cov, dead=None):
    f64 = f.astype(np.float64)
    want_mean, want_cov = np.mean(f64, axis=0), np.cov(f64, rowvar=False)
    v = np.diagonal(want_cov)
    sd = np.sqrt(v)
    live = sd > 0
    e_m = float((np.abs(mean - want_mean)[live] / (np.abs(want_mean) + sd)[live]).max())
    e_c = float((np.abs(cov - want_cov)[np.ix_(live, live)] / np.sqrt(np.outer(v, v))[np.ix_(live, live)]).max())
    print(f"pd_feature_moments {what}: max |d mean| / (|mean| + sd) = {e_m:.3e}, max |d cov| / sqrt(v_i v_j) = {e_c:.3e} (bounds 1e-12)")
    assert np.isfinite(mean).all() and np.isfinite(cov).all()      # (every element written: the buffers were NaN)
    assert (np.abs(mean - want_mean) <= 1e-12 * (np.abs(want_mean) + sd)).all(), e_m
    assert (np.abs(cov - want_cov) <= 1e-12 * np.sqrt(np.outer(v, v))).all(), e_c
    if dead is not None:
        assert mean[dead] == 0.0 and not cov[dead].any() and not cov[:, dead].any()


MOMENT_CASES = [(300, 64), (515, 192), (48, 2048), (2, 64), (129, 128)]


@pytest.mark.parametrize("N,D", MOMENT_CASES)
def test_feature_moments_parity(env, N, D):
    dev, dead = env[3], D // 2 + 3
    f = features(N, D, 51, dead=dead)
    F = torch.from_numpy(f).to(dev)
    mean, cov = moments_raw(env, F)
    mean2, cov2 = moments_raw(env, F)
    assert torch.equal(cov, cov.T) and torch.equal(mean, mean2) and torch.equal(cov, cov2)
    check_moments(f"({N}, {D})", f, mean.cpu().numpy(), cov.cpu().numpy(), dead)
    import phendiff_amd.metrics as M
    mu, sigma = M.fid_statistics_device(F)
    assert mu.dtype == sigma.dtype == torch.float64 and mu.is_cuda and torch.equal(mu, mean) and torch.equal(sigma, cov)


def blocked_statistics(f, rows=16):
    """float64 mean and covariance with the contraction over the rows summed in blocks (another order of the same sums)."""
    f = f.astype(np.float64)
    mu = f.sum(axis=0) / len(f)
    xc = f - mu
    c = np.zeros((f.shape[1], f.shape[1]))
    for i in range(0, len(f), rows):
        c += xc[i:i + rows].T @ xc[i:i + rows]
    return mu, c / (len(f) - 1)


def check_fid(what, fa, fb, got):
    """fa / fb: host fp32 features; got: the FID computed from the device statistics."""
    import phendiff_amd.metrics as M
    host = M.fid_from_statistics(*M.fid_statistics(fa), *M.fid_statistics(fb))
    blocked = M.fid_from_statistics(*blocked_statistics(fa), *blocked_statistics(fb))
    d_host, bound = abs(host - blocked), max(100 * abs(host - blocked), 1e-12 * abs(host))
    print(f"FID {what}: device {got:.17g}, host {host:.17g}: |d| = {abs(got - host):.3e}; host re-ordering d_host = {d_host:.3e}, bound {bound:.3e}")
    assert np.isfinite(got) and abs(got - host) <= bound


@pytest.mark.parametrize("Na,Nb,D", [(300, 307, 64), (48, 55, 2048)])
def test_fid_scalar_from_device_statistics(env, Na, Nb, D):
    import phendiff_amd.metrics as M
    dev = env[3]
    fa, fb = features(Na, D, 61), features(Nb, D, 62) * np.float32(1.1) + np.float32(0.05)
    stats = [t.cpu().numpy() for f in (fa, fb) for t in M.fid_statistics_device(torch.from_numpy(f).to(dev))]
    check_fid(f"({Na}, {D}) vs ({Nb}, {D})", fa, fb, M.fid_from_statistics(*stats))


# ---------------------------------------------------------------------------------------------------------------- guard bands
# Feature rows are 64 elements wider than D (NaN in P1), cov rows 64 elements wider than D (canary in P2), the index tables' rows 19
# entries wider than m (all-ones in P1); guards of 64 KiB (two 64-row tiles of these rows stay below it) around every operand.
PAD = 64


def kid_guard_case(env_):
    n1, n2, m, D, S = 150, 131, 77, 64, 2
    f1, f2 = features(n1, D, 71), features(n2, D, 72)
    i1, i2 = tables(n1, n2, S, m, 73)
    ref = kid_numpy(f1, f2, i1, i2, 3, None, 1)
    ws = env_[1].pd_kid_mmd_workspace(S, m) // 8
    ins = {"f1": Op(torch.from_numpy(f1), stride=D + PAD), "f2": Op(torch.from_numpy(f2), stride=D + PAD),
           "idx1": Op(torch.from_numpy(i1), stride=m + 19), "idx2": Op(torch.from_numpy(i2), stride=m + 19)}
    outs = {"sums": out_op((S, 3), torch.float64), "mmd": out_op((S,), torch.float64), "ws": out_op((ws,), torch.float64, whole=False)}

    def launch(T):
        assert T["f1"].stride(0) == D + PAD and T["idx1"].stride(0) == m + 19
        kid_raw(env_, T["f1"], T["f2"], T["idx1"], T["idx2"], m, sums=T["sums"], mmd=T["mmd"], ws=T["ws"])

    return Case(ins, outs, launch, lambda O: check_kid("guarded", O["sums"].numpy(), O["mmd"].numpy(), ref))


def moments_guard_case(env_):
    N, D = 129, 128
    f = features(N, D, 74, dead=5)
    ws = env_[1].pd_feature_moments_workspace(N, D) // 8
    ins = {"f": Op(torch.from_numpy(f), stride=D + PAD)}
    outs = {"mean": out_op((D,), torch.float64), "cov": out_op((D, D), torch.float64, stride=D + PAD),
            "ws": out_op((ws,), torch.float64, whole=False)}

    def launch(T):
        assert T["f"].stride(0) == D + PAD and T["cov"].stride(0) == D + PAD
        moments_raw(env_, T["f"], mean=T["mean"], cov=T["cov"], ws=T["ws"])

    return Case(ins, outs, launch, lambda O: check_moments("guarded", f, O["mean"].numpy(), O["cov"].numpy(), 5))


GUARD_CASES = {"pd_kid_mmd": kid_guard_case, "pd_feature_moments": moments_guard_case}
assert MIN_GUARD_BYTES >= 64 * 1024


@pytest.mark.parametrize("entry", sorted(GUARD_CASES))
def test_p1_poisoned_surroundings(env, monkeypatch, entry):
    p1_poisoned_surroundings(GUARD_CASES[entry](env), env[3], monkeypatch)


@pytest.mark.parametrize("entry", sorted(GUARD_CASES))
def test_p2_canaried_outputs(env, monkeypatch, entry):
    p2_canaried_outputs(GUARD_CASES[entry](env), env[3], monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- the product path
def test_calculate_metrics_with_device_statistics(env):
    """48 + 48 synthetic images through the f32 InceptionV3 (random-init: structure): calculate_metrics(device_statistics=True) against the
    host functions applied to the same device features copied to the host."""
    import phendiff_amd.metrics as M
    from test_gpu_metrics import _oracle_side
    o = _oracle_side()
    net = M.InceptionV3Features("f32")
    net.load_state_dict(o["ref"].state_dict())
    net = net.to("cuda:0")
    gen, real = o["gen"], o["real"]
    got = M.calculate_metrics(net, gen, real, isc=True, fid=True, kid=True, kid_subset_size=24, batch_size=48, device_statistics=True)
    assert set(got) == {M.KEY_ISC_MEAN, M.KEY_ISC_STD, M.KEY_FID, M.KEY_KID_MEAN, M.KEY_KID_STD}
    d1, d2 = M.extract_features_device(net, gen, 48), M.extract_features_device(net, torch.from_numpy(real).to("cuda:0"), 48)
    assert all(v.is_cuda and v.dtype == torch.float32 for v in d1.values()) and d1["2048"].shape == (48, 2048)
    h1, h2 = d1["2048"].cpu().numpy(), d2["2048"].cpu().numpy()
    isc = M.inception_score(d1["logits_unbiased"].double().cpu().numpy())
    assert got[M.KEY_ISC_MEAN] == isc[M.KEY_ISC_MEAN] and got[M.KEY_ISC_STD] == isc[M.KEY_ISC_STD]
    kid = M.kernel_inception_distance(h1, h2, kid_subset_size=24)
    i1, i2 = M.kid_subset_indices(48, 48, 100, 24)
    scale = float(kid_numpy(h1, h2, i1, i2, 3, None, 1)[2].min())
    d_kid = abs(got[M.KEY_KID_MEAN] - kid[M.KEY_KID_MEAN])
    print(f"product path KID mean {got[M.KEY_KID_MEAN]:.17g} vs host {kid[M.KEY_KID_MEAN]:.17g}: |d| / scale = {d_kid / scale:.3e} (bound 1e-11)")
    assert d_kid <= 1e-11 * scale
    check_fid("product path", h1, h2, got[M.KEY_FID])
    # cached real-image features may be device tensors
    again = M.calculate_metrics(net, gen, isc=False, fid=False, kid=True, kid_subset_size=24, batch_size=48, input2_features=d2,
                                device_statistics=True)
    assert again[M.KEY_KID_MEAN] == got[M.KEY_KID_MEAN] and again[M.KEY_KID_STD] == got[M.KEY_KID_STD]


def test_class_metrics_hook_with_device_statistics():
    import phendiff_amd as P
    import phendiff_amd.metrics as M
    from oracle import InceptionV3FeaturesRef, randomize_inception_
    from phendiff_amd.eval_generation import generate_samples
    from test_gpu_metrics import _synthetic_sets
    net = M.InceptionV3Features("bf16")
    net.load_state_dict(randomize_inception_(InceptionV3FeaturesRef(), seed=4).state_dict())
    net = net.to("cuda:0")
    torch.manual_seed(0)
    unet = P.CustomCondUNet2DModel(compute_dtype="bf16", **dict(P.UNET_CONFIGS["super_small"], sample_size=32)).to("cuda:0")
    pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
    real0, real1 = _synthetic_sets(12, 32, 9)
    results = {}
    hook = M.class_metrics_hook(net, {0: real0, 1: real1}, results, isc=True, fid=True, kid=True, kid_subset_size=6, batch_size=16,
                                device_statistics=True)
    generate_samples(pipe, nb_classes=2, nb_generated_images=12, eval_batch_size=8, num_inference_steps=2, class_names=["a", "b"], on_class_done=hook)
    assert set(results) == {f"{m}/{c}" for c in "ab" for m in (M.KEY_ISC_MEAN, M.KEY_ISC_STD, M.KEY_FID, M.KEY_KID_MEAN, M.KEY_KID_STD)}
    assert all(np.isfinite(v) for v in results.values()) and results[f"{M.KEY_FID}/a"] > 0
