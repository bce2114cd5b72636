"""Float64 numpy reference of precision / recall / density / coverage (helper of test_host_manifold.py / test_gpu_manifold.py).

Squared distances by DIRECT DIFFERENCES, ((a - b)^2).sum() -- on purpose another formula than the library's Gram form
|a|^2 + |b|^2 - 2 a.b.  Definitions (X real, Y generated):
    rad2_k(F)[i] = the (k + 1)-th smallest of row i of d2(F, F), the row's own entry included
    precision    = mean_j [ exists i: d2(y_j, x_i) <= rad2_k(X)[i] ]       recall   = mean_i [ exists j: d2(x_i, y_j) <= rad2_k(Y)[j] ]
    density      = sum_j #{ i: d2(y_j, x_i) <= rad2_k(X)[i] } / (k Ng)     coverage = mean_i [ min_j d2(x_i, y_j) <= rad2_k(X)[i] ]

The MARGIN of a fixture is the smallest |d2 - rad2| / (|a|^2 + |b|^2) over every <= comparison these four make (for coverage: every
d2(x_i, y_j) against rad2_k(X)[i], which decides the comparison of the minimum too).  The Gram form in fp64 differs from the exact d2 by
at most (2 D + 3) 2^-53 (|a|^2 + |b|^2) <= 4.6e-13 (|a|^2 + |b|^2) at D = 2048: a fixture whose margin exceeds 1e-9 has every decision
unambiguous, so counts and the five metrics must match EXACTLY and rad2 / dmin2 within TOL (|a|^2 + |b|^2)."""
import functools

import numpy as np

TOL = 1e-11             # |d rad2|, |d dmin2| <= TOL (|a|^2 + |b|^2)
MIN_MARGIN = 1e-9

# (Nr, Ng, D, k) -> precision, recall, density, coverage to three decimals, as published with the fixture generator
TABLE = {(300, 280, 64, 3): (0.757, 0.853, 0.557, 0.503), (300, 280, 64, 5): (0.843, 0.933, 0.591, 0.613),
         (210, 200, 2048, 3): (0.680, 0.933, 0.565, 0.495), (150, 77, 64, 3): (0.610, 0.867, 0.571, 0.467),
         (260, 130, 192, 5): (0.854, 0.965, 0.608, 0.500), (70, 70, 64, 1): (0.614, 0.714, 0.886, 0.400)}


def cloud(n, d, seed, axis, part, shift=2.5, wseed=40, latent=3, noise=0.02):
    """A low-dimensional sheet in d dimensions (i.i.d. clouds in 64+ dimensions give precision ~ recall ~ 0, which tests nothing)."""
    w = np.random.default_rng(wseed).uniform(0.0, 1.0, (latent, d))
    rng = np.random.default_rng(seed)
    z = np.abs(rng.standard_normal((n, latent)))
    z[: int(part * n), axis] += shift
    return (z @ w + noise * np.abs(rng.standard_normal((n, d)))).astype(np.float32)


def real_gen(nr, ng, d):
    return cloud(nr, d, 21, axis=1, part=0.4), cloud(ng, d, 22, axis=0, part=0.5)


def d2(a, b):
    """[len(a)][len(b)] float64, by direct differences."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((len(a), len(b)))
    for i in range(len(a)):
        out[i] = ((a[i][None, :] - b) ** 2).sum(axis=1)
    return out


def norms(a):
    a = np.asarray(a, dtype=np.float64)
    return (a * a).sum(axis=1)


def radii(f, k):
    return np.sort(d2(f, f), axis=1)[:, k]


def radii_scale(f, k):
    """|a|^2 + |b|^2 of the pair behind every rad2_k(f)[i]: what TOL multiplies."""
    n = norms(f)
    return n + n[np.argsort(d2(f, f), axis=1)[:, k]]


def query_scale(q, r):
    """|a|^2 + |b|^2 of the pair behind every dmin2[j]."""
    return norms(q) + norms(r)[d2(q, r).argmin(axis=1)]


def query(q, r, rad2=None):
    """(count | None, dmin2) per row of q."""
    d = d2(q, r)
    return (None if rad2 is None else (d <= rad2[None, :]).sum(axis=1)), d.min(axis=1)


def prdc(real, gen, k):
    """{"precision", "recall", "f_score", "density", "coverage"} and the fixture's margin."""
    dyx = d2(gen, real)                      # [Ng][Nr]
    rx, ry = radii(real, k), radii(gen, k)
    in_real = dyx <= rx[None, :]
    in_gen = dyx.T <= ry[None, :]            # [Nr][Ng]
    p, r = float(in_real.any(axis=1).mean()), float(in_gen.any(axis=1).mean())
    scale = norms(gen)[:, None] + norms(real)[None, :]
    margin = min(float((np.abs(dyx - rx[None, :]) / scale).min()), float((np.abs(dyx - ry[:, None]) / scale).min()))
    return {"precision": p, "recall": r, "f_score": 2 * p * r / (p + r) if p + r > 0 else 0.0,
            "density": float(in_real.sum() / (k * len(gen))), "coverage": float((dyx.min(axis=0) <= rx).mean()), "margin": margin}


@functools.lru_cache(maxsize=None)
def fixture(nr, ng, d, k):
    """(real, gen, prdc(real, gen, k)) of a table row: computed once, shared; callers must not write into the arrays."""
    real, gen = real_gen(nr, ng, d)
    ref = prdc(real, gen, k)
    real.setflags(write=False)
    gen.setflags(write=False)
    return real, gen, ref


def check_fixture(case):
    """The rule for using a fixture: its margin is printed and must exceed MIN_MARGIN; the reference reproduces the published table."""
    ref = fixture(*case)[2]
    print(f"fixture {case}: precision {ref['precision']:.3f} recall {ref['recall']:.3f} density {ref['density']:.3f} "
          f"coverage {ref['coverage']:.3f} margin {ref['margin']:.2e}")
    assert ref["margin"] > MIN_MARGIN, (case, ref["margin"])
    got = (ref["precision"], ref["recall"], ref["density"], ref["coverage"])
    assert all(abs(g - w) <= 5.01e-4 for g, w in zip(got, TABLE[case])), (case, got, TABLE[case])
    return ref
