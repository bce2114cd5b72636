"""numpy float64 restatement of what ``pd_sample_stats`` / ``phendiff_amd.diagnostics`` compute (a plain module: no fixtures, nothing
imported from the product): the central moments, D'Agostino-Pearson's K^2 normality test from raw data, ``np.histogram`` and the
per-sample vector norms.  Sums go through ``math.fsum`` (correctly rounded), so the restatement's own error is one rounding of the mean
and one per moment."""
import math

import numpy as np


def moments(x64):
    """x64: 1-D float64.  {"n", "mean", "m2", "m3", "m4", "min", "max", "nonfinite"} with m_k = sum((x - mean)^k) / n."""
    x64 = np.asarray(x64, dtype=np.float64).reshape(-1)
    n = x64.size
    mean = math.fsum(x64) / n
    d = x64 - mean
    return dict(n=n, mean=mean, m2=math.fsum(d ** 2) / n, m3=math.fsum(d ** 3) / n, m4=math.fsum(d ** 4) / n,
                abs1=math.fsum(np.abs(x64)) / n, abs_d=[math.fsum(np.abs(d) ** k) / n for k in (0, 1, 2, 3, 4)],
                min=float(x64.min()), max=float(x64.max()), nonfinite=int((~np.isfinite(x64)).sum()))


def normaltest_of_moments(n, m2, m3, m4):
    """K2 = Z1^2 + Z2^2 from the central moments: Z1 from the sample skewness (D'Agostino 1970), Z2 from the sample kurtosis (Anscombe &
    Glynn 1983); K2 ~ chi^2(2) under normality, p = exp(-K2 / 2)."""
    if n < 8:
        raise ValueError("at least 8 observations")
    n = float(n)
    skew, kurt = m3 / m2 ** 1.5, m4 / m2 ** 2
    y = skew * np.sqrt((n + 1) * (n + 3) / (6.0 * (n - 2)))
    beta2 = 3.0 * (n ** 2 + 27 * n - 70) * (n + 1) * (n + 3) / ((n - 2) * (n + 5) * (n + 7) * (n + 9))
    w2 = -1 + np.sqrt(2 * (beta2 - 1))
    delta = 1 / np.sqrt(0.5 * np.log(w2))
    alpha = np.sqrt(2.0 / (w2 - 1))
    y = 1.0 if y == 0 else y
    z1 = delta * np.log(y / alpha + np.sqrt((y / alpha) ** 2 + 1))
    e = 3.0 * (n - 1) / (n + 1)
    var = 24.0 * n * (n - 2) * (n - 3) / ((n + 1) ** 2 * (n + 3) * (n + 5))
    x = (kurt - e) / np.sqrt(var)
    sb1 = 6.0 * (n * n - 5 * n + 2) / ((n + 7) * (n + 9)) * np.sqrt(6.0 * (n + 3) * (n + 5) / (n * (n - 2) * (n - 3)))
    a = 6.0 + 8.0 / sb1 * (2.0 / sb1 + np.sqrt(1 + 4.0 / sb1 ** 2))
    den = 1 + x * np.sqrt(2 / (a - 4.0))
    z2 = ((1 - 2 / (9.0 * a)) - np.sign(den) * ((1 - 2.0 / a) / abs(den)) ** (1 / 3.0)) / np.sqrt(2 / (9.0 * a))
    k2 = float(z1 * z1 + z2 * z2)
    return k2, math.exp(-0.5 * k2)


def normaltest(x64):
    """(K2, pvalue) of D'Agostino-Pearson's omnibus test from raw data (what ``scipy.stats.normaltest`` returns)."""
    m = moments(x64)
    return normaltest_of_moments(m["n"], m["m2"], m["m3"], m["m4"])


def histogram(x64, bins, range):
    """np.histogram's counts (int64 [bins]) and edges (float64 [bins + 1]) of one sample; NaN / inf fall in no bin."""
    x64 = np.asarray(x64, dtype=np.float64).reshape(-1)
    counts, edges = np.histogram(x64[np.isfinite(x64)], bins=bins, range=range)
    assert np.array_equal(edges, np.linspace(range[0], range[1], bins + 1))
    return counts.astype(np.int64), edges


def outside(x64, range):
    """How many elements of one sample lie in no bin: below, above, NaN or infinite."""
    x64 = np.asarray(x64, dtype=np.float64).reshape(-1)
    return int(x64.size - ((x64 >= range[0]) & (x64 <= range[1])).sum())


def distances(x64, y64):
    """x64 [B, n], y64 [B, n] or [n] (float64): {"l1", "l2", "linf"} = torch.linalg.vector_norm(x - y, ord, dim=1), plus "mse" and "psnr"
    (data range 2.0)."""
    import torch
    e = torch.from_numpy(np.asarray(x64, dtype=np.float64)) - torch.from_numpy(np.asarray(y64, dtype=np.float64))
    out = {k: torch.linalg.vector_norm(e, ord=o, dim=1).numpy() for k, o in (("l1", 1), ("l2", 2), ("linf", float("inf")))}
    out["mse"] = (e ** 2).mean(dim=1).numpy()
    with np.errstate(divide="ignore"):
        out["psnr"] = 10.0 * np.log10(4.0 / out["mse"])
    return out
