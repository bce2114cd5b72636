#!/usr/bin/env python
"""The KID / FID statistics at the reference's evaluation workload (N1 = N2 = 5000 samples of 2048 features, 100 KID subsets of 1000):
`phendiff_amd.metrics.kernel_inception_distance_device` and `fid_statistics_device` (pd_kid_mmd / pd_feature_moments, fp64 MFMA) against
the host functions `kernel_inception_distance` and `fid_statistics` (numpy) in the same process on the same machine.

Every device figure is a host clock around work that ends in a device synchronise, after a warm-up call of the same shape; the host KID is
ONE timed run (it takes minutes).  FLOP are counted from the shapes: "useful" = what numpy does (3 m^2 D multiply-adds per subset; N D^2
for the covariance), "issued" = what the tiles compute (upper-triangle tiles of the symmetric products, whole 64 x 64 tiles).
Prints one JSON line per measurement.

    python scripts/experiments/bench_metric_stats.py [--n 5000] [--d 2048] [--subsets 100] [--subset-size 1000] [--repeats 5] [--skip-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import phendiff_amd.metrics as M  # noqa: E402


def features(n, d, seed):
    rng = np.random.default_rng(seed)
    return (np.abs(rng.standard_normal((n, d))) * rng.uniform(0.2, 1.2, d) + rng.uniform(0.0, 0.5, d)).astype(np.float32)


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset-size", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X path: no GPU, no number"
    N, D, S, m = a.n, a.d, a.subsets, a.subset_size
    f1, f2 = features(N, D, 1), features(N, D, 2) * np.float32(1.05) + np.float32(0.02)
    F1, F2 = torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda()
    nt = (m + 63) // 64
    kid_issued = S * (nt * (nt + 1) + nt * nt) * 64 * 64 * D * 2
    kid_useful = S * 3 * m * m * D * 2
    nd = D // 64
    cov_issued, cov_useful = nd * (nd + 1) // 2 * 64 * 64 * N * 2, N * D * D * 2
    say = lambda **kw: print(json.dumps(kw), flush=True)      # noqa: E731

    kid_dev, ts = timed(lambda: M.kernel_inception_distance_device(F1, F2, kid_subsets=S, kid_subset_size=m), a.repeats)
    say(what="kernel_inception_distance_device", N=N, D=D, subsets=S, subset_size=m, seconds=ts, best=min(ts),
        issued_tflops=kid_issued / min(ts) / 1e12, useful_tflops=kid_useful / min(ts) / 1e12, result=kid_dev)
    i1, i2 = M.kid_subset_indices(N, N, S, m)
    I1, I2 = torch.from_numpy(i1).cuda(), torch.from_numpy(i2).cuda()
    _, ts = timed(lambda: M.kid_mmd_device(F1, F2, I1, I2), a.repeats)      # (still checks the tables on the host and copies them)
    say(what="kid_mmd_device (tables given)", seconds=ts, best=min(ts), issued_tflops=kid_issued / min(ts) / 1e12)
    (mu, sigma), ts = timed(lambda: M.fid_statistics_device(F1), max(a.repeats, 10))
    say(what="fid_statistics_device", N=N, D=D, seconds=ts, best=min(ts), issued_tflops=cov_issued / min(ts) / 1e12,
        useful_tflops=cov_useful / min(ts) / 1e12)
    t0 = time.perf_counter()
    mu_h, sigma_h = mu.cpu().numpy(), sigma.cpu().numpy()
    say(what="mean + covariance to the host", seconds=time.perf_counter() - t0)
    if a.skip_host:
        return
    t0 = time.perf_counter()
    mu_ref, sigma_ref = M.fid_statistics(f1)
    t_fid = time.perf_counter() - t0
    v = np.diagonal(sigma_ref)
    say(what="fid_statistics (host)", seconds=t_fid, speedup=t_fid / min(ts), threads=torch.get_num_threads(),
        max_cov_error=float((np.abs(sigma_h - sigma_ref) / np.sqrt(np.outer(v, v))).max()),
        max_mean_error=float((np.abs(mu_h - mu_ref) / (np.abs(mu_ref) + np.sqrt(v))).max()))
    t0 = time.perf_counter()
    kid_host = M.kernel_inception_distance(f1, f2, kid_subsets=S, kid_subset_size=m)
    t_kid = time.perf_counter() - t0
    say(what="kernel_inception_distance (host, one run)", seconds=t_kid, result=kid_host,
        mean_difference=abs(kid_host[M.KEY_KID_MEAN] - kid_dev[M.KEY_KID_MEAN]), std_difference=abs(kid_host[M.KEY_KID_STD] - kid_dev[M.KEY_KID_STD]))


if __name__ == "__main__":
    main()
