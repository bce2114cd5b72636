#!/usr/bin/env python3
"""Record the fixtures of tests/test_gpu_reduce_bits.py on the GPU: the output bits of the entry points whose reductions run through
csrc/pd_reduce.h, for the seeded cases of tests/reduce_bits_cases.py, from a library built from the kernel sources of the revision the
next change must reproduce:

    scripts/build_rev.sh <rev> parent
    PD_LIB=build_ab/parent.so PD_ALLOW_ABI_MISMATCH=1 python scripts/record_reduce_bits.py

One file per entry point.  Refuses to overwrite a fixture that exists (delete it on purpose to re-record), and records every case twice to
see that the bits repeat.  Asserted on the CPU before anything is written -- what makes a fixture evidence, not a snapshot:
  * every recorded fp64 sum of n terms lies within n * 2^-52 * sum|v| of math.fsum over the same terms formed in float64 from the inputs
    (the worst case of an fp64 sum in any order, with a factor 2 for the terms' own roundings; tests/test_gpu_objects.py's bound); a sum
    the kernel divides by n is compared after the same division, with one more rounding allowed.  Minima, maxima, counts and histograms
    equal numpy's.  Where what is recorded is a function of sums -- pd_guidance_rescale's out, pd_ssim's means, pd_kid_mmd -- the bound
    is the one the entry point's own GPU test derives for its float64 restatement;
  * every case of more than 256 partial records folds runs of per >= 2 records (pd_reduce.h's formula, restated), and every entry point
    that has such a case has one whose last run is shorter than the others;
  * every case with B >= 2 rows of odd length has slots taken by the 16-byte access and slots taken by element accesses;
  * outputs are finite except in the rows built not to be (a NaN / Inf row, a constant row, an all-zero sample, a NaN pixel), which are
    compared like every other row."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reduce_bits_cases as A  # noqa: E402
import phendiff_amd._lib as L  # noqa: E402

assert os.environ.get("PD_LIB"), "set PD_LIB to the library built from the revision whose bits are recorded (scripts/build_rev.sh)"
os.makedirs(A.GOLDEN, exist_ok=True)
lib = L.lib()
dev = torch.device("cuda:0")
EPS = 2.0 ** -52


def f64_of(got, key, shape=None):
    a = got[key].numpy().view(np.float64)
    return a if shape is None else a.reshape(shape)


def f32_of(got, key):
    return got[key].numpy().view(np.float32)


def assert_sum(what, got, terms, divide=1.0):
    """got = (an fp64 sum of ``terms`` in some order) / divide."""
    terms = np.asarray(terms, dtype=np.float64).ravel()
    if not np.isfinite(terms).all():
        with np.errstate(invalid="ignore"):
            want = terms.sum() / divide
        assert (np.isnan(got) and np.isnan(want)) or got == want, f"{what}: {got} against numpy's {want}"
        return
    want, mag = math.fsum(terms) / divide, math.fsum(np.abs(terms)) / divide
    bound = len(terms) * EPS * mag + (EPS * abs(want) if divide != 1.0 else 0.0)
    assert abs(got - want) <= bound, f"{what}: {got} against fsum's {want}: off by {abs(got - want):.3e}, bound {bound:.3e}"


def check_sample_stats(name, s, t, got):
    F = L.SAMPLE_STATS_FIELDS
    dt = A.TORCH[s["dtype"]]
    wide = lambda a: torch.from_numpy(a).to(dt).to(torch.float64).numpy()      # noqa: E731
    x = wide(t["x"])
    y = None if "y" not in t else np.broadcast_to(wide(t["y"]), x.shape)
    stats = f64_of(got, "stats", (s["B"], len(F)))
    n = s["n"]
    for b in range(s["B"]):
        row = dict(zip(F, stats[b]))
        bad = ~np.isfinite(x[b])
        assert bool(bad.any()) == (s["special"] and b == 1), f"{name}: row {b} non-finite inputs"
        assert row["nonfinite"] == bad.sum() and row["min"] == np.fmin.reduce(x[b]) and row["max"] == np.fmax.reduce(x[b]), (name, b)
        assert_sum(f"{name} row {b} sum", row["sum"], x[b])
        if not bad.any():
            assert np.isfinite(stats[b]).all(), (name, b)
            d = x[b] - row["sum"] / n
            for k in (2, 3, 4):
                assert_sum(f"{name} row {b} m{k}", row[f"m{k}"], d ** k, divide=float(n))
        if y is not None and not bad.any():
            e = x[b] - y[b]
            assert_sum(f"{name} row {b} err_l1", row["err_l1"], np.abs(e))
            assert_sum(f"{name} row {b} err_sq", row["err_sq"], e * e)
            assert row["err_max"] == np.abs(e).max(), (name, b)
        if s["bins"]:
            hist = got["hist"].numpy().view(np.uint32).reshape(s["B"], s["bins"])[b]
            assert np.array_equal(hist, np.histogram(x[b][np.isfinite(x[b])], bins=A.EDGES100)[0]), (name, b)


def check_guidance(name, s, t, got):
    import guidance_rescale_ref as G
    cond, uncond = torch.from_numpy(t["cond"]), torch.from_numpy(t["uncond"])
    live = [b for b in range(s["B"]) if b != s["constant_row"]]
    nonfinite = []
    for key, v in got.items():
        eqn, w = int(key[1]), (A.W1 if "_w1_" in key else A.W3)
        wt = torch.tensor([w[b % len(w)] for b in range(s["B"])] if len(w) > 1 else w, dtype=torch.float32)
        out = torch.from_numpy(f32_of(got, key).reshape(s["B"], s["n"]))
        want = G.reference(cond, uncond, wt, A.PHI, eqn)
        assert bool(torch.isfinite(out[live]).all()), f"{name} {key}: a non-finite element outside the constant row"
        if s["constant_row"] is not None:      # one g for the row: all of it finite (both variances rounded above zero) or none of it
            nonfinite.append(int((~torch.isfinite(out[s["constant_row"]])).sum()))
            assert nonfinite[-1] in (0, s["n"]), f"{name} {key}: {nonfinite[-1]} of {s['n']} elements of the constant row are non-finite"
        worst = float(G.ulps(out[live], want[live]).max())
        assert worst <= G.MAX_ULPS, f"{name} {key}: {worst} ulp from the float64 restatement (bound {G.MAX_ULPS})"
    assert all(torch.equal(got[f"e{e}_w{w}_in_place"], got[f"e{e}_w{w}_out_of_place"]) for e in (0, 1) for w in (1, 3)), name
    assert s["constant_row"] is None or max(nonfinite) == s["n"], f"{name}: no variant whose constant row reaches the clamp (g NaN or Inf)"


def check_contrast_mask(name, s, t, got):
    B, n = s["B"], s["n"]
    acc = t["acc"]
    stats, cmap = f32_of(got, "given_stats").reshape(B, 3), f32_of(got, "given_map").reshape(B, n)
    mask = got["given_mask"].numpy().reshape(B, n)
    assert torch.equal(got["given_mask"], got["null_mask"]), name
    for b in range(B):
        terms = acc[b].astype(np.float64)
        want, bound = math.fsum(terms), n * EPS * math.fsum(np.abs(terms))
        mean, limit = stats[b, 0], stats[b, 1]
        assert np.float32((want - bound) / n) <= mean <= np.float32((want + bound) / n), f"{name} row {b}: mean {mean} against fsum / n = {want / n}"
        assert limit == np.float32(A.RATIO) * mean, (name, b)
        assert (limit > 0) == (s["zero_row"] != b), f"{name} row {b}: limit {limit}"
        with np.errstate(all="ignore"):
            m = np.fmin(acc[b], limit) / limit if limit > 0 else np.zeros(n, np.float32)
        assert m.dtype == np.float32 and np.abs(m.view(np.int32) - cmap[b].view(np.int32)).max() <= 1, f"{name} row {b}: map (one fp32 division)"
        assert np.array_equal(mask[b], (cmap[b] > 0.5).astype(np.uint8)) and stats[b, 2] == np.float32(int(mask[b].sum()) / n), f"{name} row {b}: count"
    assert np.isfinite(stats).all() and np.isfinite(cmap).all(), name


def check_ssim(name, s, t, got):
    import ssim_ref as R
    dt = A.TORCH[s["dtype"]]
    x, y = torch.from_numpy(t["x"]).to(dt), torch.from_numpy(t["y"]).to(dt)
    want = R.maps_means(x, y, levels=s["levels"], win=s["win"], sigma=A.SSIM_SIGMA[s["win"]])
    means = f64_of(got, "means", want.shape)
    worst = float(np.abs(means - want).max())
    assert np.isfinite(means).all() and worst <= 1e-9, f"{name}: {worst:.3e} from the float64 restatement (tests/test_gpu_ssim.py's 1e-9)"


def check_object_intensity(name, s, t, got):
    import objects_ref as O
    index, count, _ = O.index_ref(t["mask"], s["conn"], s["K"])
    geometry = O.geometry_ref(index, s["K"])
    B, K = index.shape[0], s["K"]
    assert np.array_equal(got["geometry"].numpy().reshape(geometry.shape), geometry) and np.array_equal(got["count"].numpy(), count), name
    assert (count.max() > K) == (K < 1024), f"{name}: {count.max()} objects at most, max_objects = {K}"
    table, bound = O.intensity_ref(index, t["images"], K)
    raw = f64_of(got, "table", table.shape)
    hit = np.zeros(table.shape[:3], bool)
    if s["nan"]:
        (b, c, y, x), (ob, _, oy, ox) = A.HAND_NAN_INSIDE, A.HAND_NAN_OUTSIDE
        k = index[b, y, x]
        assert k > 0 and index[ob, oy, ox] == 0 and np.isnan(t["images"][ob, :, oy, ox]).any(), name
        hit[b, k - 1, c] = True
        assert np.isnan(raw[hit]).all(), f"{name}: the object that holds a NaN pixel"
    assert np.isfinite(raw[~hit]).all(), f"{name}: a non-finite row outside the object that holds the NaN"
    assert np.array_equal(raw[~hit][:, 2:], table[~hit][:, 2:]), f"{name}: min / max"
    assert (np.abs(raw[~hit][:, :2] - table[~hit][:, :2]) <= bound[~hit]).all(), f"{name}: sums against fsum"
    if s["mask"] == "hand_40x48":
        boxes = sorted((g[2] - g[1] + 1) * (g[4] - g[3] + 1) for g in geometry[0] if g[0] > 0)
        assert boxes[0] < 256 < boxes[-1], f"{name}: bounding boxes of {boxes} pixels"


def check_kid(name, s, t, got):
    from test_gpu_metric_stats import KID_CASES, check_kid as bound_check, kid_numpy
    _, _, m, _, S, degree, gamma, coef0 = KID_CASES[s["index"]]
    bound_check(name, f64_of(got, "sums", (S, 3)), f64_of(got, "mmd", (S,)), kid_numpy(t["f1"], t["f2"], t["i1"], t["i2"], degree, gamma, coef0))


def check_mask_stats(name, s, t, got):
    from mask_ops_cases import reference
    want = reference(s["mask"], "refine", s["recipe"])[1]
    assert np.array_equal(got["stats"].numpy().reshape(want.shape), want), name


CHECKS = {"sample_stats": check_sample_stats, "guidance_rescale": check_guidance, "contrast_mask": check_contrast_mask, "ssim": check_ssim,
          "object_intensity": check_object_intensity, "kid_mmd": check_kid, "mask_stats": check_mask_stats}

# ---- what the cases reach, from their sizes alone
for kind in A.KINDS:
    long_ = [n for n in A.LONG_FOLD if A.CASES[n][0] == kind]
    splits = {n: A.run_split(A.records_of(n)) for n in long_}
    assert all(per >= 2 for per, _, _ in splits.values()), splits
    if kind in A.CHUNK or kind == "ssim":
        assert any(last < per for per, _, last in splits.values()), f"{kind}: no case whose last run is shorter than the others: {splits}"
        print(f"{kind}: (per, runs, last run) of the long folds: {splits}")
for name, (kind, s) in A.CASES.items():
    if kind in A.CHUNK and s["B"] >= 2 and s["n"] % 2 == 1:
        vec = 4 if s.get("dtype", "f32") == "f32" else 8
        wide, narrow = A.slot_accesses(s["B"], s["n"], A.CHUNK[kind], vec, 16 // vec)
        assert wide > 0 and narrow > 0, f"{name}: {wide} slots by the 16-byte access, {narrow} by element accesses"

for kind in A.KINDS:
    path = A.fixture_path(kind)
    if os.path.exists(path):
        print(f"{kind}: {os.path.relpath(path, ROOT)} exists, not overwritten")
        continue
    kept = {}
    for name in A.cases_of(kind):
        s = A.CASES[name][1]
        t = A.make_inputs(name)
        got = A.run_case(L, lib, name, t, dev)
        again = A.run_case(L, lib, name, t, dev)
        assert got.keys() == again.keys() and all(torch.equal(got[k], again[k]) for k in got), f"{name}: two runs of the same library differ"
        CHECKS[kind](name, s, t, got)
        stored = A.stored_form(name, got)
        kept[f"{name}--inputs_sha256"] = np.frombuffer(bytes.fromhex(A.inputs_sha256(t)), dtype=np.uint8)
        kept.update({f"{name}--{k}": v for k, v in stored.items()})
        print(f"{name}: {len(stored)} arrays", flush=True)
    np.savez_compressed(path, **kept)
    print(f"{kind}: {len(kept)} arrays, {os.path.getsize(path)} bytes -> {os.path.relpath(path, ROOT)}")
