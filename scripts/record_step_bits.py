#!/usr/bin/env python3
"""Record the fixtures of tests/test_gpu_step_bits.py on the GPU: the output bits of the five scheduler-step entry points for the seeded
cases of tests/step_bits_cases.py, from a library built from the kernel sources of the revision the next change must reproduce:

    scripts/build_rev.sh <rev> parent
    PD_LIB=build_ab/parent.so PD_ALLOW_ABI_MISMATCH=1 python scripts/record_step_bits.py

One file per entry point.  Refuses to overwrite a fixture that exists (delete it on purpose to re-record), and records every case twice to
see that the bits repeat.  Asserted on the CPU before anything is written:
  * thresholded cases: from the fp64 raw x0 of tests/threshold_refs.py and the recorded quantile q, s = clamp(q, 1, sample_max_value); every
    case of 75 elements or more that has a finite x0 has elements on both sides of s (both branches of clamp(x0, -s, s)), and over the
    entry point's cases q falls below 1, between 1 and sample_max_value, and above it (all three branches of the clamp of q);
  * statically clipped pd_ddim_step cases of 75 elements or more: the fp64 x0 of tests/flat_refs.py has magnitudes on both sides of 1;
  * outputs are finite, except where sqrt_a == 0 meets epsilon prediction (x0 divides by zero there, in every revision) and in the case
    that feeds a non-finite gradient on purpose."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flat_refs as R  # noqa: E402
import step_bits_cases as A  # noqa: E402
import threshold_refs as T  # noqa: E402
import phendiff_amd._lib as L  # noqa: E402

assert os.environ.get("PD_LIB"), "set PD_LIB to the library built from the revision whose bits are recorded (scripts/build_rev.sh)"
os.makedirs(A.GOLDEN, exist_ok=True)
lib = L.lib()
dev = torch.device("cuda:0")


def clamp_sides(name, t, got):
    """(elements of the fp64 x0 below the limit, above it, the recorded quantiles) of a thresholded or statically clipped case."""
    kind, B, per, s = A.CASES[name]
    coef = A.coefficients(name)
    if kind in ("thr", "ms_thr"):
        q = got["a_quant"].numpy().view(np.float32)
        raw = np.abs(T.step_f64(dict(t, quantile=q), (coef[0], coef[1], 0.0, 0.0), s["pred"], 0, A.SAMPLE_MAX_VALUE, s["guidance"])[2])
        limit = T.threshold_s(q, A.SAMPLE_MAX_VALUE)
    else:
        q = None
        raw = np.abs(R.ddim_f64(t, coef, s["pred"], 0, 0, s["guidance"])[1])
        limit = R.CLIP_RANGE
    fin = np.isfinite(raw)
    return int((fin & (raw < limit)).sum()), int((fin & (raw > limit)).sum()), int(fin.sum()), q


for kind in A.KINDS:
    path = A.fixture_path(kind)
    if os.path.exists(path):
        print(f"{kind}: {os.path.relpath(path, ROOT)} exists, not overwritten")
        continue
    kept, q_all = {}, []
    for name in A.cases_of(kind):
        _, B, per, s = A.CASES[name]
        t = A.make_inputs(name)
        got = A.run_case(L, lib, name, t, dev)
        again = A.run_case(L, lib, name, t, dev)
        assert got.keys() == again.keys() and all(torch.equal(got[k], again[k]) for k in got), f"{name}: two runs of the same library differ"
        note = ""
        if kind in ("thr", "ms_thr") or (kind == "ddim" and s["clip"]):
            below, above, finite, q = clamp_sides(name, t, got)
            if q is not None:
                q_all.append(q)
            if B * per >= 75 and finite:
                assert below > 0 and above > 0, f"{name}: {below} elements below the limit, {above} above"
            note = f", x0 below / above the limit: {below} / {above}"
        singular = A.coefficients(name)[0] == 0.0 and s["pred"] == 0
        if not (singular or s["bad_grad"]):
            for k, v in got.items():
                assert k.endswith("overflow") or np.isfinite(v.numpy().view(np.float32)).all(), f"{name}: non-finite {k}"
        stored = A.stored_form(got)
        kept[f"{name}--inputs_sha256"] = np.frombuffer(bytes.fromhex(A.inputs_sha256(t)), dtype=np.uint8)
        kept.update({f"{name}--{k}": v for k, v in stored.items()})
        print(f"{name}: {len(stored)} arrays{note}")
    if q_all:
        q = np.concatenate(q_all)
        q = q[np.isfinite(q)]
        counts = (int((q < 1).sum()), int(((q > 1) & (q < A.SAMPLE_MAX_VALUE)).sum()), int((q > A.SAMPLE_MAX_VALUE).sum()))
        assert min(counts) > 0, f"{kind}: quantiles below 1 / inside / above sample_max_value: {counts}"
        print(f"{kind}: quantiles below 1 / inside / above sample_max_value: {counts}")
    np.savez_compressed(path, **kept)
    print(f"{kind}: {len(kept)} arrays, {os.path.getsize(path)} bytes -> {os.path.relpath(path, ROOT)}")
