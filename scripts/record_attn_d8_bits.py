#!/usr/bin/env python3
"""Record the fixtures of tests/test_gpu_attn_d8_bits.py (default) or of another bit test of pd_attn_d8 on the GPU: the output bits of
pd_attn_d8 / pd_attn_d8_bwd for the seeded cases of a cases module under tests/, from a library built from the kernel sources of the
revision the next change must reproduce:

    scripts/build_rev.sh <rev> parent
    PD_LIB=build_ab/parent.so PD_ALLOW_ABI_MISMATCH=1 python scripts/record_attn_d8_bits.py [--cases attn_d8_resident3_cases]

Refuses to overwrite a fixture that exists (delete it on purpose to re-record).  Asserts, per ``spread`` case, that some hundred
probabilities fall in 2^-126 .. 2^-119 (fp64 restatement, ``band_count``), and records every case twice to see that the bits repeat.
A cases module with ``check_paths`` (fp64 restatement of the kernel's per-wave decisions) has it asserted per case before anything is
launched, and one with ``reference`` has the recorded output compared with it at the module's ``TOL``: a case that does not reach the
path it is named for fails here instead of passing vacuously later."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
cases = sys.argv[sys.argv.index("--cases") + 1] if "--cases" in sys.argv else "attn_d8_bits_cases"
A = importlib.import_module(cases)
import phendiff_amd._lib as L  # noqa: E402

assert os.environ.get("PD_LIB"), "set PD_LIB to the library built from the revision whose bits are recorded (scripts/build_rev.sh)"
os.makedirs(A.GOLDEN, exist_ok=True)
lib = L.lib()
dev = torch.device("cuda:0")
for name, case in A.CASES.items():
    path = A.fixture_path(name)
    if os.path.exists(path):
        print(f"{name}: {os.path.relpath(path, ROOT)} exists, not overwritten")
        continue
    t = A.make_inputs(name)
    extra = {}
    if hasattr(A, "band_count"):
        band = A.band_count(name, t)
        if case[5] == "spread":
            assert band >= 300, f"{name}: only {band} probabilities in 2^-126 .. 2^-119"
        extra["band"] = np.int64(band)
    if hasattr(A, "check_paths"):
        print(f"{name}: {A.check_paths(name, t)}", flush=True)
    raw = A.run_case(L, lib, name, t, dev)
    got = A.stored_form(raw)
    again = A.stored_form(A.run_case(L, lib, name, t, dev))
    assert all(np.array_equal(got[k], again[k]) for k in got), f"{name}: two runs of the same library differ"
    out = got.get("out", got.get("out__sample127"))
    assert not np.any((out.astype(np.int32) & 0x7f80) == 0x7f80), f"{name}: non-finite output"
    if hasattr(A, "reference"):
        ref, _ = A.reference(t, dev)
        err = float((raw["out"].view(torch.bfloat16).double() - ref).norm() / ref.norm())
        print(f"{name}: relative L2 against fp64 {err:.3e} (tolerance {A.TOL})", flush=True)
        assert err < A.TOL, f"{name}: the recorded revision itself is {err:.3e} from the fp64 reference"
    np.savez_compressed(path, inputs_sha256=np.frombuffer(bytes.fromhex(A.inputs_sha256(t)), dtype=np.uint8), **extra, **got)
    print(f"{name}: {extra}, {os.path.getsize(path)} bytes -> {os.path.relpath(path, ROOT)}")
