"""pd_attn_d8's DMA-staged bf16 kernel, fitted into 80 registers so that three workgroups are resident per CU, reproduces bit for bit
what the kernel of the revision before wrote on the paths the cases of tests/test_gpu_attn_d8_bits.py leave open: the ragged last tile,
the exact running-maximum path to the end with rescales of o, the hand-over exact -> check-free -> ragged inside one wave, the ``lse``
output, and the safety net behind a zeroed kmax2 slot.  Cases, inputs and the fp64 restatement that proved at recording time that each
case reaches its path: tests/attn_d8_resident3_cases.py; fixtures (sha256 plus every 127th element, recorded on an MI355X by
``scripts/record_attn_d8_bits.py --cases attn_d8_resident3_cases``): tests/golden/attn_d8_resident3_bits/.  Each case is also held against
the fp64 attention of its inputs at the bf16 tolerance of the head_dim-8 parity test (relative L2 < 8e-3)."""
import hashlib

import numpy as np
import pytest
import torch

import attn_d8_resident3_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import phendiff_amd._lib as L
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L, L.lib(), torch.device("cuda:0")


@pytest.mark.parametrize("name", list(A.CASES))
def test_bits_match_the_recorded_revision(env, name):
    L, lib, dev = env
    fx = np.load(A.fixture_path(name))
    t = A.make_inputs(name)
    assert A.inputs_sha256(t) == bytes(fx["inputs_sha256"]).hex(), "the seeded inputs are not the ones the fixture was recorded on"
    got = A.run_case(L, lib, name, t, dev)
    assert ("lse" in got) == A.CASES[name][2]
    for key, v in got.items():
        a = v.contiguous().numpy()
        want = torch.from_numpy(fx[key + "__sample127"])
        sample = torch.from_numpy(a.reshape(-1)[::127].copy())
        assert torch.equal(sample, want), f"{name}: {key} differs in {int((sample != want).sum())} of {want.numel()} sampled elements"
        assert hashlib.sha256(a.tobytes()).digest() == bytes(fx[key + "__sha256"]), f"{name}: {key} differs outside the stored sample"
    ref, ref_lse = A.reference(t, dev)
    out = got["out"].view(torch.bfloat16).double()
    err = float((out - ref).norm() / ref.norm())
    print(f"{name}: relative L2 against fp64 {err:.3e}")
    assert err < A.TOL
    if "lse" in got:
        lse = got["lse"].view(torch.float32).double()
        dl = float((lse - ref_lse).abs().max())
        print(f"{name}: max |lse - fp64| {dl:.3e} (log2 domain)")
        # lse = m + log2(l).  The kernel rounds the scaled q to bf16: 8 significant bits, relative error up to 2^-8 per element, so a score
        # moves by up to sum |q_d k_d| 2^-8 <= |q||k| 2^-8, and |q||k| <= 133 in these cases (``transition``: 0.52; plain inputs: 0.12).  The
        # row sum is taken over probabilities truncated to bf16 (up to 2^-7 low): another 2^-7 log2(e) = 0.011.  Bound: 0.54.
        assert dl < 0.54
