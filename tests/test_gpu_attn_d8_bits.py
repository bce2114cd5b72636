"""pd_attn_d8 / pd_attn_d8_bwd in bf16 reproduce, bit for bit, what the kernels of the revision before the check-free body of the
DMA-staged kernel was re-scheduled wrote for the same seeded inputs (tests/golden/attn_d8_bits/, recorded on an MI355X by
scripts/record_attn_d8_bits.py from a library built with scripts/build_rev.sh).  The change kept the key order and the order of every
accumulation, so the comparison is ``torch.equal`` on the integer view, not a tolerance.  Cases and inputs: tests/attn_d8_bits_cases.py
(``spread`` inputs put thousands of probabilities between 2^-126 and 2^-119, where an instruction that treats the upper half of an fp32
word as an f16 would meet a denormal)."""
import hashlib

import numpy as np
import pytest
import torch

import attn_d8_bits_cases as A

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
    if A.CASES[name][5] == "spread":
        assert int(fx["band"]) >= 300          # (the recording script counted them: fp64 restatement, band_count)
    got = A.run_case(L, lib, name, t, dev)
    for key, v in got.items():
        if key in fx.files:
            want = torch.from_numpy(fx[key])
            assert torch.equal(v, want), f"{name}: {key} differs in {int((v != want).sum())} of {v.numel()} elements"
        else:
            a = v.contiguous().numpy()
            want = torch.from_numpy(fx[key + "__sample127"])
            sample = torch.from_numpy(a.reshape(-1)[::127].copy())
            assert torch.equal(sample, want), f"{name}: {key} differs in {int((sample != want).sum())} of {want.numel()} sampled elements"
            assert hashlib.sha256(a.tobytes()).digest() == bytes(fx[key + "__sha256"]), f"{name}: {key} differs outside the stored sample"


def test_band_counts_of_the_spread_inputs():
    """The fp64 restatement itself, on the smallest case of each kind (a CPU computation; the GPU mark is the module's)."""
    for name in ("fwd_n300_spread", "bwd_n256_spread"):
        assert A.band_count(name, A.make_inputs(name)) >= 300


def test_captured_ddib_graph_replay_equals_eager_loop():
    """One replay of a captured 3-step DDIBGraph at 32 x 32 against the eager loop: the captured launches compute the same bits."""
    import phendiff_amd as P
    torch.manual_seed(0)
    cfg = dict(P.UNET_CONFIGS["super_small"], sample_size=32)
    unet = P.CustomCondUNet2DModel(compute_dtype="bf16", **cfg).to("cuda:0")
    pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
    g = torch.Generator().manual_seed(1234)
    labels = (torch.arange(2) % 2).cuda()
    x = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).cuda()
    eager = P.ddib(pipe, x, labels, 1 - labels, 3)
    replay = P.DDIBGraph(pipe, batch_size=2, num_inference_steps=3, height=32, width=32).run(x, labels, 1 - labels).images
    torch.cuda.synchronize()
    assert torch.isfinite(replay).all()
    assert torch.equal(replay.cpu(), torch.as_tensor(eager).cpu())         # (the eager transfer returns a host array)
