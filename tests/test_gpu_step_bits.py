"""The five scheduler-step entry points reproduce, bit for bit, what the kernels of the revision before they were put on one quad walker
and operand former (csrc/pd_step.h) wrote for the same seeded inputs (tests/golden/step_bits/, recorded on an MI355X by
scripts/record_step_bits.py from a library built with scripts/build_rev.sh).  That change moved no arithmetic, so the comparison is
``torch.equal`` on the integer view -- NaN payloads included, at the sqrt_a == 0 epsilon step -- not a tolerance.  Cases and inputs:
tests/step_bits_cases.py.  The chains pd_ddim_raw_x0 -> pd_abs_quantile -> pd_ddim_step_threshold / pd_multistep_step also pin that the
thresholded x0 is the raw x0, thresholded."""
import hashlib

import numpy as np
import pytest
import torch

import step_bits_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import phendiff_amd._lib as L
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L, L.lib(), torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixtures():
    return {kind: np.load(A.fixture_path(kind)) for kind in A.KINDS}


def assert_recorded_bits(fx, name, got):
    for key, v in got.items():
        full = f"{name}--{key}"
        if full in fx.files:
            want = torch.from_numpy(fx[full])
            assert torch.equal(v, want), f"{name}: {key} differs in {int((v != want).sum())} of {v.numel()} elements"
        else:
            a = v.contiguous().numpy()
            want = torch.from_numpy(fx[full + "__sample127"])
            sample = torch.from_numpy(a.reshape(-1)[::127].copy())
            assert torch.equal(sample, want), f"{name}: {key} differs in {int((sample != want).sum())} of {want.numel()} sampled elements"
            assert hashlib.sha256(a.tobytes()).digest() == bytes(fx[full + "__sha256"]), f"{name}: {key} differs outside the stored sample"
    stored = {f.split("--", 1)[1].split("__")[0] for f in fx.files if f.startswith(name + "--")} - {"inputs_sha256"}
    assert stored == set(got), f"{name}: the fixture holds {sorted(stored)}, the run wrote {sorted(got)}"


@pytest.mark.parametrize("kind", A.KINDS)
def test_bits_match_the_recorded_revision(env, fixtures, kind):
    L, lib, dev = env
    fx = fixtures[kind]
    for name in A.cases_of(kind):
        t = A.make_inputs(name)
        assert A.inputs_sha256(t) == bytes(fx[f"{name}--inputs_sha256"]).hex(), f"{name}: the seeded inputs are not the ones the fixture was recorded on"
        assert_recorded_bits(fx, name, A.run_case(L, lib, name, t, dev))


@pytest.mark.parametrize("kind", ("thr", "ms_thr"))
def test_recorded_thresholded_x0_is_the_raw_x0_thresholded(fixtures, kind):
    """On the fixture alone (a CPU computation; the GPU mark is the module's): clamp(raw, -s, s) / s with s = clamp(q, 1, sample_max_value),
    one IEEE fp32 operation each, gives the recorded thresholded x0 bit for bit -- the x0 the update limits is the x0 whose quantile was taken."""
    fx = fixtures[kind]
    for name in A.cases_of(kind):
        for v in A.variants_of(name):
            if f"{name}--{v}_opt" not in fx.files:
                continue
            raw, x0 = (fx[f"{name}--{v}_{k}"].view(np.float32) for k in ("raw", "opt"))
            q = fx[f"{name}--{v}_quant"].view(np.float32)
            s = np.where(q < 1, np.float32(1.0), q)
            s = np.where(s > np.float32(A.SAMPLE_MAX_VALUE), np.float32(A.SAMPLE_MAX_VALUE), s)[:, None]
            with np.errstate(invalid="ignore"):
                want = (np.fmin(np.fmax(raw, -s), s) / s).astype(np.float32)          # (fmaxf / fminf: a NaN operand loses)
            same = (want.view(np.int32) == x0.view(np.int32)) | (np.isnan(want) & np.isnan(x0))
            assert same.all(), f"{name} ({v}): {int((~same).sum())} elements of the thresholded x0 are not the raw x0, thresholded"
