"""The entry points whose reductions run through csrc/pd_reduce.h reproduce, bit for bit, what the kernels of the revision before they
were put on that header wrote for the same seeded inputs (tests/golden/reduce_bits/, recorded on an MI355X by
scripts/record_reduce_bits.py from a library built with scripts/build_rev.sh; the recorder checked every recorded sum against math.fsum
before it wrote anything).  That change moved no arithmetic, so the comparison is ``torch.equal`` on the integer view -- NaN payloads
and signed zeros included -- not a tolerance.  Cases and inputs: tests/reduce_bits_cases.py.

The cases of more than 256 partial records -- where the run fold takes runs of two records, which no other test reaches -- are also run
one sample at a time: a sample's bytes alone equal its row in the batch."""
import hashlib

import numpy as np
import pytest
import torch

import reduce_bits_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import phendiff_amd._lib as L
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L, L.lib(), torch.device("cuda:0")


def assert_recorded_bits(fx, name, got):
    for key, v in got.items():
        full = f"{name}--{key}"
        if full in fx.files:
            want = torch.from_numpy(fx[full])
            assert torch.equal(v, want), f"{name}: {key} differs in {int((v != want).sum())} of {v.numel()} elements"
        else:
            a = v.contiguous().numpy()
            if full + "__sample127" in fx.files:      # (reduce_bits_cases.stored_form: six of eight outputs of the long guidance cases have none)
                want = torch.from_numpy(fx[full + "__sample127"])
                sample = torch.from_numpy(a.reshape(-1)[::127].copy())
                assert torch.equal(sample, want), f"{name}: {key} differs in {int((sample != want).sum())} of {want.numel()} sampled elements"
            assert hashlib.sha256(a.tobytes()).digest() == bytes(fx[full + "__sha256"]), f"{name}: {key} differs outside the stored sample"
    stored = {f.split("--", 1)[1].split("__")[0] for f in fx.files if f.startswith(name + "--")} - {"inputs_sha256"}
    assert stored == set(got), f"{name}: the fixture holds {sorted(stored)}, the run wrote {sorted(got)}"


@pytest.mark.parametrize("kind", A.KINDS)
def test_bits_match_the_recorded_revision(env, kind):
    L, lib, dev = env
    fx = np.load(A.fixture_path(kind))
    for name in A.cases_of(kind):
        t = A.make_inputs(name)
        assert A.inputs_sha256(t) == bytes(fx[f"{name}--inputs_sha256"]).hex(), f"{name}: the seeded inputs are not the ones the fixture was recorded on"
        assert_recorded_bits(fx, name, A.run_case(L, lib, name, t, dev))


@pytest.mark.parametrize("name", A.LONG_FOLD)
def test_a_long_fold_does_not_depend_on_the_batch(env, name):
    L, lib, dev = env
    assert A.run_split(A.records_of(name))[0] >= 2
    t = A.make_inputs(name)
    if A.CASES[name][0] == "ssim":      # a one-sample case: it is the second sample of a batch of two here
        t = {k: np.concatenate([v[:, :, ::-1], v]) for k, v in t.items()}
    B = len(next(iter(t.values())))
    assert B == 2
    whole = A.run_case(L, lib, name, t, dev)
    for b in range(B):
        alone = A.run_case(L, lib, name, t, dev, rows=slice(b, b + 1))
        for key, v in whole.items():
            assert torch.equal(v[b:b + 1], alone[key]), f"{name}: {key} of sample {b} alone differs from its row in the batch"
