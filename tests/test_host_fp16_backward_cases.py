"""The loss-scaled cases of tests/fp16_bwd_cases.py, checked on the CPU: at GAIN the fp64 reference stays below 2^15 in magnitude at every value
the kernels keep in fp16 -- the inputs, the stored outputs (dx, dq / dk / dv), and dP - delta per (query, key) for the attention backwards
(an upper bound of |dS|, since p <= 1).  Were that not so, tests/test_gpu_fp16_backward.py could not tell a kernel that saturates from a
reference that does.  A seed that breaks this is changed (or the input's standard deviation), never the threshold."""
import pytest
import torch

import fp16_bwd_cases as cases


@pytest.mark.parametrize("make,key", cases.ALL_CASES, ids=[f"{f.__name__}-{k}" for f, k in cases.ALL_CASES])
def test_reference_stays_inside_fp16_at_the_gain(make, key):
    c = make(key)
    assert c.grads and set(c.grads) <= set(c.inputs)
    for name, t in c.scaled_inputs(cases.GAIN).items():
        if name in ("x", "q", "k", "v", "kv", "dout", "dy", "dz", "du", "res"):          # the 16-bit operands (gamma, beta, scale, shift are fp32)
            assert torch.equal(t.half().float(), t), (c.name, name, "not exact in fp16")
        assert float(t.abs().max()) < cases.FP16_LIMIT, (c.name, name)
    for name, t in c.kept.items():
        assert bool(torch.isfinite(t).all())
        assert float(t.abs().max()) * cases.GAIN < cases.FP16_LIMIT, (c.name, name, float(t.abs().max()) * cases.GAIN)
    for name, t in c.ref.items():
        assert t.dtype == torch.float64 and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, (c.name, name)


def test_gain_is_a_power_of_two():
    m, _ = torch.frexp(torch.tensor(cases.GAIN))
    assert float(m) == 0.5 and cases.GAIN > 1
