"""tests/flat_refs.py proven on the CPU: for every operation and every input set tests/test_gpu_flat_kernels.py uses, the fp32
replica stays within the derived bound of the float64 reference -- the condition the reference alone passes, which must hold
before anything runs on a GPU.  Also: the uint8 excluded-share cap of pd_postproc, the bit-exact rounding reference of
pd_nchw_to_nhwc against torch's .to(dtype), and that the input sets reach what they are meant to reach."""
import numpy as np
import pytest
import torch

import flat_refs as R


def check(got, ref, bnd, what):
    ok, ratio = R.within(got, ref, bnd)
    assert ok, f"{what}: fp32 replica outside the bound (largest error / bound = {ratio:.3f})"
    return ratio


@pytest.mark.parametrize("n", R.GRAD_NORM_SIZES)
def test_grad_norm_replica(n):
    ones = R.grad_norm_input(n, "ones")
    assert R.grad_norm_f32_replica(ones) == np.float32(np.sqrt(np.float64(n)))
    x = R.grad_norm_input(n, "normal")
    ref = R.grad_norm_f64(x)
    got = R.grad_norm_f32_replica(x)
    assert abs(float(got) - ref) <= R.ulp32(ref)
    for max_norm in R.GRAD_NORM_MAX_NORMS:
        want = R.clip_coef_f32(np.float32(ref), max_norm)
        c = R.clip_coef_f32(got, max_norm)
        if max_norm > ref:
            assert want == 1.0 and c == 1.0
        else:
            assert want < 1.0 and abs(float(c) - float(want)) <= 2 * R.ulp32(want)


def test_grad_norm_max_norms_clip_and_do_not_clip():
    """The three max_norm values split the sizes: 1.0 clips every normal-data case from n = 3 on, 1e9 and inf never clip."""
    for n in R.GRAD_NORM_SIZES[1:]:
        assert 1.0 < R.grad_norm_f64(R.grad_norm_input(n, "normal")) < 1e9


@pytest.mark.parametrize("numel", R.ADAMW_SMALL + (R.ADAMW_LARGE,))
def test_adamw_ema_replica(numel):
    cases = R.adamw_cases_small() if numel != R.ADAMW_LARGE else R.adamw_cases_large()
    for t, wd, grads, (name, clip, _has_ema, _zg, ema_only) in cases:
        inp, h = R.adamw_input(numel, grads), R.adamw_hyper(t, wd)
        ref, got, bnd = (f(inp, h, clip, ema_only) for f in (R.adamw_f64, R.adamw_f32_replica, R.adamw_bound))
        for k in ref:
            check(got[k], ref[k], bnd[k], f"adamw {numel} t={t} wd={wd} {grads} {name} {k}")
        if ema_only:
            assert all(np.array_equal(got[k], inp[k]) for k in ("param", "exp_avg", "exp_avg_sq"))
        elif wd == 0.1 and numel > 1:
            # the decay is visible: without it param would land elsewhere by more than the bound
            h0 = dict(h, weight_decay=np.float32(0))
            assert np.any(np.abs(R.adamw_f64(inp, h0, clip, 0)["param"] - ref["param"]) > bnd["param"])


@pytest.mark.parametrize("shape", R.LOSS_SHAPES)
@pytest.mark.parametrize("pred", R.PRED_TYPES)
def test_diffusion_loss_replica(shape, pred):
    inp = R.loss_input(*shape)
    for gs in (1.0, 65536.0):
        (l_ref, g_ref), (l_got, g_got), (l_b, g_b) = (f(inp, pred, gs) for f in (R.loss_f64, R.loss_f32_replica, R.loss_bound))
        assert abs(float(l_got) - l_ref) <= l_b
        assert l_b < 1e-5 * l_ref                      # the bound still separates a wrong sample weight or a dropped element
        check(g_got, g_ref, g_b, f"loss grad {shape} {pred} x{gs}")
    g1, g2 = R.loss_f32_replica(inp, pred, 1.0)[1], R.loss_f32_replica(inp, pred, 65536.0)[1]
    assert np.array_equal(g1 * np.float32(65536.0), g2)


def test_ddim_coefficients_span_the_schedule():
    co = R.ddim_coefficients()
    assert co[0][0] == 0.0 and co[0][0] < co[1][0] < co[2][0] < 1.0       # sqrt_a smallest (exactly 0) at the first timestep
    assert all(c[1] > 0 for c in co)


@pytest.mark.parametrize("numel", R.DDIM_NUMEL)
def test_ddim_step_replica(numel):
    inp = R.ddim_input(1, numel)
    for ti, pred, clip, ucm in R.ddim_cases():
        coef = R.ddim_coefficients()[ti]
        ref, got, bnd = (f(inp, coef, pred, clip, ucm) for f in (R.ddim_f64, R.ddim_f32_replica, R.ddim_bound))
        for k, name in enumerate(("prev_sample", "pred_x0")):
            check(got[k], ref[k], bnd[k], f"ddim {numel} t{ti} pred{pred} clip{clip} ucm{ucm} {name}")


def test_ddim_step_inputs_reach_inside_outside_and_boundary():
    inp = R.ddim_input(1, 1025)
    for ti, pred in ((1, 0), (2, 0), (1, 1), (2, 1), (1, 2), (2, 2)):
        x0 = R.ddim_f64(inp, R.ddim_coefficients()[ti], pred, 0, 0)[1]
        assert np.any(np.abs(x0) < R.CLIP_RANGE) and np.any(np.abs(x0) > R.CLIP_RANGE), (ti, pred)
    x0 = R.ddim_f64(inp, R.ddim_coefficients()[1], 1, 0, 0)[1].reshape(-1)
    assert x0[0] == R.CLIP_RANGE and x0[1] == -R.CLIP_RANGE


@pytest.mark.parametrize("guidance", R.DDIM_GUIDANCE)
def test_ddim_step_guided_replica(guidance):
    inp = R.ddim_input(*R.DDIM_GUIDED)
    for ti, pred, clip, ucm in R.ddim_cases():
        coef = R.ddim_coefficients()[ti]
        ref, got, bnd = (f(inp, coef, pred, clip, ucm, guidance) for f in (R.ddim_f64, R.ddim_f32_replica, R.ddim_bound))
        for k, name in enumerate(("prev_sample", "pred_x0")):
            check(got[k], ref[k], bnd[k], f"ddim guided {guidance} t{ti} pred{pred} clip{clip} ucm{ucm} {name}")
    # a wrong sample index shows: with the per-sample weights rotated the result leaves the bound
    if len(guidance[1]) > 1:
        coef = R.ddim_coefficients()[2]
        ref, bnd = R.ddim_f64(inp, coef, 2, 0, 0, guidance)[0], R.ddim_bound(inp, coef, 2, 0, 0, guidance)[0]
        rot = R.ddim_f64(inp, coef, 2, 0, 0, (guidance[0], guidance[1][1:] + guidance[1][:1]))[0]
        assert np.all(np.any(np.abs(rot - ref) > bnd, axis=1))


@pytest.mark.parametrize("shape", R.ADD_NOISE_SHAPES)
@pytest.mark.parametrize("velocity", (0, 1))
def test_add_noise_replica(shape, velocity):
    inp = R.add_noise_input(*shape)
    check(R.add_noise_f32_replica(inp, velocity), R.add_noise_f64(inp, velocity), R.add_noise_bound(inp, velocity), "add_noise")


@pytest.mark.parametrize("C", R.POSTPROC_C)
@pytest.mark.parametrize("hw", R.POSTPROC_HW)
def test_postproc_replica_and_excluded_share(C, hw):
    x = R.postproc_input(C, *hw)
    (v_ref, q_ref), (v_got, q_got) = R.postproc_f64(x), R.postproc_f32_replica(x)
    check(v_got, v_ref, R.postproc_bound(x), "postproc fp32")
    assert v_got.min() >= 0.0 and v_got.max() <= 1.0 and v_ref.min() == 0.0 and v_ref.max() == 1.0
    checked = R.postproc_u8_checked(x)
    assert np.abs(q_got.astype(np.int32) - q_ref.astype(np.int32)).max() <= 1
    assert np.array_equal(q_got[checked], q_ref[checked])
    assert (~checked).mean() <= R.POSTPROC_MAX_EXCLUDED
    assert {0, 128, 255} <= set(q_ref.reshape(-1).tolist())            # -1 / -3 -> 0, 0 -> 127.5 -> 128 (half to even), 1 / 3 -> 255


def test_postproc_excluded_share_of_uniform_data():
    """The share of uniform data within 1e-4 of a half-integer of 255 v: 2e-4 of the unclamped two thirds."""
    x = np.random.default_rng(5).uniform(-1.5, 1.5, (1, 1, 1000, 1000)).astype(np.float32)
    share = (~R.postproc_u8_checked(x)).mean()
    assert 0.5e-4 < share < 3e-4


@pytest.mark.parametrize("shape", R.NHWC_SHAPES)
@pytest.mark.parametrize("dtype", ("f32", "bf16", "fp16"))
def test_nchw_to_nhwc_rounding_reference(shape, dtype):
    """torch's .to(dtype) on the CPU rounds to nearest even: bit-identical with the spelled-out rounding."""
    B, C, HW, Cpad = shape
    x = R.nhwc_input(B, C, HW)
    tdt, bits = {"f32": (torch.float32, torch.int32), "bf16": (torch.bfloat16, torch.int16), "fp16": (torch.float16, torch.int16)}[dtype]
    ref = torch.zeros(B, HW, Cpad, dtype=tdt)
    ref[:, :, :C] = torch.from_numpy(x).permute(0, 2, 1).to(tdt)
    want = R.nhwc_bits_replica(x, Cpad, dtype)
    assert np.array_equal(ref.view(bits).numpy().view(want.dtype), want)


@pytest.mark.parametrize("rows", R.LIN_ROWS)
def test_linear_backward_replica(rows):
    for in_dim in R.LIN_IN:
        for out_dim in R.LIN_OUT:
            inp = R.linear_input(rows, in_dim, out_dim)
            for flag in (0, 1):
                ref, got, bnd = (f(inp, flag) for f in (R.linear_wgrad_f64, R.linear_wgrad_f32_replica, R.linear_wgrad_bound))
                check(got[0], ref[0], bnd[0], f"wgrad dw {rows}x{in_dim}x{out_dim} silu{flag}")
                check(got[1], ref[1], bnd[1], f"wgrad db {rows}x{in_dim}x{out_dim}")
                # the contract is +=: the old values are far outside the bound of a plain "="
                assert np.any(np.abs(inp["dw0"]) > bnd[0]) and np.any(np.abs(inp["db0"]) > bnd[1])
                check(R.linear_dgrad_f32_replica(inp, flag), R.linear_dgrad_f64(inp, flag), R.linear_dgrad_bound(inp, flag),
                      f"dgrad {rows}x{in_dim}x{out_dim} pre{flag}")


def test_embedding_grad_replica():
    inp = R.embedding_input()
    ref = R.embedding_grad_f64(inp)
    check(R.embedding_grad_f32_replica(inp), ref, R.embedding_grad_bound(inp), "embedding_grad")
    absent = sorted(set(range(R.EMB["num_classes"])) - set(inp["labels"].tolist()))
    assert absent == [4] and np.array_equal(ref[4], inp["table0"][4].astype(np.float64))
    assert len(set(inp["labels"].tolist())) < len(inp["labels"])


@pytest.mark.parametrize("numel", R.GUIDANCE_APPLY_NUMEL)
def test_guidance_apply_replica(numel):
    inp = R.guidance_apply_input(numel)
    check(R.guidance_apply_f32_replica(inp), R.guidance_apply_f64(inp), R.guidance_apply_bound(inp), "guidance_apply")
