"""Kernel-level parity of the flat-buffer and time-embedding entry points on a real MI355X: raw ctypes calls against the float64
references of tests/flat_refs.py under its derived bounds (proven against an fp32 replica on the CPU by
tests/test_host_flat_refs.py, same seeds and shapes).  Every output and in-place buffer sits between canaried guard bands,
every input between NaN; a 4-byte-aligned pointer is view[1:] of a guarded tensor one element longer.

Largest error / bound measured on the MI355X, per entry point (PD_RECORD_ERRORS):
    pd_grad_norm        0.48 (of the 1 ulp allowed)      pd_adamw_ema        0.64 (small sizes 0.30)
    pd_diffusion_loss   0.51                             pd_ddim_step        0.50 (guided 0.44, through _device_step 0.18)
    pd_add_noise        0.42                             pd_postproc         0.33 (fp32 output; uint8: no mismatch)
    pd_linear_wgrad     0.44                             pd_linear_dgrad     0.32
    pd_embedding_grad   0.11                             pd_guidance_apply   0.43
    pd_nchw_to_nhwc     bit-exact
The bounds are the derived ones; none was tightened towards these figures.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import flat_refs as R
from guard_bands import guarded

pytestmark = pytest.mark.gpu

LEAD = 12345.0          # the element in front of a 4-byte-aligned view: a neighbour the kernel must not touch
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    import phendiff_amd._lib as L
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L, L.lib(), torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def ratio_ok(got, ref, bnd, what):
    from conftest import record_error
    ok, ratio = R.within(got, ref, bnd)
    record_error(ratio)
    assert ok, f"{what}: outside the bound (largest error / bound = {ratio:.3f})"


class Buf:
    """One guarded device tensor: `v` goes to the kernel.  off = 1: `v` is view[1:] of a tensor one element longer (a pointer
    that is only 4-byte aligned); the leading element must survive."""

    def __init__(self, arr, dev, name, out=False, off=0):
        t = torch.from_numpy(np.array(arr, copy=True)).reshape(-1)
        self.shape, self.off, self.out = np.shape(arr), off, out
        if off:
            t = torch.cat([torch.full((off,), LEAD, dtype=t.dtype), t])
        self.full, self.h = guarded(t, device=dev, name=name)
        self.v = self.full[off:]
        self.arm()

    def arm(self):
        (self.h.canary if self.out else self.h.poison)()
        return self

    def set(self, arr):
        self.v.copy_(torch.from_numpy(np.array(arr, copy=True)).reshape(-1))
        return self

    @property
    def ptr(self):
        return self.v.data_ptr()

    def get(self):
        return self.v.cpu().numpy().reshape(self.shape)

    def bits(self):
        return self.get().view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[self.v.element_size()])

    def check(self):
        """After a launch: surroundings untouched (outputs) and the leading element of an offset view still there."""
        if self.out:
            assert self.h.intact()
        if self.off:
            assert float(self.full[0]) == LEAD, f"{self.h.name}: the element in front of the run was overwritten"


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ================================================================================================ pd_grad_norm
class NormOut:
    def __init__(self, dev):
        self.partial = Buf(np.full(1024, NAN, dtype=np.float64), dev, "partial", out=True)       # the documented [1024] doubles
        self.norm = Buf(np.full(1, NAN, dtype=np.float32), dev, "norm_out", out=True)
        self.coef = Buf(np.full(1, NAN, dtype=np.float32), dev, "clip_coef_out", out=True)

    def run(self, env, x, n, max_norm):
        L, lib, _ = env
        L.check(lib.pd_grad_norm(x.ptr, n, self.partial.ptr, max_norm, self.norm.ptr, self.coef.ptr, stream()), "pd_grad_norm")
        torch.cuda.synchronize()
        for b in (self.partial, self.norm, self.coef, x):
            b.check()
        return self.norm.get()[0], self.coef.get()[0]


GRAD_NORM_PARAMS = [(n, 0) for n in R.GRAD_NORM_SIZES] + [(n, 1) for n in R.GRAD_NORM_MISALIGNED]


@pytest.mark.parametrize("n,off", GRAD_NORM_PARAMS)
def test_grad_norm(env, n, off):
    """Aligned (off = 0), with n4 = n // 4 16-byte groups and a stride of 262144 groups per sweep:
         1, 3           only the scalar tail (block 0)
         1027           leftover 16-byte loads + a tail of 3
         Q              every lane exactly one leftover load, no loop, no tail
         Q + 4, Q + 7   lane 0 enters the two-in-flight loop, all others take the leftover load; Q + 7 adds a tail of 3
         2Q + 1201      one two-in-flight iteration everywhere, 300 leftover loads, a tail of 1
         3Q + 5         one two-in-flight iteration, then a leftover load for every lane (+ 1 more group), a tail of 1
         4Q + 310       two two-in-flight iterations, 77 leftover loads, a tail of 2
       off = 1: the scalar fallback for a pointer that is not 16-byte aligned."""
    from conftest import record_error
    dev = env[2]
    out = NormOut(dev)
    x = Buf(R.grad_norm_input(n, "ones"), dev, "grad", off=off)
    assert x.ptr % 16 == (4 if off else 0)
    # all ones: one skipped or doubled element changes the norm
    a, _ = out.run(env, x, n, 1.0)
    b, _ = out.run(env, x, n, 1.0)
    assert a == np.float32(np.sqrt(np.float64(n))) and same_bits(a, b)
    data = R.grad_norm_input(n, "normal")
    ref = R.grad_norm_f64(data)
    x.set(data)
    for max_norm in R.GRAD_NORM_MAX_NORMS:
        nrm, coef = out.run(env, x, n, max_norm)
        nrm2, coef2 = out.run(env, x, n, max_norm)
        assert same_bits(nrm, nrm2) and same_bits(coef, coef2)
        err = abs(float(nrm) - ref) / R.ulp32(ref)
        record_error(err)
        assert err <= 1.0, f"norm {float(nrm)!r} vs {ref!r}: {err:.2f} ulp"
        want = R.clip_coef_f32(np.float32(ref), max_norm)
        if want == 1.0:
            assert coef == np.float32(1.0)          # max_norm above the norm, or inf: exactly 1
        else:
            assert abs(float(coef) - float(want)) <= 2 * R.ulp32(want)


def test_grad_norm_inf_and_nan_reach_the_norm(env):
    """n = 2Q + 1201 = 4 (2 * 262144 + 300) + 1: groups 0 .. 2 * 262144 - 1 belong to the two-in-flight loop, the next 300 to the
    leftover load, the last element to the scalar tail.  One inf in each of them must give an inf norm (the fp16 skipped-step
    decision reads exactly this), one NaN in the tail a NaN."""
    dev = env[2]
    n = 2 * R.Q + 1201
    data = R.grad_norm_input(n, "normal")
    out = NormOut(dev)
    x = Buf(data, dev, "grad")
    stride = 1024 * 256
    spots = {"last group of the two-in-flight loop": 4 * (2 * stride - 1) + 3, "leftover group": 4 * (2 * stride + 299) + 2, "scalar tail": n - 1}
    assert spots["leftover group"] < n - 1 and (n - 1) % 4 == 0
    for where, i in spots.items():
        x.v[i] = float("inf")
        nrm, coef = out.run(env, x, n, 1.0)
        assert np.isposinf(nrm) and coef == 0.0, where
        x.v[i] = float(data[i])
    x.v[n - 1] = NAN
    nrm, _ = out.run(env, x, n, 1.0)
    assert np.isnan(nrm)


# ================================================================================================ pd_adamw_ema
ADAMW_KEYS = ("param", "grad", "exp_avg", "exp_avg_sq", "ema")


def run_adamw_cases(env, numel, off, cases):
    L, lib, dev = env
    zeros = np.zeros(numel, dtype=np.float32)
    bufs = {k: Buf(zeros, dev, k, out=True, off=off) for k in ADAMW_KEYS}
    decoy = Buf(zeros, dev, "ema decoy", out=True, off=off)
    clip_buf = Buf(np.array([0.25], dtype=np.float32), dev, "clip_coef")
    for t, wd, grads, (name, clip, has_ema, zero_grad, ema_only) in cases:
        what = f"adamw_ema numel={numel} off={off} t={t} wd={wd} {grads} {name}"
        inp, h = R.adamw_input(numel, grads), R.adamw_hyper(t, wd)
        for k in ADAMW_KEYS:
            bufs[k].set(inp[k]).arm()
        decoy.set(inp["ema"]).arm()
        if clip is not None:
            clip_buf.set(np.array([clip], dtype=np.float32))
        a = L.AdamWEmaArgs(numel=numel, zero_grad=zero_grad, clip_coef=clip_buf.ptr if clip is not None else None,
                           param=bufs["param"].ptr, grad=bufs["grad"].ptr, exp_avg=bufs["exp_avg"].ptr,
                           exp_avg_sq=bufs["exp_avg_sq"].ptr, ema=bufs["ema"].ptr if has_ema else None, ema_only=ema_only,
                           **{k: float(v) for k, v in h.items()})
        L.check(lib.pd_adamw_ema(C.byref(a), stream()), "pd_adamw_ema")
        torch.cuda.synchronize()
        for b in list(bufs.values()) + [decoy]:
            b.check()
        ref, bnd = R.adamw_f64(inp, h, clip, ema_only), R.adamw_bound(inp, h, clip, ema_only)
        for k in ("param", "exp_avg", "exp_avg_sq"):
            if ema_only:
                assert same_bits(bufs[k].get(), inp[k]), f"{what}: {k} touched by an EMA-only pass"
            else:
                ratio_ok(bufs[k].get(), ref[k], bnd[k], f"{what} {k}")
        if has_ema:
            ratio_ok(bufs["ema"].get(), ref["ema"], bnd["ema"], f"{what} ema")
        else:
            # ema = NULL writes nowhere: the shadow buffers that were NOT handed over are as they were
            assert same_bits(bufs["ema"].get(), inp["ema"]) and same_bits(decoy.get(), inp["ema"]), what
        if zero_grad:
            assert not bufs["grad"].bits().any(), f"{what}: gradient not zeroed exactly"
        else:
            assert same_bits(bufs["grad"].get(), inp["grad"]), f"{what}: gradient touched"


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("numel", R.ADAMW_SMALL)
def test_adamw_ema_small(env, numel, off):
    """1: one lane; 255 / 257: one short of, one past a block.  off = 1: all five pointers one element into their buffers, as
    FlatAdamWEMA.step launches a trainable run at data_ptr() + 4 * off -- the neighbours on both sides are watched.
    Variants: clip_coef NULL / a device scalar 0.25, ema NULL, zero_grad 0 / 1, ema_only 1."""
    run_adamw_cases(env, numel, off, R.adamw_cases_small())


def test_adamw_ema_grid_stride_second_sweep(env):
    """2 097 152 + 773 elements: the grid is capped at 8192 blocks, the last 773 elements belong to the second sweep."""
    run_adamw_cases(env, R.ADAMW_LARGE, 0, R.adamw_cases_large())


# ================================================================================================ pd_diffusion_loss
@pytest.mark.parametrize("pred", R.PRED_TYPES)
@pytest.mark.parametrize("shape", R.LOSS_SHAPES)
def test_diffusion_loss(env, shape, pred):
    """(3, 75): sample boundaries at 75 and 150, multiples of nothing; (1, 1); (3, 100 003): 300 009 > 262 144 elements, the
    grid-stride second sweep.  grad_out = NULL and grad_scale = 65536 against the plain run, bit for bit."""
    L, lib, dev = env
    B, per = shape
    inp = R.loss_input(B, per)
    ins = {k: Buf(v, dev, k) for k, v in inp.items()}
    grad = Buf(np.full((B, per), NAN, dtype=np.float32), dev, "grad_out", out=True)
    partial = Buf(np.full(1024, NAN, dtype=np.float64), dev, "partial", out=True)
    loss = Buf(np.full(1, NAN, dtype=np.float32), dev, "loss_out", out=True)

    def run(grad_scale, with_grad=True):
        a = L.LossArgs(numel=B * per, per_sample=per, pred_type=pred, grad_scale=grad_scale, grad_out=grad.ptr if with_grad else None,
                       partial=partial.ptr, loss_out=loss.ptr, **{k: b.ptr for k, b in ins.items()})
        L.check(lib.pd_diffusion_loss(C.byref(a), stream()), "pd_diffusion_loss")
        torch.cuda.synchronize()
        for b in (grad, partial, loss):
            b.check()
        return loss.get()[0], grad.get()

    from conftest import record_error
    l_ref, g_ref = R.loss_f64(inp, pred)
    l_b, g_b = R.loss_bound(inp, pred)
    l1, g1 = run(1.0)
    record_error(abs(float(l1) - l_ref) / l_b)
    assert abs(float(l1) - l_ref) <= l_b, f"loss {float(l1)!r} vs {l_ref!r} (bound {l_b:.3e})"
    ratio_ok(g1, g_ref, g_b, f"loss gradient {shape} pred={pred}")
    l2, g2 = run(1.0)
    assert same_bits(l1, l2) and same_bits(g1, g2)
    grad.set(np.full((B, per), NAN, dtype=np.float32))
    l3, g3 = run(1.0, with_grad=False)
    assert same_bits(l1, l3) and np.isnan(g3).all(), "grad_out = NULL: same loss, nothing written"
    l4, g4 = run(65536.0)
    assert same_bits(l1, l4) and same_bits(g4, g1 * np.float32(65536.0))


# ================================================================================================ pd_ddim_step
def run_ddim_cases(env, inp, guidance, what):
    L, lib, dev = env
    B, per = inp["sample"].shape
    nan = np.full((B, per), NAN, dtype=np.float32)
    x, o, un = (Buf(inp[k], dev, k) for k in ("sample", "model_out", "uncond_out"))
    prev, x0, inplace = Buf(nan, dev, "prev_sample", out=True), Buf(nan, dev, "pred_x0", out=True), Buf(nan, dev, "sample (in place)", out=True)
    w = Buf(np.asarray(guidance[1], dtype=np.float32), dev, "w") if guidance else None
    coefs = R.ddim_coefficients()
    for ti, pred, clip, ucm in R.ddim_cases():
        sa, sb, sap, dc = (float(c) for c in coefs[ti])
        tag = f"{what} timestep#{ti} pred={pred} clip={clip} use_clipped={ucm}"

        def run(sample, out, want_x0):
            a = L.DdimStepArgs(numel=B * per, per_sample=per, pred_type=pred, clip=clip, clip_range=R.CLIP_RANGE,
                               use_clipped_model_output=ucm, sqrt_a=sa, sqrt_b=sb, sqrt_ap=sap, dir_coef=dc, sample=sample.ptr,
                               model_out=o.ptr, uncond_out=un.ptr if guidance else None, w=w.ptr if guidance else None,
                               w_per_sample=int(bool(guidance) and len(guidance[1]) > 1), guidance_cfg=guidance[0] if guidance else 0,
                               prev_sample=out.ptr, pred_x0=x0.ptr if want_x0 else None)
            L.check(lib.pd_ddim_step(C.byref(a), stream()), "pd_ddim_step")
            torch.cuda.synchronize()
            for b in (prev, x0, inplace):
                b.check()
            return out.get()

        prev.set(nan), x0.set(nan)
        got = run(x, prev, True)
        got_x0 = x0.get()
        (p_ref, x0_ref), (p_b, x0_b) = R.ddim_f64(inp, coefs[ti], pred, clip, ucm, guidance), R.ddim_bound(inp, coefs[ti], pred, clip, ucm, guidance)
        ratio_ok(got, p_ref, p_b, tag + " prev_sample")
        ratio_ok(got_x0, x0_ref, x0_b, tag + " pred_x0")
        # pred_x0 = NULL: the same prev_sample, and pred_x0 is not written
        prev.set(nan), x0.set(nan)
        assert same_bits(run(x, prev, False), got) and np.isnan(x0.get()).all(), tag + " pred_x0 = NULL"
        # prev_sample == sample, as the captured img2img plans run it
        inplace.set(inp["sample"])
        assert same_bits(run(inplace, inplace, False), got), tag + " in place"


@pytest.mark.parametrize("numel", R.DDIM_NUMEL)
def test_ddim_step(env, numel):
    """1, 3: only the cnt < 4 tail; 5, 1023, 1025: 4-vectors and a tail; 1024: exactly one full block; 1025: a second block that
    holds only the tail.  Prediction types x clip x use_clipped_model_output at the first (sqrt_a == 0), a middle and the last
    timestep of the 50-step schedule."""
    run_ddim_cases(env, R.ddim_input(1, numel), None, f"ddim_step numel={numel}")


@pytest.mark.parametrize("guidance", R.DDIM_GUIDANCE, ids=lambda g: f"{'cfg' if g[0] else 'imagen'}-w{len(g[1])}-{g[1][0]}")
def test_ddim_step_guided(env, guidance):
    """B = 3, per_sample = 75: 4-vectors straddle the sample boundaries at 75 and 150 (per_sample % 4 == 3) and 225 % 4 == 1 leaves
    a tail.  Both equations, one weight (w > 1, 0 < w < 1) or three different per-sample weights."""
    run_ddim_cases(env, R.ddim_input(*R.DDIM_GUIDED), guidance, f"ddim_step guided {guidance}")


@pytest.mark.parametrize("how", ("fp32", "bf16", "channel_slice"))
def test_device_step_unconditional_prediction_dtype_and_layout(env, how):
    """DDIMScheduler._device_step reads the unconditional prediction as dense fp32 whatever it is handed: an fp32 tensor, the same
    values in bf16, a non-contiguous channel slice.  Against the float64 guidance reference of the values actually passed."""
    import phendiff_amd as P
    dev = env[2]
    B, Cc, H, W = 3, 4, 5, 5
    inp = R.ddim_input(B, Cc * H * W)
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    sched.set_timesteps(50)
    t = sched.timesteps[25]
    x, o, un = (torch.from_numpy(inp[k]).reshape(B, Cc, H, W).to(dev) for k in ("sample", "model_out", "uncond_out"))
    if how == "bf16":
        un = un.to(torch.bfloat16)
    elif how == "channel_slice":
        wide = torch.full((B, Cc + 2, H, W), NAN, device=dev)
        wide[:, 1:1 + Cc] = un
        un = wide[:, 1:1 + Cc]
        assert not un.is_contiguous()
    passed = dict(inp, uncond_out=un.float().cpu().numpy().reshape(B, -1))
    prev, x0 = sched._device_step(o, t, x, 0.0, False, None, None, uncond_output=un, w=2.5, guidance_cfg=False)
    torch.cuda.synchronize()
    coef = tuple(np.float32(c) for c in sched.step_coefficients(t)[:4])
    (p_ref, x0_ref), (p_b, x0_b) = R.ddim_f64(passed, coef, 2, 1, 0, (0, (2.5,))), R.ddim_bound(passed, coef, 2, 1, 0, (0, (2.5,)))
    ratio_ok(prev.cpu().numpy().reshape(B, -1), p_ref, p_b, f"_device_step {how} prev_sample")
    ratio_ok(x0.cpu().numpy().reshape(B, -1), x0_ref, x0_b, f"_device_step {how} pred_x0")


# ================================================================================================ pd_add_noise
@pytest.mark.parametrize("velocity", (0, 1))
@pytest.mark.parametrize("shape", R.ADD_NOISE_SHAPES)
def test_add_noise(env, shape, velocity):
    """(3, 75): sample boundaries inside one block; (2, 257): a boundary one past a block, 514 elements = a third, partial block."""
    L, lib, dev = env
    B, per = shape
    inp = R.add_noise_input(B, per)
    ins = {k: Buf(v, dev, k) for k, v in inp.items()}
    out = Buf(np.full((B, per), NAN, dtype=np.float32), dev, "out", out=True)
    a = L.AddNoiseArgs(numel=B * per, per_sample=per, velocity=velocity, out=out.ptr, **{k: b.ptr for k, b in ins.items()})
    L.check(lib.pd_add_noise(C.byref(a), stream()), "pd_add_noise")
    torch.cuda.synchronize()
    out.check()
    ratio_ok(out.get(), R.add_noise_f64(inp, velocity), R.add_noise_bound(inp, velocity), f"add_noise {shape} velocity={velocity}")


# ================================================================================================ pd_postproc
@pytest.mark.parametrize("outputs", ("f32", "u8", "both"))
@pytest.mark.parametrize("hw", R.POSTPROC_HW)
@pytest.mark.parametrize("Cc", R.POSTPROC_C)
def test_postproc(env, Cc, hw, outputs):
    """5 x 7: 70 pixels, a partial block; 16 x 16: 512 pixels, two full blocks; 17 x 16: 544 pixels, a third, partial block and an
    image boundary inside the second.  Uniform [-1.5, 1.5] (both clamps) and the exact values -1, 0, 1, +-3."""
    L, lib, dev = env
    H, W = hw
    x = R.postproc_input(Cc, H, W)
    xin = Buf(x, dev, "x")
    shape = (R.POSTPROC_B, H, W, Cc)
    f32 = Buf(np.full(shape, NAN, dtype=np.float32), dev, "out_f32", out=True)
    u8 = Buf(np.full(shape, 0x5A, dtype=np.uint8), dev, "out_u8", out=True)
    a = L.PostprocArgs(B=R.POSTPROC_B, C=Cc, H=H, W=W, x=xin.ptr, out_f32=f32.ptr if outputs != "u8" else None,
                       out_u8=u8.ptr if outputs != "f32" else None)
    L.check(lib.pd_postproc(C.byref(a), stream()), "pd_postproc")
    torch.cuda.synchronize()
    f32.check(), u8.check()
    v_ref, q_ref = R.postproc_f64(x)
    if outputs == "u8":
        assert np.isnan(f32.get()).all()
    else:
        got = f32.get()
        ratio_ok(got, v_ref, R.postproc_bound(x), f"postproc fp32 C={Cc} {hw}")
        assert got.min() >= 0.0 and got.max() <= 1.0
    if outputs == "f32":
        assert (u8.get() == 0x5A).all()
    else:
        q = u8.get()
        checked = R.postproc_u8_checked(x)
        assert (~checked).mean() <= R.POSTPROC_MAX_EXCLUDED
        assert np.abs(q.astype(np.int32) - q_ref.astype(np.int32)).max() <= 1
        assert np.array_equal(q[checked], q_ref[checked])


# ================================================================================================ pd_nchw_to_nhwc
TORCH_DT = {"f32": (0, torch.float32, torch.int32), "bf16": (1, torch.bfloat16, torch.int16), "fp16": (2, torch.float16, torch.int16)}


def run_nhwc(env, shape, dtype):
    L, lib, dev = env
    B, Cc, HW, Cpad = shape
    code, tdt, bits = TORCH_DT[dtype]
    x = R.nhwc_input(B, Cc, HW)
    xin = Buf(x, dev, "x")
    # the output starts as all-ones bytes (NaN in every dtype): the zeros of channels C .. Cpad - 1 have to be written
    out_t, h = guarded(torch.full((B, HW, Cpad), -1, dtype=bits), device=dev, name="out")
    h.canary()
    a = L.NchwToNhwcArgs(dtype=code, B=B, C=Cc, HW=HW, Cpad=Cpad, x=xin.ptr, out=out_t.data_ptr())
    L.check(lib.pd_nchw_to_nhwc(C.byref(a), stream()), "pd_nchw_to_nhwc")
    torch.cuda.synchronize()
    assert h.intact()
    ref = torch.zeros(B, HW, Cpad, dtype=tdt)
    ref[:, :, :Cc] = torch.from_numpy(x).permute(0, 2, 1).to(tdt)         # rounds to nearest even, as pd_common.h states
    got = out_t.cpu()
    assert torch.equal(got, ref.view(bits)), f"nchw_to_nhwc {shape} {dtype}: not bit-exact"
    assert not got[:, :, Cc:].any(), "padding channels are not exact zeros"


@pytest.mark.parametrize("dtype", ("f32", "bf16", "fp16"))
@pytest.mark.parametrize("shape", R.NHWC_SHAPES)
def test_nchw_to_nhwc(env, shape, dtype):
    """(2, 3, 35, 8): C < 8, one 8-channel piece, 5 zero channels; (1, 4, 64, 32): three all-zero pieces of four;
    (2, 9, 300, 16): C one past a piece, the second piece is 1 value + 7 zeros, two samples."""
    run_nhwc(env, shape, dtype)


def test_nchw_to_nhwc_grid_stride(env):
    """(1, 3, 2 100 000, 16) bf16: 4 200 000 work items, more than 16384 blocks x 256 lanes: the grid-stride second sweep."""
    run_nhwc(env, R.NHWC_LARGE, "bf16")


# ================================================================================================ fp32 time-embedding backward
@pytest.mark.parametrize("in_dim", R.LIN_IN)
@pytest.mark.parametrize("rows", R.LIN_ROWS)
def test_linear_wgrad_dgrad(env, rows, in_dim):
    """in_dim 1 / 31: a masked 32-wide chunk; 33: a full chunk and a chunk of one; 96: three full chunks.  out_dim 1 / 7: fewer
    outputs than the 8 groups folded through LDS; 9: one group gets two; 130: 16 or 17 each.  dw / db are pre-filled and must come
    back as old + gradient (+=); dx is pre-filled with NaN and written with =.  Each run twice, bit-identical."""
    L, lib, dev = env
    for out_dim in R.LIN_OUT:
        inp = R.linear_input(rows, in_dim, out_dim)
        dy, x, w, pre = (Buf(inp[k], dev, k) for k in ("dy", "x", "w", "pre"))
        dw, db = Buf(inp["dw0"], dev, "dw", out=True), Buf(inp["db0"], dev, "db", out=True)
        dx = Buf(np.full((rows, in_dim), NAN, dtype=np.float32), dev, "dx", out=True)
        what = f"rows={rows} in={in_dim} out={out_dim}"
        for x_silu in (0, 1):
            for with_db in (0, 1):
                res = []
                for _ in range(2):
                    dw.set(inp["dw0"]), db.set(inp["db0"])
                    a = L.LinearWgradArgs(rows=rows, in_dim=in_dim, out_dim=out_dim, x_silu=x_silu, dy=dy.ptr, x=x.ptr, dw=dw.ptr,
                                          db=db.ptr if with_db else None)
                    L.check(lib.pd_linear_wgrad(C.byref(a), stream()), "pd_linear_wgrad")
                    torch.cuda.synchronize()
                    dw.check(), db.check()
                    res.append((dw.get(), db.get()))
                assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
                (dw_ref, db_ref), (dw_b, db_b) = R.linear_wgrad_f64(inp, x_silu), R.linear_wgrad_bound(inp, x_silu)
                ratio_ok(res[0][0], dw_ref, dw_b, f"linear_wgrad dw {what} silu={x_silu}")
                if with_db:
                    ratio_ok(res[0][1], db_ref, db_b, f"linear_wgrad db {what}")
                else:
                    assert same_bits(res[0][1], inp["db0"]), "db = NULL: nothing written"
        for with_pre in (0, 1):
            res = []
            for _ in range(2):
                dx.set(np.full((rows, in_dim), NAN, dtype=np.float32))
                a = L.LinearDgradArgs(rows=rows, in_dim=in_dim, out_dim=out_dim, dy=dy.ptr, w=w.ptr, pre=pre.ptr if with_pre else None, dx=dx.ptr)
                L.check(lib.pd_linear_dgrad(C.byref(a), stream()), "pd_linear_dgrad")
                torch.cuda.synchronize()
                dx.check()
                res.append(dx.get())
            assert same_bits(res[0], res[1])
            ratio_ok(res[0], R.linear_dgrad_f64(inp, with_pre), R.linear_dgrad_bound(inp, with_pre), f"linear_dgrad {what} pre={with_pre}")


def test_embedding_grad(env):
    """7 classes x 33 values = 231 lanes of one block; int64 labels with repeats, class 4 absent: its row stays bitwise as it was."""
    L, lib, dev = env
    inp = R.embedding_input()
    labels, d = Buf(inp["labels"], dev, "labels"), Buf(inp["d"], dev, "d")
    table = Buf(inp["table0"], dev, "dtable", out=True)
    res = []
    for _ in range(2):
        table.set(inp["table0"])
        a = L.EmbeddingGradArgs(rows=R.EMB["rows"], dim=R.EMB["dim"], num_classes=R.EMB["num_classes"], labels=labels.ptr, d=d.ptr, dtable=table.ptr)
        L.check(lib.pd_embedding_grad(C.byref(a), stream()), "pd_embedding_grad")
        torch.cuda.synchronize()
        table.check()
        res.append(table.get())
    assert same_bits(res[0], res[1])
    ratio_ok(res[0], R.embedding_grad_f64(inp), R.embedding_grad_bound(inp), "embedding_grad")
    assert same_bits(res[0][4], inp["table0"][4])


# ================================================================================================ pd_guidance_apply
@pytest.mark.parametrize("numel", R.GUIDANCE_APPLY_NUMEL)
def test_guidance_apply(env, numel):
    """1; 257: one past a block; 4096 * 256 + 300: past the 4096-block grid cap, 300 elements in the second sweep.  out == x in place
    (as img2img.py runs it) bit for bit as out of place."""
    L, lib, dev = env
    inp = R.guidance_apply_input(numel)
    x, gd, gu = Buf(inp["x"], dev, "x", out=True), Buf(inp["g_direct"], dev, "g_direct"), Buf(inp["g_unet"], dev, "g_unet")
    out = Buf(np.full(numel, NAN, dtype=np.float32), dev, "out", out=True)

    def run(dst):
        a = L.GuidanceApplyArgs(numel=numel, scale=R.GUIDANCE_APPLY_SCALE, x=x.ptr, g_direct=gd.ptr, g_unet=gu.ptr, out=dst.ptr)
        L.check(lib.pd_guidance_apply(C.byref(a), stream()), "pd_guidance_apply")
        torch.cuda.synchronize()
        x.check(), out.check()
        return dst.get()

    got = run(out)
    assert same_bits(x.get(), inp["x"])
    ratio_ok(got, R.guidance_apply_f64(inp), R.guidance_apply_bound(inp), f"guidance_apply numel={numel}")
    assert same_bits(run(x), got)
