"""The multistep solvers on a real MI355X.

  * pd_multistep_step, raw ctypes calls, against the float64 reference of tests/multistep_refs.py under its derived bound (proven against
    an fp32 replica on the CPU by tests/test_host_multistep.py, same seeds and shapes); every output between canaried guard bands, every
    input between NaN (tests/guard_bands.py);
  * the thresholded step pd_ddim_raw_x0 -> pd_abs_quantile -> pd_multistep_step;
  * the eager scheduler loops on the device against the float64 reference trajectory under the accumulated bound;
  * pipeline, inversion and DDIB with the multistep pair against the oracle UNet driven by the float64 reference schedulers, under the
    tolerances tests/test_gpu_unet_ddib.py applies to the same model, dtype and step counts with DDIM;
  * the captured runners: captured = enqueued = eager, bit for bit; replays do not depend on what the history buffers hold.

Largest error / bound measured on the MI355X (PD_RECORD_ERRORS):
    pd_multistep_step   0.53 (guided 0.44, grid stride 0.48)     thresholded step    0.41
    eager loops         0.25 (of the accumulated bound)
Relative L2 against the oracle: inversion and DDIB 1.2e-6 (tolerance 2e-5), pipeline with guidance 2.0e-6 (tolerance 2e-4).
The bounds are the derived ones; none was tightened towards these figures."""
import ctypes as C

import numpy as np
import pytest
import torch

import flat_refs as R
import multistep_refs as M
from guard_bands import guarded

pytestmark = pytest.mark.gpu

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


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


class Buf:
    """One guarded device tensor: inputs sit between NaN, outputs between canaries."""

    def __init__(self, arr, dev, name, out=False):
        self.shape, self.out = np.shape(arr), out
        self.v, self.h = guarded(torch.from_numpy(np.array(arr, copy=True)).reshape(-1), device=dev, name=name)
        (self.h.canary if out else self.h.poison)()

    def set(self, arr):
        self.v.copy_(torch.from_numpy(np.array(arr, copy=True)).reshape(-1))
        return self

    ptr = property(lambda self: self.v.data_ptr())

    def get(self):
        return self.v.cpu().numpy().reshape(self.shape)

    def check(self):
        if self.out:
            assert self.h.intact()


# ================================================================================================ pd_multistep_step
def run_kernel_cases(env, inp, guidance, what):
    L, lib, dev = env
    B, per = inp["sample"].shape
    nan = np.full((B, per), NAN, dtype=np.float32)
    x, o, un, hin = (Buf(inp[k], dev, k) for k in ("sample", "model_out", "uncond_out", "hist_in"))
    hnan = Buf(nan, dev, "hist_in (NaN)")
    prev, x0, hout, inplace = (Buf(nan, dev, k, out=True) for k in ("prev_sample", "pred_x0", "hist_out", "sample (in place)"))
    w = Buf(np.asarray(guidance[1], dtype=np.float32), dev, "w") if guidance else None
    coefs = M.schedule_coefficients()
    assert coefs[M.DATA][0][0] == 0 and coefs[M.DATA][1][4] != 0 and coefs[M.NOISE][1][4] != 0 and coefs[M.DATA][2][2:] == (0, 1, 0)
    for form, ti, pred, clip in M.multistep_cases():
        natural = coefs[form][ti]
        for coef in ([natural] if natural[4] == 0 else [natural, natural[:4] + (np.float32(0.0),)]):
            tag = f"{what} form={form} step#{ti} pred={pred} clip={clip} c={float(coef[4]):g}"
            want_x0_possible = form == M.DATA

            def run(sample, out, want_x0, hist):
                a = L.MultistepStepArgs(numel=B * per, per_sample=per, pred_type=pred, form=form, clip=clip, clip_range=R.CLIP_RANGE,
                                        sqrt_a=float(coef[0]), sqrt_b=float(coef[1]), a=float(coef[2]), b=float(coef[3]), c=float(coef[4]),
                                        sample=sample.ptr, model_out=o.ptr, uncond_out=un.ptr if guidance else None,
                                        w=w.ptr if guidance else None, w_per_sample=int(bool(guidance) and len(guidance[1]) > 1),
                                        guidance_cfg=guidance[0] if guidance else 0, hist_in=hist.ptr if hist is not None else None,
                                        prev_sample=out.ptr, hist_out=hout.ptr, pred_x0=x0.ptr if want_x0 else None, quantile=None,
                                        sample_max_value=0.0)
                hout.set(nan)
                L.check(lib.pd_multistep_step(C.byref(a), stream()), "pd_multistep_step")
                torch.cuda.synchronize()
                for b in (prev, x0, hout, inplace):
                    b.check()
                return out.get(), hout.get()

            prev.set(nan), x0.set(nan)
            got, got_m = run(x, prev, want_x0_possible, hin)
            (p_ref, m_ref), (p_b, m_b) = M.multistep_f64(inp, coef, form, pred, clip, guidance), M.multistep_bound(inp, coef, form, pred, clip, guidance)
            ratio_ok(got, p_ref, p_b, tag + " prev_sample")
            ratio_ok(got_m, m_ref, m_b, tag + " hist_out")          # (every element written: nothing of the NaN fill is inside a bound)
            if want_x0_possible:
                assert same_bits(x0.get(), got_m), tag + " pred_x0 = hist_out"
                # pred_x0 = NULL: the same outputs, and pred_x0 is not written
                prev.set(nan), x0.set(nan)
                p2, m2 = run(x, prev, False, hin)
                assert same_bits(p2, got) and same_bits(m2, got_m) and np.isnan(x0.get()).all(), tag + " pred_x0 = NULL"
            if coef[4] == 0:
                # a first-order step does not read the history: NaN there, or no buffer at all, changes not one bit
                for hist in (hnan, None):
                    prev.set(nan)
                    p2, m2 = run(x, prev, False, hist)
                    assert same_bits(p2, got) and same_bits(m2, got_m), tag + (" hist_in = NaN" if hist is not None else " hist_in = NULL")
            # prev_sample == sample, as the captured trajectories run it
            inplace.set(inp["sample"])
            p2, m2 = run(inplace, inplace, False, hin)
            assert same_bits(p2, got) and same_bits(m2, got_m), tag + " in place"


@pytest.mark.parametrize("numel", R.DDIM_NUMEL)
def test_multistep_step(env, numel):
    """1, 3: only the cnt < 4 tail; 5, 1023, 1025: 4-vectors and a tail; 1024: exactly one full block; 1025: a second block that holds
    only the tail.  Both forms x prediction types x clip at the first (sqrt_a == 0; c == 0), a middle (c != 0, and again with c = 0) and
    the last step ((0, 1, 0)) of the 50-step schedule and of its inverse."""
    run_kernel_cases(env, M.multistep_input(1, numel), None, f"multistep numel={numel}")


@pytest.mark.parametrize("guidance", R.DDIM_GUIDANCE, ids=lambda g: f"{'cfg' if g[0] else 'imagen'}-w{len(g[1])}-{g[1][0]}")
def test_multistep_step_guided(env, guidance):
    """B = 3, per_sample = 75: 4-vectors straddle the sample boundaries and 225 % 4 == 1 leaves a tail."""
    run_kernel_cases(env, M.multistep_input(*R.DDIM_GUIDED), guidance, f"multistep guided {guidance}")


def test_multistep_step_grid_stride(env):
    """1024 x 1024 + 1029 elements: the 1024-block grid walks a second sweep of one full block, one partial one and a one-element tail."""
    L, lib, dev = env
    n = 1024 * 1024 + 1029
    inp = M.multistep_input(1, n)
    coef = M.schedule_coefficients()[M.DATA][1]
    x, o, hin = (Buf(inp[k], dev, k) for k in ("sample", "model_out", "hist_in"))
    nan = np.full((1, n), NAN, dtype=np.float32)
    prev, hout = Buf(nan, dev, "prev_sample", out=True), Buf(nan, dev, "hist_out", out=True)
    a = L.MultistepStepArgs(numel=n, per_sample=n, pred_type=2, form=0, clip=1, clip_range=R.CLIP_RANGE, sqrt_a=float(coef[0]),
                            sqrt_b=float(coef[1]), a=float(coef[2]), b=float(coef[3]), c=float(coef[4]), sample=x.ptr, model_out=o.ptr,
                            hist_in=hin.ptr, prev_sample=prev.ptr, hist_out=hout.ptr)
    L.check(lib.pd_multistep_step(C.byref(a), stream()), "pd_multistep_step")
    torch.cuda.synchronize()
    prev.check(), hout.check()
    (p_ref, m_ref), (p_b, m_b) = M.multistep_f64(inp, coef, 0, 2, 1), M.multistep_bound(inp, coef, 0, 2, 1)
    ratio_ok(prev.get(), p_ref, p_b, "grid stride prev_sample")
    ratio_ok(hout.get(), m_ref, m_b, "grid stride hist_out")


# ================================================================================================ the thresholded step
@pytest.mark.parametrize("guidance", (None, R.DDIM_GUIDANCE[2]), ids=("plain", "imagen-w3"))
@pytest.mark.parametrize("pred", R.PRED_TYPES)
def test_thresholded_step(env, pred, guidance):
    """pd_ddim_raw_x0 -> pd_abs_quantile -> pd_multistep_step on (3, 75): against float64 given the device's quantiles; the x0 that is
    thresholded is bit for bit the raw x0 the quantile was taken of; and with first-order coefficients the update is, within the
    bounds, pd_ddim_step_threshold's with use_clipped_model_output (DDIM with eps from the thresholded x0: a x + b x0 is that)."""
    import threshold_refs as T
    from phendiff_amd.schedulers import quantile_rank
    L, lib, dev = env
    B, per = R.DDIM_GUIDED
    inp = M.multistep_input(B, per)
    for k in ("sample", "model_out", "uncond_out"):
        inp[k] = inp[k] * np.float32(1.5)                  # (quantiles of |x0| on both sides of 1 and of sample_max_value)
    nan = np.full((B, per), NAN, dtype=np.float32)
    x, o, un, hin = (Buf(inp[k], dev, k) for k in ("sample", "model_out", "uncond_out", "hist_in"))
    prev, hout, raw, prev_d, x0_d = (Buf(nan, dev, k, out=True) for k in ("prev_sample", "hist_out", "x0_raw", "ddim prev", "ddim x0"))
    q = Buf(np.full(B, NAN, dtype=np.float32), dev, "quantile", out=True)
    ws = torch.empty(lib.pd_abs_quantile_workspace(B, per), dtype=torch.uint8, device=dev)
    w = Buf(np.asarray(guidance[1], dtype=np.float32), dev, "w") if guidance else None
    lo, hi, wgt = quantile_rank(per, 0.9)
    qa = L.AbsQuantileArgs(B=B, n=per, rank_lo=lo, rank_hi=hi, weight=wgt, x=raw.ptr, out=q.ptr, workspace=ws.data_ptr())
    ddim = R.ddim_coefficients()
    for ti, coef in enumerate(M.schedule_coefficients()[M.DATA]):
        sa, sb, sap, dc = (float(v) for v in ddim[ti])
        first_order = (np.float32(sa), np.float32(sb), np.float32(dc / sb), np.float32(sap - dc * sa / sb), np.float32(0.0))
        common = dict(numel=B * per, per_sample=per, pred_type=pred, sample=x.ptr, model_out=o.ptr, uncond_out=un.ptr if guidance else None,
                      w=w.ptr if guidance else None, w_per_sample=int(bool(guidance)), guidance_cfg=guidance[0] if guidance else 0)
        outs = {}
        for name, cf in (("second", coef), ("first", first_order)):
            # (each with its own sqrt_a / sqrt_b in both structs: the scheduler's float64 roots and DDIM's fp32 ones may differ in the last bit)
            ta = L.DdimStepThresholdArgs(use_clipped_model_output=1, sqrt_a=float(cf[0]), sqrt_b=float(cf[1]), sqrt_ap=sap, dir_coef=dc,
                                         prev_sample=prev_d.ptr, pred_x0=x0_d.ptr, quantile=q.ptr, sample_max_value=M.SAMPLE_MAX_VALUE, **common)
            ma = L.MultistepStepArgs(form=0, clip=1, clip_range=R.CLIP_RANGE, sqrt_a=float(cf[0]), sqrt_b=float(cf[1]), a=float(cf[2]),
                                     b=float(cf[3]), c=float(cf[4]),
                                     hist_in=hin.ptr, prev_sample=prev.ptr, hist_out=hout.ptr, quantile=q.ptr,
                                     sample_max_value=M.SAMPLE_MAX_VALUE, **common)
            L.check(lib.pd_ddim_raw_x0(C.byref(ta), raw.ptr, stream()), "pd_ddim_raw_x0")
            L.check(lib.pd_abs_quantile(C.byref(qa), stream()), "pd_abs_quantile")
            L.check(lib.pd_multistep_step(C.byref(ma), stream()), "pd_multistep_step")
            L.check(lib.pd_ddim_step_threshold(C.byref(ta), stream()), "pd_ddim_step_threshold")
            torch.cuda.synchronize()
            for b in (prev, hout, raw, prev_d, x0_d, q):
                b.check()
            qs = q.get()
            tag = f"thresholded step#{ti} pred={pred} {name}"
            if float(cf[0]) != 0 or pred != 0:
                assert np.isfinite(qs).all() and same_bits(qs, T.quantile_numpy(raw.get(), 0.9)), tag
            (p_ref, m_ref), (p_b, m_b) = (f(inp, cf, M.DATA, pred, 0, guidance, qs) for f in (M.multistep_f64, M.multistep_bound))
            ratio_ok(prev.get(), p_ref, p_b, tag + " prev_sample")
            ratio_ok(hout.get(), m_ref, m_b, tag + " hist_out")
            # the x0 thresholded here is the raw x0 of the first launch, thresholded: the very bits pd_ddim_step_threshold makes of it
            assert same_bits(hout.get(), x0_d.get()), tag + " thresholded x0"
            outs[name] = prev.get()
        # first order = DDIM from the thresholded x0: both within their own bound of float64, whose two formulas differ by the one
        # rounding of (a, b) = (dir / sqrt_b, sqrt_ap - dir sqrt_a / sqrt_b) to fp32
        tinp = dict(inp, quantile=qs)
        d_ref, _, _ = T.step_f64(tinp, ddim[ti], pred, 1, M.SAMPLE_MAX_VALUE, guidance)
        d_b, _, _ = T.step_bound(tinp, ddim[ti], pred, 1, M.SAMPLE_MAX_VALUE, guidance)
        ratio_ok(prev_d.get(), d_ref, d_b, f"thresholded step#{ti} pred={pred} pd_ddim_step_threshold")
        p_b1, _ = M.multistep_bound(inp, first_order, M.DATA, pred, 0, guidance, qs)
        coef_round = R.U * (abs(float(first_order[2])) * np.abs(inp["sample"].astype(np.float64)) + abs(float(first_order[3])) * np.abs(m_ref))
        ratio_ok(outs["first"], prev_d.get().astype(np.float64), p_b1 + d_b + coef_round, f"thresholded step#{ti} pred={pred} first order vs DDIM")


# ================================================================================================ eager scheduler loops
ANALYTIC = dict(num_train_timesteps=1000, beta_schedule="scaled_linear", beta_start=1e-4, beta_end=0.02, timestep_spacing="leading")


def test_eager_loops_on_the_analytic_model(env):
    """S = 20 on (2, 3, 8, 8): the sampler from the exact flow at its first level, the inversion from clean samples, and the round trip,
    with the closed-form noise prediction evaluated by torch on the device's own state.  Every state of the way within the accumulated
    bound of the float64 reference trajectory (tests/multistep_refs.py: loop_bound)."""
    import phendiff_amd as P
    dev = env[2]
    fwd = P.DPMSolverMultistepScheduler(**ANALYTIC)
    inv = P.DPMSolverMultistepInverseScheduler.from_config(fwd.config)
    fwd.set_timesteps(20), inv.set_timesteps(20)
    z = R.normal(R.rng(12), 2, 3, 8, 8).astype(np.float64)

    def loop(sched, form, start, ref_start=None, E0=None):
        coefs = [sched.multistep_coefficients(i) for i in range(len(sched.timesteps))]
        ref_start = start.astype(np.float64) if ref_start is None else ref_start
        xs, ms = M.ref_loop(ref_start, M.analytic_eps_rounded, sched.timesteps.tolist(), sched.levels, coefs, form)
        bnds = M.loop_bound(xs, ms, sched.levels, coefs, form, E0)
        x = torch.from_numpy(start).to(dev)
        for i, t in enumerate(sched.timesteps):
            c1, c2 = M.analytic_constants(sched.levels[i])
            out = sched.step((x - c1) * c2, t, x)
            x = out.prev_sample
            ratio_ok(x.cpu().numpy(), xs[i + 1], bnds[i], f"form {form} step {i}")
            if form == M.DATA:
                assert torch.equal(out.pred_original_sample, sched._hist[i % 2])
        return x.cpu().numpy(), xs[-1], bnds[-1]

    loop(fwd, M.DATA, M.analytic_flow(fwd.levels[0], z).astype(np.float32))
    clean = M.analytic_flow(1.0, z).astype(np.float32)
    got, ref, bnd = loop(inv, M.NOISE, clean)
    fwd.set_timesteps(20)                                                           # (a new trajectory: step index and history reset)
    back, ref_back, _ = loop(fwd, M.DATA, got, ref, bnd)                            # the round trip continues both ends; the bound too
    assert np.abs(ref_back - clean).max() < 0.1 * np.abs(clean).max()               # (the reference does come back: 20 + 20 steps)


# ================================================================================================ pipeline and transfers against the oracle
def _oracle_pair(size=32):
    from test_gpu_unet_ddib import make_pair, synth_batch
    import phendiff_amd as P
    r, m = make_pair("super_small", size, "f32")
    cfg = P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
    pipe = P.ConditionalDDIMPipeline(m, P.DPMSolverMultistepScheduler.from_config(P.DDIMScheduler(**cfg).config))
    assert type(pipe.scheduler) is P.DPMSolverMultistepScheduler and pipe.scheduler.config.clip_sample is True
    return r, pipe, synth_batch


def rel(a, b):
    from conftest import record_error
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return record_error(float((a - b).norm() / (b.norm() + 1e-30)))


class _Reference:
    """The float64 reference schedulers of tests/multistep_refs.py driving the oracle UNet on the CPU."""

    def __init__(self, r, sched_config, S):
        import phendiff_amd as P
        c = sched_config
        self.r, self.pred = r, {"epsilon": 0, "sample": 1, "v_prediction": 2}[c.prediction_type]
        self.clip = float(c.clip_sample_range) if c.clip_sample else None
        acp = P.DDIMScheduler.from_config(c).alphas_cumprod.double().numpy()
        grid = M.ref_grid(c.num_train_timesteps, S, c.timestep_spacing, c.steps_offset)
        self.fwd = M.ref_sampler_path(acp, grid, "zero")
        self.inv = M.ref_inverse_path(acp, grid)

    def unet(self, labels, w=None):
        def model(x, t, abar):
            with torch.no_grad():
                xf = torch.from_numpy(x).float()
                cond = self.r(xf, t, class_labels=labels).sample.double()
                if w is None:
                    return cond.numpy()
                un = self.r(xf, t, class_emb=torch.zeros(xf.shape[0], 256)).sample.double()
                return (un + w * (cond - un)).numpy()      # imagen
        return model

    def invert(self, x, labels):
        ts, lv = self.inv
        return M.ref_loop(x.double().numpy(), self.unet(labels), ts, lv, M.as_f32(M.ref_coefficients(lv, M.NOISE, 2, False)), M.NOISE, self.pred)[0][-1]

    def sample(self, x, labels, first=0, w=None):
        ts, lv = self.fwd
        coefs = M.as_f32(M.ref_coefficients(lv, M.DATA, 2, True))[first:]
        coefs[0] = coefs[0][:4] + (0.0,)                    # the trajectory starts here: no history
        x = M.ref_loop(np.asarray(x, dtype=np.float64), self.unet(labels, w), ts[first:], lv[first:], coefs, M.DATA, self.pred, self.clip)[0][-1]
        return np.clip(x / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1)


def test_inversion_ddib_and_pipeline_vs_oracle():
    """super_small at 32 x 32, fp32 engine.  Inversion and DDIB at S = 4 under the 2e-5 test_ddib_eager_and_graph_vs_oracle applies to
    this model, engine and step count with DDIM; the pipeline from a start image part-way down a 6-step grid with imagen guidance under
    the 2e-4 of test_cfg_forward_start_eager_and_graph_vs_oracle."""
    import phendiff_amd as P
    r, pipe, synth_batch = _oracle_pair()
    x, labels = synth_batch(4, 32)
    target = P.swap_binary_labels(labels)
    ref = _Reference(r, pipe.scheduler.config, 4)
    ref_inv = ref.invert(x, labels)
    inv = P.inversion(pipe, x.cuda(), labels.cuda(), 4)
    err = rel(inv, ref_inv)
    print("inversion", err)
    assert err < 2e-5
    img = P.ddib(pipe, x.cuda(), labels.cuda(), target.cuda(), 4)
    err = rel(img, ref.sample(ref_inv, target))
    print("ddib", err)
    assert img.shape == (4, 32, 32, 3) and err < 2e-5
    regen = P.inverted_regeneration(pipe, x.cuda(), labels.cuda(), 4)
    assert rel(regen, ref.sample(ref_inv, labels)) < 2e-5
    ref6 = _Reference(r, pipe.scheduler.config, 6)
    got = pipe(class_labels=target.cuda(), w=2.5, num_inference_steps=6, start_image=x.cuda(), add_forward_noise_to_image=False,
               frac_diffusion_skipped=0.5, output_type="numpy").images
    assert [t for t in pipe.scheduler.timesteps.tolist() if t <= 1500] == ref6.fwd[0][3:]
    err = rel(got, ref6.sample(x.numpy(), target, first=3, w=2.5))
    print("pipeline", err)
    assert err < 2e-4


# ================================================================================================ captured runners
def _nan_history(runner):
    for h in runner.hist:
        h.fill_(NAN)
    torch.cuda.synchronize()


def test_ddib_graph_equals_enqueued_equals_eager():
    import phendiff_amd as P
    r, pipe, synth_batch = _oracle_pair()
    ddim_pipe = P.ConditionalDDIMPipeline(pipe.unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
    x, labels = synth_batch(4, 32)
    target = 1 - labels
    ddim_graph = P.DDIBGraph(ddim_pipe, batch_size=4, num_inference_steps=4)
    assert getattr(ddim_graph, "hist", None) is None                               # (a DDIM runner owns no history)
    before = ddim_graph.run(x.cuda(), labels.cuda(), target.cuda())
    torch.cuda.synchronize()
    before = (before.images.clone(), before.inverted.clone())
    assert torch.equal(before[0].cpu(), torch.from_numpy(P.ddib(ddim_pipe, x.cuda(), labels.cuda(), target.cuda(), 4)))

    inv = P.inversion(pipe, x.cuda(), labels.cuda(), 4)
    img = torch.from_numpy(P.ddib(pipe, x.cuda(), labels.cuda(), target.cuda(), 4))
    assert not torch.equal(img, before[0].cpu())
    for use_graph in (True, False):
        g = P.DDIBGraph(pipe, batch_size=4, num_inference_steps=4, use_graph=use_graph)
        assert len(g.hist) == 2 and all(isinstance(a, P._lib.MultistepStepArgs) for a in g.inv_args + g.gen_args)
        # (the sampler's second step is first-order too on this schedule: its first level has zero SNR, so h_prev is not finite)
        assert g.inv_args[0].c == 0 and g.inv_args[0].hist_in is None and g.inv_args[1].c != 0 and g.gen_args[0].c == 0 and g.gen_args[2].c != 0
        out = g.run(x.cuda(), labels.cuda(), target.cuda())
        torch.cuda.synchronize()
        assert torch.equal(out.images.cpu(), img) and torch.equal(out.inverted, inv), use_graph
        _nan_history(g)
        out = g.run(x.cuda(), labels.cuda(), target.cuda())
        torch.cuda.synchronize()
        assert torch.equal(out.images.cpu(), img) and torch.equal(out.inverted, inv), (use_graph, "replay over NaN history")
    again = ddim_graph.run(x.cuda(), labels.cuda(), target.cuda())
    torch.cuda.synchronize()
    assert torch.equal(again.images, before[0]) and torch.equal(again.inverted, before[1])


def test_sliced_ddib_graph(monkeypatch):
    import phendiff_amd as P
    r, pipe, synth_batch = _oracle_pair()
    x, labels = synth_batch(5, 32, seed=5)
    img = torch.from_numpy(P.ddib(pipe, x.cuda(), labels.cuda(), (1 - labels).cuda(), 3))
    monkeypatch.setattr(type(pipe.unet), "max_batch", lambda self, H, W: 3)
    g = P.DDIBGraph(pipe, batch_size=5, num_inference_steps=3)
    assert len(g._bounds) == 2
    out = g.run(x.cuda(), labels.cuda(), (1 - labels).cuda())
    torch.cuda.synchronize()
    assert torch.equal(out.images.cpu(), img)


@pytest.mark.parametrize("eqn,w", [("imagen", 2.5), ("CFG", 1.5)])
def test_cfg_forward_start_graph_equals_enqueued_equals_eager(eqn, w):
    import phendiff_amd as P
    r, pipe, synth_batch = _oracle_pair()
    x, labels = synth_batch(4, 32)
    target = 1 - labels
    eager = pipe(class_labels=target.cuda(), w=w, num_inference_steps=6, start_image=x.cuda(), frac_diffusion_skipped=0.5, guidance_eqn=eqn,
                 generator=torch.Generator().manual_seed(7), output_type="numpy").images
    if eqn == "imagen":
        assert np.array_equal(eager, P.classifier_free_guidance_forward_start(pipe, x.cuda(), target.cuda(), w, 0.5, 6,
                                                                              generator=torch.Generator().manual_seed(7)))
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(7))       # the draw the pipeline makes
    for use_graph in (True, False):
        g = P.CFGForwardStartGraph(pipe, batch_size=4, num_inference_steps=6, guidance_scale=w, frac_diffusion_skipped=0.5, guidance_eqn=eqn,
                                   use_graph=use_graph)
        assert len(g.ts) == 3 and g.step_args[0].c == 0 and g.step_args[1].c != 0 and g.step_args[1].uncond_out
        for again in (False, True):
            if again:
                _nan_history(g)
            out = g.run(x.cuda(), target.cuda(), noise.cuda())
            torch.cuda.synchronize()
            assert np.array_equal(out.images.cpu().numpy(), eager), (use_graph, again)


def test_generation_graph_equals_enqueued_equals_pipeline():
    import phendiff_amd as P
    r, pipe, synth_batch = _oracle_pair()
    dev = torch.device("cuda:0")
    labels = torch.tensor([0, 1, 1], device=dev)
    w = torch.tensor([1.5, 0.0, 3.0], device=dev)
    got = pipe(labels, generator=P.DeviceNoise(77, dev, first_index=3), w=w, num_inference_steps=5, output_type="numpy",
               add_forward_noise_to_image=False).images
    assert np.isfinite(got).all() and got.std() > 0.01
    for use_graph in (True, False):
        noise = P.DeviceNoise(77, dev, first_index=3)
        g = P.GenerationGraph(pipe, 3, 5, noise, w=w, use_graph=use_graph)
        g.run(labels)
        torch.cuda.synchronize()
        assert np.array_equal(g.images.cpu().numpy(), got), use_graph
        _nan_history(g)
        noise.seek(3)
        g.run(labels)
        torch.cuda.synchronize()
        assert np.array_equal(g.images.cpu().numpy(), got), (use_graph, "replay over NaN history")


def test_thresholding_pipeline_graph_equals_eager():
    """thresholding=True under the multistep sampler: the three-launch scheme inside the capture, captured = enqueued = eager."""
    import phendiff_amd as P
    from test_gpu_unet_ddib import make_pair, synth_batch
    _, m = make_pair("super_small", 32, "f32")
    cfg = dict(P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"], thresholding=True, sample_max_value=1.5, dynamic_thresholding_ratio=0.9)
    pipe = P.ConditionalDDIMPipeline(m, P.DPMSolverMultistepScheduler(**cfg))
    x, labels = synth_batch(3, 32)
    img = torch.from_numpy(P.ddib(pipe, x.cuda(), labels.cuda(), (1 - labels).cuda(), 4))
    from phendiff_amd.schedulers import MultistepThresholdStep
    for use_graph in (True, False):
        g = P.DDIBGraph(pipe, batch_size=3, num_inference_steps=4, use_graph=use_graph)
        assert all(isinstance(a, MultistepThresholdStep) for a in g.gen_args) and not any(isinstance(a, MultistepThresholdStep) for a in g.inv_args)
        assert g.gen_args[2].update.c != 0 and g.gen_args[2].update.quantile == g.gen_args[2].quant.data_ptr()
        out = g.run(x.cuda(), labels.cuda(), (1 - labels).cuda())
        torch.cuda.synchronize()
        assert torch.equal(out.images.cpu(), img), use_graph
