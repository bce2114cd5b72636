"""The multistep solvers without a GPU: the schedulers' coefficients against known answers and against the float64 restatement of
tests/multistep_refs.py, the order of convergence on a model with a closed-form flow, the fp32 replica of pd_multistep_step inside the
derived bound (on the inputs tests/test_gpu_multistep.py runs), the ABI, every refusal of the entry point, and the refusals of what
does not run these schedulers."""
import ctypes as C

import numpy as np
import pytest
import torch

import flat_refs as R
import multistep_refs as M
from abi_header import header_fields

ANALYTIC = dict(num_train_timesteps=1000, beta_schedule="scaled_linear", beta_start=1e-4, beta_end=0.02, timestep_spacing="leading")


def _pair(cfg=None, S=50, **kw):
    import phendiff_amd as P
    fwd = P.DPMSolverMultistepScheduler(**dict(cfg or ANALYTIC, **kw))
    inv = P.DPMSolverMultistepInverseScheduler.from_config(fwd.config)
    fwd.set_timesteps(S), inv.set_timesteps(S)
    return fwd, inv


# ================================================================================================ coefficients: known answers
def test_zero_snr_first_step_and_final_step():
    import phendiff_amd as P
    fwd, _ = _pair(P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    assert fwd.config.timestep_spacing == "trailing" and float(fwd.alphas_cumprod[int(fwd.timesteps[0])]) == 0.0
    abar_t = float(fwd.alphas_cumprod[int(fwd.timesteps[1])].double())
    sa, sb, a, b, c = fwd.multistep_coefficients(0)
    assert (sa, sb, c) == (0.0, 1.0, 0.0)
    assert (a, b) == (float(np.float32(np.sqrt(1 - abar_t))), float(np.float32(np.sqrt(abar_t))))      # (sigma_t, alpha_t): the explicit limit
    assert fwd.multistep_coefficients(49)[2:] == (0.0, 1.0, 0.0)                                       # "zero": lands on x0
    assert all(np.isfinite(fwd.multistep_coefficients(i)).all() for i in range(50))
    assert fwd.multistep_coefficients(25)[4] != 0.0


@pytest.mark.parametrize("S", (2, 14, 15, 50))
def test_c_is_zero_at_the_first_step_and_at_the_last_of_a_short_schedule(S):
    fwd, inv = _pair(S=S, final_sigmas_type="sigma_min", steps_offset=1)      # (a finite last h: only the rule can zero c)
    n = len(fwd.timesteps)
    c = [fwd.multistep_coefficients(i)[4] for i in range(n)]
    assert c[0] == 0.0 and all(v != 0.0 for v in c[1:-1])
    assert (c[-1] == 0.0) == (S < 15)
    assert fwd.multistep_coefficients(n - 1, first=True)[4] == 0.0 and fwd.multistep_coefficients(1, first=True)[4] == 0.0
    no_lof, _ = _pair(S=S, final_sigmas_type="sigma_min", steps_offset=1, lower_order_final=False)
    assert no_lof.multistep_coefficients(n - 1)[4] != 0.0
    ci = [inv.multistep_coefficients(j)[4] for j in range(len(inv.timesteps))]
    assert ci[0] == 0.0 and all(v != 0.0 for v in ci[1:])
    first_order, _ = _pair(S=S, solver_order=1)
    assert all(first_order.multistep_coefficients(i)[4] == 0.0 for i in range(S))


@pytest.mark.parametrize("S", (10, 50))
def test_first_order_coefficients_are_ddims(S):
    """solver_order = 1 is DDIM written in x0: x' = sqrt_ap x0 + dir eps with eps = (x - sqrt_a x0) / sqrt_b."""
    import phendiff_amd as P
    fwd, _ = _pair(S=S, solver_order=1)
    ddim = P.DDIMScheduler.from_config(fwd.config)
    ddim.set_timesteps(S)
    assert ddim.timesteps.tolist() == fwd.timesteps.tolist()
    for i, t in enumerate(ddim.timesteps):
        sa, sb, sap, dc, _ = ddim.step_coefficients(t)
        m_sa, m_sb, a, b, c = fwd.multistep_coefficients(i)
        assert c == 0.0
        np.testing.assert_allclose([m_sa, m_sb], [sa, sb], rtol=1e-6)
        np.testing.assert_allclose([a, b], [dc / sb, sap - dc * sa / sb], rtol=1e-6, atol=0)


def test_inverse_path_length_and_end():
    for spacing, steps in (("leading", 49), ("trailing", 50), ("linspace", 49)):
        fwd, inv = _pair(S=50, timestep_spacing=spacing)
        assert len(fwd.timesteps) == 50 and len(inv.timesteps) == steps, spacing
        assert inv.timesteps[0] == 0 and inv.levels[-1] == fwd.levels[0] == float(fwd.alphas_cumprod[int(fwd.timesteps[0])].double())
        assert inv.timesteps.tolist() == sorted(set([0] + fwd.timesteps.tolist()))[:-1]
    fwd, inv = _pair(S=50, steps_offset=1)
    assert len(inv.timesteps) == 50 and inv.timesteps[1] == 1


def test_constructor_and_config_round_trip(tmp_path):
    import phendiff_amd as P
    with pytest.raises(ValueError, match="algorithm_type"):
        P.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    with pytest.raises(ValueError, match="solver_type"):
        P.DPMSolverMultistepScheduler(solver_type="heun")
    with pytest.raises(ValueError, match="solver_order"):
        P.DPMSolverMultistepScheduler(solver_order=3)
    with pytest.raises(ValueError, match="final_sigmas_type"):
        P.DPMSolverMultistepScheduler(final_sigmas_type="karras")
    with pytest.raises(ValueError, match="sigma_min"):
        P.DPMSolverMultistepScheduler(final_sigmas_type="sigma_min").set_timesteps(50)      # leading without offset ends at t = 0
    assert P.DPMSolverMultistepScheduler().config.clip_sample is False
    ddim = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    fwd = P.DPMSolverMultistepScheduler.from_config(ddim.config, use_karras_sigmas=False)       # (an unknown diffusers key is ignored)
    assert fwd.config.clip_sample == ddim.config.clip_sample and torch.equal(fwd.alphas_cumprod, ddim.alphas_cumprod)
    fwd.save_pretrained(str(tmp_path / "f"))
    again = P.DPMSolverMultistepScheduler.from_pretrained(str(tmp_path / "f"))
    assert vars(again.config) == vars(fwd.config)
    inv = P.DPMSolverMultistepInverseScheduler.from_config(fwd.config)
    inv.save_pretrained(str(tmp_path / "i"))
    assert vars(P.DPMSolverMultistepInverseScheduler.from_pretrained(str(tmp_path / "i")).config) == vars(inv.config)
    assert vars(P.DDIMScheduler.from_config(fwd.config).config) == vars(ddim.config)            # and back
    # a pipeline keeps a multistep sampler, converts everything else to DDIM, and its folder remembers which
    with torch.device("meta"):
        unet = P.CustomCondUNet2DModel(**dict(P.UNET_CONFIGS["super_small"], sample_size=32))
    assert type(P.ConditionalDDIMPipeline(unet, fwd).scheduler) is P.DPMSolverMultistepScheduler
    assert type(P.ConditionalDDIMPipeline(unet, inv).scheduler) is P.DDIMScheduler
    from phendiff_amd.checkpoint import save_scheduler, saved_scheduler_class
    save_scheduler(ddim, str(tmp_path / "d"))
    assert saved_scheduler_class(str(tmp_path / "f")) is P.DPMSolverMultistepScheduler
    assert saved_scheduler_class(str(tmp_path / "d")) is P.DDIMScheduler


@pytest.mark.parametrize("name", ("3k_steps_clipping_rescaling", "analytic", "offset"))
def test_schedulers_against_their_restatement(name):
    """Grid, levels and every coefficient of both schedulers equal the float64 restatement rounded to fp32."""
    import phendiff_amd as P
    cfg = {"analytic": ANALYTIC, "offset": dict(ANALYTIC, steps_offset=1, final_sigmas_type="sigma_min", timestep_spacing="leading")}.get(
        name) or P.SCHEDULER_CONFIGS[name]
    for S in (7, 20, 50):
        fwd, inv = _pair(cfg, S=S)
        acp = fwd.alphas_cumprod.double().numpy()
        c = fwd.config
        grid = M.ref_grid(c.num_train_timesteps, S, c.timestep_spacing, c.steps_offset)
        for sched, (ts, levels), form, lof in ((fwd, M.ref_sampler_path(acp, grid, c.final_sigmas_type), M.DATA, True),
                                               (inv, M.ref_inverse_path(acp, grid), M.NOISE, False)):
            assert sched.timesteps.tolist() == ts and sched.levels.tolist() == levels
            ref = M.as_f32(M.ref_coefficients(levels, form, 2, lof))
            got = [sched.multistep_coefficients(i) for i in range(len(ts))]
            np.testing.assert_allclose(got, ref, rtol=2e-7, atol=0)      # (one fp32 rounding of two float64 evaluations)


# ================================================================================================ the analytic model
@pytest.fixture(scope="module")
def analytic_errors():
    """Max-abs errors of the float64 restatement on data N(0.3, 0.25) against the closed-form flow, N = 1000, scaled_linear, leading,
    "zero".  Inversions start from the clean sample x(abar = 1), regarded as at alphas_cumprod[0]."""
    import phendiff_amd as P
    acp = P.DPMSolverMultistepScheduler(**ANALYTIC).alphas_cumprod.double().numpy()

    def forward(S, order, x=None):
        ts, lv = M.ref_sampler_path(acp, M.ref_grid(1000, S, "leading"))
        xs, _ = M.ref_loop(M.analytic_flow(lv[0]) if x is None else x, M.analytic_eps, ts, lv, M.ref_coefficients(lv, M.DATA, order, True), M.DATA)
        return xs[-1]

    def invert(S, order):
        ts, lv = M.ref_inverse_path(acp, M.ref_grid(1000, S, "leading"))
        xs, _ = M.ref_loop(M.analytic_flow(1.0), M.analytic_eps, ts, lv, M.ref_coefficients(lv, M.NOISE, order, False), M.NOISE)
        return xs[-1], lv[-1]

    err = lambda x, abar: float(np.abs(x - M.analytic_flow(abar)).max())
    e = {("forward", o, S): err(forward(S, o), 1.0) for o in (1, 2) for S in (50, 100)}
    e["inversion", 2, 50] = err(*invert(50, 2))
    e["roundtrip", 2, 50] = err(forward(50, 2, invert(50, 2)[0]), 1.0)
    e["roundtrip", 1, 100] = err(forward(100, 1, invert(100, 1)[0]), 1.0)
    return e


ANALYTIC_TABLE = {("forward", 1, 50): 2.192e-2, ("forward", 2, 50): 8.933e-3, ("forward", 1, 100): 1.117e-2, ("forward", 2, 100): 2.364e-3,
                  ("inversion", 2, 50): 7.127e-3, ("roundtrip", 2, 50): 5.319e-3, ("roundtrip", 1, 100): 2.213e-2}


@pytest.mark.parametrize("key", sorted(ANALYTIC_TABLE), ids=lambda k: "-".join(str(v) for v in k))
def test_analytic_errors_reproduce_the_table(analytic_errors, key):
    print(key, analytic_errors[key])
    assert abs(analytic_errors[key] / ANALYTIC_TABLE[key] - 1) <= 0.02, (key, analytic_errors[key])


def test_analytic_second_order(analytic_errors):
    e = analytic_errors
    assert e["forward", 2, 100] / e["forward", 2, 50] <= 0.35                      # second order: 0.25 ideally (first order: 0.5)
    assert e["roundtrip", 2, 50] <= 0.5 * e["roundtrip", 1, 100]                   # half the UNet evaluations, less than half the error


# ================================================================================================ replica against reference
def _replica_cases(inp, guidance, what):
    worst = 0.0
    coefs = M.schedule_coefficients()
    for form, ti, pred, clip in M.multistep_cases():
        for coef in (coefs[form][ti], coefs[form][ti][:4] + (np.float32(0.0),)):
            ref, bnd, got = (f(inp, coef, form, pred, clip, guidance) for f in (M.multistep_f64, M.multistep_bound, M.multistep_f32_replica))
            for name, g, r, b in zip(("prev_sample", "m0"), got, ref, bnd):
                ok, ratio = R.within(g, r, b)
                assert ok, f"{what} form={form} step#{ti} pred={pred} clip={clip} c={coef[4]} {name}: ratio {ratio:.3f}"
                worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("numel", R.DDIM_NUMEL)
def test_replica_within_bound(numel):
    _replica_cases(M.multistep_input(1, numel), None, f"numel={numel}")


@pytest.mark.parametrize("guidance", R.DDIM_GUIDANCE, ids=lambda g: f"{'cfg' if g[0] else 'imagen'}-w{len(g[1])}-{g[1][0]}")
def test_replica_within_bound_guided(guidance):
    _replica_cases(M.multistep_input(*R.DDIM_GUIDED), guidance, f"guided {guidance}")


@pytest.mark.parametrize("pred", R.PRED_TYPES)
def test_replica_within_bound_thresholded(pred):
    inp = M.multistep_input(*R.DDIM_GUIDED)
    for coef in M.schedule_coefficients()[M.DATA]:
        for guidance in (None, R.DDIM_GUIDANCE[2]):
            ref, bnd, got = (f(inp, coef, M.DATA, pred, 0, guidance, M.THRESHOLD_Q) for f in (M.multistep_f64, M.multistep_bound, M.multistep_f32_replica))
            for g, r, b in zip(got, ref, bnd):
                assert R.within(g, r, b)[0], (pred, coef, guidance)
            assert np.abs(ref[1]).max() <= 1.0      # |x0| <= s / s


def test_loop_bound_covers_an_fp32_loop():
    """The accumulated bound of the eager-loop test (tests/test_gpu_multistep.py) holds for the same loop in fp32 numpy."""
    fwd, inv = _pair(S=20)
    z = R.normal(R.rng(12), 2, 192).astype(np.float64)
    for sched, form, x0 in ((fwd, M.DATA, M.analytic_flow(fwd.levels[0], z)), (inv, M.NOISE, M.analytic_flow(1.0, z))):
        coefs = [sched.multistep_coefficients(i) for i in range(len(sched.timesteps))]
        x0 = x0.astype(np.float32)
        xs, ms = M.ref_loop(x0, M.analytic_eps_rounded, sched.timesteps.tolist(), sched.levels, coefs, form)
        bnds = M.loop_bound(xs, ms, sched.levels, coefs, form)
        x, m1 = x0, None
        for i, cf in enumerate(coefs):
            c1, c2 = (np.float32(v) for v in M.analytic_constants(sched.levels[i]))
            inp = dict(sample=x, model_out=(x - c1) * c2, hist_in=m1)
            x, m1 = M.multistep_f32_replica(inp, tuple(np.float32(v) for v in cf), form, 0, 0)
            ok, ratio = R.within(x, xs[i + 1], bnds[i])
            assert ok, (form, i, ratio)


# ================================================================================================ ABI
FIELDS = ["numel", "per_sample", "pred_type", "form", "clip", "clip_range", "sqrt_a", "sqrt_b", "a", "b", "c", "sample", "model_out", "uncond_out",
          "w", "w_per_sample", "guidance_cfg", "hist_in", "prev_sample", "hist_out", "pred_x0", "quantile", "sample_max_value"]


def test_struct_and_export():
    import phendiff_amd._lib as L
    assert header_fields("pd_multistep_step_args") == FIELDS == [f[0] for f in L.MultistepStepArgs._fields_]
    types = dict(L.MultistepStepArgs._fields_)
    assert types["numel"] is C.c_int64 and types["a"] is types["c"] is C.c_float and types["hist_in"] is C.c_void_p
    lib = L.lib()
    assert hasattr(lib, "pd_multistep_step") and "pd_multistep_step" in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == 8                                   # only an entry point was added
    assert header_fields("pd_ddim_step_args") == [f[0] for f in L.DdimStepArgs._fields_]          # (unchanged)


def test_entry_point_validates_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    q = p + 1024
    ok = dict(numel=96, per_sample=48, pred_type=2, form=0, clip=1, clip_range=1.0, sqrt_a=0.8, sqrt_b=0.6, a=0.9, b=0.1, c=0.05, sample=p,
              model_out=p, uncond_out=None, w=None, w_per_sample=0, guidance_cfg=0, hist_in=p, prev_sample=p, hist_out=q, pred_x0=p,
              quantile=None, sample_max_value=0.0)
    noise = dict(form=1, clip=0, pred_x0=None)
    cases = [(dict(numel=0), b"numel"), (dict(numel=-4), b"numel"), (dict(numel=100), b"per_sample"), (dict(per_sample=0), b"per_sample"),
             (dict(pred_type=3), b"prediction type"), (dict(pred_type=-1), b"prediction type"), (dict(form=2), b"bad form"), (dict(form=-1), b"bad form"),
             (dict(sample=None), b"is NULL"), (dict(model_out=None), b"is NULL"), (dict(prev_sample=None), b"prev_sample is NULL"),
             (dict(hist_out=None), b"hist_out is NULL"), (dict(hist_in=None), b"hist_in is NULL with c"),
             (dict(hist_in=None, c=float("nan")), b"hist_in is NULL with c"), (dict(hist_out=p), b"must not alias"),
             (dict(uncond_out=p), b"guidance without weights"),
             (dict(form=1, pred_x0=None), b"no clamp"), (dict(noise, quantile=p, sample_max_value=2.0), b"no clamp"), (dict(noise, pred_x0=p), b"pred_x0"),
             (dict(sample=p + 4), b"16-byte aligned"), (dict(model_out=p + 8), b"16-byte aligned"), (dict(uncond_out=p + 4, w=p), b"16-byte aligned"),
             (dict(hist_in=p + 4), b"16-byte aligned"), (dict(prev_sample=p + 4), b"16-byte aligned"), (dict(hist_out=q + 4), b"16-byte aligned"),
             (dict(pred_x0=p + 12), b"16-byte aligned"), (dict(uncond_out=p, w=p + 2), b"w must be 4-byte aligned"),
             (dict(quantile=p + 2, sample_max_value=2.0), b"quantile must be 4-byte aligned"),
             (dict(quantile=p), b"sample_max_value"), (dict(quantile=p, sample_max_value=float("nan")), b"sample_max_value")]
    for change, word in cases:
        rc = lib.pd_multistep_step(C.byref(L.MultistepStepArgs(**dict(ok, **change))), None)
        assert rc < 0, change
        assert word in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_multistep_step:"), (change, lib.pd_last_error())
    assert lib.pd_multistep_step(None, None) < 0 and b"null args" in lib.pd_last_error()


def test_step_args_from_the_scheduler():
    """multistep_step_args with raw pointers: form, clipping and coefficients from the scheduler; a first-order step names no history."""
    import phendiff_amd as P
    fwd, inv = _pair(P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    a = fwd.multistep_step_args(25, 4096, 8192, 4096, 12288, 16384, numel=96, per_sample=48)
    assert (a.form, a.clip, a.pred_type, a.hist_in, a.hist_out, a.prev_sample) == (0, 1, 2, 12288, 16384, 4096)
    assert (a.sqrt_a, a.sqrt_b, a.a, a.b, a.c) == fwd.multistep_coefficients(25) and a.c != 0
    a = fwd.multistep_step_args(25, 4096, 8192, 4096, 12288, 16384, numel=96, per_sample=48, first=True)
    assert a.c == 0.0 and a.hist_in is None and a.hist_out == 16384
    a = inv.multistep_step_args(25, 4096, 8192, 4096, 12288, 16384, uncond_out=20480, w=24576, guidance_cfg=True, numel=96, per_sample=48)
    assert (a.form, a.clip, a.quantile, a.pred_x0, a.uncond_out, a.guidance_cfg) == (1, 0, None, None, 20480, 1)
    with pytest.raises(ValueError, match="pd_multistep_step"):
        fwd.ddim_step_args(int(fwd.timesteps[3]), 4096, 8192, 4096, numel=96, per_sample=48)
    with pytest.raises(ValueError, match="set_timesteps"):
        P.DPMSolverMultistepScheduler().multistep_coefficients(0)


# ================================================================================================ plumbing refusals
def _meta_pipe():
    import phendiff_amd as P
    with torch.device("meta"):
        unet = P.CustomCondUNet2DModel(**dict(P.UNET_CONFIGS["super_small"], sample_size=32))
    pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))
    pipe.scheduler = P.DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)      # the diffusers idiom
    return pipe


def test_guided_and_tiled_refuse_multistep_before_any_plan():
    import phendiff_amd as P
    pipe = _meta_pipe()
    x, labels = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.long)
    for call in (lambda: P.GuidedTransferGraph(pipe, 2, 3, 2, 0.5, 32, 32), lambda: P.custom_guided_generation(pipe, x, labels, 2, 0.5, 3),
                 lambda: P.linear_interp_custom_guidance_inverted_start(pipe, x, labels, 1 - labels, 2, 0.5, 3)):
        with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler.*previous step's prediction"):
            call()
    big = torch.zeros(2, 3, 48, 48)
    for call in (lambda: P.tiled_inversion(pipe, big, labels, 3, 32), lambda: P.tiled_ddib(pipe, big, labels, 1 - labels, 3, 32),
                 lambda: P.tiled_inverted_regeneration(pipe, big, labels, 3, 32), lambda: P.TiledDDIBGraph(pipe, 2, 3, 48, 48, 32)):
        with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler.*tiled"):
            call()
    assert not pipe.unet._plans and pipe.unet._weights is None


def test_stochastic_steps_are_refused():
    import phendiff_amd as P
    pipe = _meta_pipe()
    labels = torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="DPMSolverMultistepScheduler.*eta = 0.5"):
        pipe(class_labels=labels, eta=0.5, num_inference_steps=3, output_type="numpy")
    with pytest.raises(ValueError, match="DPMSolverMultistepScheduler.*eta = 0.5"):
        P.GenerationGraph(pipe, 2, 3, P.DeviceNoise.__new__(P.DeviceNoise), eta=0.5)
    assert not pipe.unet._plans and pipe.unet._weights is None
    fwd, inv = _pair(S=5)
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(ValueError, match="eta = 0.5"):
        fwd.step(x, fwd.timesteps[0], x, eta=0.5)
    with pytest.raises(ValueError, match="generator"):
        fwd.step(x, fwd.timesteps[0], x, generator=torch.Generator())
    with pytest.raises(ValueError, match="eta = 1"):
        inv.step(x, inv.timesteps[0], x, eta=1)


def test_latent_tier_refuses_multistep_before_any_plan():
    import os
    import sys
    import phendiff_amd as P
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import SD_SCHED, SD_TINY_UNET, SD_TINY_VAE
    with torch.device("meta"):
        unet, vae = P.SDUNet2DConditionModel(**SD_TINY_UNET), P.AutoencoderKL(**SD_TINY_VAE)
        emb = P.CustomEmbedding(2, SD_TINY_UNET["cross_attention_dim"])
    ms = P.DPMSolverMultistepScheduler.from_config(P.DDIMScheduler(**SD_SCHED).config)
    with pytest.raises(NotImplementedError, match="pixel tier"):
        P.CustomStableDiffusionImg2ImgPipeline(vae, unet, ms, emb)
    pipe = P.CustomStableDiffusionImg2ImgPipeline(vae, unet, P.DDIMScheduler(**SD_SCHED), emb)
    pipe.scheduler = ms                                    # swapped in after construction: every way in refuses
    x, labels = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.long)
    for call in (lambda: P.SDDDIBGraph(pipe, 2, 3, 32, 32), lambda: pipe(image=x, class_labels=labels, num_inference_steps=3),
                 lambda: P.ddib(pipe, x, labels, 1 - labels, 3), lambda: P.inversion(pipe, x, labels, 3),
                 lambda: P.classifier_free_guidance_forward_start(pipe, x, labels, 2.0, 0.5, 3)):
        with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler.*pixel tier"):
            call()
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        P.SDGuidedTransferGraph(pipe, 2, 3, 2, 0.5, 32, 32)
    assert not unet._plans
