"""Dynamic thresholding on the MI355X: pd_abs_quantile against torch.quantile on the CPU (bit for bit), its guard bands and row
independence, pd_ddim_step_threshold against the f64 reference under the derived bound, the eager scheduler step and the pixel pipelines
against the oracle driven by a thresholding reference scheduler, the captured trajectories against eager, and the refusals.
(tests/threshold_refs.py holds the references, bounds, inputs and case lists; tests/test_host_threshold.py proves them on the CPU.)"""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

import flat_refs as R
import threshold_refs as T
from guard_bands import guarded
from test_gpu_guard_bands import Case, Op, out_op, p1_poisoned_surroundings, p2_canaried_outputs, p3_sample_isolation
from test_gpu_unet_ddib import make_pair, rel, synth_batch

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    import phendiff_amd._lib as L
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L, L.lib(), torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


# ================================================================================================ pd_abs_quantile
def launch_quantile(env, x, q, out=None, workspace=None):
    """pd_abs_quantile over the device tensor x [B][n] at quantile q -> the device tensor out [B]."""
    from phendiff_amd.schedulers import quantile_rank
    L, lib, dev = env
    B, n = x.shape
    lo, hi, w = quantile_rank(n, q)
    if out is None:
        out = torch.full((B,), -7.0, dtype=torch.float32, device=dev)          # (no quantile of |x| is negative: an unwritten row shows)
    if workspace is None:
        workspace = torch.full((lib.pd_abs_quantile_workspace(B, n),), 0xA5, dtype=torch.uint8, device=dev)     # (contents irrelevant)
    a = L.AbsQuantileArgs(B=B, n=n, rank_lo=lo, rank_hi=hi, weight=w, x=x.data_ptr(), out=out.data_ptr(), workspace=workspace.data_ptr())
    L.check(lib.pd_abs_quantile(C.byref(a), stream()), "pd_abs_quantile")
    return out


def gpu_quantile(env, x, q):
    got = launch_quantile(env, torch.from_numpy(np.ascontiguousarray(x)).to(env[2]), q)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("shape", T.QUANTILE_SHAPES + T.QUANTILE_ODD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_abs_quantile_equals_cpu_truth(env, shape):
    B, n = shape
    for kind in T.QUANTILE_CONTENTS:
        x = T.quantile_input(B, n, kind)
        for q in T.QUANTILE_QS:
            got, want = gpu_quantile(env, x, q), T.quantile_truth(x, q)
            assert T.same_bits(got, want), (kind, q, got, want)


def test_abs_quantile_real_size(env):
    B, n = T.QUANTILE_REAL_SHAPE
    x = T.quantile_input(B, n, "normal")
    for q in T.QUANTILE_QS:
        got, want = gpu_quantile(env, x, q), T.quantile_truth(x, q)
        assert T.same_bits(got, want), (q, got, want)


@pytest.mark.parametrize("n", (48, 3072, 20480))
def test_abs_quantile_seam_in_the_top_digit(env, n):
    """rank lo is the largest of the tiny half, rank hi the smallest of the huge half: the two selections part in the first pass."""
    x, q = T.seam_input(n)
    got, want = gpu_quantile(env, x, q), T.quantile_truth(x, q)
    assert 1e29 < want[0] < 1e30 and T.same_bits(got, want), (got, want)


@pytest.mark.parametrize("shape", ((3, 48), (3, 20480)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_abs_quantile_nan_row(env, shape):
    B, n = shape
    x = T.quantile_input(B, n, "normal")
    clean = T.quantile_truth(x, 0.995)
    x[1, n // 2] = np.nan
    got = gpu_quantile(env, x, 0.995)
    assert np.isnan(got[1]) and T.same_bits(got, T.quantile_truth(x, 0.995))
    assert T.same_bits(got[[0, 2]], clean[[0, 2]])


def test_abs_quantile_rows_do_not_depend_on_each_other(env):
    for B, n in ((3, 20480), (3, 75)):
        x = np.concatenate([T.quantile_input(1, n, "normal"), T.quantile_input(1, n, "levels"), T.quantile_input(1, n, "inf")])
        for q in (0.995, 0.5):
            whole = gpu_quantile(env, x, q)
            alone = np.concatenate([gpu_quantile(env, x[b:b + 1], q) for b in range(B)])
            assert T.same_bits(whole, alone), (n, q, whole, alone)


def _quantile_case(env, B, n, q, workspace_is_input):
    L, lib, dev = env
    x = T.quantile_input(B, n, "normal")
    want = T.quantile_truth(x, q)
    ws = Op(torch.zeros(lib.pd_abs_quantile_workspace(B, n) // 4, dtype=torch.float32), whole=False)
    ins = {"x": Op(torch.from_numpy(x), sample_dim=0)}
    outs = {"out": out_op((B,), torch.float32, sample_dim=0)}
    (ins if workspace_is_input else outs)["workspace"] = ws

    def launch(t):
        launch_quantile(env, t["x"], q, t["out"], t["workspace"])

    def check(got):
        assert T.same_bits(got["out"].numpy(), want)

    return Case(ins, outs, launch, check, nsamples=B)


@pytest.mark.parametrize("shape", ((3, 48), (3, 20480), (5, 2880), (3, 75)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_abs_quantile_guard_bands(env, shape, monkeypatch):
    """P1: NaN around x and around the workspace changes no bit.  P2: canaries survive around out and around the workspace, every row of
    out is written.  P3: a NaN row changes no other row."""
    dev = env[2]
    p1_poisoned_surroundings(_quantile_case(env, *shape, 0.995, True), dev, monkeypatch)
    p2_canaried_outputs(_quantile_case(env, *shape, 0.995, False), dev, monkeypatch)
    p3_sample_isolation(_quantile_case(env, *shape, 0.995, True), dev, monkeypatch)


# ================================================================================================ pd_ddim_step_threshold, s given
def _step_args(env, t, inp_shape, coef, pred, ucm, mv, guidance, sample, prev, x0):
    L = env[0]
    B, per = inp_shape
    sa, sb, sap, dc = (float(c) for c in coef)
    return L.DdimStepThresholdArgs(
        numel=B * per, per_sample=per, pred_type=pred, use_clipped_model_output=ucm, sqrt_a=sa, sqrt_b=sb, sqrt_ap=sap, dir_coef=dc,
        sample=sample.data_ptr(), model_out=t["model_out"].data_ptr(), uncond_out=t["uncond_out"].data_ptr() if guidance else None,
        w=t["w"].data_ptr() if guidance else None, w_per_sample=int(bool(guidance) and len(guidance[1]) > 1),
        guidance_cfg=guidance[0] if guidance else 0, prev_sample=prev.data_ptr(),
        pred_x0=None if x0 is None else x0.data_ptr(), quantile=t["quantile"].data_ptr(), sample_max_value=mv)


@pytest.mark.parametrize("guidance", T.STEP_GUIDANCE, ids=("plain", "imagen", "cfg"))
@pytest.mark.parametrize("pred", R.PRED_TYPES)
def test_step_threshold_against_f64(env, pred, guidance):
    """The three prediction types x (no guidance, imagen, CFG) x use_clipped_model_output x three maxima x two shapes (x the first, a
    middle and the last timestep's coefficients; the first has sqrt_a == 0), out of place and in place, and the raw x0 entry."""
    L, lib, dev = env
    coefs = R.ddim_coefficients()
    worst = 0.0
    for B, per in T.STEP_SHAPES:
        inp = T.step_input(B, per)
        t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
        if guidance:
            t["w"] = torch.tensor(guidance[1], dtype=torch.float32, device=dev)
        prev, x0, raw, inplace = (torch.empty((B, per), dtype=torch.float32, device=dev) for _ in range(4))
        for coef in coefs:
            for ucm in (0, 1):
                for mv in T.STEP_MAX_VALUES:
                    tag = (B, per, [float(c) for c in coef], ucm, mv)
                    for b in (prev, x0, raw):
                        b.fill_(NAN)
                    a = _step_args(env, t, (B, per), coef, pred, ucm, mv, guidance, t["sample"], prev, x0)
                    L.check(lib.pd_ddim_raw_x0(C.byref(a), raw.data_ptr(), stream()), "pd_ddim_raw_x0")
                    L.check(lib.pd_ddim_step_threshold(C.byref(a), stream()), "pd_ddim_step_threshold")
                    inplace.copy_(t["sample"])
                    a2 = _step_args(env, t, (B, per), coef, pred, ucm, mv, guidance, inplace, inplace, None)
                    L.check(lib.pd_ddim_step_threshold(C.byref(a2), stream()), "pd_ddim_step_threshold")
                    torch.cuda.synchronize()
                    ref, bnd = T.step_f64(inp, coef, pred, ucm, mv, guidance), T.step_bound(inp, coef, pred, ucm, mv, guidance)
                    for name, got, want, b in zip(("prev_sample", "pred_x0", "raw x0"), (prev, x0, raw), ref, bnd):
                        ok, ratio = R.within(got.cpu().numpy(), want, b)
                        assert ok, (name, tag, ratio)
                        worst = max(worst, ratio)
                    assert torch.equal(inplace, prev) or (torch.isnan(prev) == torch.isnan(inplace)).all() and \
                        torch.equal(torch.nan_to_num(inplace), torch.nan_to_num(prev)), ("in place", tag)
    from conftest import record_error
    record_error(worst)


def test_step_threshold_guard_bands(env, monkeypatch):
    L, lib, dev = env
    B, per = 5, 24 * 24 * 5 // 4 + 3          # 723: per_sample % 4 == 3, a 4-vector straddles two samples; numel % 4 == 3: a ragged tail
    g = R.rng(31)
    coef = R.ddim_coefficients()[1]
    inp = dict(sample=R.normal(g, B, per, scale=1.3), model_out=R.normal(g, B, per, scale=1.3), uncond_out=R.normal(g, B, per, scale=1.3),
               quantile=np.array(T.STEP_QUANTILES[:B], dtype=R.F32))
    want = T.step_f64(inp, coef, 2, 1, 4.0, (0, (2.5,)))
    bnd = T.step_bound(inp, coef, 2, 1, 4.0, (0, (2.5,)))
    ins = {k: Op(torch.from_numpy(v), sample_dim=0) for k, v in inp.items()}
    ins["w"] = Op(torch.tensor([2.5], dtype=torch.float32))
    outs = {"prev_sample": out_op((B, per), torch.float32, sample_dim=0), "pred_x0": out_op((B, per), torch.float32, sample_dim=0)}

    def launch(t):
        a = _step_args(env, t, (B, per), coef, 2, 1, 4.0, (0, (2.5,)), t["sample"], t["prev_sample"], t["pred_x0"])
        L.check(lib.pd_ddim_step_threshold(C.byref(a), stream()), "pd_ddim_step_threshold")

    def check(got):
        for name, w, b in (("prev_sample", want[0], bnd[0]), ("pred_x0", want[1], bnd[1])):
            assert R.within(got[name].numpy(), w, b)[0], name

    case = Case(ins, outs, launch, check, nsamples=B)
    p1_poisoned_surroundings(case, dev, monkeypatch)
    p2_canaried_outputs(case, dev, monkeypatch)
    p3_sample_isolation(case, dev, monkeypatch)


@pytest.mark.parametrize("cfg", (0, 1), ids=("imagen", "cfg"))
def test_step_threshold_per_sample_weights(env, cfg):
    """One guidance weight per sample (w_per_sample = 1) where a 4-vector straddles two samples (per_sample % 4 != 0) and the tensor
    ends in a ragged vector: the row of every element decides its weight AND its quantile."""
    L, lib, dev = env
    coef = R.ddim_coefficients()[1]
    for B, per in T.PER_SAMPLE_SHAPES:
        inp, guidance = T.step_input(B, per), (cfg, T.PER_SAMPLE_WEIGHTS[:B])
        t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
        t["w"] = torch.tensor(guidance[1], dtype=torch.float32, device=dev)
        prev, x0, raw = (torch.full((B, per), NAN, dtype=torch.float32, device=dev) for _ in range(3))
        for pred in R.PRED_TYPES:
            a = _step_args(env, t, (B, per), coef, pred, 1, 4.0, guidance, t["sample"], prev, x0)
            assert a.w_per_sample == 1
            L.check(lib.pd_ddim_raw_x0(C.byref(a), raw.data_ptr(), stream()), "pd_ddim_raw_x0")
            L.check(lib.pd_ddim_step_threshold(C.byref(a), stream()), "pd_ddim_step_threshold")
            torch.cuda.synchronize()
            ref, bnd = T.step_f64(inp, coef, pred, 1, 4.0, guidance), T.step_bound(inp, coef, pred, 1, 4.0, guidance)
            for name, got, want, b in zip(("prev_sample", "pred_x0", "raw x0"), (prev, x0, raw), ref, bnd):
                assert R.within(got.cpu().numpy(), want, b)[0], (name, B, per, pred)


# ================================================================================================ eager scheduler.step
@pytest.mark.parametrize("pred_name", ("epsilon", "sample", "v_prediction"))
def test_eager_step_against_reference_scheduler(env, pred_name):
    import phendiff_amd as P
    L, lib, dev = env
    cfg = dict(P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"], prediction_type=pred_name)
    mv, ratio = 4.0, 0.995
    got_s = P.DDIMScheduler(**cfg, thresholding=True, dynamic_thresholding_ratio=ratio, sample_max_value=mv)
    ref_s = T.make_threshold_ref(cfg, ratio, mv)
    got_s.set_timesteps(4), ref_s.set_timesteps(4)
    B, shape = 3, (3, 3, 16, 16)
    g = R.rng(37, L.PD_PRED[pred_name])
    x, out = R.normal(g, *shape), R.normal(g, *shape)
    pred = L.PD_PRED[pred_name]
    for ti in (1, 3):                           # (index 0 of this config has sqrt_a == 0: x0 of epsilon prediction is not finite there)
        t = int(got_s.timesteps[ti])
        coef = [R.F32(c) for c in got_s.step_coefficients(t)[:4]]
        for ucm in (False, True):
            ref_s.s_raw = []
            want = ref_s.step(torch.from_numpy(out), t, torch.from_numpy(x), use_clipped_model_output=ucm)
            got = got_s.step(torch.from_numpy(out).to(dev), t, torch.from_numpy(x).to(dev), use_clipped_model_output=ucm)
            torch.cuda.synchronize()
            s_ref = ref_s.s_raw[0].numpy()
            assert (s_ref > 1.0).all()                                  # (the inputs exercise the quantile)
            s_got = got_s._threshold_buffers[(B, x[0].size, dev, stream())][1].cpu().numpy()
            inp = dict(sample=x.reshape(B, -1), model_out=out.reshape(B, -1), quantile=s_ref)
            x0_ref = want.pred_original_sample.numpy().reshape(B, -1).astype(R.F64)
            e_s, e_x0, e_prev = T.eager_step_bounds(inp, coef, pred, ucm, mv, x0_ref)
            assert (np.abs(s_got.astype(R.F64) - s_ref) <= e_s).all(), (ti, ucm, s_got, s_ref, e_s)
            assert R.within(got.pred_original_sample.cpu().numpy().reshape(B, -1), x0_ref, e_x0)[0], (ti, ucm)
            assert R.within(got.prev_sample.cpu().numpy().reshape(B, -1), want.prev_sample.numpy().reshape(B, -1), e_prev)[0], (ti, ucm)
    # eta > 0 adds its noise afterwards, as without thresholding
    noise = torch.from_numpy(R.normal(g, *shape))
    t = int(got_s.timesteps[1])                 # (the last step's sigma is 0)
    want = ref_s.step(torch.from_numpy(out), t, torch.from_numpy(x), eta=0.5, variance_noise=noise).prev_sample
    got = got_s.step(torch.from_numpy(out).to(dev), t, torch.from_numpy(x).to(dev), eta=0.5, variance_noise=noise.to(dev)).prev_sample
    assert rel(got, want) < 1e-6


# ================================================================================================ pipelines and captured trajectories
STEPS, MAX_VALUE, CFG_SCALE, FRAC = 4, 4.0, 2.5, 0.5
DDIB_SEED, DDIB_SEED_2, CFG_SEED, CFG_SEED_2 = 10, 1234, 1234, 99       # (chosen on the CPU: the premise below holds for them)


@functools.lru_cache(maxsize=None)
def pipes():
    import phendiff_amd as P
    from oracle import ConditionalDDIMPipelineRef, DDIMSchedulerRef
    r, m = make_pair("super_small", 32, "f32")
    cfg = P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
    pref = ConditionalDDIMPipelineRef(r, DDIMSchedulerRef(**cfg))
    pref.scheduler = T.make_threshold_ref(cfg, 0.995, MAX_VALUE)          # (the pipeline re-makes its scheduler from the config: set afterwards)
    return pref, P.ConditionalDDIMPipeline(m, P.DDIMScheduler(**cfg, thresholding=True, sample_max_value=MAX_VALUE))


def assert_premise(pref, B):
    """For every sample the reference's unclamped s exceeds 1 in at least one step: otherwise thresholding was clipping to [-1, 1]."""
    s = torch.stack(pref.scheduler.s_raw)
    assert s.shape[1] == B and bool((s.max(0).values > 1.0).all()), s


@functools.lru_cache(maxsize=None)
def ddib_reference(seed):
    from oracle import ddib_ref
    pref, _ = pipes()
    x, labels = synth_batch(4, 32, seed)
    pref.scheduler.s_raw = []
    img, inv = ddib_ref(pref, x, labels, 1 - labels, STEPS)
    if seed == DDIB_SEED:
        assert_premise(pref, 4)
    return x, labels, img, inv


def _cfg_noise(seed):
    return torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def cfg_reference(seed):
    """The oracle's CFG forward start with the forward noise of _cfg_noise(seed) (its generator draws exactly that tensor)."""
    pref, _ = pipes()
    x, labels = synth_batch(3, 32, seed)
    pref.scheduler.s_raw = []
    img = pref(class_labels=1 - labels, num_inference_steps=STEPS, start_image=x, frac_diffusion_skipped=FRAC, w=CFG_SCALE,
               generator=torch.Generator().manual_seed(seed)).images
    assert_premise(pref, 3)
    return x, labels, img


def runner_owns_its_scratch(steps, st):
    """Every step of a runner is a ThresholdStep of the runner's stream that holds the tensors its structs point at."""
    from phendiff_amd.schedulers import ThresholdStep
    assert len(steps) > 0
    for a in steps:
        assert isinstance(a, ThresholdStep) and a.stream == st
        assert (a.quantile.x, a.quantile.out, a.quantile.workspace, a.step.quantile) == \
            (a.x0_raw.data_ptr(), a.quant.data_ptr(), a.workspace.data_ptr(), a.quant.data_ptr())


def test_pipeline_cfg_generation_vs_oracle():
    """Tolerance: test_pipeline_cfg_and_forward_noise_f32's (tests/test_gpu_unet_ddib.py), the same comparison without thresholding."""
    import phendiff_amd as P
    _, pgot = pipes()
    x, labels, ref = cfg_reference(CFG_SEED)
    got = P.classifier_free_guidance_forward_start(pgot, x.cuda(), (1 - labels).cuda(), CFG_SCALE, FRAC, STEPS,
                                                   generator=torch.Generator().manual_seed(CFG_SEED))
    assert got.shape == ref.shape and rel(got, ref) < 2e-4
    got = pgot(class_labels=(1 - labels).cuda(), num_inference_steps=STEPS, start_image=x.cuda(), frac_diffusion_skipped=FRAC, w=CFG_SCALE,
               generator=torch.Generator().manual_seed(CFG_SEED), output_type="numpy").images
    assert rel(got, ref) < 2e-4


def test_pipeline_ddib_vs_oracle():
    """Tolerance: test_ddib_eager_and_graph_vs_oracle's f32 one."""
    import phendiff_amd as P
    _, pgot = pipes()
    x, labels, ref_img, _ = ddib_reference(DDIB_SEED)
    img = P.ddib(pgot, x.cuda(), labels.cuda(), (1 - labels).cuda(), STEPS)
    assert img.shape == ref_img.shape and rel(img, ref_img) < 2e-5


def test_ddib_graph_equals_eager_and_follows_the_batch():
    import phendiff_amd as P
    _, pgot = pipes()
    x, labels, _, _ = ddib_reference(DDIB_SEED)
    eager = P.ddib(pgot, x.cuda(), labels.cuda(), (1 - labels).cuda(), STEPS)
    graph = P.DDIBGraph(pgot, batch_size=4, num_inference_steps=STEPS)
    first = graph.run(x.cuda(), labels.cuda(), (1 - labels).cuda()).images.clone()
    again = graph.run(x.cuda(), labels.cuda(), (1 - labels).cuda()).images.clone()
    torch.cuda.synchronize()
    assert torch.equal(first.cpu(), torch.from_numpy(eager)) and torch.equal(first, again)
    # other contents: that batch's eager result -- the quantile is recomputed on replay, not baked in at capture
    x2, l2, ref2, _ = ddib_reference(DDIB_SEED_2)
    out2 = graph.run(x2.cuda(), l2.cuda(), (1 - l2).cuda()).images.clone()
    torch.cuda.synchronize()
    assert torch.equal(out2.cpu(), torch.from_numpy(P.ddib(pgot, x2.cuda(), l2.cuda(), (1 - l2).cuda(), STEPS)))
    assert rel(out2, ref2) < 2e-5 and not torch.equal(out2, first)
    back = graph.run(x.cuda(), labels.cuda(), (1 - labels).cuda()).images.clone()       # ... and nothing of it stays behind
    torch.cuda.synchronize()
    assert torch.equal(back, first)
    # the graph outlives the scheduler it was captured under: its steps own the scratch they launch into
    runner_owns_its_scratch(graph.gen_args, graph.stream.cuda_stream)
    ws_bytes, n = graph.gen_args[0].workspace.numel(), graph.gen_args[0].x0_raw.numel()
    pgot.scheduler = P.DDIMScheduler.from_config(pgot.scheduler.config)
    gc.collect()
    decoys = [torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(4)] + \
             [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(4)]      # what freed blocks would be handed to
    after = graph.run(x.cuda(), labels.cuda(), (1 - labels).cuda()).images.clone()
    torch.cuda.synchronize()
    assert torch.equal(after, first)
    assert all(bool((d == (0x5A if d.dtype == torch.uint8 else 7.0)).all()) for d in decoys)


def test_cfg_graph_equals_eager_and_follows_the_batch():
    import phendiff_amd as P
    _, pgot = pipes()
    graph = P.CFGForwardStartGraph(pgot, batch_size=3, num_inference_steps=STEPS, guidance_scale=CFG_SCALE, frac_diffusion_skipped=FRAC)
    outs = []
    for seed in (CFG_SEED, CFG_SEED, CFG_SEED_2):
        x, labels, ref = cfg_reference(seed)
        # randn_tensor with a CPU generator draws on the CPU: the eager pipeline's forward noise is this tensor
        eager = P.classifier_free_guidance_forward_start(pgot, x.cuda(), (1 - labels).cuda(), CFG_SCALE, FRAC, STEPS,
                                                         generator=torch.Generator().manual_seed(seed))
        out = graph.run(x.cuda(), (1 - labels).cuda(), _cfg_noise(seed).cuda()).images.clone()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(eager)), seed
        assert rel(out, ref) < 2e-4
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    runner_owns_its_scratch(graph.step_args, graph.stream.cuda_stream)


# ================================================================================================ refusals
def test_guided_and_latent_runners_refuse_on_the_device():
    import os
    import sys
    import phendiff_amd as P
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import SD_SCHED, SD_TINY_UNET, SD_TINY_VAE
    cfg = P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
    unet = P.CustomCondUNet2DModel(compute_dtype="f32", **dict(P.UNET_CONFIGS["super_small"], sample_size=32)).to("cuda:0")
    pipe = P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**cfg, thresholding=True, sample_max_value=MAX_VALUE))
    x, labels = synth_batch(2, 32)
    with pytest.raises(ValueError, match="no derivative through"):
        P.GuidedTransferGraph(pipe, 2, 3, 2, 0.5)
    with pytest.raises(ValueError, match="no derivative through"):
        P.linear_interp_custom_guidance_inverted_start(pipe, x.cuda(), labels.cuda(), (1 - labels).cuda(), 2, 0.5, 3)
    with pytest.raises(ValueError, match="no derivative through"):
        P.custom_guided_generation(pipe, x.cuda(), labels.cuda(), 2, 0.5, 3)
    assert not unet._plans and unet._weights is None
    sd_unet, vae = P.SDUNet2DConditionModel(compute_dtype="f32", **SD_TINY_UNET).to("cuda:0"), P.AutoencoderKL(compute_dtype="f32", **SD_TINY_VAE).to("cuda:0")
    emb = P.CustomEmbedding(2, SD_TINY_UNET["cross_attention_dim"]).to("cuda:0")
    th = P.DDIMScheduler(**dict(SD_SCHED, thresholding=True, sample_max_value=2.0))
    with pytest.raises(ValueError, match="pixel-space method"):
        P.CustomStableDiffusionImg2ImgPipeline(vae, sd_unet, th, emb)
    sd = P.CustomStableDiffusionImg2ImgPipeline(vae, sd_unet, P.DDIMScheduler(**SD_SCHED), emb)
    sd.scheduler = th
    with pytest.raises(ValueError, match="pixel-space method"):
        P.SDDDIBGraph(sd, 2, 3, 32, 32)
    with pytest.raises(ValueError, match="thresholding=True"):
        P.SDGuidedTransferGraph(sd, 2, 3, 2, 0.5, 32, 32)
    with pytest.raises(ValueError, match="pixel-space method"):
        P.ddib(sd, x.cuda(), labels.cuda(), (1 - labels).cuda(), 3)
    assert not sd_unet._plans and not vae._plans
