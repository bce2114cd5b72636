"""Dynamic thresholding without a GPU: the host arithmetic of the quantile (quantile_rank against torch.quantile, bit for bit), the
calibration of the step's bound, the scheduler's constructor surface (thresholding, trained_betas, from_config), the C ABI of the new
entry points (struct layout, exports, every refusal before a launch) and what the guided and latent runners refuse."""
import ctypes as C

import numpy as np
import pytest
import torch

import flat_refs as R
import threshold_refs as T
from abi_header import header_fields


def test_quantile_rank_sort_lerp_equals_torch_quantile():
    """n x q grid x 3 rows (one of them with an infinity), plus the contents the GPU test uses at its smallest shape."""
    g = torch.Generator().manual_seed(0)
    for n in T.RANK_GRID_N:
        x = torch.randn(3, n, generator=g) * 1.7
        x[1, n // 3] = float("inf")
        for q in T.RANK_GRID_Q:
            assert T.same_bits(T.quantile_numpy(x.numpy(), q), T.quantile_truth(x, q)), (n, q)
    for kind in T.QUANTILE_CONTENTS:
        x = T.quantile_input(3, 48, kind)
        for q in T.QUANTILE_QS:
            assert T.same_bits(T.quantile_numpy(x, q), T.quantile_truth(x, q)), (kind, q)
    x = T.quantile_input(3, 200, "normal")
    x[1, 17] = np.nan
    got = T.quantile_numpy(x, 0.995)
    assert np.isnan(got[1]) and T.same_bits(got, T.quantile_truth(x, 0.995))


def test_quantile_rank_values_and_refusals():
    from phendiff_amd.schedulers import quantile_rank
    assert quantile_rank(196608, 0.995)[:2] == (195623, 195624)
    assert quantile_rank(48, 0.0) == (0, 0, 0.0) and quantile_rank(48, 1.0) == (47, 47, 0.0) and quantile_rank(1, 0.3) == (0, 0, 0.0)
    lo, hi, w = quantile_rank(8, 0.5)
    assert (lo, hi, w) == (3, 4, 0.5)
    for n, q in ((0, 0.5), (8, -0.1), (8, 1.5), (16_000_001, 0.5)):
        with pytest.raises(ValueError):
            quantile_rank(n, q)
    x, q = T.seam_input(3072)
    want = T.quantile_truth(x, q)
    assert 1e29 < want[0] < 1e30 and T.same_bits(T.quantile_numpy(x, q), want)      # (between a tiny and a huge value)


@pytest.mark.parametrize("pred", R.PRED_TYPES)
def test_step_replica_within_bound(pred):
    """The fp32 replica of the thresholded step lies within the derived bound of the f64 reference: calibrates the bound."""
    worst = 0.0
    for ci, coef in enumerate(R.ddim_coefficients()):
        for B, per in T.STEP_SHAPES:
            inp = T.step_input(B, per)
            for guidance in T.STEP_GUIDANCE:
                for ucm in (0, 1):
                    for mv in T.STEP_MAX_VALUES:
                        ref = T.step_f64(inp, coef, pred, ucm, mv, guidance)
                        rep = T.step_f32_replica(inp, coef, pred, ucm, mv, guidance)
                        bnd = T.step_bound(inp, coef, pred, ucm, mv, guidance)
                        for name, got, want, b in zip(("prev", "x0", "raw"), rep, ref, bnd):
                            ok, ratio = R.within(got, want, b)
                            assert ok, (name, ci, B, per, guidance, ucm, mv, ratio)
                            worst = max(worst, ratio)
    assert 0.0 < worst <= 1.0
    # the inputs exercise all three regimes of s
    s = T.threshold_s(T.step_input(8, 48)["quantile"], 4.0)
    assert (s == 1.0).any() and (s == 4.0).any() and ((s > 1.0) & (s < 4.0)).any()


def test_step_replica_within_bound_per_sample_weights():
    coef = R.ddim_coefficients()[1]
    for B, per in T.PER_SAMPLE_SHAPES:
        inp = T.step_input(B, per)
        for cfg in (0, 1):
            guidance = (cfg, T.PER_SAMPLE_WEIGHTS[:B])
            for pred in R.PRED_TYPES:
                ref, rep = T.step_f64(inp, coef, pred, 1, 4.0, guidance), T.step_f32_replica(inp, coef, pred, 1, 4.0, guidance)
                for got, want, b in zip(rep, ref, T.step_bound(inp, coef, pred, 1, 4.0, guidance)):
                    assert R.within(got, want, b)[0], (B, per, cfg, pred)
                # a neighbour's weight does not pass: the bound tells the rows apart
                wrong = T.step_f32_replica(inp, coef, pred, 1, 4.0, (cfg, T.PER_SAMPLE_WEIGHTS[1:B + 1] if B < 5 else T.PER_SAMPLE_WEIGHTS[::-1]))
                assert not R.within(wrong[0], ref[0], T.step_bound(inp, coef, pred, 1, 4.0, guidance)[0])[0]


def test_threshold_step_holds_what_its_structs_point_at():
    """Host tensors stand in for device ones (nothing is launched): the step a runner keeps owns all three scratch tensors, so a captured
    graph's addresses stay allocated whatever becomes of the scheduler; the scheduler itself keeps a bounded number of sets."""
    import gc
    import weakref
    import phendiff_amd as P
    from phendiff_amd.schedulers import THRESHOLD_SCRATCH_SETS, ThresholdStep
    s = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"], thresholding=True, sample_max_value=4.0)
    s.set_timesteps(4)
    x, out = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4)
    t = int(s.timesteps[1])
    a = s.threshold_step(t, x, out, x, 0x10)
    assert isinstance(a, ThresholdStep) and a.stream == 0x10
    assert (a.quantile.x, a.quantile.out, a.quantile.workspace) == (a.x0_raw.data_ptr(), a.quant.data_ptr(), a.workspace.data_ptr())
    assert a.step.quantile == a.quant.data_ptr() and a.step.sample == a.step.prev_sample == x.data_ptr()
    assert a.x0_raw.shape == (2, 48) and a.quant.shape == (2,) and a.workspace.numel() == P.lib().pd_abs_quantile_workspace(2, 48)
    b = s.threshold_step(int(s.timesteps[2]), x, out, x, 0x10)              # the same (B, n, device, stream): the same set
    assert b.workspace.data_ptr() == a.workspace.data_ptr() and b.x0_raw.data_ptr() == a.x0_raw.data_ptr()
    assert s.threshold_step(t, x, out, x, 0x20).workspace.data_ptr() != a.workspace.data_ptr()       # another stream: its own
    with pytest.raises(ValueError, match="enqueued on stream"):             # (refused before anything is launched)
        a.enqueue(0x20)
    for st in range(0x30, 0x30 + 2 * THRESHOLD_SCRATCH_SETS):
        s.threshold_step(t, x, out, x, st)
    assert len(s._threshold_buffers) == THRESHOLD_SCRATCH_SETS and (2, 48, x.device, 0x10) not in s._threshold_buffers
    alive = [weakref.ref(v) for v in (a.x0_raw, a.quant, a.workspace)]
    ptrs = (a.x0_raw.data_ptr(), a.quant.data_ptr(), a.workspace.data_ptr())
    del s, b
    gc.collect()
    assert all(r() is not None for r in alive) and ptrs == (a.quantile.x, a.quantile.out, a.quantile.workspace)


def test_constructor_accepts_thresholding_and_trained_betas():
    import phendiff_amd as P
    from phendiff_amd.schedulers import make_betas
    s = P.DDIMScheduler(thresholding=True, dynamic_thresholding_ratio=0.99, sample_max_value=4.0)
    assert s.config.thresholding is True and s.config.dynamic_thresholding_ratio == 0.99 and s.config.sample_max_value == 4.0
    s2 = P.DDIMScheduler.from_config(s.config)
    assert vars(s2.config) == vars(s.config)
    assert P.DDIMScheduler().config.thresholding is False
    with pytest.raises(ValueError):
        P.DDIMScheduler(thresholding=True, dynamic_thresholding_ratio=1.5)
    with pytest.raises(ValueError):
        P.DDIMScheduler(thresholding=True, sample_max_value=0.0)
    # trained_betas: the values of a named schedule give that schedule's tables, in both schedulers, and round-trip through a config
    betas = make_betas("linear", 1e-4, 0.02, 1000)
    for cls in (P.DDIMScheduler, P.DDIMInverseScheduler):
        named = cls(beta_schedule="linear")
        for given in (betas, betas.tolist(), betas.numpy()):
            t = cls(beta_schedule="scaled_linear", trained_betas=given)
            assert torch.equal(t.betas, named.betas) and torch.equal(t.alphas_cumprod, named.alphas_cumprod)
            assert isinstance(t.config.trained_betas, list)
        assert torch.equal(cls.from_config(t.config).alphas_cumprod, named.alphas_cumprod)
        with pytest.raises(ValueError):
            cls(trained_betas=[0.1, 0.2])
    # the inverse scheduler is made from the forward one's config (trajectories._schedules): it keeps working and does not threshold
    inv = P.DDIMInverseScheduler.from_config(P.DDIMScheduler(thresholding=True, sample_max_value=2.0, trained_betas=betas).config)
    assert not getattr(inv.config, "thresholding", False) and torch.equal(inv.betas, betas)


def test_thresholding_false_builds_the_same_ddim_step_args():
    import phendiff_amd as P
    import phendiff_amd._lib as L
    cfg = P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
    s = P.DDIMScheduler(**cfg, thresholding=False, sample_max_value=4.0)
    s.set_timesteps(4)
    t = int(s.timesteps[1])
    a = s.ddim_step_args(t, 4096, 8192, 4096, uncond_out=12288, w=16384, guidance_cfg=True, use_clipped_model_output=True, pred_x0=20480,
                         numel=96, per_sample=48, w_per_sample=False)
    assert isinstance(a, L.DdimStepArgs)
    sa, sb, sap, dc, _ = s.step_coefficients(t)
    want = dict(numel=96, per_sample=48, pred_type=L.PD_PRED[cfg["prediction_type"]], clip=int(cfg["clip_sample"]),
                clip_range=float(cfg.get("clip_sample_range", 1.0)), use_clipped_model_output=1, sqrt_a=np.float32(sa), sqrt_b=np.float32(sb),
                sqrt_ap=np.float32(sap), dir_coef=np.float32(dc), sample=4096, model_out=8192, uncond_out=12288, w=16384, w_per_sample=0,
                guidance_cfg=1, prev_sample=4096, pred_x0=20480)
    assert {k: getattr(a, k) for k in want} == want
    th = P.DDIMScheduler(**cfg, thresholding=True, sample_max_value=4.0)
    th.set_timesteps(4)
    with pytest.raises(ValueError, match="threshold_step"):
        th.ddim_step_args(t, 4096, 8192, 4096, numel=96, per_sample=48)


QUANTILE_FIELDS = ["B", "n", "rank_lo", "rank_hi", "weight", "x", "out", "workspace"]
STEP_FIELDS = ["numel", "per_sample", "pred_type", "use_clipped_model_output", "sqrt_a", "sqrt_b", "sqrt_ap", "dir_coef", "sample", "model_out",
               "uncond_out", "w", "w_per_sample", "guidance_cfg", "prev_sample", "pred_x0", "quantile", "sample_max_value"]


def test_structs_and_exports():
    import phendiff_amd._lib as L
    assert header_fields("pd_abs_quantile_args") == QUANTILE_FIELDS == [f[0] for f in L.AbsQuantileArgs._fields_]
    assert header_fields("pd_ddim_step_threshold_args") == STEP_FIELDS == [f[0] for f in L.DdimStepThresholdArgs._fields_]
    # the fields shared with pd_ddim_step, in that struct's order (ddim_x0_eps / ddim_prev read either); clip / clip_range are not shared
    ddim = [f for f in header_fields("pd_ddim_step_args") if f not in ("clip", "clip_range")]
    assert STEP_FIELDS[:len(ddim)] == ddim
    assert header_fields("pd_ddim_step_args") == [f[0] for f in L.DdimStepArgs._fields_]          # (unchanged)
    lib = L.lib()
    for name in ("pd_abs_quantile", "pd_abs_quantile_workspace", "pd_ddim_raw_x0", "pd_ddim_step_threshold"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == 8
    assert lib.pd_abs_quantile_workspace(32, 196608) > 0 and lib.pd_abs_quantile_workspace(2, 196608) * 16 == lib.pd_abs_quantile_workspace(32, 196608)
    for B, n in ((0, 8), (8, 0), (65536, 8), (2, 1 << 31)):
        assert lib.pd_abs_quantile_workspace(B, n) == 0


def _aligned():
    buf = (C.c_char * 8192)()
    return buf, (C.addressof(buf) + 255) // 256 * 256


def test_abs_quantile_validates_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf, p = _aligned()
    ok = dict(B=2, n=48, rank_lo=46, rank_hi=47, weight=0.25, x=p, out=p, workspace=p)
    cases = [(dict(x=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(workspace=None), b"null pointer"),
             (dict(B=0), b"B = 0"), (dict(B=-1), b"B = -1"), (dict(n=0), b"n = 0"),
             (dict(rank_lo=-1), b"rank_lo"), (dict(rank_hi=48), b"rank_hi"), (dict(rank_lo=47, rank_hi=46), b"rank_lo"),
             (dict(rank_lo=40), b"at most 1 apart"),
             (dict(weight=1.0), b"weight"), (dict(weight=-0.5), b"weight"), (dict(weight=float("nan")), b"weight"),
             (dict(x=p + 4), b"x must be 16-byte aligned"),                          # n % 4 == 0: 16-byte loads
             (dict(n=47, rank_lo=45, rank_hi=46, x=p + 2), b"x must be 4-byte aligned"),
             (dict(out=p + 2), b"4-byte aligned"), (dict(workspace=p + 1), b"4-byte aligned"),
             (dict(B=65536), b"overflows the grid"), (dict(n=1 << 31, rank_lo=5, rank_hi=5), b"overflows the 32-bit counters")]
    for change, word in cases:
        rc = lib.pd_abs_quantile(C.byref(L.AbsQuantileArgs(**dict(ok, **change))), None)
        assert rc < 0, change
        assert word in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_abs_quantile:"), (change, lib.pd_last_error())
    assert lib.pd_abs_quantile(None, None) < 0 and b"null args" in lib.pd_last_error()


def test_step_threshold_validates_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf, p = _aligned()
    ok = dict(numel=96, per_sample=48, pred_type=2, use_clipped_model_output=0, sqrt_a=0.8, sqrt_b=0.6, sqrt_ap=0.9, dir_coef=0.43, sample=p,
              model_out=p, uncond_out=None, w=None, w_per_sample=0, guidance_cfg=0, prev_sample=p, pred_x0=p, quantile=p, sample_max_value=4.0)
    both = [(dict(numel=0), b"numel"), (dict(numel=100), b"per_sample"), (dict(per_sample=0), b"per_sample"), (dict(numel=1 << 41, per_sample=1), b"overflows the grid"),
            (dict(pred_type=3), b"prediction type"), (dict(sample=None), b"is NULL"), (dict(model_out=None), b"is NULL"),
            (dict(uncond_out=p), b"guidance without weights"), (dict(sample=p + 4), b"16-byte aligned"), (dict(model_out=p + 8), b"16-byte aligned"),
            (dict(uncond_out=p + 4, w=p), b"16-byte aligned"), (dict(uncond_out=p, w=p + 2), b"w must be 4-byte aligned")]
    step_only = [(dict(prev_sample=None), b"prev_sample is NULL"), (dict(quantile=None), b"quantile is NULL"), (dict(prev_sample=p + 4), b"16-byte aligned"),
                 (dict(pred_x0=p + 4), b"16-byte aligned"), (dict(quantile=p + 2), b"quantile must be 4-byte aligned"),
                 (dict(sample_max_value=0.0), b"sample_max_value"), (dict(sample_max_value=float("nan")), b"sample_max_value")]
    for change, word in both + step_only:
        rc = lib.pd_ddim_step_threshold(C.byref(L.DdimStepThresholdArgs(**dict(ok, **change))), None)
        assert rc < 0, change
        assert word in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_ddim_step_threshold:"), (change, lib.pd_last_error())
    for change, word in both:
        rc = lib.pd_ddim_raw_x0(C.byref(L.DdimStepThresholdArgs(**dict(ok, **change))), p, None)
        assert rc < 0, change
        assert word in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_ddim_raw_x0:"), (change, lib.pd_last_error())
    for x0, word in ((None, b"x0 is NULL"), (p + 4, b"16-byte aligned")):
        assert lib.pd_ddim_raw_x0(C.byref(L.DdimStepThresholdArgs(**ok)), x0, None) < 0 and word in lib.pd_last_error()
    assert lib.pd_ddim_step_threshold(None, None) < 0 and b"null args" in lib.pd_last_error()
    assert lib.pd_ddim_raw_x0(None, p, None) < 0 and b"null args" in lib.pd_last_error()


def _thresholding_scheduler():
    import phendiff_amd as P
    return P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"], thresholding=True, sample_max_value=4.0)


def test_guided_transfer_refuses_thresholding_before_any_plan():
    """Meta-device models: whatever is raised comes before anything is packed or launched."""
    import phendiff_amd as P
    with torch.device("meta"):
        unet = P.CustomCondUNet2DModel(**dict(P.UNET_CONFIGS["super_small"], sample_size=32))
    pipe = P.ConditionalDDIMPipeline(unet, _thresholding_scheduler())
    assert pipe.scheduler.config.thresholding and pipe.scheduler.config.sample_max_value == 4.0      # (the pipeline keeps the config)
    x, labels = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="no derivative through"):
        P.GuidedTransferGraph(pipe, 2, 3, 2, 0.5, 32, 32)
    with pytest.raises(ValueError, match="no derivative through"):
        P.custom_guided_generation(pipe, x, labels, 2, 0.5, 3)
    with pytest.raises(ValueError, match="no derivative through"):
        P.linear_interp_custom_guidance_inverted_start(pipe, x, labels, 1 - labels, 2, 0.5, 3)
    assert not pipe.unet._plans and pipe.unet._weights is None


def test_latent_tier_refuses_thresholding_before_any_plan():
    import os
    import sys
    import phendiff_amd as P
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import SD_SCHED, SD_TINY_UNET, SD_TINY_VAE
    with torch.device("meta"):
        unet, vae = P.SDUNet2DConditionModel(**SD_TINY_UNET), P.AutoencoderKL(**SD_TINY_VAE)
        emb = P.CustomEmbedding(2, SD_TINY_UNET["cross_attention_dim"])
    th = P.DDIMScheduler(**dict(SD_SCHED, thresholding=True, sample_max_value=2.0))
    with pytest.raises(ValueError, match="pixel-space method"):
        P.CustomStableDiffusionImg2ImgPipeline(vae, unet, th, emb)
    pipe = P.CustomStableDiffusionImg2ImgPipeline(vae, unet, P.DDIMScheduler(**SD_SCHED), emb)
    pipe.scheduler = th                                    # swapped in after construction: every way in refuses
    x, labels = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="pixel-space method"):
        P.SDDDIBGraph(pipe, 2, 3, 32, 32)
    with pytest.raises(ValueError, match="thresholding=True"):
        P.SDGuidedTransferGraph(pipe, 2, 3, 2, 0.5, 32, 32)
    with pytest.raises(ValueError, match="pixel-space method"):
        pipe(image=x, class_labels=labels, num_inference_steps=3)
    assert not unet._plans
