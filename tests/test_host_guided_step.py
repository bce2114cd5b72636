"""``pd_guided_step`` / ``pd_lp_guidance_scaled`` and the two guided runners without a GPU: the C ABI of the new entry points (struct
layout, export, every refusal before a launch) and what ``GuidedTransferGraph`` / ``SDGuidedTransferGraph`` refuse before they pack a
weight or build a plan."""
import ctypes as C

import pytest

from abi_header import header_fields

FIELDS = ["numel", "per_sample", "pred_type", "clip", "clip_range", "use_clipped_model_output", "sqrt_a", "sqrt_b", "sqrt_ap", "dir_coef",
          "guidance_scale", "grad_scale", "sample", "g_direct", "g_unet", "model_out", "prev_sample", "pushed", "overflow"]
TENSORS = ["sample", "g_direct", "g_unet", "model_out", "prev_sample", "pushed"]
REQUIRED = ["sample", "g_direct", "g_unet", "model_out", "prev_sample"]


def test_guided_step_struct_and_exports():
    import phendiff_amd._lib as L
    assert header_fields("pd_guided_step_args") == FIELDS == [f[0] for f in L.GuidedStepArgs._fields_]
    # the part shared with pd_ddim_step keeps that struct's order (ddim_step_elem reads either)
    ddim = [f for f in header_fields("pd_ddim_step_args") if f in FIELDS]
    assert [f for f in FIELDS if f in ddim] == ddim
    lib = L.lib()
    for name in ("pd_guided_step", "pd_lp_guidance_scaled"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == 8


def _ok_step(p):
    return dict(numel=96, per_sample=48, pred_type=2, clip=1, clip_range=1.0, use_clipped_model_output=0, sqrt_a=0.8, sqrt_b=0.6,
                sqrt_ap=0.9, dir_coef=0.43, guidance_scale=0.5, grad_scale=p, sample=p, g_direct=p, g_unet=p, model_out=p, prev_sample=p,
                pushed=p, overflow=p)


def test_guided_step_validates_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    ok = _ok_step(p)
    cases = [(dict(numel=0), b"numel"), (dict(numel=-4), b"numel"), (dict(numel=100), b"per_sample"), (dict(per_sample=0), b"per_sample"),
             (dict(pred_type=3), b"prediction type"), (dict(pred_type=-1), b"prediction type")]
    for name in TENSORS:                                 # 16 k + 4: every tensor goes through 16-byte vector accesses
        cases.append(({name: p + 16 * 3 + 4}, name.encode() + b" must be 16-byte aligned"))
    for name in REQUIRED:
        cases.append(({name: None}, name.encode() + b" is NULL"))
    cases += [(dict(grad_scale=p + 2), b"4-byte aligned"), (dict(overflow=p + 2), b"4-byte aligned")]
    for change, word in cases:
        rc = lib.pd_guided_step(C.byref(L.GuidedStepArgs(**dict(ok, **change))), None)
        assert rc < 0, change
        assert word in lib.pd_last_error(), (change, lib.pd_last_error())
    assert lib.pd_guided_step(None, None) < 0 and b"null args" in lib.pd_last_error()


def test_lp_guidance_scaled_validates_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    ok = dict(numel=96, per_sample=48, pred_type=2, clip=1, clip_range=1.0, sqrt_a=0.8, sqrt_b=0.6, p=2.0, sample=p, model_out=p, target=p,
              partial=p, splits=1, d_model_out=p, d_sample_direct=p, losses=p)
    assert lib.pd_lp_guidance_scaled(C.byref(L.LpGuidanceArgs(**ok)), None, None) == -1
    assert b"pd_lp_guidance_scaled" in lib.pd_last_error() and b"grad_scale is NULL" in lib.pd_last_error()
    # every refusal of pd_lp_guidance, under the new entry point's name
    cases = [(dict(numel=0), -1, b"bad sizes"), (dict(numel=100), -1, b"bad sizes"), (dict(pred_type=5), -1, b"bad prediction type"),
             (dict(p=0.5), -4, b"finite p >= 1"), (dict(p=1e6), -4, b"finite p >= 1"), (dict(p=float("inf")), -4, b"finite p >= 1"),
             (dict(p=float("nan")), -4, b"finite p >= 1"), (dict(splits=0), -1, b"null pointer")]
    cases += [({name: None}, -1, b"null pointer") for name in ("sample", "model_out", "target", "partial", "d_model_out", "d_sample_direct")]
    for change, code, word in cases:
        rc = lib.pd_lp_guidance_scaled(C.byref(L.LpGuidanceArgs(**dict(ok, **change))), p, None)
        assert rc == code, (change, rc)
        msg = lib.pd_last_error()
        assert word in msg and msg.startswith(b"pd_lp_guidance_scaled:"), (change, msg)
        assert lib.pd_lp_guidance(C.byref(L.LpGuidanceArgs(**dict(ok, **change))), None) == code      # ... which refuses the same
        assert lib.pd_last_error().startswith(b"pd_lp_guidance:")
    assert lib.pd_lp_guidance_scaled(None, p, None) < 0


def _cpu_pixel_pipe():
    import torch
    import phendiff_amd as P
    with torch.device("meta"):
        unet = P.CustomCondUNet2DModel(**dict(P.UNET_CONFIGS["super_small"], sample_size=32))
    return P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))


def test_runners_refuse_before_any_plan_exists():
    """Neither a GPU nor parameters here (meta device): whatever is raised comes before anything is packed."""
    import phendiff_amd as P
    pipe = _cpu_pixel_pipe()
    for runner in (P.GuidedTransferGraph, P.SDGuidedTransferGraph):
        for bad in ("inf", "2", 0.5, 1e6, float("inf"), float("nan")):
            with pytest.raises(NotImplementedError, match="finite p >= 1"):
                runner(pipe, 2, 3, bad, 0.5, 32, 32)
    with pytest.raises(NotImplementedError, match="CustomStableDiffusionImg2ImgPipeline"):      # the wrong kind of pipeline
        P.SDGuidedTransferGraph(pipe, 2, 3, 2, 0.5, 32, 32)
    with pytest.raises(P.PhenDiffHipError, match="no CPU fallback"):
        P.GuidedTransferGraph(pipe, 2, 3, 2, 0.5)
    assert not pipe.unet._plans and pipe.unet._weights is None


def test_sd_runner_refuses_a_cpu_pipeline():
    import sys
    import os
    import torch
    import phendiff_amd as P
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import SD_SCHED, SD_TINY_UNET, SD_TINY_VAE
    with torch.device("meta"):
        unet, vae = P.SDUNet2DConditionModel(**SD_TINY_UNET), P.AutoencoderKL(**SD_TINY_VAE)
        emb = P.CustomEmbedding(2, SD_TINY_UNET["cross_attention_dim"])
    pipe = P.CustomStableDiffusionImg2ImgPipeline(vae, unet, P.DDIMScheduler(**SD_SCHED), emb)
    with pytest.raises(P.PhenDiffHipError, match="no CPU fallback"):
        P.SDGuidedTransferGraph(pipe, 2, 3, 2, 0.5, 32, 32)
    with pytest.raises(NotImplementedError, match="ConditionalDDIMPipeline"):
        P.GuidedTransferGraph(pipe, 2, 3, 2, 0.5, 32, 32)
    assert not unet._plans
