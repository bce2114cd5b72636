"""Guidance rescale without a GPU: the properties of the float64 restatement (tests/guidance_rescale_ref.py) that
tests/test_gpu_guidance_rescale.py holds the kernel to, the ABI, every refusal of ``pd_guidance_rescale`` (all of them before any HIP
call), and the ``ValueError`` of every guided entry point for a ``guidance_rescale`` outside [0, 1], before anything is packed."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import guidance_rescale_ref as G
from abi_header import header_fields

BAD = (-0.1, 1.5, float("nan"))
FIELDS = ["numel", "per_sample", "model_out", "uncond_out", "w", "w_per_sample", "guidance_cfg", "rescale", "out", "workspace"]


def _chunk():
    import phendiff_amd._lib as L
    return L.CONSTANTS["PD_GUIDANCE_RESCALE_CHUNK"]


def _case(B, n, guidance):
    cond, uncond = G.inputs(B, n)
    return cond, uncond, G.weights(B, guidance[1]), guidance[0]


# ================================================================================================ the restatement
@pytest.mark.parametrize("guidance", G.GUIDANCE, ids=lambda g: f"{'cfg' if g[0] else 'imagen'}-w{len(g[1])}")
def test_restatement_properties(guidance):
    for B, n in G.shapes(_chunk()):
        cond, uncond, w, eqn = _case(B, n, guidance)
        cfg = G.combine_f32(cond, uncond, w, eqn)
        assert cfg.dtype == torch.float32
        # phi = 0 is the identity on the guided prediction
        assert torch.equal(G.reference(cond, uncond, w, 0.0, eqn), cfg.double())
        # phi = 1 gives every sample the standard deviation of its conditional prediction
        one = G.reference(cond, uncond, w, 1.0, eqn)
        np.testing.assert_allclose(one.std(dim=1).numpy(), cond.double().std(dim=1).numpy(), rtol=1e-12)
        # the factored form the kernel evaluates is diffusers' form
        for phi in (0.3, 0.7, 1.0):
            a, b = G.rescale_noise_cfg(cfg.double(), cond.double(), phi), G.rescale_factored(cfg.double(), cond.double(), phi)
            assert float(((a - b).abs() / a.abs().clamp_min(1e-300)).max()) <= 1e-12, (B, n, phi)


def test_combine_is_the_step_kernels_order():
    """u + w (c - u) with one fp32 rounding per operation: what flat_refs' fp32 replica of pd_ddim_step forms."""
    cond, uncond, w, _ = _case(3, 105, G.GUIDANCE[2])
    c, u, wv = cond.numpy(), uncond.numpy(), w.numpy()[:, None]
    assert np.array_equal(G.combine_f32(cond, uncond, w, 0).numpy(), u + (wv * (c - u)).astype(np.float32))
    assert np.array_equal(G.combine_f32(cond, uncond, w, 1).numpy(), c + (wv * (c - u)).astype(np.float32))


def test_ulp_measure():
    want = torch.tensor([1.0, -3.0, 2.0 ** -10, 0.0, 1e-3], dtype=torch.float64)
    got = want.float().clone()
    assert G.ulps(got, want).tolist()[:4] == [0.0] * 4 and 0.0 < float(G.ulps(got, want)[4]) <= 0.5      # (1e-3 is no fp32 value)
    got[0] = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    got[1] = float(np.nextafter(np.nextafter(np.float32(-3.0), np.float32(-4.0)), np.float32(-4.0)))
    assert G.ulps(got, want).tolist()[:2] == [1.0, 2.0]
    assert G.abi_phi(0.7) == float(np.float32(0.7)) != 0.7


# ================================================================================================ ABI
def test_struct_and_export():
    import phendiff_amd._lib as L
    assert header_fields("pd_guidance_rescale_args") == FIELDS == [f[0] for f in L.GuidanceRescaleArgs._fields_]
    types = dict(L.GuidanceRescaleArgs._fields_)
    assert types["numel"] is types["per_sample"] is C.c_int64 and types["rescale"] is C.c_float
    assert types["model_out"] is types["out"] is types["workspace"] is C.c_void_p
    lib = L.lib()
    for name in ("pd_guidance_rescale", "pd_guidance_rescale_workspace"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert L.SYMBOLS["pd_guidance_rescale_workspace"][0] is C.c_size_t
    assert lib.pd_abi_version() == L.ABI_VERSION == 8                                   # only an entry point was added
    assert header_fields("pd_ddim_step_args") == [f[0] for f in L.DdimStepArgs._fields_]          # (unchanged)
    chunk = _chunk()
    assert chunk > 0 and chunk % 1024 == 0
    ws = lib.pd_guidance_rescale_workspace
    assert ws(1, 2) == 32 and ws(3, chunk) == 3 * 32 and ws(3, chunk + 1) == 6 * 32 and ws(32, 3 * 256 * 256) == 32 * -(-3 * 256 * 256 // chunk) * 32
    assert ws(0, 8) == ws(-1, 8) == ws(2, 1) == ws(2, 0) == ws(1 << 40, 1 << 40) == 0


def test_entry_point_validates_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    u, w, ws = p + 1024, p + 2048, p + 4096
    ok = dict(numel=96, per_sample=48, model_out=p, uncond_out=u, w=w, w_per_sample=0, guidance_cfg=0, rescale=0.7, out=p, workspace=ws)
    ARG, SHAPE = L.CONSTANTS["PD_ERR_ARG"], L.CONSTANTS["PD_ERR_SHAPE"]
    cases = [(dict(model_out=None), ARG, b"model_out is NULL"), (dict(uncond_out=None), ARG, b"uncond_out is NULL"),
             (dict(w=None), ARG, b"w is NULL"), (dict(out=None), ARG, b"out is NULL"), (dict(workspace=None), ARG, b"null workspace"),
             (dict(rescale=-0.1), ARG, b"rescale"), (dict(rescale=1.5), ARG, b"rescale"), (dict(rescale=float("nan")), ARG, b"rescale"),
             (dict(rescale=float("inf")), ARG, b"rescale"), (dict(rescale=float("-inf")), ARG, b"rescale"),
             (dict(model_out=p + 4), ARG, b"16-byte aligned"), (dict(uncond_out=u + 8), ARG, b"16-byte aligned"),
             (dict(out=p + 12), ARG, b"16-byte aligned"), (dict(w=w + 2), ARG, b"w must be 4-byte aligned"),
             (dict(workspace=ws + 4), ARG, b"workspace must be 8-byte aligned"),
             (dict(numel=0), SHAPE, b"numel"), (dict(numel=-96), SHAPE, b"numel"), (dict(per_sample=1), SHAPE, b"per_sample"),
             (dict(per_sample=0), SHAPE, b"per_sample"), (dict(per_sample=-48), SHAPE, b"per_sample"), (dict(numel=100), SHAPE, b"not a multiple"),
             (dict(numel=1 << 62, per_sample=1 << 31), SHAPE, b"chunks")]
    for change, code, word in cases:
        rc = lib.pd_guidance_rescale(C.byref(L.GuidanceRescaleArgs(**dict(ok, **change))), None)
        assert rc == code, (change, rc)
        assert word in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_guidance_rescale:"), (change, lib.pd_last_error())
    assert lib.pd_guidance_rescale(None, None) == ARG and b"null args" in lib.pd_last_error()


# ================================================================================================ the entry points refuse before they pack
def _meta_pipe():
    import phendiff_amd as P
    with torch.device("meta"):
        unet = P.CustomCondUNet2DModel(**dict(P.UNET_CONFIGS["super_small"], sample_size=32))
    return P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))


def _meta_sd_pipe():
    import phendiff_amd as P
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import SD_SCHED, SD_TINY_UNET, SD_TINY_VAE
    with torch.device("meta"):
        unet, vae = P.SDUNet2DConditionModel(**SD_TINY_UNET), P.AutoencoderKL(**SD_TINY_VAE)
        emb = P.CustomEmbedding(2, SD_TINY_UNET["cross_attention_dim"])
    return P.CustomStableDiffusionImg2ImgPipeline(vae, unet, P.DDIMScheduler(**SD_SCHED), emb)


@pytest.mark.parametrize("bad", BAD, ids=str)
def test_pixel_entry_points_refuse_before_any_plan(bad):
    import phendiff_amd as P
    pipe = _meta_pipe()
    x, labels = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.long)
    noise = P.DeviceNoise.__new__(P.DeviceNoise)
    gen = dict(nb_classes=2, nb_generated_images=4, eval_batch_size=2, num_inference_steps=3, guidance_factor=3.0)
    calls = (lambda: pipe(class_labels=labels, w=3.0, num_inference_steps=3, output_type="numpy", guidance_rescale=bad),
             lambda: P.classifier_free_guidance_forward_start(pipe, x, labels, 3.0, 0.5, 3, guidance_rescale=bad),
             lambda: P.eval_generation.generate_samples(pipe, guidance_rescale=bad, **gen),
             lambda: P.eval_generation.generate_samples(pipe, device_noise=noise, guidance_rescale=bad, **gen),
             lambda: P.GenerationGraph(pipe, 2, 3, noise, w=3.0, guidance_rescale=bad),
             lambda: P.CFGForwardStartGraph(pipe, 2, 3, guidance_scale=3.0, guidance_rescale=bad),
             lambda: P.guidance_rescale(x, x, 3.0, bad),
             lambda: P.GuidanceRescale(x, x, torch.ones(1), bad))
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match=r"guidance_rescale must be a finite number in \[0, 1\]"):
            call()
    assert not pipe.unet._plans and pipe.unet._weights is None


@pytest.mark.parametrize("bad", BAD, ids=str)
def test_latent_entry_points_refuse_before_any_plan(bad):
    import phendiff_amd as P
    pipe = _meta_sd_pipe()
    x, labels = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.long)
    calls = (lambda: pipe(image=x, class_labels=labels, num_inference_steps=3, guidance_scale=3.0, guidance_rescale=bad),
             lambda: P.classifier_free_guidance_forward_start(pipe, x, labels, 3.0, 0.5, 3, guidance_rescale=bad),
             lambda: P.eval_generation.generate_samples(pipe, nb_classes=2, nb_generated_images=4, eval_batch_size=2, num_inference_steps=3,
                                                        guidance_factor=3.0, model_type="StableDiffusion", guidance_rescale=bad))
    for call in calls:
        with pytest.raises(ValueError, match=r"guidance_rescale must be a finite number in \[0, 1\]"):
            call()
    assert not pipe.unet._plans


def test_the_parameter_is_the_last_one_and_defaults_to_off():
    import phendiff_amd as P
    for fn in (P.ConditionalDDIMPipeline.__call__, P.classifier_free_guidance_forward_start, P.eval_generation.generate_samples,
               P.GenerationGraph.__init__, P.CFGForwardStartGraph.__init__, P.CustomStableDiffusionImg2ImgPipeline.__call__):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "guidance_rescale" and last.default == 0.0, fn


def test_public_function_has_no_cpu_fallback():
    import phendiff_amd as P
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(P.PhenDiffHipError, match="no CPU fallback"):
        P.guidance_rescale(x, x, 3.0, 0.7)
    with pytest.raises(P.PhenDiffHipError, match="no CPU fallback"):
        P.GuidanceRescale(x, x, torch.ones(1), 0.7)
