"""A Stable Diffusion 1.x-shaped UNet2DConditionModel on MI355X: 1x1-conv ``proj_in`` / ``proj_out``, head dimensions 40, 80 and 160
(``pd_attn_hd``) in one network, against the CPU oracle (whose Linear-form projection holds the same numbers); the cross-attention
k / v cache, DDIB eager and as one graph, and the refused training plans."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_unet_ddib import rel

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden import SD_SCHED, SD_TINY_VAE, DDIMSchedulerRef, synth_batch  # noqa: E402

# head dimensions 40, 80 and 160 in one network; 36 014 724 parameters
SD15_TINY = dict(
    in_channels=4,
    out_channels=4,
    block_out_channels=(160, 320, 320),
    layers_per_block=1,
    down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
    up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
    attention_head_dim=(4, 4, 2),
    cross_attention_dim=64,
    norm_num_groups=32,
    use_linear_projection=False,
)
# head_dim 64 on the first block (pd_attn_d64), 40 on the second and the mid block (pd_attn_hd)
MIXED = dict(in_channels=4, out_channels=4, block_out_channels=(64, 320), layers_per_block=1,
             down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
             attention_head_dim=(1, 8), cross_attention_dim=64, norm_num_groups=32, use_linear_projection=False)


def to_conv_form(sd):
    return {k: (v[:, :, None, None] if k.endswith(("proj_in.weight", "proj_out.weight")) else v) for k, v in sd.items()}


_REF = {}


def reference(cfg_name):
    """Oracle UNet + embedding and its outputs on the fixed inputs, computed once per config and shared (never modified)."""
    if cfg_name not in _REF:
        from oracle import CustomEmbeddingRef, UNet2DConditionRef
        from oracle import class_emb_to_encoder_hidden_states as ehs_ref
        cfg = {"SD15_TINY": SD15_TINY, "MIXED": MIXED}[cfg_name]
        torch.manual_seed(0)
        r = UNet2DConditionRef(**dict(cfg, use_linear_projection=True)).eval()
        emb = CustomEmbeddingRef(2, cfg["cross_attention_dim"])
        g = torch.Generator().manual_seed(2)
        x = torch.randn(2, 4, 16, 16, generator=g)
        labels, ts = torch.tensor([0, 1]), torch.tensor([980, 37])
        with torch.no_grad():
            ehs = ehs_ref(emb(labels))
            out = dict(labelled=r(x, ts, ehs).sample, uncond=r(x, ts, torch.zeros(2, 77, cfg["cross_attention_dim"])).sample,
                       scalar=r(x, 500, ehs).sample)
        _REF[cfg_name] = (cfg, r, emb, x, labels, ts, ehs, out)
    return _REF[cfg_name]


def engine(cfg, r, mode):
    import phendiff_amd as P
    m = P.SDUNet2DConditionModel(compute_dtype=mode, **cfg)
    m.load_state_dict(to_conv_form(r.state_dict()), strict=True)
    return m.to("cuda:0")


# tolerances: those of test_sd_unet_forward (tests/test_gpu_sd_unet.py)
@pytest.mark.parametrize("mode,tol", [("f32", 2e-5), ("bf16", 2.5e-2), ("fp16", 3e-3)])
def test_sd15_unet_forward(mode, tol):
    cfg, r, emb, x, labels, ts, ehs, ref = reference("SD15_TINY")
    assert sum(p.numel() for p in r.parameters()) == 36_014_724
    m = engine(cfg, r, mode)
    assert m.head_dims == (40, 80, 160)
    e = ehs.cuda()
    got = m(x.cuda(), ts.cuda(), e).sample
    assert got.shape == ref["labelled"].shape and got.dtype == torch.float32
    errs = [rel(got, ref["labelled"]),
            rel(m(x.cuda(), ts.cuda(), encoder_hidden_states=torch.zeros_like(e), cross_attention_kwargs=None, return_dict=False)[0], ref["uncond"]),
            rel(m(x.cuda(), 500, e).sample, ref["scalar"])]
    print(f"SD15_TINY forward {mode}: labelled {errs[0]:.3e} zero-context {errs[1]:.3e} scalar-t {errs[2]:.3e}")
    assert max(errs) < tol, errs
    names = {op.what for p in m._plans.values() for op in p.ops}
    assert "attn_hd" in names and "attn_d64" not in names


@pytest.mark.parametrize("mode,tol", [("f32", 2e-5), ("bf16", 2.5e-2)])
def test_mixed_head_dims_run_both_kernels(mode, tol):
    cfg, r, emb, x, labels, ts, ehs, ref = reference("MIXED")
    m = engine(cfg, r, mode)
    assert m.head_dims == (40, 64)
    err = rel(m(x.cuda(), ts.cuda(), ehs.cuda()).sample, ref["labelled"])
    print(f"MIXED forward {mode}: {err:.3e}")
    assert err < tol
    names = [op.what for p in m._plans.values() for op in p.ops]
    assert "attn_hd" in names and "attn_d64" in names


def test_cross_attention_cache_with_the_new_widths():
    cfg, r, emb, x, labels, ts, ehs, ref = reference("SD15_TINY")
    m = engine(cfg, r, "bf16")
    E, other = ehs.cuda(), (ehs.flip(0) * 0.5).cuda()
    xc, tc = x.cuda(), ts.cuda()
    first = m(xc, tc, E).sample.clone()
    again = m(xc, tc, E).sample.clone()             # same tensor object: the cached k / v
    moved = m(xc, tc, other).sample.clone()
    back = m(xc, tc, E).sample.clone()
    fresh = engine(cfg, r, "bf16")(xc, tc, E).sample
    assert torch.equal(first, fresh) and torch.equal(again, fresh) and torch.equal(back, fresh)
    assert not torch.equal(moved, fresh)
    E.mul_(0.5)                                     # in-place change of the context: the cache must notice
    assert not torch.equal(m(xc, tc, E).sample, fresh)


# ---- DDIB on the tiny latent-diffusion stack ---------------------------------------------------------------------------------------------
_DDIB = {}


def ddib_reference():
    if not _DDIB:
        from oracle import AutoencoderKLRef, CustomEmbeddingRef, SDImg2ImgPipelineRef, UNet2DConditionRef, sd_ddib_ref
        torch.manual_seed(0)
        unet = UNet2DConditionRef(**dict(SD15_TINY, use_linear_projection=True)).eval()
        vae = AutoencoderKLRef(**SD_TINY_VAE).eval()
        emb = CustomEmbeddingRef(2, SD15_TINY["cross_attention_dim"])
        pipe = SDImg2ImgPipelineRef(vae, unet, DDIMSchedulerRef(**SD_SCHED), emb)
        x, labels = synth_batch(2, 32)
        out, inverted, latents = sd_ddib_ref(pipe, x, labels, 1 - labels, 2, generator=torch.Generator().manual_seed(11))
        _DDIB.update(pipe=pipe, x=x, labels=labels, out=out, inverted=inverted, latents=latents)
    return _DDIB


def make_pipe(mode):
    import phendiff_amd as P
    d = ddib_reference()
    ref = d["pipe"]
    unet = P.SDUNet2DConditionModel(compute_dtype=mode, **SD15_TINY)
    unet.load_state_dict(to_conv_form(ref.unet.state_dict()), strict=True)
    vae = P.AutoencoderKL(compute_dtype=mode, **SD_TINY_VAE)
    vae.load_state_dict(ref.vae.state_dict())
    emb = P.CustomEmbedding(2, SD15_TINY["cross_attention_dim"])
    emb.load_state_dict(ref.class_embedding.state_dict())
    return d, P.CustomStableDiffusionImg2ImgPipeline(vae.to("cuda:0"), unet.to("cuda:0"), P.DDIMScheduler(**SD_SCHED), emb.to("cuda:0"))


# bounds: those of test_sd_ddib_matches_golden for its tiny pipeline (latent trajectory; decoded images)
@pytest.mark.parametrize("mode,tol,img_tol", [("f32", 2e-5, 2e-5), ("bf16", 3e-2, 6e-2)])
def test_sd15_ddib_eager_and_graph(mode, tol, img_tol):
    import phendiff_amd as P
    d, pipe = make_pipe(mode)
    x, labels = d["x"].cuda(), d["labels"].cuda()
    lat, [cond] = P.LDM_preprocess(pipe, x, [labels], generator=torch.Generator().manual_seed(11))
    inv = P.inversion(pipe, lat, cond, 2)
    eager = P.ddib(pipe, x, labels, 1 - labels, 2, generator=torch.Generator().manual_seed(11))
    errs = (rel(lat, d["latents"]), rel(inv, d["inverted"]), rel(eager, d["out"]))
    print(f"SD15_TINY DDIB {mode}: latents {errs[0]:.3e} inverted {errs[1]:.3e} images {errs[2]:.3e}")
    assert isinstance(eager, np.ndarray) and eager.shape == (2, 32, 32, 3)
    assert errs[0] < tol and errs[1] < tol and errs[2] < img_tol
    g = P.SDDDIBGraph(pipe, batch_size=2, num_inference_steps=2, height=32, width=32)
    out = g.run(x, labels, 1 - labels, generator=torch.Generator().manual_seed(11))
    torch.cuda.synchronize()
    assert torch.equal(out.images.cpu(), torch.from_numpy(eager))


def test_training_plans_are_refused_before_any_launch():
    import phendiff_amd as P
    from phendiff_amd.sd_unet_train import SDUNetTrainer
    m = P.SDUNet2DConditionModel(compute_dtype="bf16", **SD15_TINY).to("cuda:0")
    with pytest.raises(NotImplementedError, match="attention backward"):
        m.input_grad_plan(2, 16, 16, 77, torch.device("cuda:0"))
    with pytest.raises(NotImplementedError, match="attention backward"):
        SDUNetTrainer(m, P.CustomEmbedding(2, 64).to("cuda:0"), P.DDIMScheduler(**SD_SCHED), 1e-4)
    assert m._weights is None and not m._plans           # nothing was packed, no plan exists: no kernel has run
