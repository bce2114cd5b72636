"""`--components_to_train autoencoder` on MI355X (args_parser.py:34-41; train.py:189-199, 268-285; utils_training.py:237-256,
415-433): pd_latent_chain_bwd, the encoder's backward plan and `SDUNetTrainer.step_images` against torch.autograd /
torch.optim.AdamW over the oracle's fp32 CPU modules (oracle.vae_ref, oracle.sd_unet_ref, oracle.schedulers_ref)."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from test_gpu_guard_bands import Case, Op, out_op, p1_poisoned_surroundings, p2_canaried_outputs
from test_gpu_kernels import DT, bf16_round, env, rel, stream  # noqa: F401
from test_gpu_sd_unet import TINY
from test_gpu_sd_unet import make_pair as make_unet_pair
from test_gpu_unet_backward import compare
from test_gpu_vae import CFGS
from test_gpu_vae import make_pair as make_vae_pair

pytestmark = pytest.mark.gpu

TINY_VAE = CFGS["d64"][0]                       # the tiny configuration tests/test_gpu_vae.py encodes / decodes with
SD_SHAPED_VAE = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2)      # the SD VAE: one 512-wide head in the mid block
# per-parameter / global gradient tolerances of tests/test_gpu_sd_unet_backward.py for the same engines
GRAD_TOL = {"f32": (3e-4, 3e-5), "bf16": (1e-1, 2.5e-2), "fp16": (4e-2, 8e-3)}
# Where the bf16 engine needs more than those bounds at these shapes, the bound is 2 x the error of the ORACLE run under
# torch.autocast("cpu", bfloat16) against its fp32 self on the same weights, input and upstream gradient (measured on the CPU, docs/LAB_r7.md):
#   tiny VAE, 32 x 32, B = 2: parameters whose gradient is mathematically zero (conv1.bias in front of a GroupNorm with ONE channel per group:
#     32 channels / 32 groups) hold round-off of 3.56e-5 x the global gradient norm under autocast  ->  7.1e-5 (f32 / fp16 keep compare()'s 1e-5)
#   SD-shaped VAE, 128 x 128, B = 2: global relative error 2.92e-2 under autocast  ->  5.85e-2 (the per-parameter bound 1e-1 stays)
BF16_ZERO_GRAD_TOL_TINY = 7.1e-5
BF16_GLOBAL_TOL_SD_SHAPED = 5.85e-2
SCALE = 0.18215


def compare_grads(ref, got, per_param_tol, global_tol, zero_tol=1e-5):
    """tests/test_gpu_unet_backward.py::compare with the bound on mathematically-zero gradients as a parameter (its 1e-5 by default);
    prints every figure before it asserts."""
    gnorm = sum(float(g.double().pow(2).sum()) for g in ref.values()) ** 0.5
    num, worst, worst_zero = 0.0, (0.0, None), (0.0, None)
    for n, gr in ref.items():
        d = got[n].cpu() - gr
        num += float(d.double().pow(2).sum())
        if float(gr.norm()) > 1e-6 * gnorm:
            worst = max(worst, (float(d.norm() / gr.norm()), n))
        else:
            worst_zero = max(worst_zero, (float(d.norm()) / gnorm, n))
    print("gradients: global", num ** 0.5 / gnorm, "worst parameter", worst, "worst zero-gradient parameter (/ global norm)", worst_zero)
    assert worst[0] < per_param_tol, worst
    assert worst_zero[0] < zero_tol, worst_zero
    assert num ** 0.5 / gnorm < global_tol
SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
             set_alpha_to_one=False, steps_offset=1)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------
def chain_inputs(B=3, Cl=4, h=6, w=5, seed=11):
    g = torch.Generator().manual_seed(seed)
    moments = torch.randn(B, 2 * Cl, h, w, generator=g)
    lv = moments[:, Cl:] * 3.0
    flat = lv.view(-1)                           # log-variances below -30, inside the range, above 20, and AT both ends (inclusive mask)
    flat[0::7] = -35.0 - flat[0::7].abs()
    flat[1::7] = 22.0 + flat[1::7].abs()
    flat[2], flat[3] = -30.0, 20.0
    moments[:, Cl:] = lv
    eps, noise = torch.randn(B, Cl, h, w, generator=g), torch.randn(B, Cl, h, w, generator=g)
    g_noisy, g_out = torch.randn(B, Cl, h, w, generator=g), torch.randn(B, Cl, h, w, generator=g)
    acp = torch.tensor([0.9, 0.35, 0.02][:B])
    return moments, eps, noise, g_noisy, g_out, acp.sqrt(), (1 - acp).sqrt()


def chain_autograd(moments, eps, noise, sa, sb, pt, model_out):
    """d loss / d moments by autograd of scale * (mean + exp(0.5 clamp(logvar, -30, 20)) eps) -> add_noise -> the three losses
    (utils_training.py:415-433; clean_images is NOT detached in the target); also d loss / d noisy and d loss / d model_out."""
    m = moments.clone().requires_grad_(True)
    Cl = m.shape[1] // 2
    z = SCALE * (m[:, :Cl] + torch.exp(0.5 * m[:, Cl:].clamp(-30.0, 20.0)) * eps)
    a, b = sa.view(-1, 1, 1, 1), sb.view(-1, 1, 1, 1)
    noisy = a * z + b * noise
    # the UNet stands between noisy and model_out: any differentiable map does for the kernel's contract -- here out = tanh(noisy) + model_out
    out = torch.tanh(noisy) + model_out
    out.retain_grad()
    if pt == "epsilon":
        loss = F.mse_loss(out, noise)
    elif pt == "sample":
        snr = (sa ** 2 / sb ** 2).view(-1, 1, 1, 1)
        loss = (snr * F.mse_loss(out, z, reduction="none")).mean()
    else:
        loss = F.mse_loss(out, a * noise - b * z)
    loss.backward()
    g_out = out.grad
    g_noisy = g_out * (1 - torch.tanh(noisy.detach()) ** 2)          # what the UNet's input gradient hands over (without the direct path a * ...)
    return m.grad, g_noisy, g_out


def launch_chain(L, lib, mode, moments, eps, g_noisy, g_out, sa, sb, pt, out):
    code, _ = DT[mode]
    B, C2, h, w = moments.shape
    a = L.LatentChainBwdArgs(dtype=code, B=B, C=C2 // 2, HW=h * w, Cpad=out.shape[-1], pred_type=L.PD_PRED[pt], scale=SCALE,
                             g_noisy=g_noisy.data_ptr(), g_out=g_out.data_ptr(), moments=moments.data_ptr(), eps=eps.data_ptr(),
                             sa=sa.data_ptr(), sb=sb.data_ptr(), out=out.data_ptr())
    L.check(lib.pd_latent_chain_bwd(C.byref(a), stream()), "pd_latent_chain_bwd")


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("pt", ["epsilon", "sample", "v_prediction"])
def test_latent_chain_bwd_matches_autograd(env, mode, pt):
    L, lib, _, dev = env
    _, tdt = DT[mode]
    moments, eps, noise, _, _, sa, sb = chain_inputs()
    model_out = torch.randn(moments.shape[0], 4, *moments.shape[2:], generator=torch.Generator().manual_seed(5))
    ref, g_noisy, g_out = chain_autograd(moments, eps, noise, sa, sb, pt, model_out)
    lv = moments[:, 4:]
    assert int((lv < -30).sum()) > 3 and int((lv > 20).sum()) > 3 and int(((lv > -30) & (lv < 20)).sum()) > 3
    assert float(ref[:, 4:][lv < -30].abs().max()) == 0.0 and float(ref[:, 4:][lv > 20].abs().max()) == 0.0
    d = [t.to(dev).contiguous() for t in (moments, eps, g_noisy, g_out, sa, sb)]
    out = torch.full((moments.shape[0], moments.shape[2], moments.shape[3], 32), float("nan"), dtype=tdt, device=dev)
    launch_chain(L, lib, mode, *d, pt, out)
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert float(got[..., 8:].abs().max()) == 0.0                   # the pad lanes are WRITTEN, as zero
    want = ref.permute(0, 2, 3, 1)
    if mode == "f32":                                               # rtol of the scheduler kernel tests
        assert torch.allclose(got[..., :8], want, rtol=1e-5, atol=1e-7), float((got[..., :8] - want).abs().max())
    else:                                                           # only the output cast may differ: compare after the same cast
        cast = want.to(tdt).float()
        # The fp32 values before the cast agree within the f32 criterion above (rtol 1e-5, atol 1e-7: `sa g_noisy - g_out` cancels, and
        # expf / torch.exp differ by fp32 round-off); the cast can then land on the neighbouring 16-bit number: one unit in the last place
        # (2^-7 of the value for bf16, 2^-10 for fp16; 6e-8 = fp16's subnormal spacing).  Bound = that fp32 difference + one 16-bit step.
        ulp = 2.0 ** (-7 if mode == "bf16" else -10)
        # (an element both sides cast to the same value -- an fp16 overflow to the same infinity included -- has no error: inf - inf is NaN)
        same = got[..., :8] == cast
        assert bool(torch.isfinite(got[..., :8][~same]).all()) and bool(torch.isfinite(cast[~same]).all())
        err = torch.where(same, torch.zeros_like(cast), (got[..., :8] - cast).abs())
        tol = torch.where(same, torch.ones_like(cast), ulp * cast.abs() + 6e-8 + 1e-5 * want.abs() + 1e-7)
        print(mode, pt, "max err / tol", float((err / tol).max()), "exact", float((got[..., :8] == cast).float().mean()))
        assert bool((err <= tol).all())
        assert float((got[..., :8] == cast).float().mean()) > 0.98


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("prop", ["poisoned-surroundings", "canaried-outputs"])
def test_latent_chain_bwd_guard_bands(env, mode, prop, monkeypatch):
    """P1 / P2 of tests/test_gpu_guard_bands.py on every operand; the canaried output's body starts as NaN, so finite pad lanes were written."""
    L, lib, _, dev = env
    _, tdt = DT[mode]
    moments, eps, noise, g_noisy, g_out, sa, sb = chain_inputs(B=3, h=9, w=7)
    ins = {k: Op(v, sample_dim=0) for k, v in dict(moments=moments, eps=eps, g_noisy=g_noisy, g_out=g_out, sa=sa, sb=sb).items()}
    outs = {"out": out_op((3, 9, 7, 32), tdt, sample_dim=0)}

    def launch(T):
        launch_chain(L, lib, mode, T["moments"], T["eps"], T["g_noisy"], T["g_out"], T["sa"], T["sb"], "v_prediction", T["out"])

    def check(got):
        o = got["out"].float()
        g = SCALE * (sa.view(-1, 1, 1, 1) * g_noisy + sb.view(-1, 1, 1, 1) * g_out)
        lv = moments[:, 4:]
        want = torch.cat([g, torch.where((lv >= -30) & (lv <= 20), g * eps * 0.5 * torch.exp(0.5 * lv), torch.zeros_like(g))], 1).permute(0, 2, 3, 1)
        assert float(o[..., 8:].abs().max()) == 0.0
        assert rel(o[..., :8], want) < (1e-6 if mode == "f32" else 4e-3)

    case = Case(ins, outs, launch, check, nsamples=3)
    (p1_poisoned_surroundings if prop == "poisoned-surroundings" else p2_canaried_outputs)(case, dev, monkeypatch)


# ---- 2 / 3. the encoder's gradient ---------------------------------------------------------------------------------------------------
def encoder_plan(m, B, H, W):
    """A VaeEncodeTrainPlan over flat fp32 buffers laid out as the trainer lays them out."""
    import phendiff_amd as P
    from phendiff_amd.training import FlatAdamWEMA
    from phendiff_amd.vae import _VaeWeights
    from phendiff_amd.vae_train import VaeEncodeTrainPlan, VaeTrainWeights, vae_never_graded
    order = P.vae_training_param_order(m)
    opt = FlatAdamWEMA([p for _, p in order], 0.0, use_ema=False)
    params, grads = {n: p.data for n, p in order}, {n: p.grad for n, p in order}
    m.invalidate()
    m._weights = _VaeWeights(m, m.device)
    tw = VaeTrainWeights(m, m.device, m._weights.tdt)
    return VaeEncodeTrainPlan(m, m._weights, tw, B, H, W, m.device, params, grads, frozen=vae_never_graded(m)), grads, opt


def encoder_grads_vs_autograd(cfg, mode, B, H, W, tol, zero_tol=1e-5):
    _, tdt = DT[mode]
    r, m = make_vae_pair(cfg, mode)
    g = torch.Generator().manual_seed(21)
    x = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    for p in r.parameters():
        p.requires_grad_(True)
    mom_ref = r.quant_conv(r.encoder(x))
    G = bf16_round(torch.randn(mom_ref.shape, generator=g), mode)          # d loss / d moments, as the engine stores it
    (mom_ref * G).sum().backward()
    ref = {n: p.grad for n, p in r.named_parameters() if n.startswith("encoder.") or n.startswith("quant_conv.")}
    assert len(ref) == sum(1 for n, _ in m.named_parameters() if n.startswith("encoder.") or n.startswith("quant_conv."))
    plan, grads, _ = encoder_plan(m, B, H, W)
    mom = torch.empty(mom_ref.shape, device="cuda:0")
    plan.forward(x.cuda(), mom, stream())
    d = torch.zeros(B, mom.shape[2], mom.shape[3], 32, dtype=tdt, device="cuda:0")
    d[..., :mom.shape[1]] = G.permute(0, 2, 3, 1).to(tdt)
    plan.backward(d, stream())
    torch.cuda.synchronize()
    assert rel(mom, mom_ref.detach()) < {"f32": 3e-5, "bf16": 5e-2, "fp16": 8e-3}[mode]      # tests/test_gpu_vae.py's encode bounds
    compare_grads(ref, grads, *tol, zero_tol=zero_tol)
    # the decoder and post_quant_conv never receive a gradient
    assert all(float(grads[n].abs().max()) == 0.0 for n in grads if n.startswith("decoder.") or n.startswith("post_quant_conv."))
    return plan, grads, ref


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
def test_encoder_backward_matches_autograd_tiny(mode):
    """Every encoder.* / quant_conv.* gradient of the tiny VAE at 32 x 32, B = 2; a second backward accumulates."""
    zero_tol = BF16_ZERO_GRAD_TOL_TINY if mode == "bf16" else 1e-5
    plan, grads, ref = encoder_grads_vs_autograd(TINY_VAE, mode, 2, 32, 32, GRAD_TOL[mode], zero_tol)
    plan.backward(plan.dmom, stream())
    torch.cuda.synchronize()
    compare_grads({n: 2 * g for n, g in ref.items()}, grads, *GRAD_TOL[mode], zero_tol=zero_tol)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encoder_backward_matches_autograd_sd_shaped(mode):
    """The SD VAE's widths (128 / 256 / 512 / 512, one 512-wide attention head) at 128 x 128, B = 2: the 128-channel full-resolution
    layers, the pre-applied GroupNorm path (512 output channels) and pd_attn_wide_bwd."""
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    tol = GRAD_TOL[mode] if mode == "f32" else (GRAD_TOL[mode][0], BF16_GLOBAL_TOL_SD_SHAPED)
    encoder_grads_vs_autograd(SD_SHAPED_VAE, mode, 2, 128, 128, tol)


# ---- 4 .. 7. the trainer ---------------------------------------------------------------------------------------------------------------
def trainer_batch(B=2, size=32, seed=31):
    import phendiff_amd as P
    sched = P.DDIMScheduler(**SCHED, prediction_type="v_prediction")
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, size, size, generator=g) * 2 - 1
    noise, pn = torch.randn(B, 4, size // 2, size // 2, generator=g), torch.randn(B, 4, size // 2, size // 2, generator=g)
    ts = torch.tensor([850, 300, 12, 999][:B])
    return sched, x, noise, pn, ts, torch.arange(B) % 2


def make_trainer(mode, sched, lr=2e-4, freeze_vae=False, **kw):
    import phendiff_amd as P
    r, emb, m, e2 = make_unet_pair(TINY, mode)
    rv, v = make_vae_pair(TINY_VAE, mode, seed=1)
    if freeze_vae:
        v.requires_grad_(False)
    return (r, emb, rv), P.SDUNetTrainer(m, e2, sched, lr=lr, vae=v, **kw)


def oracle_step(r, emb, rv, sched, x, noise, pn, ts, labels):
    """utils_training.py:237-256, 415-433 with v_prediction: encode INSIDE the step, the target is not detached."""
    from oracle import class_emb_to_encoder_hidden_states as ehs_ref
    acp = sched.alphas_cumprod[ts]
    sa, sb = (acp ** 0.5).view(-1, 1, 1, 1), ((1 - acp) ** 0.5).view(-1, 1, 1, 1)
    lat = rv.encode(x).latent_dist.sample(noise=pn) * rv.config.scaling_factor
    out = r(sa * lat + sb * noise, ts, ehs_ref(emb(labels))).sample
    loss = F.mse_loss(out, sa * noise - sb * lat)
    loss.backward()
    return loss.detach()


def test_chunked_encoder_accumulates_the_same_gradients():
    sched, x, noise, pn, ts, labels = trainer_batch()
    got = []
    for chunk in (1, 2):
        _, tr = make_trainer("f32", sched, use_ema=False, _vae_chunk=chunk)
        tr.images_forward_backward(x.cuda(), ts.cuda(), noise.cuda(), labels.cuda(), posterior_noise=pn.cuda())
        torch.cuda.synchronize()
        assert len(tr._vplans) == 2 // chunk
        got.append({n: g.clone() for n, g in tr.grads.items()})
    whole = {n: g.cpu() for n, g in got[1].items() if n.startswith("vae.") and n not in tr.never_graded}
    assert whole and all(float(g.abs().max()) > 0 for n, g in whole.items())
    compare(whole, got[0], *GRAD_TOL["f32"])


def test_step_images_follows_torch_adamw_f32():
    """Three steps with a fixed posterior noise against ONE torch.optim.AdamW over (vae, unet, class embedding) and
    clip_grad_norm_(..., 1.0), plus a test-local EMA (the update tests/test_oracle_training.py checks the decay of)."""
    from oracle import ema_decay_ref
    sched, x, noise, pn, ts, labels = trainer_batch()
    (r, emb, rv), tr = make_trainer("f32", sched)
    v = tr.vae
    init = {n: p.detach().clone() for n, p in v.named_parameters()}
    allp = list(rv.parameters()) + list(r.parameters()) + list(emb.parameters())
    for p in allp:
        p.requires_grad_(True)
    opt = torch.optim.AdamW(allp, lr=2e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)
    ema = [p.detach().clone() for p in rv.parameters()]
    for k in range(3):
        opt.zero_grad(set_to_none=True)
        loss_ref = oracle_step(r, emb, rv, sched, x, noise, pn, ts, labels)
        assert all(p.grad is None for n, p in rv.named_parameters() if n.startswith("decoder.") or n.startswith("post_quant_conv."))
        torch.nn.utils.clip_grad_norm_(allp, 1.0)
        opt.step()
        d = ema_decay_ref(k + 1)
        for s, p in zip(ema, rv.parameters()):
            s.sub_((1 - d) * (s - p.detach()))
        loss = tr.step_images(x.cuda(), ts.cuda(), noise.cuda(), labels.cuda(), posterior_noise=pn.cuda())
        assert abs(float(loss) - float(loss_ref)) < 2e-4 * abs(float(loss_ref)), (k, float(loss), float(loss_ref))
    torch.cuda.synchronize()

    def rel_sd(named, sd):
        num = den = 0.0
        for n, p in named:
            num += float((p.detach().cpu() - sd[n]).double().pow(2).sum())
            den += float(sd[n].double().pow(2).sum())
        return (num / den) ** 0.5
    assert rel_sd(v.named_parameters(), rv.state_dict()) < 1e-5
    assert rel_sd(tr.model.named_parameters(), r.state_dict()) < 1e-5
    assert rel(tr.class_embedding.inner_module.weight.detach(), emb.inner_module.weight.detach()) < 1e-5
    moved = [n for n, p in v.named_parameters() if not torch.equal(p.detach(), init[n])]
    assert moved and all(n.startswith("encoder.") or n.startswith("quant_conv.") for n in moved)      # decoder / post_quant_conv: bit-identical
    # EMA of the autoencoder (never-graded parameters included: their shadow is the unchanged parameter)
    off, shadow = 0, {}
    for n, t in tr.params.items():
        shadow[n] = tr.opt.ema[off:off + t.numel()].view_as(t)
        off += t.numel()
    assert rel_sd([(n, shadow["vae." + n]) for n, _ in rv.named_parameters()], dict(zip([n for n, _ in rv.named_parameters()], ema))) < 1e-5
    # the inference entry point sees the stepped weights
    with torch.no_grad():
        want = rv.encode(x).latent_dist
    got = v.encode(x.cuda()).latent_dist
    assert rel(got.mean, want.mean) < 1e-4 and rel(got.sample(noise=pn.cuda()), want.sample(noise=pn)) < 1e-4


def test_vae_device_repack_equals_host_packing():
    """After `step_images` the pd_pack_weight path must leave exactly what packing.py builds from the new parameters in the
    `encoder.*` / `quant_conv` entries of `_VaeWeights` and in all of `VaeTrainWeights`; the decoder's entries are not touched."""
    from phendiff_amd.vae import _VaeWeights
    from phendiff_amd.vae_train import VaeTrainWeights
    from test_host_weight_layout import tensors
    sched, x, noise, pn, ts, labels = trainer_batch()
    _, tr = make_trainer("f32", sched, lr=1e-3)
    v = tr.vae
    tr._bind_vae_weights()                   # (what the first encoder plan does: the sets the step and the re-pack are bound to)
    w = v._weights
    decoder = {path: t.clone() for path, t in tensors(w, "w") if ".decoder." in path or path.split(".")[1].startswith(("dec_", "post_quant_"))}
    before = v.encoder.conv_in.weight.detach().clone()
    tr.step_images(x.cuda(), ts.cuda(), noise.cuda(), labels.cuda(), posterior_noise=pn.cuda())
    torch.cuda.synchronize()
    assert v._weights is w and not torch.equal(v.encoder.conv_in.weight.detach(), before)
    have = dict(list(tensors(w, "w")) + list(tensors(tr._vtw, "tw")))
    fresh = dict(list(tensors(_VaeWeights(v, "cuda:0"), "w")) + list(tensors(VaeTrainWeights(v, "cuda:0", w.tdt), "tw")))
    assert set(have) == set(fresh) and decoder and len(have) > len(decoder)
    for kind in ("w.enc_in_w", "w.enc_out_w", "w.enc_out_b", "w.quant_w", "w.quant_b", "tw.enc_out_d", "tw.quant_d", ".wqkvd", ".wsd", ".wd"):
        assert any(path.endswith(kind) for path in have), kind
    for path, t in have.items():
        assert torch.equal(t, fresh[path]), path
    for path, t in decoder.items():
        assert torch.equal(have[path], t), path


def test_step_images_with_a_frozen_vae_is_todays_step():
    sched, x, noise, pn, ts, labels = trainer_batch()
    _, a = make_trainer("bf16", sched, freeze_vae=True)
    _, b = make_trainer("bf16", sched, freeze_vae=True)
    assert not a._vae_trains and not any(n.startswith("vae.") for n in a.params)
    assert [i for i, _, _ in a.checkpoint_modules()] == [0, 2]
    lat = b.vae.encode(x.cuda()).latent_dist.sample(noise=pn.cuda(), scale=b.vae.config.scaling_factor)
    noisy = sched.add_noise(lat, noise.cuda(), ts.cuda())
    for _ in range(2):
        la = a.step_images(x.cuda(), ts.cuda(), noise.cuda(), labels.cuda(), posterior_noise=pn.cuda())
        lb = b.step(noisy, ts.cuda(), lat, noise.cuda(), labels.cuda())
    torch.cuda.synchronize()
    assert float(la) == float(lb) and torch.equal(a.opt.flat, b.opt.flat)
    with pytest.raises(ValueError, match="step_images"):
        make_trainer("bf16", sched)[1].step(noisy, ts.cuda(), lat, noise.cuda(), labels.cuda())


def test_fp16_overflow_skips_the_step_for_the_vae_too():
    sched, x, noise, pn, ts, labels = trainer_batch()
    _, tr = make_trainer("fp16", sched, lr=5e-4)
    args = (x.cuda(), ts.cuda(), noise.cuda(), labels.cuda())
    tr.opt.scaler.scale = 2.0 ** 40
    before = tr.opt.flat.clone()
    tr.step_images(*args, posterior_noise=pn.cuda())
    torch.cuda.synchronize()
    assert tr.opt.scaler.scale == 2.0 ** 39 and tr.opt.t == 0 and tr.opt.scaler.skipped == 1
    assert torch.equal(tr.opt.flat, before) and float(tr.opt.exp_avg.abs().max()) == 0.0 and float(tr.opt.exp_avg_sq.abs().max()) == 0.0
    assert float(tr.opt.grad.abs().max()) == 0.0
    tr.opt.scaler.scale = 65536.0
    losses = [float(tr.step_images(*args, posterior_noise=pn.cuda())) for _ in range(6)]
    torch.cuda.synchronize()
    assert tr.opt.t == 6 and torch.isfinite(tr.opt.flat).all() and min(losses[-2:]) < losses[0]
    off = 0
    for n, t in tr.params.items():
        if n == "vae.encoder.conv_in.weight":
            assert float((tr.opt.flat[off:off + t.numel()] - before[off:off + t.numel()]).abs().max()) > 0
        off += t.numel()


def test_save_state_resume_continues_bitwise_with_the_vae(tmp_path):
    """tests/test_gpu_sd_unet_backward.py::test_sd_save_state_resume_continues_bitwise with the VAE as model 1."""
    sched, x, noise, pn, ts, labels = trainer_batch()
    args = (x.cuda(), ts.cuda(), noise.cuda(), labels.cuda())
    _, a = make_trainer("bf16", sched, lr=3e-4)
    for _ in range(2):
        a.step_images(*args, posterior_noise=pn.cuda())
    folder = str(tmp_path / "step_2")
    a.save_state(folder)
    assert sorted(os.listdir(folder)) == ["custom_checkpoint_0.pkl", "custom_checkpoint_1.pkl", "custom_checkpoint_2.pkl", "optimizer.bin",
                                          "pytorch_model.bin", "pytorch_model_1.bin", "pytorch_model_2.bin", "random_states_0.pkl", "scheduler.bin"]
    sd1 = torch.load(os.path.join(folder, "pytorch_model_1.bin"))
    assert sorted(sd1) == sorted(a.vae.state_dict()) and "decoder.conv_in.weight" in sd1
    osd = torch.load(os.path.join(folder, "optimizer.bin"))
    vnames = [n for n, _ in a.vae.named_parameters()]
    assert all((i in osd["state"]) == (n.startswith("encoder.") or n.startswith("quant_conv.")) for i, n in enumerate(vnames))
    third = float(a.step_images(*args, posterior_noise=pn.cuda()))
    _, b = make_trainer("bf16", sched, lr=3e-4)
    with torch.no_grad():
        b.vae.quant_conv.weight.data.add_(1.0)           # a resumed run starts from different weights: the checkpoint must win
    b.load_state(folder)
    assert b.opt.t == 2
    resumed = float(b.step_images(*args, posterior_noise=pn.cuda()))
    torch.cuda.synchronize()
    assert resumed == third
    assert torch.equal(b.opt.flat, a.opt.flat) and torch.equal(b.opt.ema, a.opt.ema)
    assert torch.equal(b.opt.exp_avg, a.opt.exp_avg) and torch.equal(b.opt.exp_avg_sq, a.opt.exp_avg_sq)
