"""``attention_head_dim`` 16 and 32 of the pixel UNet on MI355X (``pd_attn_hd`` / ``pd_attn_hd_bwd`` on the fused NHWC q|k|v tensor):
``super_small`` with that one key changed against the CPU oracle on identical seeded weights -- forward in the three engines, the full
gradient against torch.autograd, optimisation steps against torch.optim.AdamW, the DDIB transfer eager and captured, and the input
gradient of the guided transfer.  Every bound is the one of the head_dim-8 test named beside it.  64 x 64 inputs put N = 256 tokens on
the attention level (four 64-key tiles, two 128-query blocks); 32 x 32 (N = 64: one tile) where the head_dim-8 test uses it."""
import numpy as np
import pytest
import torch

from test_gpu_unet_backward import batch, compare, oracle_grads
from test_gpu_unet_ddib import rel, synth_batch

pytestmark = pytest.mark.gpu

HEAD_DIMS = (16, 32)


def make_pair(d, size, mode, seed=0):
    import phendiff_amd as P
    from oracle import CondUNet2DRef
    torch.manual_seed(seed)
    cfg = dict(P.UNET_CONFIGS["super_small"], sample_size=size, attention_head_dim=d)
    keys = CondUNet2DRef.__init__.__code__.co_varnames
    r = CondUNet2DRef(**{k: v for k, v in cfg.items() if k in keys}).eval()
    m = P.CustomCondUNet2DModel(compute_dtype=mode, **cfg)
    m.load_state_dict(r.state_dict())
    return r, m.to("cuda:0")


def op_names(m):
    """The forward op names of every launch plan the model has built, one list per plan."""
    plans = [[op.what for op in p.ops] for p in m._plans.values()]
    assert plans
    return plans


# bounds: test_gpu_unet_ddib.py::test_unet_forward_super_small
@pytest.mark.parametrize("mode,tol", [("f32", 2e-5), ("bf16", 2.5e-2), ("fp16", 3e-3)])
@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_unet_forward_head_dims(d, mode, tol, size):
    r, m = make_pair(d, size, mode)
    x, labels = synth_batch(3, size)
    for t in (2999, 640, 0):
        with torch.no_grad():
            ref = r(x, t, class_labels=labels).sample
        got = m(x.cuda(), t, class_labels=labels.cuda()).sample
        assert got.shape == ref.shape and got.dtype == torch.float32
        err = rel(got, ref)
        print(f"unet forward head_dim {d} {mode} {size}x{size} t={t}: {err:.3e}")
        assert err < tol, (d, mode, size, t, err)
    for names in op_names(m):
        assert names.count("attn_hd") == 6 and "attn_d8" not in names and "attn_d64" not in names and "attn_wide" not in names


def test_plans_of_head_dim_8_are_unchanged():
    from test_gpu_unet_ddib import make_pair as make_pair_d8
    _, m = make_pair_d8("super_small", 32, "bf16")
    x, labels = synth_batch(2, 32)
    m(x.cuda(), 10, class_labels=labels.cuda())
    for names in op_names(m):
        assert "attn_hd" not in names and names.count("attn_d8") == 6


# bounds: test_gpu_unet_backward.py::test_unet_backward_matches_autograd (f32, bf16) and
# ::test_scale_shift_resnets_and_the_timestep_class_mlp_train (fp16, under the trainer's loss scale)
@pytest.mark.parametrize("mode,per_tol,glob_tol", [("f32", 2e-4, 2e-5), ("bf16", 8e-2, 2e-2), ("fp16", 3e-2, 6e-3)])
@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_unet_backward_head_dims(d, mode, per_tol, glob_tol, size):
    from phendiff_amd.unet_train import UNetTrainer
    r, m = make_pair(d, size, mode)
    sched, clean, noise, ts, labels, noisy, target = batch(3, size)
    loss_ref, ref = oracle_grads(r, noisy, ts, target, labels=labels)
    tr = UNetTrainer(m, sched, lr=1e-4, use_ema=False)
    scale = tr.opt.scaler.scale if tr.opt.scaler is not None else 1.0
    loss, _ = tr.forward_backward(noisy.cuda(), ts.cuda(), clean.cuda(), noise.cuda(), class_labels=labels.cuda())
    torch.cuda.synchronize()
    assert set(ref) == set(tr.grads)
    assert abs(float(loss) - float(loss_ref)) < {"f32": 1e-5, "bf16": 5e-3, "fp16": 2e-3}[mode] * float(loss_ref)
    kinds = [op.what for op in tr.plan_for(3, size, size).bwd_ops]
    assert kinds.count("attn_hd_bwd") == 6 and "attn_d8_bwd" not in kinds
    compare(ref, {n: g / scale for n, g in tr.grads.items()}, per_tol, glob_tol)


# as test_gpu_unet_backward.py::test_training_steps_follow_torch_adamw_f32, two steps
@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_training_steps_follow_torch_adamw_f32_head_dims(d, size):
    from phendiff_amd.unet_train import UNetTrainer
    r, m = make_pair(d, size, "f32")
    sched, clean, noise, ts, labels, noisy, target = batch(4, size)
    tr = UNetTrainer(m, sched, lr=2e-4, use_ema=True)
    opt = torch.optim.AdamW(r.parameters(), lr=2e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)
    losses_ref, losses = [], []
    for _ in range(2):
        loss_ref, _ = oracle_grads(r, noisy, ts, target, labels=labels)
        torch.nn.utils.clip_grad_norm_(r.parameters(), 1.0)
        opt.step()
        losses_ref.append(float(loss_ref))
        losses.append(float(tr.step(noisy.cuda(), ts.cuda(), clean.cuda(), noise.cuda(), class_labels=labels.cuda())))
    torch.cuda.synchronize()
    assert losses_ref[-1] < losses_ref[0]
    for a, b in zip(losses, losses_ref):
        assert abs(a - b) < 2e-4 * abs(b), (losses, losses_ref)
    sd = r.state_dict()
    num = den = 0.0
    for n, p in m.named_parameters():
        num += float((p.detach().cpu() - sd[n]).double().pow(2).sum())
        den += float((sd[n] - 0).double().pow(2).sum())
    assert (num / den) ** 0.5 < 1e-5
    with torch.no_grad():
        ref_out = r(noisy, ts, class_labels=labels).sample
    got = m(noisy.cuda(), ts.cuda(), class_labels=labels.cuda()).sample
    assert rel(got, ref_out) < 1e-4


# the DDIB transfer, S = 2: eager against the oracle (bounds: test_gpu_unet_ddib.py::test_unet_forward_config_variants), the captured
# trajectory bit-identical to the eager one
@pytest.mark.parametrize("mode,tol", [("f32", 2e-5), ("bf16", 2e-2)])
@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_ddib_head_dims(d, mode, tol, size):
    import phendiff_amd as P
    from oracle import ConditionalDDIMPipelineRef, DDIMSchedulerRef, ddib_ref
    r, m = make_pair(d, size, mode)
    scfg = dict(P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    rpipe = ConditionalDDIMPipelineRef(r, DDIMSchedulerRef(**scfg))
    pipe = P.ConditionalDDIMPipeline(m, P.DDIMScheduler(**scfg))
    x, orig = synth_batch(3, size)
    target = 1 - orig
    want, _ = ddib_ref(rpipe, x, orig, target, 2)
    got = P.ddib(pipe, x.cuda(), orig.cuda(), target.cuda(), 2)
    err = rel(got, want)
    print(f"ddib head_dim {d} {mode} {size}x{size}: {err:.3e}")
    assert err < tol
    runner = P.DDIBGraph(pipe, batch_size=3, num_inference_steps=2, height=size, width=size)
    got_g = runner.run(x.cuda(), orig.cuda(), target.cuda()).images
    assert np.array_equal(got_g.cpu().numpy(), got)
    assert all("attn_hd" in names and "attn_d8" not in names for names in op_names(m))


# as test_gpu_unet_backward.py::test_guidance_gradient_through_unet_matches_autograd, f32
@pytest.mark.parametrize("p", [2, 1.5])
@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_guidance_gradient_head_dims(d, size, p):
    import ctypes as C
    import phendiff_amd as P
    import phendiff_amd._lib as L
    from oracle import ConditionalDDIMPipelineRef, DDIMSchedulerRef, lp_loss_ref
    r, m = make_pair(d, size, "f32")
    cfg = P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
    rp, pp = ConditionalDDIMPipelineRef(r, DDIMSchedulerRef(**cfg)), P.ConditionalDDIMPipeline(m, P.DDIMScheduler(**cfg))
    x, labels = synth_batch(2, size)
    g = torch.Generator().manual_seed(3)
    images = (x + 0.3 * torch.randn(x.shape, generator=g)).requires_grad_(True)
    target = x.clone()
    rp.scheduler.set_timesteps(4)
    t = rp.scheduler.timesteps[1]
    mo = rp.unet(images, t, labels).sample
    x0 = rp.scheduler.step(mo, t, images).pred_original_sample
    losses = lp_loss_ref(x0, target, p)
    (ref,) = torch.autograd.grad([losses[0], losses[1]], images)

    dev = "cuda:0"
    plan = pp.unet.input_grad_plan(2, size, size, torch.device(dev))
    assert [op.what for op in plan.bwd_ops].count("attn_hd_bwd") == 6
    st = torch.cuda.current_stream().cuda_stream
    im, tg, lb = images.detach().to(dev).contiguous(), target.to(dev), labels.to(dev)
    out, d_out, d_dir = (torch.empty_like(im) for _ in range(3))
    pp.scheduler.set_timesteps(4)
    plan.forward(im, torch.full((2,), float(t), device=dev), lb, None, out, st)
    sa, sb, _, _, _ = pp.scheduler.step_coefficients(t)
    partial = torch.empty(2 * 4, dtype=torch.float64, device=dev)
    ls = torch.empty(2, device=dev)
    a = L.LpGuidanceArgs(numel=im.numel(), per_sample=im[0].numel(), pred_type=2, clip=1, clip_range=1.0, sqrt_a=sa, sqrt_b=sb,
                         p=float(p), sample=im.data_ptr(), model_out=out.data_ptr(), target=tg.data_ptr(),
                         partial=partial.data_ptr(), splits=4, d_model_out=d_out.data_ptr(), d_sample_direct=d_dir.data_ptr(),
                         losses=ls.data_ptr())
    L.check(L.lib().pd_lp_guidance(C.byref(a), st), "pd_lp_guidance")
    plan.backward(d_out, st)
    torch.cuda.synchronize()
    assert torch.isfinite(plan.dsample).all()
    assert rel(ls, losses.detach()) < 1e-5
    err = rel(d_dir + plan.dsample, ref)
    print(f"guidance gradient head_dim {d} {size}x{size} p={p}: {err:.3e}")
    assert err < 2e-5
