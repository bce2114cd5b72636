"""The pixel UNet with 4 to 32 image channels on MI355X: conv_in over a 32-channel zero-padded NHWC buffer (the latent tier's form)
instead of the im2col form, which ends at 3.  Forward against the CPU oracle, backward against torch.autograd, two AdamW steps against
torch.optim.AdamW, and every driver of the UNet at C = 5 against the oracle and against itself (eager == captured, bit for bit).  The
bounds are those of the 3-channel tests, read from their parametrisation."""
import numpy as np
import pytest
import torch

import test_gpu_unet_backward as UB
import test_gpu_unet_ddib as UD
from test_gpu_guided_graph import PIXEL_TOL, _marks
from test_gpu_unet_ddib import rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 3

FWD_TOL = dict(_marks(UD.test_unet_forward_super_small, "mode,tol"))
BWD_TOL = {m: (p, g) for m, p, g in _marks(UB.test_unet_backward_matches_autograd, "mode,per_tol,glob_tol")}
# fp16 under the loss scale: the fp16 row of the parametrisation that has one
BWD_TOL["fp16"] = next((p, g) for m, p, g in _marks(UB.test_scale_shift_resnets_and_the_timestep_class_mlp_train, "mode,per_tol,glob_tol")
                       if m == "fp16")
DDIB_TOL = dict(_marks(UD.test_ddib_eager_and_graph_vs_oracle, "mode,tol"))
PIPELINE_TOL = 2e-4        # test_pipeline_cfg_and_forward_noise_f32 / test_cfg_forward_start_eager_and_graph_vs_oracle (literals in their bodies)


def make_pair(cin, cout, mode, hw=(32, 32), seed=0, **extra):
    """(oracle, engine model on the GPU) of a super_small-shaped config with `cin` / `cout` image channels, same seeded weights."""
    import phendiff_amd as P
    from oracle import CondUNet2DRef
    torch.manual_seed(seed)
    cfg = dict(P.UNET_CONFIGS["super_small"], sample_size=hw[0] if hw[0] == hw[1] else list(hw), in_channels=cin, out_channels=cout, **extra)
    keys = CondUNet2DRef.__init__.__code__.co_varnames
    r = CondUNet2DRef(**{k: v for k, v in cfg.items() if k in keys}).eval()
    m = P.CustomCondUNet2DModel(compute_dtype=mode, **cfg)
    m.load_state_dict(r.state_dict())
    return r, m.to(DEV)


def synth(B, c, hw=(32, 32), seed=1234):
    g = torch.Generator().manual_seed(seed + c)
    labels = torch.arange(B) % 2
    x = torch.rand(B, c, *hw, generator=g) * 2 - 1
    return (x + 0.25 * (2 * labels.float() - 1).view(B, 1, 1, 1)).clamp(-1, 1), labels


def pipes(mode, c=5):
    import phendiff_amd as P
    from oracle import ConditionalDDIMPipelineRef, DDIMSchedulerRef
    r, m = make_pair(c, c, mode)
    cfg = P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]
    return ConditionalDDIMPipelineRef(r, DDIMSchedulerRef(**cfg)), P.ConditionalDDIMPipeline(m, P.DDIMScheduler(**cfg))


def plan_kinds(plan):
    return [op.what for op in plan.ops]


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("cin,cout,hw", [(4, 4, (32, 32)), (5, 5, (32, 32)), (8, 8, (32, 32)), (32, 32, (32, 32)), (5, 2, (32, 32)),
                                         (5, 5, (16, 48))], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_forward_vs_oracle(cin, cout, hw, mode):
    r, m = make_pair(cin, cout, mode, hw)
    x, labels = synth(2, cin, hw)
    for t in (2999, 640):
        with torch.no_grad():
            ref = r(x, t, class_labels=labels).sample
        got = m(x.cuda(), t, class_labels=labels.cuda()).sample
        assert got.shape == ref.shape == (2, cout, *hw) and got.dtype == torch.float32
        e = rel(got, ref)
        print(f"forward {cin}->{cout} {hw} {mode} t={t}: rel L2 {e:.3e} (bound {FWD_TOL[mode]})")
        assert e < FWD_TOL[mode]
    kinds = plan_kinds(m.plan_for(2, *hw, torch.device(DEV)))
    assert kinds[:2] == ["nchw_to_nhwc", "conv_in"] and kinds.count("nchw_to_nhwc") == 1


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_forward_centered_input(mode):
    r, m = make_pair(5, 5, mode, center_input_sample=True)
    x, labels = synth(2, 5)
    x = x / 2 + 0.5                                     # the [0, 1] range such a model is fed
    with torch.no_grad():
        ref = r(x, 640, class_labels=labels).sample
    got = m(x.cuda(), 640, class_labels=labels.cuda()).sample
    e = rel(got, ref)
    print(f"forward centred 5->5 {mode}: rel L2 {e:.3e} (bound {FWD_TOL[mode]})")
    assert e < FWD_TOL[mode]
    assert plan_kinds(m.plan_for(2, 32, 32, torch.device(DEV)))[:3] == ["center", "nchw_to_nhwc", "conv_in"]


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
def test_pad_channels_are_rewritten_on_every_run(mode):
    """A zero weight does not cancel a NaN: whatever the padded input buffer held, channels C..31 are zero when conv_in reads them."""
    _, m = make_pair(5, 5, mode)
    x, labels = synth(2, 5)
    first = m(x.cuda(), 640, class_labels=labels.cuda()).sample.clone()
    plan = m.plan_for(2, 32, 32, torch.device(DEV))
    rec = plan.tape[0]
    assert rec.kind == "conv_in_padded" and tuple(rec.x.shape) == (2, 32, 32, 32)
    rec.x.fill_(float("nan"))
    again = m(x.cuda(), 640, class_labels=labels.cuda()).sample
    torch.cuda.synchronize()
    assert torch.isfinite(again).all() and torch.equal(first.view(torch.int32), again.view(torch.int32))
    assert float(rec.x[..., 5:].float().abs().max()) == 0.0 and torch.isfinite(rec.x).all()


@pytest.mark.parametrize("cin", [1, 3])
def test_three_channels_and_fewer_keep_the_im2col_form(cin):
    _, m = make_pair(cin, cin, "bf16")
    plan = m.plan_for(2, 32, 32, torch.device(DEV))
    kinds = plan_kinds(plan)
    assert kinds[0] == "conv_in" and "nchw_to_nhwc" not in kinds
    assert plan.ops[0].args.im2col3 == cin and plan.ops[0].args.ksize == 1 and plan.tape[0].kind == "conv_in"
    assert m._weights.conv_in_wp is None and m._weights.conv_in_wv is not None


# ---- backward --------------------------------------------------------------------------------------------------------------------------
def train_batch(B, c, size=32, seed=5):
    import phendiff_amd as P
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    g = torch.Generator().manual_seed(seed)
    clean = torch.rand(B, c, size, size, generator=g) * 2 - 1
    noise = torch.randn(B, c, size, size, generator=g)
    ts = torch.tensor([2500, 700, 40, 1500][:B])
    labels = torch.arange(B) % 2
    acp = sched.alphas_cumprod[ts]
    sa, sb = (acp ** 0.5).view(-1, 1, 1, 1), ((1 - acp) ** 0.5).view(-1, 1, 1, 1)
    return sched, clean, noise, ts, labels, sa * clean + sb * noise, sa * noise - sb * clean


def autograd_reference(r, noisy, ts, target, labels):
    x = noisy.clone().requires_grad_(True)
    for p in r.parameters():
        p.requires_grad_(True)
        p.grad = None
    loss = torch.nn.functional.mse_loss(r(x, ts, class_labels=labels).sample, target)
    loss.backward()
    return loss.detach(), {n: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for n, p in r.named_parameters()}, x.grad


@pytest.mark.parametrize("mode,centered", [("f32", False), ("f32", True), ("bf16", False), ("bf16", True), ("fp16", False)],
                         ids=["f32", "f32-centred", "bf16", "bf16-centred", "fp16"])
def test_backward_matches_autograd(mode, centered):
    from phendiff_amd.img2img import GUIDANCE_GRAD_SCALE
    from phendiff_amd.unet_train import UNetTrainer
    per_tol, glob_tol = BWD_TOL[mode]
    r, m = make_pair(5, 5, mode, center_input_sample=centered)
    sched, clean, noise, ts, labels, noisy, target = train_batch(2, 5)
    loss_ref, ref, gx = autograd_reference(r, noisy, ts, target, labels)
    tr = UNetTrainer(m, sched, lr=1e-4, use_ema=False)
    scale = tr.opt.scaler.scale if tr.opt.scaler is not None else 1.0
    assert (scale == 65536.0) == (mode == "fp16")
    loss, _ = tr.forward_backward(noisy.cuda(), ts.cuda(), clean.cuda(), noise.cuda(), class_labels=labels.cuda())
    torch.cuda.synchronize()
    assert set(ref) == set(tr.grads) and tuple(tr.grads["conv_in.weight"].shape) == (m.config.block_out_channels[0], 5, 3, 3)
    assert abs(float(loss) - float(loss_ref)) < {"f32": 1e-5, "bf16": 5e-3, "fp16": 2e-3}[mode] * float(loss_ref)
    got = {n: g / scale for n, g in tr.grads.items()}
    for n in ("conv_in.weight", "conv_in.bias"):
        assert float(ref[n].norm()) > 0
        print(f"backward {mode} {'centred ' if centered else ''}{n}: rel L2 {rel(got[n], ref[n]):.3e} (bound {per_tol})")
    UB.compare(ref, got, per_tol, glob_tol)
    plan = tr.plan_for(2, 32, 32)
    assert set(plan.grad_ready) == set(tr.grads)
    UB.assert_grad_ready_is_the_last_writer(plan, tr.grads)
    # d loss / d sample (what the gradient-guided transfer differentiates); fp16: the caller scales dout and un-scales dsample
    ig = m.input_grad_plan(2, 32, 32, torch.device(DEV))
    st = torch.cuda.current_stream().cuda_stream
    o = torch.empty(2, 5, 32, 32, device=DEV)
    ig.forward(noisy.cuda().contiguous(), ts.cuda().float(), labels.cuda(), None, o, st)
    k = float(GUIDANCE_GRAD_SCALE) if mode == "fp16" else 1.0
    ig.backward((k * (2.0 / o.numel()) * (o - target.cuda())).contiguous(), st)
    torch.cuda.synchronize()
    e = rel(ig.dsample / k, gx)
    # f32 / bf16: test_centered_input_and_identity_class_rows_train; fp16: the fp16 row of test_guidance_gradient_through_unet_matches_autograd
    bound = {"f32": 2e-5, "bf16": 4e-2, "fp16": dict(_marks(UB.test_guidance_gradient_through_unet_matches_autograd, "mode,tol"))["fp16"]}[mode]
    print(f"backward {mode} {'centred ' if centered else ''}d sample: rel L2 {e:.3e} (bound {bound})")
    assert tuple(ig.dsample.shape) == (2, 5, 32, 32) and e < bound


def test_frozen_conv_in_emits_no_gradient_launch():
    from phendiff_amd.unet_train import UNetTrainer
    _, m = make_pair(5, 5, "bf16")
    sched, clean, noise, ts, labels, noisy, _ = train_batch(2, 5)
    tr = UNetTrainer(m, sched, lr=1e-4, use_ema=False, trainable=lambda n, p: not n.startswith("conv_in."))
    assert tr.frozen == {"conv_in.weight", "conv_in.bias"}
    plan = tr.plan_for(2, 32, 32)
    free = UNetTrainer(make_pair(5, 5, "bf16")[1], sched, lr=1e-4, use_ema=False).plan_for(2, 32, 32)
    segs = [(tr.grads[n].data_ptr(), tr.grads[n].data_ptr() + 4 * tr.grads[n].numel()) for n in ("conv_in.weight", "conv_in.bias")]
    import ctypes as C
    for op in plan.bwd_ops:
        for f, ctype in op.args._fields_:
            v = getattr(op.args, f)
            if ctype is C.c_void_p and v:
                assert not any(lo <= v < hi for lo, hi in segs), (op.what, f)
    assert "conv_in.weight" not in plan.grad_ready and "conv_in.bias" not in plan.grad_ready
    assert len(free.bwd_ops) - len(plan.bwd_ops) == 3          # the bias sums, the 3x3 weight-gradient GEMM and its fold
    before = {n: m.state_dict()[n].clone() for n in ("conv_in.weight", "conv_in.bias")}
    tr.step(noisy.cuda(), ts.cuda(), clean.cuda(), noise.cuda(), class_labels=labels.cuda())
    torch.cuda.synchronize()
    assert all(torch.equal(m.state_dict()[n], v) for n, v in before.items())


def test_two_adamw_steps_follow_torch_and_every_plan_sees_the_new_conv_in():
    """The rule of test_training_steps_follow_torch_adamw_f32 at C = 5 (5 -> 5; in != out trains in test_in_and_out_channels_differ_forward_and_backward), then the two traps of
    tests/test_gpu_unet_backward.py:224,246: the inference plan reads the re-packed padded forward weight, the input-gradient plan the
    re-packed dgrad copy."""
    from phendiff_amd.unet_train import UNetTrainer
    r, m = make_pair(5, 5, "f32")
    sched, clean, noise, ts, labels, noisy, target = train_batch(4, 5)
    early = m.input_grad_plan(4, 32, 32, torch.device(DEV))
    w0 = m.conv_in.weight.detach().clone()
    tr = UNetTrainer(m, sched, lr=2e-4, use_ema=True)
    opt = torch.optim.AdamW(r.parameters(), lr=2e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)
    for _ in range(2):
        loss_ref, _ = UB.oracle_grads(r, noisy, ts, target, labels=labels)
        torch.nn.utils.clip_grad_norm_(r.parameters(), 1.0)
        opt.step()
        loss = float(tr.step(noisy.cuda(), ts.cuda(), clean.cuda(), noise.cuda(), class_labels=labels.cuda()))
        assert abs(loss - float(loss_ref)) < 2e-4 * abs(float(loss_ref)), (loss, float(loss_ref))
    torch.cuda.synchronize()
    sd = r.state_dict()
    num = sum(float((p.detach().cpu() - sd[n]).double().pow(2).sum()) for n, p in m.named_parameters())
    den = sum(float(sd[n].double().pow(2).sum()) for n, _ in m.named_parameters())
    print(f"two AdamW steps, C = 5: parameters differ by {(num / den) ** 0.5:.3e} (bound 1e-5)")
    assert (num / den) ** 0.5 < 1e-5
    # two larger steps, so that a stale copy of conv_in could not hide inside the bounds below; the oracle takes the trained state
    for _ in range(2):
        tr.step(noisy.cuda(), ts.cuda(), clean.cuda(), noise.cuda(), class_labels=labels.cuda(), lr=2e-3)
    torch.cuda.synchronize()
    assert float((m.conv_in.weight.detach().cpu() - w0.cpu()).abs().max()) > 1e-3          # the steps moved conv_in
    r.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    for p in r.parameters():
        p.requires_grad_(False)
    x = noisy.clone().requires_grad_(True)
    out_ref = r(x, ts, class_labels=labels).sample
    dout = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (gx,) = torch.autograd.grad((out_ref * dout).sum(), x)
    got = m(noisy.cuda(), ts.cuda(), class_labels=labels.cuda()).sample
    assert rel(got, out_ref.detach()) < 2e-5
    plan = m.input_grad_plan(4, 32, 32, torch.device(DEV))
    assert plan is not early
    st = torch.cuda.current_stream().cuda_stream
    o = torch.empty(4, 5, 32, 32, device=DEV)
    plan.forward(noisy.cuda().contiguous(), ts.cuda().float(), labels.cuda(), None, o, st)
    plan.backward(dout.cuda().contiguous(), st)
    torch.cuda.synchronize()
    assert rel(o, out_ref.detach()) < 2e-5 and rel(plan.dsample, gx) < 2e-5


def test_in_and_out_channels_differ_forward_and_backward():
    """The bare UNet with in_channels != out_channels (5 -> 2): the forward, the parameter gradients (the loss is taken on the two output
    channels) and d out / d sample against autograd."""
    from phendiff_amd.unet_train import UNetTrainer
    r, m = make_pair(5, 2, "f32")
    sched, clean, noise, ts, labels, _, target = train_batch(2, 2)
    noisy, _ = synth(2, 5)
    loss_ref, ref, _ = autograd_reference(r, noisy, ts, target, labels)
    tr = UNetTrainer(m, sched, lr=1e-4, use_ema=False)
    loss, out = tr.forward_backward(noisy.cuda(), ts.cuda(), clean.cuda(), noise.cuda(), class_labels=labels.cuda())
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 2, 32, 32) and abs(float(loss) - float(loss_ref)) < 1e-5 * float(loss_ref)
    UB.compare(ref, tr.grads, *BWD_TOL["f32"])
    for p in r.parameters():
        p.requires_grad_(False)
    x = noisy.clone().requires_grad_(True)
    out_ref = r(x, ts, class_labels=labels).sample
    dout = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(5))
    (gx,) = torch.autograd.grad((out_ref * dout).sum(), x)
    got = m(noisy.cuda(), ts.cuda(), class_labels=labels.cuda()).sample
    assert tuple(got.shape) == (2, 2, 32, 32) and rel(got, out_ref.detach()) < FWD_TOL["f32"]
    plan = m.input_grad_plan(2, 32, 32, torch.device(DEV))
    st = torch.cuda.current_stream().cuda_stream
    o = torch.empty(2, 2, 32, 32, device=DEV)
    plan.forward(noisy.cuda().contiguous(), ts.cuda().float(), labels.cuda(), None, o, st)
    plan.backward(dout.cuda().contiguous(), st)
    torch.cuda.synchronize()
    assert tuple(plan.dsample.shape) == (2, 5, 32, 32) and rel(plan.dsample, gx) < 2e-5
    with pytest.raises(ValueError, match="in_channels"):
        m(noisy[:, :2].cuda(), ts.cuda(), class_labels=labels.cuda())


# ---- everything that drives the UNet, C = 5 --------------------------------------------------------------------------------------------
def test_pipeline_from_noise_vs_oracle():
    pref, pgot = pipes("f32")
    labels = torch.tensor([0, 1])
    ref = pref(class_labels=labels, num_inference_steps=S, generator=torch.Generator().manual_seed(5)).images
    got = pgot(class_labels=labels.cuda(), num_inference_steps=S, generator=torch.Generator().manual_seed(5), output_type="numpy").images
    e = rel(got, ref)
    print(f"pipeline from noise, C = 5, f32: rel L2 {e:.3e} (bound {PIPELINE_TOL})")
    assert got.shape == (2, 32, 32, 5) and e < PIPELINE_TOL
    with pytest.raises(ValueError, match='output_type="numpy"'):
        pgot(class_labels=labels.cuda(), num_inference_steps=S)


def assert_u8(runner):
    assert torch.equal(runner.images_u8.cpu(), (runner.images * 255).round().to(torch.uint8).cpu())
    assert tuple(runner.images_u8.shape) == tuple(runner.images.shape) and runner.images.shape[-1] == 5


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
def test_ddib_eager_and_captured_vs_oracle(mode):
    import phendiff_amd as P
    from oracle import ddib_ref
    tol = DDIB_TOL[mode]
    pref, pgot = pipes(mode)
    x, labels = synth(2, 5)
    target = 1 - labels
    ref_img, ref_inv = ddib_ref(pref, x, labels, target, S)
    inv = P.inversion(pgot, x.cuda(), labels.cuda(), S)
    img = P.ddib(pgot, x.cuda(), labels.cuda(), target.cuda(), S)
    print(f"DDIB C = 5 {mode}: inverted {rel(inv, ref_inv):.3e}, images {rel(img, ref_img):.3e} (bound {tol})")
    assert img.shape == ref_img.shape == (2, 32, 32, 5) and rel(inv, ref_inv) < tol and rel(img, ref_img) < tol
    for use_graph in (True, False):
        out = P.DDIBGraph(pgot, batch_size=2, num_inference_steps=S, use_graph=use_graph).run(x.cuda(), labels.cuda(), target.cuda())
        torch.cuda.synchronize()
        assert bool(out.graph) == use_graph
        assert torch.equal(out.images.cpu(), torch.from_numpy(img)) and torch.equal(out.inverted.cpu(), inv.cpu())
        assert_u8(out)


def test_ddib_sliced_runner(monkeypatch):
    import phendiff_amd as P
    from oracle import ddib_ref
    pref, pgot = pipes("f32")
    monkeypatch.setattr(type(pgot.unet), "max_batch", lambda self, H, W: 2)
    x, labels = synth(3, 5)
    g = P.DDIBGraph(pgot, batch_size=3, num_inference_steps=S)
    assert len(g._bounds) == 2
    out = g.run(x.cuda(), labels.cuda(), (1 - labels).cuda())
    torch.cuda.synchronize()
    ref_img, ref_inv = ddib_ref(pref, x, labels, 1 - labels, S)
    assert rel(out.images, ref_img) < DDIB_TOL["f32"] and rel(out.inverted, ref_inv) < DDIB_TOL["f32"]
    assert_u8(out)


def test_cfg_forward_start_eager_and_captured_vs_oracle():
    import phendiff_amd as P
    pref, pgot = pipes("f32")
    x, labels = synth(2, 5)
    target = 1 - labels
    steps, frac, w = 6, 0.5, 2.5                            # 3 of the 6 timesteps are kept
    ref = pref(class_labels=target, w=w, num_inference_steps=steps, start_image=x, frac_diffusion_skipped=frac, guidance_eqn="imagen",
               generator=torch.Generator().manual_seed(7)).images
    eager = P.classifier_free_guidance_forward_start(pgot, x.cuda(), target.cuda(), w, frac, steps, generator=torch.Generator().manual_seed(7))
    e = rel(eager, ref)
    print(f"CFG forward start C = 5 f32: rel L2 {e:.3e} (bound {PIPELINE_TOL})")
    assert eager.shape == (2, 32, 32, 5) and e < PIPELINE_TOL
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(7))
    for use_graph in (True, False):
        g = P.CFGForwardStartGraph(pgot, batch_size=2, num_inference_steps=steps, guidance_scale=w, frac_diffusion_skipped=frac,
                                   use_graph=use_graph)
        assert len(g.ts) == 3
        out = g.run(x.cuda(), target.cuda(), noise.cuda())
        torch.cuda.synchronize()
        assert torch.equal(out.images.cpu(), torch.from_numpy(eager))
        assert_u8(out)


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
def test_guided_transfer_eager_and_captured_vs_oracle(mode):
    import phendiff_amd as P
    from oracle import linear_interp_custom_guidance_inverted_start_ref
    pref, pp = pipes(mode)
    x, labels = synth(2, 5)
    target = 1 - labels
    p, gls = 2, 0.5
    ref = linear_interp_custom_guidance_inverted_start_ref(pref, x, labels, target, p, gls, S)
    xg, lg, tg = x.cuda(), labels.cuda(), target.cuda()
    pt = P.linear_interp_custom_guidance_inverted_start(pp, xg, lg, tg, p, gls, S, output_type="pt")
    arr = P.linear_interp_custom_guidance_inverted_start(pp, xg, lg, tg, p, gls, S, output_type="numpy")
    e = rel(pt, ref)
    print(f"guided transfer C = 5 {mode}: rel L2 {e:.3e} (bound {PIXEL_TOL[mode]})")
    assert tuple(pt.shape) == (2, 5, 32, 32) and e < PIXEL_TOL[mode]
    with pytest.raises(ValueError, match='output_type="numpy"'):
        P.linear_interp_custom_guidance_inverted_start(pp, xg, lg, tg, p, gls, S, output_type="pil")
    for use_graph in (True, False):
        runner = P.GuidedTransferGraph(pp, 2, S, p, gls, use_graph=use_graph).run(xg, lg, tg)
        torch.cuda.synchronize()
        assert bool(runner.graph) == use_graph
        assert torch.equal(runner.guided, pt) and torch.equal(runner.images.cpu(), torch.from_numpy(arr))
        assert_u8(runner)
    plain = P.ddib(pp, xg, lg, tg, S)
    assert float(np.abs(arr - plain).max()) > 1e-2                      # the guidance had an effect


def test_trainer_with_device_sampler_checkpoint_and_generation(tmp_path):
    """UNetTrainer + DeviceTrainingSampler at C = 5: the loss falls, save_state / load_state resumes bit for bit, save_pretrained /
    from_pretrained returns the same model, generate_samples samples from it."""
    import phendiff_amd as P
    from phendiff_amd.eval_generation import generate_samples
    _, m = make_pair(5, 5, "bf16")
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    clean, labels = synth(4, 5)
    clean, labels = clean.cuda(), labels.cuda()
    tr = P.UNetTrainer(m, sched, lr=5e-4)
    tr.attach_sampler(P.DeviceTrainingSampler(sched, 77, DEV))
    losses = [float(tr.step_clean(clean, class_labels=labels)) for _ in range(4)]
    assert all(l == l for l in losses) and min(losses[1:]) < losses[0], losses
    tr.save_state(str(tmp_path / "state"))
    rest = [float(tr.step_clean(clean, class_labels=labels)) for _ in range(2)]
    _, m2 = make_pair(5, 5, "bf16", seed=1)
    tr2 = P.UNetTrainer(m2, sched, lr=5e-4)
    tr2.attach_sampler(P.DeviceTrainingSampler(sched, 1, DEV))
    tr2.load_state(str(tmp_path / "state"))
    assert [float(tr2.step_clean(clean, class_labels=labels)) for _ in range(2)] == rest
    assert torch.equal(tr2.opt.flat, tr.opt.flat)
    pipe = P.ConditionalDDIMPipeline(m, sched)
    pipe.save_pretrained(str(tmp_path / "pipe"))
    back = P.ConditionalDDIMPipeline.from_pretrained(str(tmp_path / "pipe"), compute_dtype="bf16").to(DEV)
    assert back.unet.config.in_channels == 5 == back.unet.config.out_channels
    x, lb = synth(2, 5)
    assert torch.equal(back.unet(x.cuda(), 640, lb.cuda()).sample, m(x.cuda(), 640, lb.cuda()).sample)
    gen = generate_samples(pipe, nb_classes=2, nb_generated_images=3, eval_batch_size=2, num_inference_steps=2, trainer=tr)
    assert [b.images.shape for b in gen.batches] == [(2, 32, 32, 5), (1, 32, 32, 5)] * 2
    assert all(np.isfinite(b.images).all() and b.uint8.dtype == np.uint8 for b in gen.batches)
