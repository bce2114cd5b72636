"""Guidance rescale on the MI355X: ``pd_guidance_rescale`` against the float64 restatement of diffusers' ``rescale_noise_cfg``
(tests/guidance_rescale_ref.py; tests/test_host_guidance_rescale.py proves the restatement), its exact properties (in place, row alone =
row in a batch, repeatable, a NaN row stays alone), its guard bands, and every guided entry point: ``guidance_rescale=0`` is today's
output, ``guidance_rescale=0.7`` is the hand loop of ``pipe.unet`` + ``phendiff_amd.guidance_rescale`` + ``scheduler.step``, and the
captured trajectories equal the enqueued ones and the eager pipeline, bit for bit.

The kernel's tolerance: every element within 2 fp32 ulp of the float64 result.  g is rounded to fp32 once (half an ulp of g, which is up
to one ulp of the product where the product sits at the bottom of its binade and g at the top of its own), and the product is rounded
once (half an ulp).  The fp64 summation order moves g by ~1e-16 relative, far below half an fp32 ulp, so it matters only where g lies at
a rounding boundary.  Hence 2 and not 1."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import guidance_rescale_ref as G
from test_gpu_guard_bands import Case, Op, out_op, p1_poisoned_surroundings, p2_canaried_outputs, p3_sample_isolation
from test_gpu_unet_ddib import make_pair, synth_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SEED = 0xC0FFEE1234
S, B, SIZE = 3, 4, 32
SCHED = "3k_steps_clipping_rescaling"
PHI = 0.7


@pytest.fixture(scope="module")
def env():
    import phendiff_amd._lib as L
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L, L.lib(), torch.device(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def chunk():
    import phendiff_amd._lib as L
    return L.CONSTANTS["PD_GUIDANCE_RESCALE_CHUNK"]


def _ids(v):
    if isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], tuple):
        return f"{'cfg' if v[0] else 'imagen'}-w{len(v[1])}"
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


# ================================================================================================ the kernel
def launch(env, cond, uncond, w, phi, eqn, out=None, workspace=None):
    """pd_guidance_rescale over device tensors cond / uncond [B][n] -> out [B][n] (NaN-filled unless given; the workspace too: every
    partial the apply pass reads must have been written by the first launch)."""
    L, lib, dev = env
    Bn, n = cond.shape
    if out is None:
        out = torch.full((Bn, n), NAN, dtype=torch.float32, device=dev)
    if workspace is None:
        workspace = torch.full((lib.pd_guidance_rescale_workspace(Bn, n) // 8,), NAN, dtype=torch.float64, device=dev)
    a = L.GuidanceRescaleArgs(numel=Bn * n, per_sample=n, model_out=cond.data_ptr(), uncond_out=uncond.data_ptr(), w=w.data_ptr(),
                              w_per_sample=int(w.numel() > 1), guidance_cfg=int(eqn), rescale=phi, out=out.data_ptr(),
                              workspace=workspace.data_ptr())
    L.check(lib.pd_guidance_rescale(C.byref(a), stream()), "pd_guidance_rescale")
    return out


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _shapes():
    return G.shapes(chunk())


@pytest.mark.parametrize("guidance", G.GUIDANCE, ids=_ids)
@pytest.mark.parametrize("shape", _shapes(), ids=_ids)
def test_kernel_against_the_restatement(env, shape, guidance):
    dev = env[2]
    Bn, n = shape
    cond, uncond = G.inputs(Bn, n)
    w, eqn = G.weights(Bn, guidance[1]), guidance[0]
    for phi in G.PHIS:
        got = launch(env, cond.to(dev), uncond.to(dev), w.to(dev), phi, eqn).cpu()
        want = G.reference(cond, uncond, w, phi, eqn)
        assert bool(torch.isfinite(got).all())
        worst = float(G.ulps(got, want).max())
        print(f"pd_guidance_rescale {Bn}x{n} {_ids(guidance)} phi={phi}: largest error {worst:.3f} ulp (bound {G.MAX_ULPS})")
        assert worst <= G.MAX_ULPS, (shape, guidance, phi, worst)
        if phi == 1.0:
            np.testing.assert_allclose(got.double().std(dim=1).numpy(), cond.double().std(dim=1).numpy(), rtol=1e-6)


@pytest.mark.parametrize("guidance", (G.GUIDANCE[0], G.GUIDANCE[3]), ids=_ids)
def test_exact_properties(env, guidance):
    """In place = out of place; a row alone = the same row inside a batch of 5; two calls give the same bits; a NaN in row 1 makes
    row 1 NaN and leaves row 0 as it was."""
    dev = env[2]
    for n in (105, chunk() + 1, 2 * chunk() + 1003):
        cond, uncond = (t.to(dev) for t in G.inputs(5, n))
        w, eqn = G.weights(5, guidance[1]).to(dev), guidance[0]
        base = launch(env, cond, uncond, w, PHI, eqn)
        assert same_bits(launch(env, cond, uncond, w, PHI, eqn), base), ("repeat", n)
        inplace = cond.clone()
        launch(env, inplace, uncond, w, PHI, eqn, out=inplace)
        assert same_bits(inplace, base), ("in place", n)
        for b in range(5):
            # (a row of an odd-sized batch starts 4, 8 or 12 bytes past a 16-byte boundary; alone it starts on one)
            alone = launch(env, cond[b:b + 1].clone(), uncond[b:b + 1].clone(), w[b:b + 1].clone() if w.numel() > 1 else w, PHI, eqn)
            assert same_bits(alone[0], base[b]), ("alone", n, b)
        poisoned = cond.clone()
        poisoned[1, n // 2] = NAN
        got = launch(env, poisoned, uncond, w, PHI, eqn)
        assert bool(torch.isnan(got[1]).all()) and same_bits(got[0], base[0]) and same_bits(got[2:], base[2:]), ("nan row", n)


@pytest.mark.parametrize("shape", ((3, 105), (3, chunk() + 1)), ids=_ids)
def test_guard_bands(env, shape, monkeypatch):
    """P1: NaN around both inputs (and the weights) changes no output bit.  P2: the byte pattern around out and around the workspace
    survives, and every output element is written.  P3: a NaN row changes no other row."""
    L, lib, dev = env
    Bn, n = shape
    cond, uncond = G.inputs(Bn, n)
    w = G.weights(Bn, G.GUIDANCE[2][1])
    want = G.reference(cond, uncond, w, PHI, 0)
    ins = {"cond": Op(cond, sample_dim=0), "uncond": Op(uncond, sample_dim=0), "w": Op(w)}
    outs = {"out": out_op((Bn, n), torch.float32, sample_dim=0),
            "workspace": Op(torch.full((lib.pd_guidance_rescale_workspace(Bn, n) // 8,), NAN, dtype=torch.float64), whole=False)}

    def run(t):
        launch(env, t["cond"], t["uncond"], t["w"], PHI, 0, t["out"], t["workspace"])

    def check(got):
        assert float(G.ulps(got["out"], want).max()) <= G.MAX_ULPS

    case = Case(ins, outs, run, check, nsamples=Bn)
    p1_poisoned_surroundings(case, dev, monkeypatch)
    p2_canaried_outputs(case, dev, monkeypatch)
    p3_sample_isolation(case, dev, monkeypatch)


def test_public_function_and_object(env):
    """phendiff_amd.guidance_rescale: a number or a (B,) tensor for w, 4-D tensors, out= (also the conditional prediction itself); the
    object refuses another stream and keeps one workspace per (B, n, device, stream)."""
    import phendiff_amd as P
    dev = env[2]
    cond, uncond = (t.view(3, 5, 7, 3).to(dev) for t in G.inputs(3, 105))
    want = G.reference(cond.cpu(), uncond.cpu(), torch.tensor([3.0]), PHI, 0)
    got = P.guidance_rescale(cond, uncond, 3.0, PHI)
    assert got.shape == cond.shape and got.dtype == torch.float32 and float(G.ulps(got.cpu(), want).max()) <= G.MAX_ULPS
    w = torch.tensor([1.5, 0.0, 3.0])
    per = P.guidance_rescale(cond, uncond, w, PHI, guidance_cfg=True)
    assert float(G.ulps(per.cpu(), G.reference(cond.cpu(), uncond.cpu(), w, PHI, 1)).max()) <= G.MAX_ULPS
    into = cond.clone()
    assert P.guidance_rescale(into, uncond, 3.0, PHI, out=into) is into and same_bits(into, got)
    # phi = 0: the plain combine, bit for bit
    assert same_bits(P.guidance_rescale(cond, uncond, 3.0, 0.0).cpu(), G.combine_f32(cond.cpu(), uncond.cpu(), torch.tensor([3.0]), 0))
    wd = torch.tensor([3.0], device=dev)
    a, b = P.GuidanceRescale(cond, uncond, wd, PHI, stream=stream()), P.GuidanceRescale(cond.clone(), uncond, wd, PHI, stream=stream())
    assert a.workspace.data_ptr() == b.workspace.data_ptr() and a.out is cond
    with pytest.raises(ValueError, match="enqueued on stream"):
        a.enqueue(stream() + 8)


# ================================================================================================ the pixel tier
_pairs = {}


def pipe_of(mode, multistep=False, **sched_kw):
    import phendiff_amd as P
    if mode not in _pairs:
        _pairs[mode] = make_pair("super_small", SIZE, mode)
    pipe = P.ConditionalDDIMPipeline(_pairs[mode][1], P.DDIMScheduler(**dict(P.SCHEDULER_CONFIGS[SCHED], **sched_kw)))
    if multistep:
        pipe.scheduler = P.DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    return pipe


def labels():
    return (torch.arange(B) % 2).to(DEV)


def _uncond_of(a):
    """The unconditional output a runner's step entry names: the entry is an argument struct, or a (Multistep)ThresholdStep holding one."""
    return getattr(a, "update", getattr(a, "step", a)).uncond_out


def _hand_loop(pipe, w, phi, eqn, generator):
    """ConditionalDDIMPipeline.__call__ from noise, written out: per step the two evaluations, phendiff_amd.guidance_rescale, scheduler.step."""
    import phendiff_amd as P
    from phendiff_amd.schedulers import randn_tensor
    sch = pipe.scheduler
    image = randn_tensor((B, 3, SIZE, SIZE), generator, pipe.device)
    sch.set_timesteps(S)
    zeros = torch.zeros((B, pipe.unet.time_embed_dim), device=pipe.device)
    for t in sch.timesteps:
        cond = pipe.unet(sample=image, timestep=t, class_labels=labels(), class_emb=None).sample
        uncond = pipe.unet(sample=image, timestep=t, class_labels=None, class_emb=zeros).sample
        out = P.guidance_rescale(cond, uncond, w, phi, guidance_cfg=(eqn == "CFG"))
        image = sch.step(out, t, image).prev_sample
    return (image / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).contiguous().cpu().numpy()


@pytest.mark.parametrize("kind", ("ddim", "threshold", "multistep"))
def test_pipeline_off_is_todays_output_and_on_is_the_hand_loop(kind):
    pipe = pipe_of("bf16", multistep=(kind == "multistep"), **(dict(thresholding=True, sample_max_value=1.5) if kind == "threshold" else {}))
    for eqn, w in (("imagen", 3.0), ("CFG", torch.tensor([1.5, 0.0, 3.0, 2.0], device=DEV))):
        kw = dict(w=w, guidance_eqn=eqn, num_inference_steps=S, output_type="numpy", add_forward_noise_to_image=False)
        gen = lambda: torch.Generator().manual_seed(7)
        today = pipe(labels(), generator=gen(), **kw).images
        assert np.array_equal(pipe(labels(), generator=gen(), guidance_rescale=0.0, **kw).images, today)
        on = pipe(labels(), generator=gen(), guidance_rescale=PHI, **kw).images
        assert np.isfinite(on).all() and not np.array_equal(on, today)
        assert np.array_equal(on, _hand_loop(pipe, w, PHI, eqn, gen())), (kind, eqn)
    # guidance not active (w <= 1 under the imagen equation): the argument changes nothing
    off = dict(w=1.0, num_inference_steps=S, output_type="numpy", add_forward_noise_to_image=False)
    assert np.array_equal(pipe(labels(), generator=torch.Generator().manual_seed(7), guidance_rescale=PHI, **off).images,
                          pipe(labels(), generator=torch.Generator().manual_seed(7), **off).images)


GRAPH_CASES = {
    "ddim_imagen_w3": (dict(w=3.0, guidance_eqn="imagen"), dict(), False),
    "ddim_cfg_w2_eta": (dict(w=2.0, guidance_eqn="CFG", eta=0.7), dict(), False),
    "ddim_per_sample_w": (dict(w=[1.5, 0.0, 3.0, 2.0]), dict(), False),
    "threshold_imagen_w3": (dict(w=3.0), dict(thresholding=True, sample_max_value=1.5), False),
    "threshold_cfg_per_sample_w": (dict(w=[1.5, 0.0, 3.0, 2.0], guidance_eqn="CFG"), dict(thresholding=True, sample_max_value=1.5), False),
    "multistep_imagen_w3": (dict(w=3.0), dict(), True),
    "multistep_cfg_per_sample_w": (dict(w=[1.5, 0.0, 3.0, 2.0], guidance_eqn="CFG"), dict(), True),
}


@pytest.mark.parametrize("case", list(GRAPH_CASES))
def test_generation_graph_equals_enqueued_equals_pipeline(case):
    import phendiff_amd as P
    kw, sched_kw, multistep = GRAPH_CASES[case]
    kw = {k: (torch.tensor(v, device=DEV) if isinstance(v, list) else v) for k, v in kw.items()}
    mode = "f32" if case == "ddim_imagen_w3" else "bf16"
    pipe = pipe_of(mode, multistep=multistep, **sched_kw)
    outs = []
    for use_graph in (True, False):
        noise = P.DeviceNoise(SEED, DEV, first_index=3)
        g = P.GenerationGraph(pipe, B, S, noise, use_graph=use_graph, guidance_rescale=PHI, **kw)
        assert g.rescale is not None and all(_uncond_of(a) is None for a in g.step_args)
        g.run(labels())
        first = (g.images.clone(), g.images_u8.clone())
        assert noise.index == 3 + B
        noise.seek(3)                                                       # a second replay of the same images reproduces the first
        g.run(labels())
        assert torch.equal(g.images, first[0]) and torch.equal(g.images_u8, first[1]), (case, use_graph, "replay")
        outs.append(first)
    got = pipe(labels(), generator=P.DeviceNoise(SEED, DEV, first_index=3), num_inference_steps=S, output_type="numpy",
               add_forward_noise_to_image=False, guidance_rescale=PHI, **kw).images
    assert bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][0].std()) > 0.01
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0].cpu(), torch.from_numpy(got))
    plain = P.GenerationGraph(pipe, B, S, P.DeviceNoise(SEED, DEV, first_index=3), use_graph=False, guidance_rescale=0.0, **kw)
    assert plain.rescale is None and all(_uncond_of(a) for a in plain.step_args)
    plain.run(labels())
    assert not torch.equal(plain.images, outs[0][0])                       # the rescale matters


@pytest.mark.parametrize("eqn,w", (("imagen", 3.0), ("CFG", 2.0)))
@pytest.mark.parametrize("multistep", (False, True), ids=("ddim", "multistep"))
def test_cfg_forward_start_graph_equals_eager(multistep, eqn, w):
    import phendiff_amd as P
    pipe = pipe_of("bf16", multistep=multistep)
    x, lab = synth_batch(B, SIZE)
    target = (1 - lab).to(DEV)
    eager = pipe(class_labels=target, w=w, num_inference_steps=6, start_image=x.to(DEV), frac_diffusion_skipped=0.5, guidance_eqn=eqn,
                 generator=torch.Generator().manual_seed(7), output_type="numpy", guidance_rescale=PHI).images
    if eqn == "imagen":
        assert np.array_equal(eager, P.classifier_free_guidance_forward_start(pipe, x.to(DEV), target, w, 0.5, 6, generator=torch.Generator().manual_seed(7),
                                                                              guidance_rescale=PHI))
        assert not np.array_equal(eager, P.classifier_free_guidance_forward_start(pipe, x.to(DEV), target, w, 0.5, 6,
                                                                                  generator=torch.Generator().manual_seed(7)))
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(7))       # the draw the pipeline makes
    for use_graph in (True, False):
        g = P.CFGForwardStartGraph(pipe, batch_size=B, num_inference_steps=6, guidance_scale=w, frac_diffusion_skipped=0.5, guidance_eqn=eqn,
                                   use_graph=use_graph, guidance_rescale=PHI)
        assert len(g.ts) == 3 and g.rescale is not None and all(_uncond_of(a) is None for a in g.step_args)
        for again in (False, True):
            out = g.run(x.to(DEV), target, noise.to(DEV))
            torch.cuda.synchronize()
            assert np.array_equal(out.images.cpu().numpy(), eager), (use_graph, again)


def test_generate_samples_passes_the_rescale_on():
    """Both forms of the pixel tier's evaluation loop: the captured one equals GenerationGraph's images, the eager one the pipeline's."""
    import phendiff_amd as P
    from phendiff_amd.eval_generation import generate_samples, images_to_uint8
    pipe = pipe_of("bf16")
    kw = dict(nb_classes=2, nb_generated_images=B, eval_batch_size=B, num_inference_steps=S, guidance_factor=3.0)
    got = generate_samples(pipe, device_noise=P.DeviceNoise(SEED, DEV), guidance_rescale=PHI, **kw)
    g = P.GenerationGraph(pipe, B, S, P.DeviceNoise(SEED, DEV), w=3.0, guidance_rescale=PHI)
    for c in (0, 1):
        g.noise.seek(c * B)
        want = g.run(torch.full((B,), c, device=DEV).long())
        assert torch.equal(got.batches[c].images_u8_device, want)
    eager = generate_samples(pipe, guidance_rescale=PHI, **kw)
    gen = torch.Generator(device=DEV).manual_seed(P.eval_generation.EVAL_SEED)
    for c in (0, 1):
        want = pipe(torch.full((B,), c, device=DEV).long(), None, 3.0, generator=gen, num_inference_steps=S, output_type="numpy",
                    guidance_rescale=PHI).images
        assert np.array_equal(eager.batches[c].images, want)
    assert not np.array_equal(images_to_uint8(eager.batches[0].images), images_to_uint8(generate_samples(pipe, **kw).batches[0].images))


# ================================================================================================ the latent tier
def _sd_pipe(mode):
    import phendiff_amd as P
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import SD_SCHED, SD_TINY_UNET, SD_TINY_VAE, sd_tiny_pipe
    ref = sd_tiny_pipe()
    unet = P.SDUNet2DConditionModel(compute_dtype=mode, **SD_TINY_UNET)
    unet.load_state_dict(ref.unet.state_dict())
    vae = P.AutoencoderKL(compute_dtype=mode, **SD_TINY_VAE)
    vae.load_state_dict(ref.vae.state_dict())
    emb = P.CustomEmbedding(2, SD_TINY_UNET["cross_attention_dim"])
    emb.load_state_dict(ref.class_embedding.state_dict())
    return P.CustomStableDiffusionImg2ImgPipeline(vae.to(DEV), unet.to(DEV), P.DDIMScheduler(**SD_SCHED), emb.to(DEV))


def _sd_hand_loop(pipe, lat, lab, w, phi):
    import phendiff_amd as P
    dev, n = pipe.device, lat.shape[0]
    ehs = P.hack_class_embedding(pipe._encode_class(class_labels=lab, device=dev, do_classifier_free_guidance=True))
    pipe.scheduler.set_timesteps(S, device=dev)
    timesteps, _ = pipe.get_timesteps(S, 1, dev)
    latents = pipe.prepare_latents(image=pipe.image_processor.preprocess(lat), timestep=timesteps[:1].repeat(n), batch_size=n,
                                   dtype=torch.float32, device=dev, latent_shape=None, generator=None,
                                   add_forward_noise_to_image=False).contiguous()
    for t in timesteps:
        pred = pipe.unet(torch.cat([latents, latents]), t, encoder_hidden_states=ehs, return_dict=False)[0]
        out = P.guidance_rescale(pred[n:], pred[:n], w, phi)
        latents = pipe.scheduler.step(out, t, latents).prev_sample
    return latents


@pytest.mark.parametrize("mode", ("f32", "bf16"))
def test_sd_pipeline_off_is_todays_output_and_on_is_the_hand_loop(mode):
    pipe = _sd_pipe(mode)
    lat = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    lab = torch.tensor([1, 0], device=DEV)
    kw = dict(image=lat, class_labels=lab, strength=1, add_forward_noise_to_image=False, num_inference_steps=S, output_type="latent")
    for w in (3.0, torch.tensor([1.5, 4.0], device=DEV)):
        today = pipe(guidance_scale=w, **kw)
        assert torch.equal(pipe(guidance_scale=w, guidance_rescale=0.0, **kw), today)
        on = pipe(guidance_scale=w, guidance_rescale=PHI, **kw)
        assert bool(torch.isfinite(on).all()) and not torch.equal(on, today)
        assert torch.equal(on, _sd_hand_loop(pipe, lat, lab, w, PHI))
    # guidance not active (guidance_scale <= 1): the argument changes nothing
    assert torch.equal(pipe(guidance_scale=1.0, guidance_rescale=PHI, **kw), pipe(guidance_scale=1.0, **kw))
