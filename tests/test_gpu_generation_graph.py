"""From-noise generation with noise drawn on the device: ``DDIMScheduler.step(generator=DeviceNoise)`` against the oracle schedulers fed
the same noise, ``GenerationGraph`` captured = enqueued eagerly = ``ConditionalDDIMPipeline(generator=DeviceNoise)`` bit for bit, the
trajectory against the CPU oracle, replays / seeks, and the evaluation loop on top of it.  super_small at 32 x 32, 3 steps, batch 4."""
import numpy as np
import pytest
import torch

from test_gpu_unet_ddib import make_pair, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0xC0FFEE1234
S, B, SIZE = 3, 4, 32
SCHED = "3k_steps_clipping_rescaling"
_pairs = {}


def pair(mode):
    if mode not in _pairs:
        _pairs[mode] = make_pair("super_small", SIZE, mode)
    return _pairs[mode]


def pipe_of(mode, **sched_kw):
    import phendiff_amd as P
    return P.ConditionalDDIMPipeline(pair(mode)[1], P.DDIMScheduler(**dict(P.SCHEDULER_CONFIGS[SCHED], **sched_kw)))


def labels():
    return (torch.arange(B) % 2).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- scheduler step
@pytest.mark.parametrize("ucm", [False, True], ids=["model_out", "clipped_model_out"])
@pytest.mark.parametrize("thresholding", [False, True], ids=["clip", "threshold"])
def test_stochastic_step_draws_the_variance_noise_on_the_device(thresholding, ucm):
    """eta = 0.7 with generator=DeviceNoise against the oracle scheduler (the subclass of tests/threshold_refs.py where it thresholds)
    fed ``variance_noise(i, shape)``: the tolerance of test_scheduler_step_options_f32, the same step with host noise."""
    import phendiff_amd as P
    from oracle import DDIMSchedulerRef
    from threshold_refs import make_threshold_ref
    g = torch.Generator().manual_seed(21)
    x, out = (torch.randn(2, 3, 8, 8, generator=g) for _ in range(2))
    for pt in ("epsilon", "sample", "v_prediction"):
        cfg = dict(num_train_timesteps=1000, beta_schedule="linear", prediction_type=pt, timestep_spacing="linspace", clip_sample=True,
                   clip_sample_range=0.8)
        if thresholding:
            a = make_threshold_ref(cfg, 0.9, 1.5)
            b = P.DDIMScheduler(**cfg, thresholding=True, dynamic_thresholding_ratio=0.9, sample_max_value=1.5)
        else:
            a, b = DDIMSchedulerRef(**cfg), P.DDIMScheduler(**cfg)
        a.set_timesteps(7); b.set_timesteps(7)
        noise = P.DeviceNoise(SEED, DEV, first_index=9)
        for i in (1, 2, 3):
            t = a.timesteps[i]
            assert b.step_index(t) == i
            z = noise.variance_noise(i, x.shape)
            ra = a.step(out, t, x, eta=0.7, use_clipped_model_output=ucm, variance_noise=z.cpu())
            rb = b.step(out.cuda(), t, x.cuda(), eta=0.7, use_clipped_model_output=ucm, generator=noise)
            assert torch.allclose(rb.prev_sample.cpu(), ra.prev_sample, rtol=1e-5, atol=1e-5), (pt, int(t))
            assert torch.allclose(rb.pred_original_sample.cpu(), ra.pred_original_sample, rtol=1e-5, atol=1e-6)
            # and it is the explicit-noise path of the same scheduler plus one rounding-identical launch
            rc = b.step(out.cuda(), t, x.cuda(), eta=0.7, use_clipped_model_output=ucm, variance_noise=z)
            assert torch.equal(rb.prev_sample, rc.prev_sample)
        assert noise.index == 9                                             # a step does not advance: the pipeline does, per batch


# ---------------------------------------------------------------------------------------------------------------- graph = eager = pipeline
CASES = {
    "plain": (dict(), dict()),
    "imagen_w2_eta": (dict(w=2.0, guidance_eqn="imagen", eta=0.7), dict()),
    "cfg_w1.5": (dict(w=1.5, guidance_eqn="CFG"), dict()),
    "per_sample_w_eta_clipped": (dict(w=[1.5, 0.0, 3.0, 2.0], eta=0.7, use_clipped_model_output=True), dict()),
    "threshold": (dict(w=2.0), dict(thresholding=True, sample_max_value=1.5)),
    "threshold_eta": (dict(eta=0.7), dict(thresholding=True, sample_max_value=1.5)),
}


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_graph_equals_eager_equals_pipeline(case, mode):
    import phendiff_amd as P
    from phendiff_amd.eval_generation import images_to_uint8
    kw, sched_kw = CASES[case]
    kw = {k: (torch.tensor(v, device=DEV) if isinstance(v, list) else v) for k, v in kw.items()}
    pipe = pipe_of(mode, **sched_kw)
    outs = []
    for use_graph in (True, False):
        noise = P.DeviceNoise(SEED, DEV, first_index=3)
        g = P.GenerationGraph(pipe, B, S, noise, use_graph=use_graph, **kw)
        u8 = g.run(labels())
        assert u8 is g.images_u8 and u8.dtype == torch.uint8 and tuple(u8.shape) == (B, SIZE, SIZE, 3) and u8.is_cuda
        assert noise.index == 3 + B and noise.state.cpu().tolist()[1] == 3 + B
        assert np.array_equal(u8.cpu().numpy(), images_to_uint8(g.images.cpu().numpy()))
        outs.append((g.images.clone(), u8.clone()))
    noise = P.DeviceNoise(SEED, DEV, first_index=3)
    got = pipe(labels(), generator=noise, num_inference_steps=S, output_type="numpy", add_forward_noise_to_image=False, **kw).images
    assert noise.index == 3 + B and noise.state.cpu().tolist()[1] == 3 + B
    assert bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][0].std()) > 0.01
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0].cpu(), torch.from_numpy(got))
    if kw.get("eta"):                                                       # the variance noise matters: eta = 0 gives other images
        other = P.GenerationGraph(pipe, B, S, P.DeviceNoise(SEED, DEV, first_index=3), **dict(kw, eta=0.0))
        other.run(labels())
        assert not torch.equal(other.images, outs[0][0])


@pytest.mark.parametrize("variant", ["channels5", "identity", "timestep"])
def test_other_channel_counts_and_class_embeddings(variant):
    """What the other pixel trajectories run: 5 image channels (the padded conv_in), class_embed_type "identity" (the conditioning IS
    the embedding rows) and "timestep" (the class MLP inside the graph); guidance and eta on; captured = enqueued = pipeline."""
    import phendiff_amd as P
    if variant == "channels5":
        from test_gpu_unet_channels import pipes
        pipe, channels = pipes("bf16")[1], 5
    else:
        torch.manual_seed(3)
        unet = P.CustomCondUNet2DModel(compute_dtype="bf16", **dict(P.UNET_CONFIGS["super_small"], sample_size=SIZE, class_embed_type=variant))
        pipe, channels = P.ConditionalDDIMPipeline(unet.to(DEV), P.DDIMScheduler(**P.SCHEDULER_CONFIGS[SCHED])), 3
    if variant == "identity":
        rows = torch.randn(B, pipe.unet.time_embed_dim, generator=torch.Generator().manual_seed(5)).to(DEV)
        cond, call = dict(class_emb=rows), dict(class_labels=None, class_emb=rows)
    else:
        cond = call = dict(class_labels=labels())
    kw = dict(w=2.0, eta=0.7)
    outs = []
    for use_graph in (True, False):
        g = P.GenerationGraph(pipe, B, S, P.DeviceNoise(SEED, DEV, first_index=1), use_graph=use_graph, **kw)
        u8 = g.run(**cond)
        assert tuple(u8.shape) == (B, SIZE, SIZE, channels) and torch.equal(u8, (g.images * 255).round().to(torch.uint8))
        outs.append(g.images.clone())
    got = pipe(generator=P.DeviceNoise(SEED, DEV, first_index=1), num_inference_steps=S, output_type="numpy",
               add_forward_noise_to_image=False, **call, **kw).images
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].std()) > 0.01
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0].cpu(), torch.from_numpy(got))


def test_graph_refuses_what_it_cannot_run():
    import phendiff_amd as P
    pipe = pipe_of("bf16")
    noise = P.DeviceNoise(SEED, DEV)
    with pytest.raises(TypeError, match="DeviceNoise"):
        P.GenerationGraph(pipe, B, S, torch.Generator())
    with pytest.raises(ValueError, match="guidance equation"):
        P.GenerationGraph(pipe, B, S, noise, guidance_eqn="other")
    with pytest.raises(ValueError, match="exceeds what one launch plan holds"):
        P.GenerationGraph(pipe, pipe.unet.max_batch(SIZE, SIZE) + 1, S, noise)
    g = P.GenerationGraph(pipe, B, S, noise, use_graph=False)
    with pytest.raises(ValueError, match="class_labels or class_emb"):
        g.run()
    with pytest.raises(ValueError, match="batch of 4"):
        g.run(labels()[:2])
    assert noise.index == 0


# ---------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_trajectory_against_the_oracle_f32(eta):
    """The oracle pipeline fed the device-drawn initial sample (as start_image, no forward noise) and the device-drawn variance noise of
    every step; the tolerance of test_pipeline_cfg_and_forward_noise_f32 (this config, this engine)."""
    import phendiff_amd as P
    from oracle import ConditionalDDIMPipelineRef, DDIMSchedulerRef
    cfg = P.SCHEDULER_CONFIGS[SCHED]
    pref = ConditionalDDIMPipelineRef(pair("f32")[0], DDIMSchedulerRef(**cfg))
    noise = P.DeviceNoise(SEED, DEV, first_index=11)
    shape = (B, 3, SIZE, SIZE)
    x_T = noise.randn(shape, P.DeviceNoise.PURPOSE_INITIAL_SAMPLE).cpu()
    zs = iter([noise.variance_noise(i, shape).cpu() for i in range(S)])
    step = pref.scheduler.step
    pref.scheduler.step = lambda mo, t, x, generator=None, **kw: step(mo, t, x, variance_noise=next(zs), **kw)
    ref = pref(class_labels=labels().cpu(), num_inference_steps=S, start_image=x_T, add_forward_noise_to_image=False,
               frac_diffusion_skipped=0, w=2.0, eta=eta).images
    g = P.GenerationGraph(pipe_of("f32"), B, S, noise, w=2.0, eta=eta)
    g.run(labels())
    err = rel(g.images, ref)
    print(f"GenerationGraph f32 eta={eta}: relative error to the oracle {err:.3e}")
    assert err < 2e-4


# ---------------------------------------------------------------------------------------------------------------- replays and seeks
def test_replays_advance_and_seeks_reproduce():
    import phendiff_amd as P
    noise = P.DeviceNoise(SEED, DEV)
    g = P.GenerationGraph(pipe_of("bf16"), B, S, noise, w=2.0, eta=0.7)
    first = g.run(labels()).clone()
    second = g.run(labels()).clone()
    assert noise.index == 2 * B and not torch.equal(first, second)
    noise.seek(0)
    assert torch.equal(g.run(labels()), first) and noise.index == B
    noise.seek(B)
    assert torch.equal(g.run(labels()), second)
    sd = noise.state_dict()
    third = g.run(labels()).clone()
    noise.load_state_dict(sd)
    assert torch.equal(g.run(labels()), third)
    # image k draws the same noise as row 2 of a batch of 4 and as a batch of 1
    k, shape = 6, (3, SIZE, SIZE)
    for purpose, base in ((P.DeviceNoise.PURPOSE_INITIAL_SAMPLE, 0), (P.DeviceNoise.PURPOSE_FORWARD_NOISE, 0),
                          (P.DeviceNoise.PURPOSE_VARIANCE_NOISE, 2 * 3 * SIZE * SIZE)):
        four = noise.seek(k - 2).randn((4,) + shape, purpose, elem_base=base)
        one = noise.seek(k).randn((1,) + shape, purpose, elem_base=base)
        assert torch.equal(four[2], one[0])
    # and the one-step trajectories' initial samples agree: x_T is what a 1-step, eta = 0 run starts from; compare through randn
    assert torch.equal(noise.seek(k).variance_noise(2, (1,) + shape), one)


# ---------------------------------------------------------------------------------------------------------------- evaluation
def _evaluate(pipe, noise, **kw):
    from phendiff_amd.eval_generation import generate_samples
    return generate_samples(pipe, nb_classes=2, nb_generated_images=6, eval_batch_size=4, num_inference_steps=S, guidance_factor=2.0,
                            device_noise=noise, **kw)


def test_evaluation_generates_on_the_device():
    import phendiff_amd as P
    from phendiff_amd.eval_generation import generation_indices
    pipe = pipe_of("bf16")
    single = _evaluate(pipe, P.DeviceNoise(SEED, DEV))
    assert [(b.class_label, len(b.filenames)) for b in single.batches] == [(0, 4), (0, 2), (1, 4), (1, 2)]
    for b in single.batches:
        u8 = b.images_u8_device
        assert u8.is_cuda and u8.dtype == torch.uint8 and tuple(u8.shape) == (len(b.filenames), SIZE, SIZE, 3)
        assert b.images.dtype == np.float32 and np.array_equal(b.images, u8.cpu().numpy().astype(np.float32) / np.float32(255))
        assert np.array_equal(b.uint8, u8.cpu().numpy())
    assert single.images_of(1).shape == (6, SIZE, SIZE, 3)
    # image j of class c is global image 6 c + j: the first batch of class 1 is what a graph of 4 draws at index 6
    noise = P.DeviceNoise(SEED, DEV, first_index=6)
    direct = P.GenerationGraph(pipe, 4, S, noise, w=2.0).run(torch.ones(4, dtype=torch.long, device=DEV))
    assert torch.equal(direct, single.batches[2].images_u8_device)
    # two processes: every image is drawn from the noise the single process draws for it (here the batches coincide, so the images do)
    per_rank = [_evaluate(pipe, P.DeviceNoise(SEED, DEV), num_processes=2, process_index=r) for r in (0, 1)]
    assert [len(b.filenames) for b in per_rank[0].batches] == [4, 4] and [len(b.filenames) for b in per_rank[1].batches] == [2, 2]
    for c in (0, 1):
        both = torch.cat([per_rank[0].batches[c].images_u8_device, per_rank[1].batches[c].images_u8_device])
        assert torch.equal(both, torch.cat([b.images_u8_device for b in single.batches if b.class_label == c]))
    assert sorted(k for r in (0, 1) for _, _, k in generation_indices(2, 6, 4, 2, r)) == [0, 4, 6, 10]
    # use_graph=False: the same launches
    eager = _evaluate(pipe, P.DeviceNoise(SEED, DEV), use_graph=False)
    assert all(torch.equal(a.images_u8_device, b.images_u8_device) for a, b in zip(eager.batches, single.batches))
    with pytest.raises(NotImplementedError, match="DDIM"):
        _evaluate(pipe, P.DeviceNoise(SEED, DEV), model_type="StableDiffusion")


class _ProjectionFeatures:
    """A feature extractor with InceptionV3Features' call surface and a fraction of its cost: a fixed projection of the pixels to 2048
    features (what the statistics read) and 1008 logits.  The routing of the images is what the test is about, not the features."""

    def __init__(self):
        self.device = torch.device(DEV)
        g = torch.Generator().manual_seed(0)
        self.w = (torch.randn(3 * SIZE * SIZE, 2048 + 1008, generator=g) / 4000).to(DEV)
        self.seen = []

    def __call__(self, u8):
        assert u8.is_cuda and u8.dtype == torch.uint8 and tuple(u8.shape[1:]) == (SIZE, SIZE, 3)
        self.seen.append(u8.clone())
        f = u8.reshape(u8.shape[0], -1).float() @ self.w
        return {"2048": f[:, :2048].contiguous(), "logits_unbiased": f[:, 2048:].contiguous(), "logits": f[:, 2048:].contiguous()}


def test_metrics_from_device_tensors_equal_those_from_host_arrays():
    """class_metrics_hook(device_statistics=True): the same uint8 in -- as device tensors, or as the host arrays of the same images --
    gives the same numbers out (KID, precision / recall, density / coverage: the statistics that stay on the device)."""
    import phendiff_amd as P
    import phendiff_amd.metrics as M
    from phendiff_amd.eval_generation import GeneratedBatch
    single = _evaluate(pipe_of("bf16"), P.DeviceNoise(SEED, DEV))
    g = torch.Generator().manual_seed(9)
    real = {c: torch.randint(0, 256, (12, SIZE, SIZE, 3), generator=g, dtype=torch.uint8).numpy() for c in (0, 1)}
    nets, res = [_ProjectionFeatures(), _ProjectionFeatures()], [{}, {}]
    hooks = [M.class_metrics_hook(n, real, r, isc=False, fid=False, kid=True, kid_subset_size=4, batch_size=16, device_statistics=True,
                                  prc=True, dc=True) for n, r in zip(nets, res)]
    for c in (0, 1):
        batches = [b for b in single.batches if b.class_label == c]
        hooks[0](c, str(c), batches)
        hooks[1](c, str(c), [GeneratedBatch(b.class_label, b.class_name, b.batch_idx, b.filenames, b.images) for b in batches])
    # both extractors saw the same uint8 batches: the class's real images, then its 6 generated ones in order
    assert len(nets[0].seen) == len(nets[1].seen) == 4 and all(torch.equal(a, b) for a, b in zip(nets[0].seen, nets[1].seen))
    assert torch.equal(nets[0].seen[3], torch.cat([b.images_u8_device for b in single.batches if b.class_label == 1]))
    assert list(res[0]) == list(res[1]) and len(res[0]) == 2 * 7 and f"{M.KEY_KID_MEAN}/0" in res[0] and "coverage/1" in res[0]
    assert all(np.isfinite(v) for v in res[0].values())
    assert res[0] == res[1], (res[0], res[1])
