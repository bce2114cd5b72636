"""pd_train_sample / DeviceTrainingSampler on the MI355X against the numpy restatement of the stream (tests/philox_ref.py): timesteps bit
for bit, noise within 8 ulp of the pair's radius, ``noisy`` bit-identical to ``pd_add_noise``, independence of the launch geometry,
guard bands, graph replay, and the trainers' ``step_clean`` / checkpoint resume.

Noise bound: |z_gpu - z_ref| <= 2^-21 r with r the reference radius of the element's Box-Muller pair (8 ulp of r, 1 ulp = 2^-24 r):
logf / log1pf and sqrtf contribute about 1.5 ulp of r, sincospif <= 2 ulp of 1, the product 0.5 ulp -- roughly 4.5 ulp of r, about 1.8 x margin.
The measured maximum is printed before the assertion."""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_ref as R
from guard_bands import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5EED0123456789AB
NOISE_BOUND = 2.0 ** -21


def scheduler(N=3000):
    import phendiff_amd as P
    return P.DDIMScheduler(**dict(P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"], num_train_timesteps=N))


def tables(sched):
    acp = sched.alphas_cumprod.float()
    return (acp ** 0.5).contiguous().to(DEV), ((1 - acp) ** 0.5).contiguous().to(DEV)


def launch(noise, B, per, step=0, rank=0, purpose=0, elem_base=0, N=0, clean=None, sa=None, sb=None, ts_in=None, ts_out=None, noisy=None,
           seed=SEED):
    import phendiff_amd._lib as L
    a = L.TrainSampleArgs(seed=seed, step=step, rank=rank, purpose=purpose, B=B, per_sample=per, elem_base=elem_base, N=N,
                          clean=L.ptr(clean), sqrt_acp=L.ptr(sa), sqrt_1m_acp=L.ptr(sb), timesteps_in=L.ptr(ts_in),
                          timesteps_out=L.ptr(ts_out), noise=noise.data_ptr(), noisy=L.ptr(noisy))
    L.check(L.lib().pd_train_sample(C.byref(a), torch.cuda.current_stream().cuda_stream), "pd_train_sample")


def randn_fill(n, **kw):
    out = torch.full((n,), float("nan"), device=DEV)
    launch(out, 1, n, **kw)
    return out


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("B,N", [(1, 1), (3, 10), (130, 3000)])
def test_timesteps_equal_the_restatement(B, N):
    noise = torch.empty(B * 5, device=DEV)
    ts = torch.full((B,), -1, dtype=torch.long, device=DEV)
    launch(noise, B, 5, step=7, rank=2, N=N, ts_out=ts)
    want = R.timesteps(SEED, 7, 2, B, N)
    assert ts.dtype == torch.long and np.array_equal(ts.cpu().numpy(), want)
    assert 0 <= int(ts.min()) and int(ts.max()) < N


@pytest.mark.parametrize("elem_base", [0, 3, (1 << 34) - 2])
@pytest.mark.parametrize("B,per", [(1, 1), (3, 105), (2, 256), (5, 4099)])
def test_noise_within_8_ulp_of_the_radius(B, per, elem_base):
    sched = scheduler()
    sa, sb = tables(sched)
    clean = torch.rand(B, per, device=DEV) * 2 - 1
    noise, noisy = torch.full((B, per), float("nan"), device=DEV), torch.full((B, per), float("nan"), device=DEV)
    ts = torch.full((B,), -1, dtype=torch.long, device=DEV)
    launch(noise, B, per, step=11, rank=1, elem_base=elem_base, N=3000, clean=clean, sa=sa, sb=sb, ts_out=ts, noisy=noisy)
    want, radius = R.normal(SEED, 11, 1, B * per, elem_base=elem_base, with_radius=True)
    got = noise.cpu().numpy().reshape(-1)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / radius
    print(f"pd_train_sample noise B={B} per_sample={per} elem_base={elem_base}: max |z - z_ref| = {err.max() * 2 ** 24:.3f} ulp of r")
    assert err.max() <= NOISE_BOUND, (err.max() * 2 ** 24, int(err.argmax()))
    # timesteps do not depend on elem_base; noisy is what pd_add_noise makes of this noise and these timesteps, bit for bit
    assert np.array_equal(ts.cpu().numpy(), R.timesteps(SEED, 11, 1, B, 3000))
    assert torch.equal(noisy, sched.add_noise(clean, noise, ts))


def test_sampler_tuple_matches_add_noise_on_images():
    """The Python surface on an NCHW batch: (noise, timesteps, noisy) as ``sample_training_inputs`` returns them, step counting, randn."""
    import phendiff_amd as P
    from phendiff_amd.training import sample_training_inputs
    sched = scheduler()
    s = P.DeviceTrainingSampler(sched, SEED, DEV, rank=3)
    clean = torch.rand(3, 3, 7, 5, device=DEV) * 2 - 1
    noise, ts, noisy = sample_training_inputs(clean, sched, sampler=s)
    assert s.step == 1 and noise.shape == clean.shape and ts.shape == (3,) and ts.dtype == torch.long
    assert np.array_equal(ts.cpu().numpy(), R.timesteps(SEED, 0, 3, 3, 3000))
    assert torch.equal(noisy, sched.add_noise(clean, noise, ts))
    want, radius = R.normal(SEED, 0, 3, clean.numel(), with_radius=True)
    assert (np.abs(noise.cpu().numpy().reshape(-1).astype(np.float64) - want) / radius).max() <= NOISE_BOUND
    r = s.randn((2, 4, 3))
    assert s.step == 2 and r.shape == (2, 4, 3)
    want, radius = R.normal(SEED, 1, 3, 24, purpose=R.PURPOSE_RANDN, with_radius=True)
    assert (np.abs(r.cpu().numpy().reshape(-1).astype(np.float64) - want) / radius).max() <= NOISE_BOUND
    assert s.randn_like(clean).shape == clean.shape and s.step == 3
    # sample_noise: the draw of `sample` without the clean batch
    s2 = P.DeviceTrainingSampler(sched, SEED, DEV, rank=3)
    n2, t2 = s2.sample_noise(clean.shape)
    assert torch.equal(n2, noise) and torch.equal(t2, ts) and s2.step == 1


# ---------------------------------------------------------------------------------------------------------------- geometry
def test_split_launches_equal_the_whole():
    n, cut = 1001, 333                       # an odd boundary: the quad 332..335 is written by both launches' edge paths
    whole = randn_fill(n, step=4, purpose=2)
    parts = torch.full((n,), float("nan"), device=DEV)
    launch(parts[:cut], 1, cut, step=4, purpose=2)
    launch(parts[cut:], 1, n - cut, step=4, purpose=2, elem_base=cut)
    assert torch.equal(whole, parts)
    assert torch.equal(whole, randn_fill(n, step=4, purpose=2))          # the same arguments twice: the same bits
    # with clean and timesteps_in the split goes through the batch: samples 0..1 and 2..4
    sched = scheduler()
    sa, sb = tables(sched)
    B, per = 5, 37
    clean = torch.rand(B, per, device=DEV)
    ts = torch.tensor([5, 2999, 0, 1234, 77], device=DEV)
    outs = []
    for pieces in ([(0, 5)], [(0, 2), (2, 5)]):
        noise, noisy = torch.empty(B, per, device=DEV), torch.empty(B, per, device=DEV)
        for b0, b1 in pieces:
            launch(noise[b0:b1], b1 - b0, per, step=9, elem_base=b0 * per, N=3000, clean=clean[b0:b1], sa=sa, sb=sb, ts_in=ts[b0:b1],
                   noisy=noisy[b0:b1])
        outs.append((noise, noisy))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_rank_step_purpose_and_seed_change_every_quad():
    n = 1 << 16
    base = randn_fill(n, step=5, rank=1, purpose=0)
    for kw in (dict(step=6, rank=1, purpose=0), dict(step=5, rank=2, purpose=0), dict(step=5, rank=1, purpose=2),
               dict(step=5 + (1 << 32), rank=1, purpose=0), dict(step=5, rank=1, purpose=0, seed=SEED + 1),
               dict(step=5, rank=1, purpose=0, seed=SEED + (1 << 32))):
        other = randn_fill(n, **kw)
        assert int((other == base).sum()) < n // 1000, kw
    ts = [torch.empty(256, dtype=torch.long, device=DEV) for _ in range(2)]
    for t, rank in zip(ts, (0, 1)):
        launch(torch.empty(256, device=DEV), 256, 1, step=5, rank=rank, N=3000, ts_out=t)
    assert int((ts[0] == ts[1]).sum()) < 8            # distinct timesteps per data-parallel rank


def test_timesteps_in_is_used_and_not_overwritten():
    sched = scheduler()
    sa, sb = tables(sched)
    B, per = 3, 105
    clean = torch.rand(B, per, device=DEV) * 2 - 1
    ts_in = torch.tensor([2999, 0, 1500], device=DEV)
    keep = ts_in.clone()
    ts_out = torch.full((B,), -7, dtype=torch.long, device=DEV)
    noise, noisy = torch.empty(B, per, device=DEV), torch.empty(B, per, device=DEV)
    launch(noise, B, per, step=2, N=3000, clean=clean, sa=sa, sb=sb, ts_in=ts_in, ts_out=ts_out, noisy=noisy)
    assert torch.equal(ts_in, keep) and bool((ts_out == -7).all())
    assert torch.equal(noisy, sched.add_noise(clean, noise, ts_in))
    # the noise is the one a drawing launch of the same step produces
    n2 = torch.empty(B, per, device=DEV)
    launch(n2, B, per, step=2)
    assert torch.equal(n2, noise)


# ---------------------------------------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("B,per", [(3, 105), (1, 1)])
def test_guard_bands(B, per):
    """P2: canaried outputs (pattern intact around noise, noisy and timesteps_out; bodies pre-filled with NaN / -1, every element written).
    P1: zero, then NaN around clean and the tables: bit-identical outputs."""
    sched = scheduler()
    sa0, sb0 = tables(sched)
    clean, hc = guarded(torch.rand(B, per) * 2 - 1, device=DEV, name="clean")
    sa, hsa = guarded(sa0, device=DEV, name="sqrt_acp")
    sb, hsb = guarded(sb0, device=DEV, name="sqrt_1m_acp")
    outs = []
    for fill in ("clear", "poison"):
        for h in (hc, hsa, hsb):
            getattr(h, fill)()
        noise, hn = guarded(torch.full((B, per), float("nan")), device=DEV, name="noise")
        noisy, hy = guarded(torch.full((B, per), float("nan")), device=DEV, name="noisy")
        ts, ht = guarded(torch.full((B,), -1, dtype=torch.long), device=DEV, name="timesteps_out")
        for h in (hn, hy, ht):
            h.canary()
        launch(noise, B, per, step=3, N=3000, clean=clean, sa=sa, sb=sb, ts_out=ts, noisy=noisy)
        torch.cuda.synchronize()
        for h in (hn, hy, ht):
            assert h.intact()
        assert bool(torch.isfinite(noise).all()) and bool(torch.isfinite(noisy).all()) and int(ts.min()) >= 0
        outs.append((noise.clone(), noisy.clone(), ts.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # the pure randn fill at an unaligned output address (element-wise path on every quad)
    buf, hb = guarded(torch.full((B * per + 1,), float("nan")), device=DEV, name="randn")
    hb.canary()
    launch(buf[1:], 1, B * per, step=3, purpose=2)
    assert hb.intact() and bool(torch.isnan(buf[0])) and bool(torch.isfinite(buf[1:]).all())
    assert torch.equal(buf[1:], randn_fill(B * per, step=3, purpose=2))


# ---------------------------------------------------------------------------------------------------------------- graph replay
def test_graph_replay_equals_eager():
    sched = scheduler()
    sa, sb = tables(sched)
    B, per = 4, 999
    clean = torch.rand(B, per, device=DEV) * 2 - 1
    eager = [torch.empty(B, per, device=DEV), torch.empty(B, per, device=DEV), torch.empty(B, dtype=torch.long, device=DEV)]
    launch(eager[0], B, per, step=21, N=3000, clean=clean, sa=sa, sb=sb, ts_out=eager[2], noisy=eager[1])
    torch.cuda.synchronize()
    noise, noisy = torch.zeros(B, per, device=DEV), torch.zeros(B, per, device=DEV)
    ts = torch.zeros(B, dtype=torch.long, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(noise, B, per, step=21, N=3000, clean=clean, sa=sa, sb=sb, ts_out=ts, noisy=noisy)
    for _ in range(2):
        noise.zero_(), noisy.zero_(), ts.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(noise, eager[0]) and torch.equal(noisy, eager[1]) and torch.equal(ts, eager[2])


# ---------------------------------------------------------------------------------------------------------------- trainers
def pixel_trainer():
    import phendiff_amd as P
    from test_gpu_unet_ddib import make_pair
    _, m = make_pair("super_small", 32, "bf16")
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    tr = P.UNetTrainer(m, sched, lr=3e-4)
    return tr, sched


def test_step_clean_equals_step_fed_by_an_equal_sampler():
    import phendiff_amd as P
    g = torch.Generator().manual_seed(3)
    clean = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(DEV)
    labels = torch.tensor([1, 0], device=DEV)
    a, sched = pixel_trainer()
    with pytest.raises(P.PhenDiffHipError):
        a.step_clean(clean, class_labels=labels)                 # no sampler attached
    a.attach_sampler(P.DeviceTrainingSampler(sched, 77, DEV))
    b, sched_b = pixel_trainer()
    feeder = P.DeviceTrainingSampler(sched_b, 77, DEV)
    for _ in range(2):
        la = a.step_clean(clean, class_labels=labels)
        noise, ts, noisy = feeder.sample(clean)
        lb = b.step(noisy, ts, clean, noise, class_labels=labels)
        assert torch.equal(la, lb)
    assert a.sampler.step == 2 == feeder.step
    assert torch.equal(a.opt.flat, b.opt.flat) and torch.equal(a.opt.ema, b.opt.ema)


def test_save_load_continues_the_sampler(tmp_path):
    import os
    import pickle
    import phendiff_amd as P
    from phendiff_amd.train_state import DEVICE_SAMPLER_KEY
    g = torch.Generator().manual_seed(4)
    clean = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(DEV)
    labels = torch.tensor([0, 1], device=DEV)

    def fresh(seed):
        tr, sched = pixel_trainer()
        tr.attach_sampler(P.DeviceTrainingSampler(sched, seed, DEV))
        return tr
    a = fresh(123)
    for _ in range(2):
        a.step_clean(clean, class_labels=labels)
    folder = str(tmp_path / "step_2")
    a.save_state(folder)
    assert sorted(os.listdir(folder)) == ["custom_checkpoint_0.pkl", "optimizer.bin", "pytorch_model.bin", "random_states_0.pkl",
                                          "scheduler.bin"]
    with open(os.path.join(folder, "random_states_0.pkl"), "rb") as f:
        assert pickle.load(f)[DEVICE_SAMPLER_KEY] == {"seed": 123, "rank": 0, "step": 2}
    a.step_clean(clean, class_labels=labels)
    b = fresh(999)                                               # another seed: the checkpoint's must win
    b.load_state(folder)
    assert b.sampler.state_dict() == {"seed": 123, "rank": 0, "step": 2}
    b.step_clean(clean, class_labels=labels)
    assert torch.equal(a.opt.flat, b.opt.flat) and torch.equal(a.opt.ema, b.opt.ema)
    # without a sampler the file carries today's keys only, and a checkpoint without the entry loads into a trainer that has one
    c, _ = pixel_trainer()
    plain = str(tmp_path / "plain")
    c.save_state(plain)
    with open(os.path.join(plain, "random_states_0.pkl"), "rb") as f:
        assert DEVICE_SAMPLER_KEY not in pickle.load(f)
    b.load_state(plain)
    assert b.sampler.state_dict() == {"seed": 123, "rank": 0, "step": 3}


def test_sd_step_clean_equals_step_fed_by_an_equal_sampler():
    """SDUNetTrainer on the tiny latent config: ``step_clean`` on latents, a conditional and an unconditional step."""
    import phendiff_amd as P
    from test_gpu_sd_unet import TINY, make_pair
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["SD_orig_config"])
    g = torch.Generator().manual_seed(8)
    latents = (torch.randn(2, 4, 16, 16, generator=g) * 0.8).to(DEV)
    labels = torch.tensor([1, 0], device=DEV)

    def fresh():
        _, _, m, e2 = make_pair(TINY, "bf16")
        return P.SDUNetTrainer(m, e2, sched, lr=3e-4)
    a, b = fresh(), fresh()
    a.attach_sampler(P.DeviceTrainingSampler(sched, 5, DEV))
    feeder = P.DeviceTrainingSampler(sched, 5, DEV)
    for uncond in (False, True):
        la = a.step_clean(latents, labels, unconditional=uncond)
        noise, ts, noisy = feeder.sample(latents)
        lb = b.step(noisy, ts, latents, noise, labels, unconditional=uncond)
        assert torch.equal(la, lb)
    assert torch.equal(a.opt.flat, b.opt.flat) and torch.equal(a.opt.ema, b.opt.ema)


@pytest.mark.parametrize("freeze_vae", [True, False])
def test_step_images_draws_inside(freeze_vae):
    """``step_images(images, class_labels=...)`` with a sampler: posterior noise (``randn``), then noise and timesteps, drawn inside --
    equal to the same step fed with those tensors, for a frozen and for a training autoencoder."""
    import phendiff_amd as P
    from test_gpu_vae_training import make_trainer, trainer_batch
    sched, x, _, _, _, labels = trainer_batch()
    _, a = make_trainer("bf16", sched, freeze_vae=freeze_vae)
    _, b = make_trainer("bf16", sched, freeze_vae=freeze_vae)
    assert a._vae_trains == (not freeze_vae)
    with pytest.raises(AttributeError):
        a.step_images(x.cuda(), None, None, labels.cuda())          # no sampler: None is not drawn for the caller
    a.attach_sampler(P.DeviceTrainingSampler(sched, 6, DEV))
    feeder = P.DeviceTrainingSampler(sched, 6, DEV)
    la = a.step_images(x.cuda(), class_labels=labels.cuda())
    shape = (x.shape[0], 4, x.shape[2] // 2, x.shape[3] // 2)
    pn = feeder.randn(shape)
    nz, ts = feeder.sample_noise(shape)
    lb = b.step_images(x.cuda(), ts, nz, labels.cuda(), posterior_noise=pn)
    assert a.sampler.step == feeder.step == 2
    assert torch.equal(la, lb) and torch.equal(a.opt.flat, b.opt.flat)
