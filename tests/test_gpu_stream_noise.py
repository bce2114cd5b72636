"""pd_stream_noise / pd_stream_advance on the MI355X: the stream of pd_train_sample bit for bit (and the numpy restatement within
8 ulp of the pair's radius), the coefficient forms against torch arithmetic and pd_add_noise, independence of the batch split, replay
of a captured launch, guard bands, and the moments of 2^20 draws."""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_ref as R
from guard_bands import guarded
from test_gpu_train_sampler import NOISE_BOUND, launch as train_sample
from test_host_stream_noise import MOMENT_N, MOMENT_SEED, moments_hold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5EED0123456789AB
# (B, per_sample, elem_base): unaligned head and tail quads, and ((3, 20, *): rows of 80 bytes) buffers whose 16-byte grid is not the quads'
SHAPES = [(3, 20, 0), (3, 20, 3), (1, 4, 1), (2, 3072, 0), (2, 3072, 6)]


def signed(v):
    """A uint64 as the int64 a torch tensor holds."""
    return v - (1 << 64) if v >= 1 << 63 else v


def state_of(seed, index):
    return torch.tensor([signed(seed), index], dtype=torch.int64).to(DEV)


def launch(out, state, B, per, rank=0, purpose=3, elem_base=0, index_offset=0, x=None, a=1.0, b=1.0, sa=None, sb=None):
    import phendiff_amd._lib as L
    args = L.StreamNoiseArgs(state=state.data_ptr(), index_offset=index_offset, rank=rank, purpose=purpose, B=B, per_sample=per,
                             elem_base=elem_base, a=a, b=b, sa=L.ptr(sa), sb=L.ptr(sb), x=L.ptr(x), out=out.data_ptr())
    L.check(L.lib().pd_stream_noise(C.byref(args), torch.cuda.current_stream().cuda_stream), "pd_stream_noise")


def advance(state, n):
    import phendiff_amd._lib as L
    L.check(L.lib().pd_stream_advance(state.data_ptr(), n, torch.cuda.current_stream().cuda_stream), "pd_stream_advance")


def draw(B, per, index=0, seed=SEED, **kw):
    out = torch.full((B, per), float("nan"), device=DEV)
    launch(out, state_of(seed, index), B, per, **kw)
    return out


# ---------------------------------------------------------------------------------------------------------------- the stream
@pytest.mark.parametrize("B,per,elem_base", SHAPES)
def test_rows_equal_pd_train_sample_bit_for_bit(B, per, elem_base):
    index, rank, purpose = 5, 3, 4
    got = draw(B, per, index, rank=rank, purpose=purpose, elem_base=elem_base)
    assert bool(torch.isfinite(got).all())
    worst = 0.0
    for b in range(B):
        want = torch.full((per,), float("nan"), device=DEV)
        train_sample(want, 1, per, step=index + b, rank=rank, purpose=purpose, elem_base=elem_base, seed=SEED)
        assert torch.equal(got[b], want), (b, int((got[b] != want).sum()))
        ref, radius = R.normal(SEED, index + b, rank, per, elem_base=elem_base, purpose=purpose, with_radius=True)
        worst = max(worst, float((np.abs(got[b].cpu().numpy().astype(np.float64) - ref) / radius).max()))
    print(f"pd_stream_noise B={B} per_sample={per} elem_base={elem_base}: max |z - z_ref| = {worst * 2 ** 24:.3f} ulp of r")
    assert worst <= NOISE_BOUND
    # the index may come from either side: the state or index_offset
    assert torch.equal(draw(B, per, 2, rank=rank, purpose=purpose, elem_base=elem_base, index_offset=3), got)
    # a step above 2^32 reaches the counter's high step bits as pd_train_sample's does
    hi = draw(1, per, (1 << 40) + 9, rank=rank, purpose=purpose, elem_base=elem_base)
    want = torch.full((per,), float("nan"), device=DEV)
    train_sample(want, 1, per, step=(1 << 40) + 9, rank=rank, purpose=purpose, elem_base=elem_base, seed=SEED)
    assert torch.equal(hi[0], want)


# ---------------------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("B,per,elem_base", SHAPES)
def test_coefficients_round_like_torch_and_pd_add_noise(B, per, elem_base):
    import phendiff_amd as P
    kw = dict(index=7, purpose=5, elem_base=elem_base)
    z = draw(B, per, **kw)
    g = torch.Generator().manual_seed(B * per + elem_base)
    x = (torch.rand(B, per, generator=g) * 2 - 1).to(DEV)
    a, b = 0.8125, 0.37                                            # (0.37 is no fp32 number: the kernel gets float32(0.37), and so does torch)
    scalar = draw(B, per, x=x, a=a, b=b, **kw)
    assert torch.equal(scalar, torch.tensor(a, dtype=torch.float32) * x + torch.tensor(b, dtype=torch.float32, device=DEV) * z)
    assert torch.equal(draw(B, per, b=b, **kw), torch.tensor(b, dtype=torch.float32, device=DEV) * z)        # x == NULL: b z
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    ts = torch.tensor([2999, 0, 1234][:B], device=DEV)
    sa, sb = sched._per_sample_coefs(ts, DEV)
    table = draw(B, per, x=x, sa=sa, sb=sb, a=float("nan"), b=float("nan"), **kw)      # (the scalars are not read)
    assert torch.equal(table, sa[:, None] * x + sb[:, None] * z)
    assert torch.equal(table, sched.add_noise(x, z, ts))
    # in place
    for form in (dict(a=a, b=b), dict(sa=sa, sb=sb)):
        buf = x.clone()
        launch(buf, state_of(SEED, 7), B, per, purpose=5, elem_base=elem_base, x=buf, **form)
        assert torch.equal(buf, scalar if "a" in form else table)


# ---------------------------------------------------------------------------------------------------------------- geometry
def test_batch_split_invariance():
    per = 3072
    whole = draw(8, per, 0)
    assert torch.equal(whole[5:8], draw(3, per, 5))
    assert torch.equal(whole[2:3], draw(1, per, 0, index_offset=2))
    rows = whole.cpu()
    assert len({rows[b].numpy().tobytes() for b in range(8)}) == 8


def test_seed_rank_purpose_and_index_change_every_quad():
    n = 1 << 16
    ref = dict(index=5, rank=1, purpose=3, seed=SEED)
    base = draw(1, n, **ref)
    for change in (dict(index=6), dict(rank=2), dict(purpose=4), dict(index=5 + (1 << 32)), dict(seed=SEED + 1), dict(seed=SEED + (1 << 32))):
        other = draw(1, n, **dict(ref, **change))
        assert int((other == base).sum()) < n // 1000, change


# ---------------------------------------------------------------------------------------------------------------- replay
def test_captured_launch_draws_the_next_images_on_every_replay():
    B, per = 3, 3072
    eager = [draw(B, per, i * B) for i in range(3)]
    state = state_of(SEED, 0)
    out = torch.zeros(B, per, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(out, state, B, per)
        advance(state, B)
    state.copy_(state_of(SEED, 0))                    # (whatever the capture did to it)
    got = []
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got.append(out.clone())
    for i in range(3):
        assert torch.equal(got[i], eager[i]), i
        for j in range(i):
            assert int((got[i] == got[j]).sum()) < B * per // 1000
    assert state.cpu().tolist() == [signed(SEED), 3 * B]


# ---------------------------------------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("B,per,elem_base", [(3, 20, 3), (1, 4, 1), (2, 3072, 6)])
def test_guard_bands(B, per, elem_base):
    """P2: a canary around out (pre-filled with NaN: every element written).  P1: zeros, then NaN around x, the tables and the state: the
    same bits.  P3: one row of x replaced by NaN changes that row only."""
    g = torch.Generator().manual_seed(per)
    x, hx = guarded(torch.rand(B, per, generator=g) * 2 - 1, device=DEV, name="x")
    sa, hsa = guarded(torch.rand(B, generator=g), device=DEV, name="sa")
    sb, hsb = guarded(torch.rand(B, generator=g), device=DEV, name="sb")
    state, hst = guarded(torch.tensor([signed(SEED), 11], dtype=torch.int64), device=DEV, name="state")
    outs = []
    for fill in ("clear", "poison"):
        for h in (hx, hsa, hsb, hst):
            getattr(h, fill)()
        for form in (dict(sa=sa, sb=sb), dict(a=0.5, b=2.0)):
            out, ho = guarded(torch.full((B, per), float("nan")), device=DEV, name="out")
            ho.canary()
            launch(out, state, B, per, elem_base=elem_base, x=x, **form)
            torch.cuda.synchronize()
            assert ho.intact() and bool(torch.isfinite(out).all())
            outs.append(out.clone())
        out, ho = guarded(torch.full((B * per + 1,), float("nan")), device=DEV, name="out+4")       # no 16-byte store fits
        ho.canary()
        launch(out[1:], state, B, per, elem_base=elem_base)
        assert ho.intact() and bool(torch.isnan(out[0])) and bool(torch.isfinite(out[1:]).all())
        outs.append(out[1:].clone())
    for a, b in zip(outs[:3], outs[3:]):
        assert torch.equal(a, b)
    assert torch.equal(outs[2].view(B, per), draw(B, per, 11, elem_base=elem_base))
    assert state.cpu().tolist() == [signed(SEED), 11]
    for row in sorted({0, B // 2, B - 1}):
        bad = x.clone()
        bad[row] = float("nan")
        out = torch.full((B, per), float("nan"), device=DEV)
        launch(out, state, B, per, elem_base=elem_base, x=bad, sa=sa, sb=sb)
        keep = [r for r in range(B) if r != row]
        assert bool(torch.isnan(out[row]).all()) and torch.equal(out[keep], outs[0][keep])


# ---------------------------------------------------------------------------------------------------------------- moments
def test_moments_of_a_million_draws():
    """Mean, variance and the mass beyond 3 sigma of 2^20 draws, each within 5 standard deviations of the normal's (the float64
    restatement satisfies all three for this seed: tests/test_host_stream_noise.py)."""
    z = draw(1, MOMENT_N, 0, seed=MOMENT_SEED, purpose=2).cpu().numpy().reshape(-1)
    zz = z.astype(np.float64)
    print(f"mean {zz.mean():.3e}  var - 1 {zz.var() - 1:.3e}  P(|z| > 3) {(np.abs(zz) > 3).mean():.6f}")
    assert all(moments_hold(z)), moments_hold(z)


# ---------------------------------------------------------------------------------------------------------------- DeviceNoise
def test_device_noise_surface():
    import phendiff_amd as P
    n = P.DeviceNoise(SEED, DEV, rank=2, first_index=4)
    assert n.index == 4 and n.state.cpu().tolist() == [signed(SEED), 4]
    r = n.randn((3, 3, 8, 8), P.DeviceNoise.PURPOSE_INITIAL_SAMPLE)
    assert torch.equal(r.view(3, -1), draw(3, 192, 4, rank=2, purpose=3)) and n.index == 4      # a draw does not advance
    v = n.variance_noise(2, (3, 3, 8, 8))
    assert torch.equal(v.view(3, -1), draw(3, 192, 4, rank=2, purpose=5, elem_base=2 * 192))
    buf = r.clone()
    assert n.add_variance_noise(buf, 0.25, 2) is buf and torch.equal(buf, r + 0.25 * v)
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    ts = torch.tensor([10, 2000, 2999], device=DEV)
    z = n.randn(r.shape, P.DeviceNoise.PURPOSE_FORWARD_NOISE)
    assert torch.equal(n.add_noise(sched, r, ts), sched.add_noise(r, z, ts))
    n.advance(3)
    assert n.index == 7 and n.state.cpu().tolist()[1] == 7
    assert torch.equal(n.randn((1, 192), 3), draw(1, 192, 7, rank=2, purpose=3))
    sd = n.state_dict()
    assert sd == {"seed": SEED, "rank": 2, "index": 7}
    m = P.DeviceNoise(1, DEV)
    m.load_state_dict(sd)
    assert m.index == 7 and torch.equal(m.randn((1, 192), 3), n.randn((1, 192), 3))
    assert torch.equal(n.seek(4).randn((3, 192), 3), r.view(3, -1))
    with pytest.raises(ValueError, match="step field"):
        n.seek(1 << 48).randn((1, 4))
    top = (1 << 64) - 5                                  # a seed with bit 63 set, held as a negative int64
    assert torch.equal(P.DeviceNoise(top, DEV).randn((1, 192), 3), draw(1, 192, 0, seed=top))
