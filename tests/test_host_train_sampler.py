"""The device training sampler without a GPU: the numpy restatement of its stream (tests/philox_ref.py) against the Philox4x32-10
known-answer vectors and plain statistics, the C ABI of ``pd_train_sample`` (struct layout, export, every refusal before a launch),
the sampler's ``state_dict`` and the untouched default path of ``sample_training_inputs``."""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_ref as R
from abi_header import header_fields

SEED = 1          # the statistics below hold for this seed (restatement alone, on the CPU)

# Random123's kat_vectors for philox4x32-10: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
    assert tuple(int(g[0]) for g in got) == want


def test_counter_layout_of_the_restatement():
    """The four counter words and the key, against a direct Philox call: q's carry into word 1, step's high 16 bits, rank and purpose."""
    seed, step, rank = 0x0123456789ABCDEF, (0xBEEF << 32) | 0x89ABCDEF, 0xABC
    e = (1 << 34) - 2                                         # q = 2^32 - 1 for e, e + 1; q = 2^32 for e + 2, e + 3
    z = R.normal(seed, step, rank, 4, elem_base=e, purpose=2)
    key = (0x89ABCDEF, 0x01234567)
    c3 = (0xBEEF << 16) | (0xABC << 4) | 2
    lo = R.philox4x32_10([np.array([v], dtype=np.uint64) for v in (0xFFFFFFFF, 0, 0x89ABCDEF, c3)], key)
    hi = R.philox4x32_10([np.array([v], dtype=np.uint64) for v in (0, 1, 0x89ABCDEF, c3)], key)

    def pair(xa, xb):
        ua, ub = (int(xa) >> 8) * 2.0 ** -24 + 2.0 ** -25, (int(xb) >> 8) * 2.0 ** -24 + 2.0 ** -25
        r = np.sqrt(-2.0 * np.log(ua))
        return r * np.cos(2 * np.pi * ub), r * np.sin(2 * np.pi * ub)
    want = [*pair(lo[2][0], lo[3][0]), *pair(hi[0][0], hi[1][0])]
    assert np.array_equal(z, np.array(want, dtype=np.float32))
    x = R.philox4x32_10([np.array([v], dtype=np.uint64) for v in (5, 0, 0x89ABCDEF, (c3 & ~0xF) | 1)], key)[0][0]
    assert R.timesteps(seed, step, rank, 6, 1000)[5] == (int(x) * 1000) >> 32


def test_statistics_of_the_restatement():
    n = 1 << 20
    z = R.normal(SEED, 0, 0, n).astype(np.float64)
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    draws, N = 1 << 16, 10
    t = R.timesteps(SEED, 0, 0, draws, N)
    assert t.min() >= 0 and t.max() < N
    hist = np.bincount(t, minlength=N)
    sigma = np.sqrt(draws * (1 / N) * (1 - 1 / N))
    assert np.all(np.abs(hist - draws / N) < 5 * sigma), hist


def test_restatement_slices_agree():
    """Any window of the stream equals the same window of a longer draw (elem_base is a position, not a seed)."""
    whole = R.normal(SEED, 3, 1, 64)
    for base, n in ((0, 1), (3, 7), (5, 59), (62, 2)):
        assert np.array_equal(R.normal(SEED, 3, 1, n, elem_base=base), whole[base:base + n])
    assert not np.array_equal(R.normal(SEED, 3, 1, 64, purpose=2), whole)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_struct_field_order_matches_header():
    import phendiff_amd._lib as L
    fields = header_fields("pd_train_sample_args")
    assert fields == [f[0] for f in L.TrainSampleArgs._fields_]
    assert fields == ["seed", "step", "rank", "purpose", "B", "per_sample", "elem_base", "N", "clean", "sqrt_acp", "sqrt_1m_acp",
                      "timesteps_in", "timesteps_out", "noise", "noisy"]
    # the 64-bit members sit where a C compiler puts them (natural alignment, no packing)
    T = L.TrainSampleArgs
    assert (T.seed.offset, T.step.offset, T.rank.offset, T.purpose.offset, T.B.offset, T.per_sample.offset, T.elem_base.offset,
            T.N.offset, T.clean.offset) == (0, 8, 16, 20, 24, 32, 40, 48, 56)
    assert C.sizeof(T) == 56 + 7 * 8


def test_symbol_is_exported_and_abi_stays_8():
    import phendiff_amd._lib as L
    lib = L.lib()
    assert hasattr(lib, "pd_train_sample") and "pd_train_sample" in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == 8


def test_refusals_before_any_launch():
    """Every refusal returns a negative code and names its reason; the stream is null and the pointers are never dereferenced."""
    import phendiff_amd._lib as L
    lib = L.lib()
    ok = dict(seed=1, step=0, rank=0, purpose=0, B=2, per_sample=8, elem_base=0, N=10, clean=0x10000, sqrt_acp=0x20000,
              sqrt_1m_acp=0x30000, timesteps_out=0x40000, noise=0x50000, noisy=0x60000)

    def refused(code, word, **change):
        rc = lib.pd_train_sample(C.byref(L.TrainSampleArgs(**dict(ok, **change))), None)
        msg = lib.pd_last_error()
        assert rc == code, (change, rc, msg)
        assert word in msg, (change, msg)

    assert lib.pd_train_sample(None, None) == -1 and b"null args" in lib.pd_last_error()
    refused(-1, b"null noise", noise=None)
    refused(-1, b"null noisy", noisy=None)
    refused(-1, b"null timesteps", timesteps_out=None)
    refused(-1, b"N = 0", N=0)
    refused(-1, b"N = -3", N=-3)
    refused(-1, b"rank", rank=4096)
    refused(-1, b"rank", rank=-1)
    refused(-1, b"step", step=1 << 48)
    refused(-1, b"purpose", purpose=1)
    refused(-1, b"purpose", purpose=16)
    refused(-1, b"tables", sqrt_acp=None)
    refused(-1, b"tables", sqrt_1m_acp=None)
    refused(-1, b"noisy without clean", clean=None)
    refused(-2, b"positive", B=0)
    refused(-2, b"positive", per_sample=-4)
    refused(-2, b"2^62", B=1 << 20, per_sample=1 << 50)
    refused(-2, b"2^62", elem_base=1 << 63)
    refused(-2, b"grid too large", B=1, per_sample=1 << 45)


# ---------------------------------------------------------------------------------------------------------------- Python surface
def test_sampler_needs_a_device_and_is_exported():
    import phendiff_amd as P
    assert P.DeviceTrainingSampler is P.training.DeviceTrainingSampler
    with pytest.raises(P.PhenDiffHipError):
        P.DeviceTrainingSampler(P.DDIMScheduler(), seed=1, device="cpu")


def test_state_dict_round_trip():
    import phendiff_amd as P
    sched = P.DDIMScheduler(num_train_timesteps=50)
    a = P.DeviceTrainingSampler(sched, seed=(1 << 63) + 5, device="cuda:0", rank=3)      # (constructing touches no device)
    a._step = 41
    sd = a.state_dict()
    assert sd == {"seed": (1 << 63) + 5, "rank": 3, "step": 41} and a.step == 41
    b = P.DeviceTrainingSampler(sched, seed=0, device="cuda:0")
    b.load_state_dict(sd)
    assert b.state_dict() == sd and b.step == 41
    # a rank given at construction is kept; an unset one follows the trainer's
    a.bind_rank(7)
    assert a.rank == 3
    c = P.DeviceTrainingSampler(sched, seed=0, device="cuda:0")
    assert c.rank == 0
    c.bind_rank(7)
    assert c.rank == 7
    with pytest.raises(ValueError):
        P.DeviceTrainingSampler(sched, seed=0, device="cuda:0", rank=4096)


def test_default_path_is_untouched():
    """Without a sampler ``sample_training_inputs`` draws from the caller's generators as before: called twice with equally seeded CPU
    generators it returns the same noise, which is torch's own ``randn`` of that seed (the timesteps come from an unseeded ``randint``
    here and ``add_noise`` needs a device: only the noise is compared)."""
    import inspect
    from phendiff_amd import training as T
    assert inspect.signature(T.sample_training_inputs).parameters["sampler"].default is None

    class Sched:
        class config:
            num_train_timesteps = 10

        def add_noise(self, clean, noise, t):
            assert t.dtype == torch.long and t.shape == (clean.shape[0],) and int(t.min()) >= 0 and int(t.max()) < 10
            return clean

    shape = (2, 3, 8, 8)
    got = [T.sample_training_inputs(torch.zeros(shape), Sched(), cpu_generator=torch.Generator().manual_seed(123))[0] for _ in range(2)]
    assert torch.equal(got[0], got[1])
    assert torch.equal(got[0], torch.randn(shape, generator=torch.Generator().manual_seed(123)))
