"""pd_stream_noise / pd_stream_advance without a GPU: the args struct as the header declares it and as the binding derives it, the exports,
every refusal (they all come before the launch), the evaluation's image-index arithmetic, and the seed of the moment test (the numpy
restatement of the stream itself satisfies the three bounds the device draws are held to)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import philox_ref as R

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "phendiff_hip.h")
FIELDS = ["state", "index_offset", "rank", "purpose", "B", "per_sample", "elem_base", "a", "b", "sa", "sb", "x", "out"]
MOMENT_SEED, MOMENT_N = 20261020, 1 << 20      # tests/test_gpu_stream_noise.py draws the same numbers on the device


def header_fields(struct):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*" + struct + r"\s*;", text).group(1)
    names = []
    for decl in body.split(";"):
        names += [re.search(r"(\w+)\s*$", part).group(1) for part in decl.split(",") if part.strip()]
    return names


def moments_hold(z):
    """The three bounds of the moment test over n draws: mean, variance, the mass beyond 3 sigma (5 standard deviations each)."""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    p = 0.0027
    tail = float((np.abs(z) > 3).mean())
    return (abs(z.mean()) <= 5 / np.sqrt(n), abs(z.var() - 1) <= 5 * np.sqrt(2 / n), abs(tail - p) <= 5 * np.sqrt(p * (1 - p) / n))


def test_struct_exports_and_abi():
    import phendiff_amd._lib as L
    assert header_fields("pd_stream_noise_args") == FIELDS == [f[0] for f in L.StreamNoiseArgs._fields_]
    types = dict(L.StreamNoiseArgs._fields_)
    assert types["index_offset"] is C.c_uint64 and types["elem_base"] is C.c_uint64 and types["B"] is C.c_int64
    assert types["a"] is C.c_float and types["b"] is C.c_float and types["state"] is C.c_void_p and types["out"] is C.c_void_p
    lib = L.lib()
    for name in ("pd_stream_noise", "pd_stream_advance"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert L.SYMBOLS["pd_stream_advance"][1] == [C.c_void_p, C.c_uint64, C.c_void_p]
    assert lib.pd_abi_version() == L.ABI_VERSION == 8
    assert (L.CONSTANTS["PD_PURPOSE_INITIAL_SAMPLE"], L.CONSTANTS["PD_PURPOSE_FORWARD_NOISE"], L.CONSTANTS["PD_PURPOSE_VARIANCE_NOISE"]) == (3, 4, 5)


def test_refusals_come_before_any_launch():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    ok = dict(state=p, index_offset=0, rank=0, purpose=3, B=2, per_sample=8, elem_base=0, a=1.0, b=1.0, sa=None, sb=None, x=None, out=p)
    cases = [(dict(state=None), b"null state", L.CONSTANTS["PD_ERR_ARG"]), (dict(out=None), b"null out", -1),
             (dict(state=p + 4), b"misaligned", -1), (dict(out=p + 2), b"misaligned", -1), (dict(x=p + 1), b"misaligned", -1),
             (dict(rank=-1), b"rank -1", -1), (dict(rank=4096), b"rank 4096", -1),
             (dict(purpose=-1), b"purpose -1", -1), (dict(purpose=16), b"purpose 16", -1), (dict(purpose=1), b"purpose 1", -1),
             (dict(B=0), b"B = 0", L.PD_ERR_SHAPE), (dict(B=-3), b"B = -3", -2),
             (dict(per_sample=0), b"per_sample = 0", -2), (dict(per_sample=-4), b"per_sample = -4", -2),
             (dict(per_sample=6), b"per_sample = 6", -2), (dict(per_sample=3073), b"multiple of 4", -2),
             (dict(sa=p), b"both sa and sb", -1), (dict(sb=p), b"both sa and sb", -1),
             (dict(B=1 << 20, per_sample=1 << 24), b"grid too large", -2), (dict(B=1 << 41, per_sample=4), b"grid too large", -2),
             (dict(B=4, per_sample=1 << 61), b"grid too large", -2),
             (dict(index_offset=(1 << 48) - 1), b"beyond 2^48", -1), (dict(index_offset=1 << 63), b"beyond 2^48", -1),
             (dict(index_offset=(1 << 64) - 1), b"beyond 2^48", -1)]
    for change, word, code in cases:
        rc = lib.pd_stream_noise(C.byref(L.StreamNoiseArgs(**dict(ok, **change))), None)
        assert rc == code, (change, rc, lib.pd_last_error())
        assert word in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_stream_noise:"), (change, lib.pd_last_error())
    assert lib.pd_stream_noise(None, None) < 0 and b"null args" in lib.pd_last_error()
    assert lib.pd_stream_advance(None, 1, None) < 0 and lib.pd_last_error().startswith(b"pd_stream_advance:")
    assert lib.pd_stream_advance(p + 4, 1, None) < 0 and b"misaligned" in lib.pd_last_error()


def test_device_noise_needs_a_device():
    import phendiff_amd as P
    with pytest.raises(P.PhenDiffHipError, match="no CPU fallback"):
        P.DeviceNoise(1, "cpu")
    with pytest.raises(ValueError, match="rank"):
        P.DeviceNoise(1, "cuda:0", rank=4096)
    with pytest.raises(ValueError, match="step field"):
        P.DeviceNoise(1, "cuda:0", first_index=(1 << 48) + 1)


@pytest.mark.parametrize("world,nb,bs", [(1, 20, 7), (2, 20, 7), (3, 22, 4), (3, 6, 4), (4, 5, 8)])
def test_global_indices_partition_the_evaluation(world, nb, bs):
    """(world 1, batches of 7 for 20 images), two ranks, three ranks with a ragged last batch (22 = 5 x 4 + 2), more ranks than batches:
    over all ranks the images' global indices are 0 .. nb_classes * nb - 1, each once; within a rank a class's batches are contiguous."""
    from phendiff_amd.eval_generation import eval_batch_offsets, eval_batch_sizes, generation_indices
    classes = 3
    seen = []
    for rank in range(world):
        sizes, offs = eval_batch_sizes(nb, bs, world, rank), eval_batch_offsets(nb, bs, world, rank)
        assert len(sizes) == len(offs)
        plan = generation_indices(classes, nb, bs, world, rank)
        assert [(c, s) for c, s, _ in plan] == [(c, s) for c in range(classes) for s in sizes]
        for c, size, first in plan:
            assert c * nb <= first and first + size <= (c + 1) * nb            # image j of class c: c * nb + j, 0 <= j < nb
            seen += list(range(first, first + size))
        for (s0, o0), o1 in zip(zip(sizes, offs), offs[1:]):
            assert o0 + s0 == o1
    assert sorted(seen) == list(range(classes * nb))
    if world == 1:
        assert [k for _, _, k in generation_indices(1, nb, bs)] == list(range(0, nb, bs))


def test_moment_seed_holds_on_the_reference_stream():
    """The seed of the device moment test is chosen so that the float64 restatement satisfies all three bounds: a failure on the device is
    then the kernel's, not the seed's."""
    z = R.normal(MOMENT_SEED, 0, 0, MOMENT_N, purpose=2)
    assert all(moments_hold(z)), moments_hold(z)
