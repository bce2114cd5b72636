"""The masked class transfer without a GPU: the float64 reference's known answers, the margin condition under which the GPU test may
demand exact masks, the C ABI of the three entry points (struct layout, export, validation before any launch) and the host logic of
``phendiff_amd.masked`` (the blend's index rule, the encode level, every refusal -- on meta / CPU objects, with nothing packed)."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_header import define, header_fields
from contrast_mask_cases import CASES, RATIO, case_id, inputs, reference
from contrast_mask_ref import class_contrast_ref, contrast_mask_ref, mask_blend_ref

CONTRAST_FIELDS = ["B", "C", "per_pixel", "a", "b", "acc", "first"]
MASK_FIELDS = ["B", "per_pixel", "acc", "ratio", "mask", "map", "stats", "workspace"]
BLEND_FIELDS = ["B", "C", "per_pixel", "x", "keep", "mask", "out"]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def test_reference_hand_computed_example():
    a = np.array([[[[1.0, -2.0], [3.0, 4.0]], [[0.0, 0.0], [0.0, 2.0]]]])      # (1, 2, 2, 2)
    b = np.zeros_like(a)
    acc = class_contrast_ref(a, b)
    assert np.array_equal(acc, [[[0.5, 1.0], [1.5, 3.0]]])
    acc = class_contrast_ref(a, b, acc)      # a second draw of the same
    assert np.array_equal(acc, [[[1.0, 2.0], [3.0, 6.0]]])
    mask, cmap, stats = contrast_mask_ref([[[1.0, 1.0], [1.0, 5.0]]], 3.0)      # mean 2, limit 6
    assert np.array_equal(mask, [[[0, 0], [0, 1]]])
    assert np.allclose(cmap, [[[1 / 6, 1 / 6], [1 / 6, 5 / 6]]], rtol=0, atol=1e-15)
    assert stats.tolist() == [[2.0, 6.0, 0.25]]
    mask, cmap, _ = contrast_mask_ref([[[1.0, 1.0], [1.0, 50.0]]], 3.0)      # mean 13.25, limit 39.75: the outlier saturates at 1
    assert cmap[0, 1, 1] == 1.0 and mask.sum() == 1
    x, keep = np.full((1, 2, 2, 2), 7.0), np.full((1, 2, 2, 2), np.nan)
    out = mask_blend_ref(x, keep, [[[1, 0], [0, 1]]])
    assert np.array_equal(np.isnan(out), [[[[False, True], [True, False]]] * 2])


def test_reference_equal_inputs_give_an_empty_mask():
    a = np.random.default_rng(0).standard_normal((2, 3, 4, 4))
    acc = class_contrast_ref(a, a)
    assert not acc.any()
    mask, cmap, stats = contrast_mask_ref(acc, 3.0)
    assert not mask.any() and not cmap.any() and not stats.any()      # limit = 0
    acc[1, 0, 0] = np.nan                                             # a broken sample: empty too, its neighbour unchanged
    acc[0, 1, 1] = 4.0
    mask, cmap, stats = contrast_mask_ref(acc, 3.0)
    assert not mask[1].any() and not cmap[1].any() and stats[1, 2] == 0 and np.isnan(stats[1, 0])
    assert mask[0].sum() == 1 and stats[0, 2] == np.float32(1 / 16)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_is_invariant_to_scaling_acc(case):
    ref = reference(case)
    for scale in (0.25, 8.0):      # powers of two: every rounding scales with them
        mask, cmap, stats = contrast_mask_ref(ref["acc32"] * np.float32(scale), RATIO)
        assert np.array_equal(mask, ref["mask"]) and np.array_equal(cmap, ref["map"])
        assert np.array_equal(stats[:, 2], ref["stats"][:, 2])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_margin_condition(case):
    """No pixel of the reference map within 1e-3 of the threshold: the condition under which the GPU test demands exact mask equality
    (the GPU map may differ from the reference by 2 fp32 ulp ~ 1.2e-7).  Masks are neither empty nor full."""
    ref = reference(case)
    assert float(np.abs(ref["map"] - 0.5).min()) > 1e-3
    for s in range(case[0]):
        assert 0 < int(ref["mask"][s].sum()) < ref["mask"][s].size
    a, b = inputs(case)
    assert len(a) == len(b) == case[4] and a[0].shape == case[:4] and a[0].dtype == np.float32


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_structs_and_exports():
    import phendiff_amd._lib as L
    assert header_fields("pd_class_contrast_args") == CONTRAST_FIELDS == [f[0] for f in L.ClassContrastArgs._fields_]
    assert header_fields("pd_contrast_mask_args") == MASK_FIELDS == [f[0] for f in L.ContrastMaskArgs._fields_]
    assert header_fields("pd_mask_blend_args") == BLEND_FIELDS == [f[0] for f in L.MaskBlendArgs._fields_]
    lib = L.lib()
    for name in ("pd_class_contrast", "pd_contrast_mask", "pd_contrast_mask_workspace", "pd_mask_blend"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == 8
    chunk = define("PD_CONTRAST_MASK_CHUNK")
    assert L.CONSTANTS["PD_CONTRAST_MASK_CHUNK"] == chunk and chunk % 1024 == 0
    # one fp64 partial per (sample, chunk); 0 for the sizes the call refuses
    assert lib.pd_contrast_mask_workspace(3, 67 * 61) == 3 * -(-67 * 61 // chunk) * 8
    assert lib.pd_contrast_mask_workspace(1, 1) == 8
    assert lib.pd_contrast_mask_workspace(0, 5) == lib.pd_contrast_mask_workspace(2, 0) == lib.pd_contrast_mask_workspace(-1, 5) == 0
    assert 67 * 61 > chunk and (67 * 61) % chunk      # the large shared case spans chunks and ends inside one


def _aligned_buffer(nbytes=4096):
    buf = (C.c_char * (nbytes + 16))()
    return buf, (C.addressof(buf) + 15) // 16 * 16


def test_entry_points_validate_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    _keep, p = _aligned_buffer()
    nan, inf = float("nan"), float("inf")
    shapes = [dict(C=0), dict(C=33), dict(C=-1), dict(per_pixel=0), dict(per_pixel=-4), dict(B=0), dict(B=-2)]
    table = [
        ("pd_class_contrast", L.ClassContrastArgs, dict(B=2, C=3, per_pixel=35, a=p, b=p, acc=p, first=1),
         shapes + [{n: None} for n in ("a", "b", "acc")] + [{n: p + 4} for n in ("a", "b", "acc")] + [dict(B=1 << 40, per_pixel=1 << 40)]),
        ("pd_contrast_mask", L.ContrastMaskArgs, dict(B=2, per_pixel=35, acc=p, ratio=3.0, mask=p, map=p, stats=p, workspace=p),
         [dict(per_pixel=0), dict(B=0), dict(B=-1)] + [{n: None} for n in ("acc", "mask", "workspace")]
         + [dict(acc=p + 4), dict(map=p + 8), dict(stats=p + 2), dict(workspace=p + 4)]
         + [dict(ratio=r) for r in (0.0, -1.0, nan, inf)] + [dict(B=1 << 20, per_pixel=1 << 40)]),
        ("pd_mask_blend", L.MaskBlendArgs, dict(B=2, C=3, per_pixel=35, x=p, keep=p, mask=p, out=p),
         shapes + [{n: None} for n in ("x", "keep", "mask", "out")] + [{n: p + 4} for n in ("x", "keep", "out")]),
    ]
    for name, struct, ok, bad in table:
        fn = getattr(lib, name)
        for change in bad:
            rc = fn(C.byref(struct(**dict(ok, **change))), None)
            assert rc < 0, (name, change)
            assert name.encode() in lib.pd_last_error(), (name, change, lib.pd_last_error())
        assert fn(None, None) < 0 and name.encode() in lib.pd_last_error() and b"null args" in lib.pd_last_error()
    # sizes answer PD_ERR_SHAPE, pointers and the ratio PD_ERR_ARG
    assert lib.pd_class_contrast(C.byref(L.ClassContrastArgs(**dict(table[0][2], C=33))), None) == L.PD_ERR_SHAPE
    assert lib.pd_contrast_mask(C.byref(L.ContrastMaskArgs(**dict(table[1][2], ratio=nan))), None) == -1
    assert lib.pd_mask_blend(C.byref(L.MaskBlendArgs(**dict(table[2][2], mask=None))), None) == -1


# ---- host logic --------------------------------------------------------------------------------------------------------------------------
def test_blend_state_index():
    import phendiff_amd as P
    for S in (1, 2, 50):
        idx = [P.blend_state_index(k, S) for k in range(S)]
        assert idx == list(range(S - 1, -1, -1))      # after step k the state of S - 1 - k inverse steps; the last one is the input
        assert idx[-1] == 0 and idx[0] == S - 1
        for k in (-1, S, S + 3):
            with pytest.raises(ValueError):
                P.blend_state_index(k, S)


def _scheduler(**over):
    import phendiff_amd as P
    return P.DDIMScheduler(**dict(P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"], **over))


@pytest.mark.parametrize("spacing", ["leading", "trailing"])
def test_encode_timestep_follows_get_timesteps(spacing):
    import phendiff_amd as P
    S = 50
    sched = _scheduler(timestep_spacing=spacing)
    for strength in (0.02, 0.5, 1.0):
        got = P.encode_timestep(sched, S, strength)
        # diffusers' get_timesteps, written out
        init_timestep = min(int(S * strength), S)
        t_start = max(S - init_timestep, 0)
        sched.set_timesteps(S)
        assert got == int(sched.timesteps[t_start:][0]) and isinstance(got, int)
    assert P.encode_timestep(sched, S, 1.0) == int(sched.timesteps[0])
    assert P.encode_timestep(sched, S, 0.02) == int(sched.timesteps[-1])
    for bad in (0.0, 0.01, -0.5, 1.5, float("nan"), None):      # 0.01: int(50 * 0.01) = 0 steps
        with pytest.raises(ValueError):
            P.encode_timestep(sched, S, bad)


def _meta_pipe(scheduler=None):
    import phendiff_amd as P
    with torch.device("meta"):
        unet = P.CustomCondUNet2DModel(**dict(P.UNET_CONFIGS["super_small"], sample_size=32))
    return P.ConditionalDDIMPipeline(unet, scheduler if scheduler is not None else _scheduler())


def _nothing_packed(pipe):
    return pipe.unet._weights is None and not pipe.unet._plans


def test_refusals_before_anything_is_packed():
    import phendiff_amd as P
    from phendiff_amd.schedulers import MULTISTEP_NOT_MASKED
    x = torch.zeros(2, 3, 32, 32)
    labels = torch.tensor([0, 1])
    ones = torch.ones(2, 1, 32, 32, dtype=torch.uint8)
    entries = {
        "masked_ddib": lambda pipe, B=2, **kw: P.masked_ddib(pipe, torch.zeros(B, 3, 32, 32, device="meta") if B != 2 else x, labels, 1 - labels, 4, **kw),
        "class_contrast_mask": lambda pipe, B=2, **kw: P.class_contrast_mask(pipe, torch.zeros(B, 3, 32, 32, device="meta") if B != 2 else x,
                                                                            labels, 1 - labels, 4, **kw),
        "MaskedDDIBGraph": lambda pipe, B=2, **kw: P.MaskedDDIBGraph(pipe, B, 4, **kw),
    }
    # the multistep schedulers, with the new reason
    multistep = _meta_pipe(P.DPMSolverMultistepScheduler())
    for name, call in entries.items():
        with pytest.raises(NotImplementedError) as e:
            call(multistep)
        assert MULTISTEP_NOT_MASKED in str(e.value) and name in str(e.value)
    assert "invalidates" in MULTISTEP_NOT_MASKED
    # the latent-diffusion pipeline, named
    latent = object.__new__(P.CustomStableDiffusionImg2ImgPipeline)
    for name, call in entries.items():
        with pytest.raises(NotImplementedError, match="CustomStableDiffusionImg2ImgPipeline"):
            call(latent)
    pipe = _meta_pipe()
    most = pipe.unet.max_batch(32, 32)
    for name, call in entries.items():
        with pytest.raises(ValueError, match="no sliced form"):      # batches beyond one launch plan
            call(pipe, B=most + 1)
    for name in ("masked_ddib", "class_contrast_mask", "MaskedDDIBGraph"):
        call = entries[name]
        for bad in (0, -1, 2.5, True):
            with pytest.raises(ValueError, match="num_maps"):
                call(pipe, num_maps=bad)
        for bad in (0.0, -3.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="threshold_ratio"):
                call(pipe, threshold_ratio=bad)
    for bad in (0.0, 0.1, 1.5):      # 0.1 of 4 steps: no step at all
        with pytest.raises(ValueError, match="encode_strength"):
            P.class_contrast_mask(pipe, x, labels, 1 - labels, 4, encode_strength=bad)
        with pytest.raises(ValueError, match="encode_strength"):
            P.MaskedDDIBGraph(pipe, 2, 4, noise=object.__new__(P.DeviceNoise), encode_strength=bad)
    # a mask of the wrong shape, dtype or device
    for bad in (torch.ones(2, 1, 32, 31, dtype=torch.uint8), torch.ones(3, 32, 32, dtype=torch.uint8), torch.ones(2, 3, 32, 32, dtype=torch.uint8),
                torch.ones(2, 1, 32, 32), torch.ones(2, 1, 32, 32, dtype=torch.int64), torch.ones(2, 1, 32, 32, dtype=torch.uint8, device="meta"),
                np.ones((2, 1, 32, 32), np.uint8)):
        with pytest.raises(ValueError, match="mask"):
            P.masked_ddib(pipe, x, labels, 1 - labels, 4, mask=bad)
        with pytest.raises(ValueError, match="mask"):
            P.mask_blend(x, x, bad)
    assert P.check_mask(ones[:, 0].bool(), 2, 32, 32, "cpu").shape == (2, 1, 32, 32)
    # a graph that computes its mask draws from a DeviceNoise; one that is given its mask draws nothing
    with pytest.raises(TypeError, match="DeviceNoise"):
        P.MaskedDDIBGraph(pipe, 2, 4, mask="contrast", noise=torch.Generator())
    with pytest.raises(ValueError, match="noise"):
        P.MaskedDDIBGraph(pipe, 2, 4, mask="given", noise=object.__new__(P.DeviceNoise))
    with pytest.raises(ValueError, match='"contrast" or "given"'):
        P.MaskedDDIBGraph(pipe, 2, 4, mask="soft")
    # what is left is the device: no CPU fallback -- and still nothing was packed
    with pytest.raises(P.PhenDiffHipError):
        P.masked_ddib(pipe, x, labels, 1 - labels, 4, mask=ones)
    with pytest.raises(P.PhenDiffHipError):
        P.MaskedDDIBGraph(pipe, 2, 4, mask="given")
    with pytest.raises(P.PhenDiffHipError):
        P.mask_blend(x, x, ones)
    assert _nothing_packed(pipe) and _nothing_packed(multistep)


def test_step_lists_of_different_length_are_refused(monkeypatch):
    """The blend pairs forward step k with inversion state S - 1 - k: an inverse scheduler that walks another number of steps is refused."""
    import phendiff_amd as P
    import phendiff_amd.masked as M
    pipe = _meta_pipe()

    def short_schedules(pipe_, S, variant, gen_timesteps=None, **kw):
        inv, fwd, inv_ts, gen_ts = P.trajectories._schedules(pipe_, S, variant, gen_timesteps)
        return inv, fwd, inv_ts[:-1], gen_ts
    monkeypatch.setattr(M, "_schedules", short_schedules)
    with pytest.raises(ValueError, match="3 inversion steps against 4 forward steps"):
        P.masked_ddib(pipe, torch.zeros(2, 3, 32, 32), torch.tensor([0, 1]), torch.tensor([1, 0]), 4, mask=torch.ones(2, 32, 32, dtype=torch.bool))
    assert _nothing_packed(pipe)
