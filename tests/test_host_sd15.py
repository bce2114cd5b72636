"""Stable Diffusion 1.x denoisers without a GPU: the module tree (parameter count, diffusers' key names and shapes with the 1x1-conv
``proj_in`` / ``proj_out``), config round trips, the refusals, and the C ABI of ``pd_attn_hd`` (struct layout, export, validation)."""
import ctypes as C

import pytest
import torch

from abi_header import header_fields

SD15_PARAMS = 859_520_964       # the public SD 1.x UNet count; re-derived from the oracle below

TINY15 = dict(in_channels=4, out_channels=4, block_out_channels=(160, 320), layers_per_block=1,
              down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
              attention_head_dim=(4, 4), cross_attention_dim=64, norm_num_groups=32, use_linear_projection=False)


def to_conv_form(sd):
    """The oracle's Linear-form state_dict with proj_in / proj_out viewed as 1x1 convolutions (the SD 1.x checkpoint form)."""
    return {k: (v[:, :, None, None] if k.endswith(("proj_in.weight", "proj_out.weight")) else v) for k, v in sd.items()}


def test_sd15_parameter_count_on_meta():
    import phendiff_amd as P
    from oracle import UNet2DConditionRef
    assert P.SD15_UNET_CONFIG is P.configs.SD15_UNET_CONFIG
    with torch.device("meta"):
        m = P.SDUNet2DConditionModel(**P.SD15_UNET_CONFIG)
        r = UNet2DConditionRef(block_out_channels=(320, 640, 1280, 1280), attention_head_dim=8, cross_attention_dim=768)
    assert sum(p.numel() for p in m.parameters()) == SD15_PARAMS
    assert sum(p.numel() for p in r.parameters()) == SD15_PARAMS
    assert m.head_dims == (40, 80, 160)
    c = m.config
    assert (c.use_linear_projection, c.cross_attention_dim, c.sample_size, c.attention_head_dim) == (False, 768, 64, (8, 8, 8, 8))


def test_projection_shapes_and_strict_loading():
    import phendiff_amd as P
    from oracle import UNet2DConditionRef
    torch.manual_seed(0)
    r = UNet2DConditionRef(**dict(TINY15, use_linear_projection=True))
    m = P.SDUNet2DConditionModel(compute_dtype="f32", **TINY15)
    ref, got = r.state_dict(), m.state_dict()
    assert list(ref) == list(got)
    nproj = 0
    for k, v in ref.items():
        if k.endswith(("proj_in.weight", "proj_out.weight")):
            nproj += 1
            assert got[k].shape == tuple(v.shape) + (1, 1) and v.shape[0] == v.shape[1], k
        else:
            assert got[k].shape == v.shape, k
    assert nproj == 8            # one down, the mid and two up transformers
    m.load_state_dict(to_conv_form(ref), strict=True)
    for k, v in to_conv_form(ref).items():
        assert torch.equal(m.state_dict()[k], v), k
    with pytest.raises(RuntimeError):
        m.load_state_dict(ref, strict=True)             # the 2-D (SD 2.x) form does not fit a v1-shaped model
    # the Linear form is untouched
    m2 = P.SDUNet2DConditionModel(compute_dtype="f32", **dict(TINY15, use_linear_projection=True))
    m2.load_state_dict(ref, strict=True)


def test_round_trip_and_config_filtering(tmp_path):
    import phendiff_amd as P
    torch.manual_seed(1)
    m = P.SDUNet2DConditionModel(compute_dtype="f32", **TINY15)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p))
    m.save_pretrained(str(tmp_path / "unet"))
    m2 = P.SDUNet2DConditionModel.from_pretrained(str(tmp_path / "unet"), compute_dtype="f32")
    assert m2.config.use_linear_projection is False and m2.config.attention_head_dim == (4, 4)
    assert m2.config.block_out_channels == (160, 320) and m2.config.cross_attention_dim == 64
    a, b = m.state_dict(), m2.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert b["mid_block.attentions.0.proj_in.weight"].ndim == 4
    # a diffusers config.json carries keys this engine has no use for
    cfg = dict(TINY15, upcast_attention=False, only_cross_attention=False, dual_cross_attention=False, _class_name="UNet2DConditionModel")
    m3 = P.SDUNet2DConditionModel.from_config(cfg, compute_dtype="f32")
    assert m3.config.use_linear_projection is False and not hasattr(m3.config, "upcast_attention")
    m3.load_state_dict(a, strict=True)


@pytest.mark.parametrize("boc,heads", [((96, 192), (2, 4)),         # head_dim 48
                                       ((192, 192), (8, 8))])       # 8 heads on 192 channels: head_dim 24
def test_other_head_dims_stay_refused(boc, heads):
    import phendiff_amd as P
    with pytest.raises(NotImplementedError) as e:
        with torch.device("meta"):
            P.SDUNet2DConditionModel(**dict(TINY15, block_out_channels=boc, attention_head_dim=heads))
    assert "40 / 64 / 80 / 160" in str(e.value)


def test_training_is_refused_before_anything_runs():
    """No GPU here: the refusal comes first, so it is all that can be raised."""
    import phendiff_amd as P
    from phendiff_amd.sd_unet_train import SDUNetTrainer
    with torch.device("meta"):
        m = P.SDUNet2DConditionModel(**TINY15)
    with pytest.raises(NotImplementedError, match="pd_attn_hd.*backward"):
        m.input_grad_plan(1, 16, 16, 77, "cuda:0")
    with pytest.raises(NotImplementedError, match="pd_attn_hd.*backward"):
        SDUNetTrainer(m, P.CustomEmbedding(2, 64), None, 1e-4, device="cuda:0")


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_attn_hd_struct_and_export():
    import phendiff_amd._lib as L
    want = ["dtype", "B", "heads", "D", "Nq", "Nkv", "scale", "q", "q_stride", "k", "v", "kv_stride", "out", "out_stride", "lse"]
    assert header_fields("pd_attn_hd_args") == want == [f[0] for f in L.AttnHdArgs._fields_]
    lib = L.lib()
    assert hasattr(lib, "pd_attn_hd") and "pd_attn_hd" in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == 8


def test_attn_hd_validates_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    ok = dict(dtype=1, B=1, heads=2, D=40, Nq=4, Nkv=4, scale=40 ** -0.5, q=p, q_stride=80, k=p, v=p, kv_stride=80, out=p, out_stride=80)
    for change, word in [(dict(D=64), b"head dimension"), (dict(D=48), b"head dimension"), (dict(Nq=0), b"shape"),
                         (dict(q=None), b"null"), (dict(q_stride=72), b"stride"), (dict(kv_stride=84), b"stride"),
                         (dict(dtype=7), b"dtype"), (dict(scale=float("nan")), b"scale")]:
        rc = lib.pd_attn_hd(C.byref(L.AttnHdArgs(**dict(ok, **change))), None)
        assert rc < 0, change
        assert word in lib.pd_last_error(), (change, lib.pd_last_error())
    assert lib.pd_attn_hd(None, None) < 0
