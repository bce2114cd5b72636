"""``pd_attn_hd_bwd`` and head_dim 16 / 32 of the pixel UNet without a GPU: the C ABI of the new entry point (struct layout, export,
validation before any launch), ``pd_attn_hd``'s acceptance of D = 16 / 32, and the module tree for ``attention_head_dim`` 16 / 32."""
import ctypes as C

import pytest
import torch

from abi_header import header_fields

BWD_FIELDS = ["dtype", "B", "heads", "D", "Nq", "Nkv", "scale", "q", "q_stride", "k", "v", "kv_stride", "o", "dout", "o_stride",
              "lse", "delta", "dq", "dq_stride", "dk", "dv", "dkv_stride"]


def test_attn_hd_bwd_struct_and_export():
    import phendiff_amd._lib as L
    assert header_fields("pd_attn_hd_bwd_args") == BWD_FIELDS == [f[0] for f in L.AttnHdBwdArgs._fields_]
    assert header_fields("pd_attn_wide_bwd_args") == BWD_FIELDS            # the same fields in the same order
    assert [f[1] for f in L.AttnHdBwdArgs._fields_] == [f[1] for f in L.AttnWideBwdArgs._fields_]
    lib = L.lib()
    assert hasattr(lib, "pd_attn_hd_bwd") and "pd_attn_hd_bwd" in L.SYMBOLS
    assert lib.pd_abi_version() == L.ABI_VERSION == 8


def test_attn_hd_bwd_validates_without_gpu():
    import phendiff_amd._lib as L
    lib = L.lib()
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    ok = dict(dtype=1, B=1, heads=5, D=16, Nq=4, Nkv=4, scale=16 ** -0.5, q=p, q_stride=80, k=p, v=p, kv_stride=80, o=p, dout=p,
              o_stride=80, lse=p, delta=p, dq=p, dq_stride=80, dk=p, dv=p, dkv_stride=80)
    cases = [(dict(D=40), b"head dimension"), (dict(D=64), b"head dimension"), (dict(D=24), b"head dimension"),
             (dict(Nq=0), b"shape"), (dict(dtype=7), b"dtype"), (dict(scale=float("nan")), b"scale"),
             (dict(scale=float("inf")), b"scale"), (dict(scale=0.0), b"scale")]
    cases += [({name: None}, b"null") for name in ("q", "k", "v", "o", "dout", "lse", "delta", "dq", "dk", "dv")]
    # 72 < heads * D = 80 (and 84 is no multiple of 8): each of the five strides in turn
    cases += [({name: bad}, b"stride") for name in ("q_stride", "kv_stride", "o_stride", "dq_stride", "dkv_stride") for bad in (72, 84)]
    for change, word in cases:
        rc = lib.pd_attn_hd_bwd(C.byref(L.AttnHdBwdArgs(**dict(ok, **change))), None)
        assert rc < 0, change
        assert word in lib.pd_last_error(), (change, lib.pd_last_error())
    for d in (40, 64, 24):       # the refusal names the built set
        assert lib.pd_attn_hd_bwd(C.byref(L.AttnHdBwdArgs(**dict(ok, D=d))), None) == -2
        assert b"(16, 32)" in lib.pd_last_error()
    # one sample's rows must stay below the selected out-of-range offset
    assert lib.pd_attn_hd_bwd(C.byref(L.AttnHdBwdArgs(**dict(ok, Nkv=1 << 20, kv_stride=1 << 10))), None) == -2
    assert b"3 GiB" in lib.pd_last_error()
    assert lib.pd_attn_hd_bwd(None, None) < 0 and b"null args" in lib.pd_last_error()


@pytest.mark.parametrize("D", [16, 32])
def test_attn_hd_takes_16_and_32(D):
    """Bad strides with D = 16 / 32 fail on the STRIDE: the head dimension itself is accepted."""
    import phendiff_amd._lib as L
    lib = L.lib()
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    c = 5 * D
    ok = dict(dtype=1, B=1, heads=5, D=D, Nq=4, Nkv=4, scale=D ** -0.5, q=p, q_stride=c, k=p, v=p, kv_stride=c, out=p, out_stride=c)
    for change in (dict(q_stride=c - 8), dict(kv_stride=c + 4), dict(out_stride=c - 8)):
        assert lib.pd_attn_hd(C.byref(L.AttnHdArgs(**dict(ok, **change))), None) < 0, change
        msg = lib.pd_last_error()
        assert b"stride" in msg and b"head dimension" not in msg, (change, msg)
    for d in (48, 64, 24):
        assert lib.pd_attn_hd(C.byref(L.AttnHdArgs(**dict(ok, D=d))), None) == -2
        assert b"head dimension" in lib.pd_last_error() and b"16, 32, 40, 80, 160" in lib.pd_last_error()


@pytest.mark.parametrize("d", [16, 32])
def test_model_tree_for_head_dim_16_and_32(d):
    import phendiff_amd as P
    from oracle import CondUNet2DRef
    from phendiff_amd.unet import _Attention
    cfg = dict(P.configs.UNET_CONFIGS["super_small"], attention_head_dim=d)
    keys = CondUNet2DRef.__init__.__code__.co_varnames
    with torch.device("meta"):
        m = P.CustomCondUNet2DModel(**cfg)
        r = CondUNet2DRef(**{k: v for k, v in cfg.items() if k in keys})
    got, ref = m.state_dict(), r.state_dict()
    assert list(got) == list(ref)
    assert all(got[k].shape == ref[k].shape for k in ref)
    attns = [a for a in m.modules() if isinstance(a, _Attention)]
    assert len(attns) == 6          # two down, the mid block's, three up: all on 256 channels
    for a in attns:
        ch = a.to_q.weight.shape[0]
        assert a.heads == ch // d and a.heads * d == ch
