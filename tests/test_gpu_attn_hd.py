"""pd_attn_hd (head_dim 40 / 80 / 160, the Stable Diffusion 1.x attention) on MI355X: parity with F.scaled_dot_product_attention in
fp32 on the CPU, the hazards of its deferred-rescale softmax, guard bands (tests/guard_bands.py through the engine of
tests/test_gpu_guard_bands.py) and graph capture."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from guard_bands import guard_size
from test_gpu_guard_bands import Case, Op, out_op, p1_poisoned_surroundings, p2_canaried_outputs, p3_sample_isolation
from test_gpu_kernels import DT, bf16_round, env, rel, stream  # noqa: F401

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634

# The project's bounds for this arithmetic (16-bit or exact-fp32 MFMA products, fp32 accumulation, fp32 softmax), restated from
# tests/test_gpu_sd_kernels.py:14-16 (ATTN_D64_TOL, ATTN_D64_LSE_TOL): only the contraction length differs from pd_attn_d64.
ATTN_HD_TOL = {"f32": 5e-6, "bf16": 8e-3, "fp16": 1e-3}
ATTN_HD_LSE_TOL = {"f32": 1e-5, "bf16": 2e-3}

DIMS = (40, 80, 160)
# ragged queries and keys, one key tile and several, more than one workgroup per head, the 77-token context, single elements
PARITY_CASES = [(2, 2, 256, 256), (2, 3, 200, 77), (1, 1, 16, 16), (2, 2, 130, 4), (1, 8, 64, 64), (1, 2, 1, 1), (1, 2, 333, 517)]


def split(t, B, n, heads, D):
    return t.reshape(B, n, heads, D).transpose(1, 2)


def sdpa(q, k, v, B, heads, D, Nq, Nkv):
    return F.scaled_dot_product_attention(split(q, B, Nq, heads, D), split(k, B, Nkv, heads, D),
                                          split(v, B, Nkv, heads, D)).transpose(1, 2).reshape(B, Nq, heads * D)


def lse_ref(q, k, B, heads, D, Nq, Nkv):
    s = torch.einsum("bhid,bhjd->bhij", split(q, B, Nq, heads, D).double(), split(k, B, Nkv, heads, D).double()) * float(D) ** -0.5
    return torch.logsumexp(s, -1) * LOG2E


def launch(L, lib, code, B, heads, D, Nq, Nkv, qp, qs, kp, vp, kvs, out, out_stride, lse=None):
    a = L.AttnHdArgs(dtype=code, B=B, heads=heads, D=D, Nq=Nq, Nkv=Nkv, scale=float(D) ** -0.5, q=qp, q_stride=qs, k=kp, v=vp,
                     kv_stride=kvs, out=out.data_ptr(), out_stride=out_stride, lse=lse.data_ptr() if lse is not None else None)
    L.check(lib.pd_attn_hd(C.byref(a), stream()), "pd_attn_hd")


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("cfg", PARITY_CASES)
def test_attention_hd(env, mode, D, cfg):
    L, lib, _, dev = env
    code, tdt = DT[mode]
    B, heads, Nq, Nkv = cfg
    Cc = heads * D
    g = torch.Generator().manual_seed(41)
    if Nq == Nkv:       # q, k, v are slices of one fused projection output [B][N][3C]
        qkv = bf16_round(torch.randn(B, Nq, 3 * Cc, generator=g), mode)
        q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        QKV = qkv.to(tdt).to(dev).contiguous()
        esz = QKV.element_size()
        qptr, kptr, vptr, qs, kvs = QKV.data_ptr(), QKV.data_ptr() + Cc * esz, QKV.data_ptr() + 2 * Cc * esz, 3 * Cc, 3 * Cc
    else:               # cross attention: q [B][Nq][C], kv = fused [B][Nkv][2C]
        q = bf16_round(torch.randn(B, Nq, Cc, generator=g), mode)
        kv = bf16_round(torch.randn(B, Nkv, 2 * Cc, generator=g), mode)
        k, v = kv[..., :Cc], kv[..., Cc:]
        Q, KV = q.to(tdt).to(dev).contiguous(), kv.to(tdt).to(dev).contiguous()
        qptr, kptr, vptr, qs, kvs = Q.data_ptr(), KV.data_ptr(), KV.data_ptr() + Cc * KV.element_size(), Cc, 2 * Cc
    out = torch.full((B, Nq, Cc), float("nan"), dtype=tdt, device=dev)
    lse = torch.full((B, heads, Nq), float("nan"), dtype=torch.float32, device=dev)
    launch(L, lib, code, B, heads, D, Nq, Nkv, qptr, qs, kptr, vptr, kvs, out, Cc, lse)
    torch.cuda.synchronize()
    err = rel(out.float(), sdpa(q, k, v, B, heads, D, Nq, Nkv))
    lerr = rel(lse.cpu(), lse_ref(q, k, B, heads, D, Nq, Nkv))
    print(f"pd_attn_hd {mode} D={D} {cfg}: out {err:.3e} lse {lerr:.3e}")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    assert err < ATTN_HD_TOL[mode]
    if mode in ATTN_HD_LSE_TOL:
        assert lerr < ATTN_HD_LSE_TOL[mode]


# ---- softmax hazards: where a deferred rescale breaks ----------------------------------------------------------------------------------
# The kernel keeps a reference maximum and raises it only when a sub-tile's score exceeds it by RESCALE_THR = 8 (log2 domain).
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("hazard", ["rising", "late_spike", "all_equal"])
def test_attention_hd_softmax_hazards(env, mode, D, hazard):
    L, lib, _, dev = env
    code, tdt = DT[mode]
    B, heads, N = 1, 2, 320                     # five 64-key (ten 32-key) tiles
    Cc = heads * D
    g = torch.Generator().manual_seed(7)
    q = torch.randn(B, N, Cc, generator=g)
    k = torch.randn(B, N, Cc, generator=g) * 0.05
    v = torch.randn(B, N, Cc, generator=g)
    qh, kh = split(q, B, N, heads, D), split(k, B, N, heads, D)          # views: writes land in q / k
    scale_l2 = float(D) ** -0.5 * LOG2E
    u = qh[:, :, 3] / qh[:, :, 3].norm(dim=-1, keepdim=True)            # unit vector along query 3
    qn = float(qh[:, :, 3].norm(dim=-1).min())
    if hazard == "rising":                      # query 3: score rises by ~12 (log2) per 32 keys -- more than the threshold in EVERY sub-tile
        ramp = torch.arange(N, dtype=torch.float32) * (12.0 / 32.0) / (scale_l2 * qn)
        kh += ramp[None, None, :, None] * u[:, :, None, :]
    elif hazard == "late_spike":                # query 3: one key in the last tile ~60 (log2) above everything before it
        kh[:, :, 301] = u * (60.0 / (scale_l2 * qn))
    else:                                       # every key the same vector: every score of a row equal, out = v's mean
        kh[:] = kh[:, :, :1]
    q, k, v = (bf16_round(t, mode) for t in (q, k, v))
    Q, K, V = (t.to(tdt).to(dev).contiguous() for t in (q, k, v))
    out = torch.full((B, N, Cc), float("nan"), dtype=tdt, device=dev)
    lse = torch.full((B, heads, N), float("nan"), dtype=torch.float32, device=dev)
    launch(L, lib, code, B, heads, D, N, N, Q.data_ptr(), Cc, K.data_ptr(), V.data_ptr(), Cc, out, Cc, lse)
    torch.cuda.synchronize()
    s = torch.einsum("bhid,bhjd->bhij", split(q, B, N, heads, D).double(), split(k, B, N, heads, D).double()) * float(D) ** -0.5
    s3 = s[:, :, 3] * LOG2E
    if hazard == "rising":
        assert float((s3[..., 32:] .reshape(B, heads, -1, 32).max(-1).values - s3[..., :-32].reshape(B, heads, -1, 32).max(-1).values).min()) > 8.0
    elif hazard == "late_spike":
        assert float((s3[..., 301] - s3[..., :301].max(-1).values).min()) > 50.0
    else:
        assert float((s.max(-1).values - s.min(-1).values).max()) < 1e-12
    ref = (torch.softmax(s, -1) @ split(v, B, N, heads, D).double()).transpose(1, 2).reshape(B, N, Cc)
    err, lerr = rel(out.float(), ref), rel(lse.cpu(), torch.logsumexp(s, -1) * LOG2E)
    print(f"pd_attn_hd {mode} D={D} {hazard}: out {err:.3e} lse {lerr:.3e}")
    assert bool(torch.isfinite(out).all())
    assert err < ATTN_HD_TOL[mode]
    assert lerr < ATTN_HD_LSE_TOL[mode]


# ---- guard bands -------------------------------------------------------------------------------------------------------------------------
# (B, heads, Nq, Nkv): cross layout (q [B][Nq][C], kv fused [B][Nkv][2C]) resp. self layout (one fused [B][N][3C]).  Every operand's
# rows are 64 elements wider than their contents (q_stride = C + 64 resp. 3C + 64, kv_stride = 2C + 64 resp. 3C + 64, out_stride = C + 64):
# the gap columns behind each row are NaN in P1 (inputs; the last head's pad pieces would read them) and canary in P2 (out).
# Guards: 128 rows (two 64-key tiles) of the operand's row stride, >= 64 KiB, before and after -- NaN directly behind the last
# sample's last key row in P1.
GUARD_CASES = {"cross-B2-h2-130x77": ((2, 2, 130, 77), "cross"), "self-B1-h3-64": ((1, 3, 64, 64), "self")}
IPAD = 64
OPAD = 64


def attn_hd_case(env_, mode, D, key):
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    (B, heads, Nq, Nkv), layout = GUARD_CASES[key]
    Cc = heads * D
    g = torch.Generator().manual_seed(141)
    if layout == "self":
        qkv = bf16_round(torch.randn(B, Nq, 3 * Cc, generator=g), mode)
        q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        ins = {"qkv": Op(qkv.to(tdt), guard_size(64, 3 * Cc + IPAD, tdt), stride=3 * Cc + IPAD, sample_dim=0)}
    else:
        q = bf16_round(torch.randn(B, Nq, Cc, generator=g), mode)
        kv = bf16_round(torch.randn(B, Nkv, 2 * Cc, generator=g), mode)
        k, v = kv[..., :Cc], kv[..., Cc:]
        ins = {"q": Op(q.to(tdt), guard_size(64, Cc + IPAD, tdt), stride=Cc + IPAD, sample_dim=0),
               "kv": Op(kv.to(tdt), guard_size(64, 2 * Cc + IPAD, tdt), stride=2 * Cc + IPAD, sample_dim=0)}
    outs = {"out": out_op((B, Nq, Cc), tdt, guard=guard_size(64, Cc + OPAD, tdt), stride=Cc + OPAD, sample_dim=0),
            "lse": out_op((B, heads, Nq), torch.float32, sample_dim=0)}

    def run(T):
        esz = T["out"].element_size()
        if layout == "self":
            p = T["qkv"].data_ptr()
            qp, kp, vp, qs, kvs = p, p + Cc * esz, p + 2 * Cc * esz, 3 * Cc + IPAD, 3 * Cc + IPAD
        else:
            qp, kp, vp, qs, kvs = T["q"].data_ptr(), T["kv"].data_ptr(), T["kv"].data_ptr() + Cc * esz, Cc + IPAD, 2 * Cc + IPAD
        assert T["out"].stride(-2) == Cc + OPAD and all(T[n].stride(-2) == T[n].shape[-1] + IPAD for n in ins)
        launch(L, lib, code, B, heads, D, Nq, Nkv, qp, qs, kp, vp, kvs, T["out"], Cc + OPAD, T["lse"])

    def check(O):
        assert rel(O["out"].float(), sdpa(q, k, v, B, heads, D, Nq, Nkv)) < ATTN_HD_TOL[mode]
        if mode in ATTN_HD_LSE_TOL:
            assert rel(O["lse"], lse_ref(q, k, B, heads, D, Nq, Nkv)) < ATTN_HD_LSE_TOL[mode]

    return Case(ins, outs, run, check, nsamples=B)


GUARD_PARAMS = [(D, k, m) for D in DIMS for k in GUARD_CASES for m in ("f32", "bf16", "fp16")]


@pytest.mark.parametrize("D,key,mode", GUARD_PARAMS)
def test_attn_hd_p1_poisoned_surroundings(env, monkeypatch, D, key, mode):
    p1_poisoned_surroundings(attn_hd_case(env, mode, D, key), env[3], monkeypatch)


@pytest.mark.parametrize("D,key,mode", GUARD_PARAMS)
def test_attn_hd_p2_canaried_outputs(env, monkeypatch, D, key, mode):
    p2_canaried_outputs(attn_hd_case(env, mode, D, key), env[3], monkeypatch)


@pytest.mark.parametrize("D,key,mode", [p for p in GUARD_PARAMS if GUARD_CASES[p[1]][0][0] > 1])
def test_attn_hd_p3_sample_isolation(env, monkeypatch, D, key, mode):
    p3_sample_isolation(attn_hd_case(env, mode, D, key), env[3], monkeypatch)


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_attn_hd_graph_replay_is_bit_identical(env, D):
    L, lib, _, dev = env
    code, tdt = DT["bf16"]
    B, heads, N = 2, 2, 200
    Cc = heads * D
    g = torch.Generator().manual_seed(5)
    QKV = torch.randn(B, N, 3 * Cc, generator=g).to(tdt).to(dev)
    p, esz = QKV.data_ptr(), 2
    eager = torch.full((B, N, Cc), float("nan"), dtype=tdt, device=dev)
    lse_e = torch.full((B, heads, N), float("nan"), dtype=torch.float32, device=dev)
    launch(L, lib, code, B, heads, D, N, N, p, 3 * Cc, p + Cc * esz, p + 2 * Cc * esz, 3 * Cc, eager, Cc, lse_e)
    torch.cuda.synchronize()
    out = torch.full((B, N, Cc), float("nan"), dtype=tdt, device=dev)
    lse = torch.full((B, heads, N), float("nan"), dtype=torch.float32, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(L, lib, code, B, heads, D, N, N, p, 3 * Cc, p + Cc * esz, p + 2 * Cc * esz, 3 * Cc, out, Cc, lse)
    out.fill_(float("nan"))
    lse.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), eager.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse_e.view(torch.int32))
