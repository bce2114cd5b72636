"""Guard-band tests: does a kernel read or write OUTSIDE the tensors it was given?  (tests/guard_bands.py holds the helper.)

Every operand sits in the middle of one larger allocation the test owns (at least two tiles of the consuming kernel along its streamed
dimension, never less than 64 KiB, before and after).  Three properties per case and engine:

  P1 poisoned surroundings  inputs guarded; guards zero, then NaN (same allocations, same pointers): outputs bit-identical, and the clean
                            run meets the tolerance of the kernel's parity test (imported, not restated)
  P2 canaried outputs       outputs guarded with a byte pattern, bodies pre-filled with NaN: pattern untouched (gap columns of strided
                            rows included), every body element finite
  P3 sample / row isolation ONE sample (row) of every per-sample input replaced by NaN -- first, middle, last in turn: every output
                            element of the OTHER samples (rows) keeps its bits

How to read a failure: P1 / P3 name the output and how many elements changed (an over-read reached NaN it should never have seen: a bound
computed too large, a masked element multiplied by zero instead of selected away); P2 names the operand and the first guard byte that
changed relative to the tensor's end / start / row end.

Guard sizes (bytes before AND after every operand), per entry point:
  pd_attn_d64 / _bwd   128 rows (2 tiles of 64 keys / queries) x the operand's row stride (kv_stride, q_stride, ...), >= 64 KiB
  pd_attn_d8           128 keys x 8 channels < 64 KiB -> 64 KiB
  pd_linear            2 x 256 rows (the largest token tile) x x_stride resp. N, >= 64 KiB
  pd_token_wgrad       2 x 256 rows x x_stride resp. dy_stride, >= 64 KiB
  pd_layernorm, pd_geglu   2 x 16 rows per workgroup x row width -> 64 KiB
  pd_conv              two whole image rows (2 x W pixels x C channels; a 64-pixel tile's halo stays inside them), >= 64 KiB
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from guard_bands import MIN_GUARD_BYTES, guard_size, guarded, guarded_rows
from test_gpu_kernels import ATTN_D8_TOL, DT, bf16_round, env, rel, stream  # noqa: F401
from test_gpu_sd_kernels import (ATTN_D64_BWD_TOL, ATTN_D64_LSE_TOL, ATTN_D64_TOL, GEGLU_BWD_TOL, KMAX2_RTOL, LINEAR_FOLD_TOL, LINEAR_GN_TOL, LN_BWD_PARAM_TOL, LN_BWD_TOL, ROW_OP_TOL,
                                 TOKEN_WGRAD_TOL)

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
class Op:
    """One operand.  Input: `t` = its contents.  Output: `t` = what the body holds before the launch (NaN unless the kernel accumulates).
    `stride`: row stride in elements (> last dimension) -> guarded_rows.  `sample_dim`: the dimension P3 walks (None: shared by all
    samples -- weights, bias)."""

    def __init__(self, t, guard=MIN_GUARD_BYTES, stride=None, sample_dim=None, whole=True):
        self.t, self.guard, self.stride, self.sample_dim, self.whole = t, guard, stride, sample_dim, whole      # whole: every body element is written


def out_op(shape, dtype, **kw):
    return Op(torch.full(shape, float("nan"), dtype=dtype), **kw)


class Case:
    def __init__(self, ins, outs, launch, check, nsamples=None, environ=None):
        self.ins, self.outs, self.launch, self.check, self.nsamples, self.environ = ins, outs, launch, check, nsamples, environ or {}


def _bits(t):
    t = t.contiguous()
    return t.view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)


class Placed:
    def __init__(self, case, dev, monkeypatch):
        self.case, self.T, self.H = case, {}, {}
        for k, v in case.environ.items():
            monkeypatch.setenv(k, v)
        for name, op in list(case.ins.items()) + list(case.outs.items()):
            if op.stride:
                self.T[name], self.H[name] = guarded_rows(op.t, op.stride, op.guard, dev, name)
            else:
                self.T[name], self.H[name] = guarded(op.t, op.guard, dev, name)

    def run(self):
        for name, op in self.case.outs.items():
            self.T[name].copy_(op.t)
            self.H[name].canary()
        self.case.launch(self.T)
        torch.cuda.synchronize()
        return {name: self.T[name].clone() for name in self.case.outs}

    def surround_inputs(self, how):
        for name in self.case.ins:
            getattr(self.H[name], how)()


def p1_poisoned_surroundings(case, dev, monkeypatch):
    p = Placed(case, dev, monkeypatch)
    p.surround_inputs("clear")
    clean = p.run()
    p.surround_inputs("poison")
    poisoned = p.run()
    for name in case.outs:
        changed = int((_bits(clean[name]) != _bits(poisoned[name])).sum())
        nans = int(torch.isnan(poisoned[name].float()).sum())
        assert changed == 0, f"{name}: {changed} bytes differ once the inputs' surroundings are NaN ({nans} output elements are NaN)"
    case.check({k: v.cpu() for k, v in clean.items()})


def p2_canaried_outputs(case, dev, monkeypatch):
    p = Placed(case, dev, monkeypatch)
    got = p.run()
    for name in case.outs:
        assert p.H[name].intact()
        bad = int((~torch.isfinite(got[name].float())).sum()) if case.outs[name].whole else 0
        assert bad == 0, f"{name}: {bad} of {got[name].numel()} elements were not written (or are not finite)"


def p3_sample_isolation(case, dev, monkeypatch):
    assert case.nsamples
    p = Placed(case, dev, monkeypatch)
    base = p.run()
    n = case.nsamples
    for i in (range(n) if n <= 5 else sorted({0, n // 2, n - 1})):      # small batches: every sample (both partners of a stacked pair)
        saved = {}
        for name, op in case.ins.items():
            if op.sample_dim is not None and op.t.dtype.is_floating_point:
                sl = p.T[name].select(op.sample_dim, i)
                saved[name] = sl.clone()
                sl.fill_(float("nan"))
        assert saved
        got = p.run()
        for name, t in saved.items():
            p.T[name].select(case.ins[name].sample_dim, i).copy_(t)
        others = torch.tensor([j for j in range(n) if j != i], device=dev, dtype=torch.long)
        for name, op in case.outs.items():
            if op.sample_dim is None or not others.numel():
                continue
            a, b = base[name].movedim(op.sample_dim, 0).index_select(0, others), got[name].movedim(op.sample_dim, 0).index_select(0, others)
            changed = (_bits(a) != _bits(b)).reshape(others.numel(), -1)
            hit = [int(others[j]) for j in changed.any(1).nonzero().flatten()[:8]]
            assert not hit, f"{name}: NaN in sample / row {i} of the inputs changed {int(changed.sum())} bytes of OTHER samples' output (first: {hit})"


# ---- pd_attn_d64 -----------------------------------------------------------------------------------------------------------------------
# (B, heads, Nq, Nkv), layout, lse.  Cross layout: q [B][Nq][C], kv fused [B][Nkv][2C]; self layout: one fused [B][N][3C], N % 64 != 0.
# qb2: Nkv % 64 == 0, Nkv >= 512 and (Nq / 256) * heads * B >= 1024 select the 64-queries-per-wave kernel in the 16-bit engines.
ATTN_D64_CASES = {
    "cross-B3-h3-200x77-lse": ((3, 3, 200, 77), "cross", True),
    "cross-B1-h5-130x4": ((1, 5, 130, 4), "cross", False),
    "cross-B3-h1-130x200-lse": ((3, 1, 130, 200), "cross", True),
    "cross-B1-h3-1100x1000": ((1, 3, 1100, 1000), "cross", False),
    "cross-B3-h5-200x77": ((3, 5, 200, 77), "cross", False),
    "cross-B3-h1-1100x4-lse": ((3, 1, 1100, 4), "cross", True),
    "self-B3-h3-200-lse": ((3, 3, 200, 200), "self", True),
    "self-B1-h5-130": ((1, 5, 130, 130), "self", False),
    "self-B3-h1-1100": ((3, 1, 1100, 1100), "self", False),
    "qb2-cross-B16-h16-1100x1024-lse": ((16, 16, 1100, 1024), "cross", True),
    # out written into a wider row (out_stride = C + 64): the gap columns are canary
    "cross-B3-h3-200x77-lse-outstrided": ((3, 3, 200, 77), "cross", True, 64),
    "self-B3-h3-200-outstrided": ((3, 3, 200, 200), "self", False, 64),
}


def attn_d64_case(env_, mode, key):
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    (B, heads, Nq, Nkv), layout, with_lse = ATTN_D64_CASES[key][:3]
    Cc = heads * 64
    opad = ATTN_D64_CASES[key][3] if len(ATTN_D64_CASES[key]) > 3 else 0
    g = torch.Generator().manual_seed(141)
    if layout == "self":
        qkv = bf16_round(torch.randn(B, Nq, 3 * Cc, generator=g), mode)
        q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        ins = {"qkv": Op(qkv.to(tdt), guard_size(64, 3 * Cc, tdt), sample_dim=0)}
    else:
        q = bf16_round(torch.randn(B, Nq, Cc, generator=g), mode)
        kv = bf16_round(torch.randn(B, Nkv, 2 * Cc, generator=g), mode)
        k, v = kv[..., :Cc], kv[..., Cc:]
        ins = {"q": Op(q.to(tdt), guard_size(64, Cc, tdt), sample_dim=0), "kv": Op(kv.to(tdt), guard_size(64, 2 * Cc, tdt), sample_dim=0)}
    outs = {"out": out_op((B, Nq, Cc), tdt, guard=guard_size(64, Cc + opad, tdt), stride=Cc + opad if opad else None, sample_dim=0)}
    if with_lse:
        outs["lse"] = out_op((B, heads, Nq), torch.float32, sample_dim=0)

    def launch(T):
        esz = T["out"].element_size()
        if layout == "self":
            p = T["qkv"].data_ptr()
            qp, kp, vp, qs, kvs = p, p + Cc * esz, p + 2 * Cc * esz, 3 * Cc, 3 * Cc
        else:
            qp, kp, vp, qs, kvs = T["q"].data_ptr(), T["kv"].data_ptr(), T["kv"].data_ptr() + Cc * esz, Cc, 2 * Cc
        a = L.AttnD64Args(dtype=code, B=B, heads=heads, Nq=Nq, Nkv=Nkv, q=qp, q_stride=qs, k=kp, v=vp, kv_stride=kvs,
                          out=T["out"].data_ptr(), out_stride=Cc + opad, lse=T["lse"].data_ptr() if with_lse else None)
        L.check(lib.pd_attn_d64(C.byref(a), stream()), "pd_attn_d64")

    def check(O):
        sp = lambda t, n: t.reshape(B, n, heads, 64).transpose(1, 2)
        ref = F.scaled_dot_product_attention(sp(q, Nq), sp(k, Nkv), sp(v, Nkv)).transpose(1, 2).reshape(B, Nq, Cc)
        assert rel(O["out"].float(), ref) < ATTN_D64_TOL[mode]
        if with_lse and mode in ATTN_D64_LSE_TOL and B * heads * Nq * Nkv < 1 << 26:
            s = torch.einsum("bhid,bhjd->bhij", sp(q, Nq), sp(k, Nkv)) / 8
            assert rel(O["lse"], torch.logsumexp(s, -1) * LOG2E) < ATTN_D64_LSE_TOL[mode]

    return Case(ins, outs, launch, check, nsamples=B)


# ---- pd_attn_d64_bwd -------------------------------------------------------------------------------------------------------------------
ATTN_D64_BWD_CASES = {"B2-h3-200x77": (2, 3, 200, 77), "B2-h2-130x4": (2, 2, 130, 4), "B1-h2-70x200": (1, 2, 70, 200),
                      "B3-h3-200x77": (3, 3, 200, 77), "B3-h2-130x4": (3, 2, 130, 4), "B3-h2-70x200": (3, 2, 70, 200),
                      "B3-h3-200x77-dq-dkv-strided": (3, 3, 200, 77, 64)}      # dq_stride = C + 64, dkv_stride = 2C + 64: gap columns canaried


def attn_d64_bwd_case(env_, mode, key):
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    B, heads, Nq, Nkv = ATTN_D64_BWD_CASES[key][:4]
    Cc = heads * 64
    gpad = ATTN_D64_BWD_CASES[key][4] if len(ATTN_D64_BWD_CASES[key]) > 4 else 0
    g = torch.Generator().manual_seed(151)
    q = bf16_round(torch.randn(B, Nq, Cc, generator=g), mode).requires_grad_()
    kv = bf16_round(torch.randn(B, Nkv, 2 * Cc, generator=g), mode).requires_grad_()
    do = bf16_round(torch.randn(B, Nq, Cc, generator=g), mode)
    # o and lse as the forward kernel leaves them (plain allocations: the forward has its own cases above)
    Q, KV = q.detach().to(tdt).to(dev), kv.detach().to(tdt).to(dev)
    o = torch.empty((B, Nq, Cc), dtype=tdt, device=dev)
    lse = torch.empty((B, heads, Nq), dtype=torch.float32, device=dev)
    esz = Q.element_size()
    a = L.AttnD64Args(dtype=code, B=B, heads=heads, Nq=Nq, Nkv=Nkv, q=Q.data_ptr(), q_stride=Cc, k=KV.data_ptr(), v=KV.data_ptr() + Cc * esz,
                      kv_stride=2 * Cc, out=o.data_ptr(), out_stride=Cc, lse=lse.data_ptr())
    L.check(lib.pd_attn_d64(C.byref(a), stream()), "pd_attn_d64")
    torch.cuda.synchronize()
    gq, gkv = guard_size(64, Cc, tdt), guard_size(64, 2 * Cc, tdt)
    ins = {"q": Op(Q, gq, sample_dim=0), "kv": Op(KV, gkv, sample_dim=0), "dout": Op(do.to(tdt), gq, sample_dim=0), "o": Op(o, gq, sample_dim=0),
           "lse": Op(lse, sample_dim=0)}
    outs = {"delta": out_op((B, heads, Nq), torch.float32, sample_dim=0), "dq": out_op((B, Nq, Cc), tdt, guard=guard_size(64, Cc + gpad, tdt), stride=Cc + gpad if gpad else None, sample_dim=0),
            "dkv": out_op((B, Nkv, 2 * Cc), tdt, guard=guard_size(64, 2 * Cc + gpad, tdt), stride=2 * Cc + gpad if gpad else None, sample_dim=0)}        # dk and dv interleave: [B][Nkv][dk C | dv C]

    def launch(T):
        b = L.AttnD64BwdArgs(dtype=code, B=B, heads=heads, Nq=Nq, Nkv=Nkv, q=T["q"].data_ptr(), q_stride=Cc, k=T["kv"].data_ptr(),
                             v=T["kv"].data_ptr() + Cc * esz, kv_stride=2 * Cc, o=T["o"].data_ptr(), dout=T["dout"].data_ptr(), o_stride=Cc,
                             lse=T["lse"].data_ptr(), delta=T["delta"].data_ptr(), dq=T["dq"].data_ptr(), dq_stride=Cc + gpad, dk=T["dkv"].data_ptr(),
                             dv=T["dkv"].data_ptr() + Cc * esz, dkv_stride=2 * Cc + gpad)
        L.check(lib.pd_attn_d64_bwd(C.byref(b), stream()), "pd_attn_d64_bwd")

    def check(O):
        sp = lambda t, n: t.reshape(B, n, heads, 64).transpose(1, 2)
        ref = F.scaled_dot_product_attention(sp(q, Nq), sp(kv[..., :Cc], Nkv), sp(kv[..., Cc:], Nkv)).transpose(1, 2).reshape(B, Nq, Cc)
        ref.backward(do)
        tol = ATTN_D64_BWD_TOL[mode]
        assert rel(O["dq"].float(), q.grad) < tol
        assert rel(O["dkv"].float()[..., :Cc], kv.grad[..., :Cc]) < tol
        assert rel(O["dkv"].float()[..., Cc:], kv.grad[..., Cc:]) < tol

    return Case(ins, outs, launch, check, nsamples=B)


# ---- pd_attn_d8 (index clamps today; covered so that a later switch to buffer loads is) ------------------------------------------------------
# (B, heads, N), kmax2: the producer's key bound selects the DMA-staged kernel in the 16-bit engines (refused in f32: not a case there)
ATTN_D8_CASES = {"B3-h2-16": ((3, 2, 16), False), "B3-h8-200": ((3, 8, 200), False), "B4-h32-2100": ((4, 32, 2100), False),      # (8-wave workgroups in bf16)
                 "B4-h32-2100-dma-kmax2": ((4, 32, 2100), True)}


def attn_d8_case(env_, mode, key):
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    (B, heads, N), with_kmax2 = ATTN_D8_CASES[key]
    g = torch.Generator().manual_seed(107)
    q, k, v = (bf16_round(torch.randn(B, heads, N, 8, generator=g) * 1.5, mode) for _ in range(3))
    ins = {n: Op(t.to(tdt), sample_dim=0) for n, t in (("q", q), ("k", k), ("v", v))}
    if with_kmax2:
        ins["kmax2"] = Op((k.to(tdt).float() ** 2).sum(-1).amax(-1).contiguous(), sample_dim=None)      # (a finite bound stays: NaN there is a caller's bug)
    outs = {"out": out_op((B, N, heads * 8), tdt, sample_dim=0), "lse": out_op((B, heads, N), torch.float32, sample_dim=0)}

    def launch(T):
        a = L.AttnArgs(dtype=code, B=B, heads=heads, N=N, q=T["q"].data_ptr(), k=T["k"].data_ptr(), v=T["v"].data_ptr(), out=T["out"].data_ptr(),
                       lse=T["lse"].data_ptr(), kmax2=T["kmax2"].data_ptr() if with_kmax2 else None)
        L.check(lib.pd_attn_d8(C.byref(a), stream()), "pd_attn_d8")

    def check(O):
        ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, heads * 8)
        assert rel(O["out"].float(), ref) < ATTN_D8_TOL[mode]

    return Case(ins, outs, launch, check, nsamples=B)


# ---- pd_linear -------------------------------------------------------------------------------------------------------------------------
# (M, K, N, residual, xpad), environment.  plain: linear_kernel (M below the DMA threshold); dma: linear_dma_kernel in the 16-bit engines
# (M >= 32768, see test_linear_gemm); p8: PD_LIN_P8=1 forces the eight-phase kernel wherever it is eligible (16-bit engines).
LINEAR_CASES = {
    "plain-231x96x256-strided": ((77 * 3, 96, 256, 0, 32), {}),
    "plain-300x64x64-res": ((300, 64, 64, 1, 0), {}),
    "plain-515x1280x320-res-strided": ((515, 1280, 320, 1, 64), {}),
    "plain-40x32x8-below-a-tile-strided": ((40, 32, 8, 0, 8), {}),
    "dma-33000x192x384-res-strided": ((33000, 192, 384, 1, 64), {"16bit": "1"}),      # linear_dma_kernel is a 16-bit form: not run in f32
    "dma3-515x192x384-res-strided": ((515, 192, 384, 1, 64), {"PD_LIN_DMA": "3"}),      # PD_LIN_DMA=3 / 4: that variant at any token count
    "dma4-300x128x1024": ((300, 128, 1024, 0, 0), {"PD_LIN_DMA": "4"}),
    "p8-300x128x256-res": ((300, 128, 256, 1, 0), {"PD_LIN_P8": "1"}),
    "p8-515x640x1920-strided": ((515, 640, 1920, 0, 64), {"PD_LIN_P8": "1"}),
    "p8-231x320x320-res-strided": ((231, 320, 320, 1, 64), {"PD_LIN_P8": "1"}),
}


def linear_case(env_, mode, key):
    from phendiff_amd.packing import pack_conv_weight
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    (M, K, N, with_res, xpad), environ = LINEAR_CASES[key]
    environ = {k: v for k, v in environ.items() if k.startswith("PD_")}
    g = torch.Generator().manual_seed(161)
    x = bf16_round(torch.randn(M, K, generator=g), mode)
    w = bf16_round(torch.randn(N, K, generator=g) / K ** 0.5, mode)
    bias = torch.randn(N, generator=g)
    res = bf16_round(torch.randn(M, N, generator=g), mode) if with_res else None
    npad = ((N + 31) // 32) * 32
    bp = torch.zeros(npad)
    bp[:N] = bias
    xs = K + xpad
    ins = {"x": Op(x.to(tdt), guard_size(256, xs, tdt), stride=xs if xpad else None, sample_dim=0),
           "w_packed": Op(pack_conv_weight(w[:, :, None, None], tdt, npad)), "bias": Op(bp)}
    if with_res:
        ins["residual"] = Op(res.to(tdt), guard_size(256, N, tdt), sample_dim=0)
    outs = {"y": out_op((M, N), tdt, guard=guard_size(256, N, tdt), sample_dim=0)}

    def launch(T):
        a = L.LinearArgs(dtype=code, M=M, K=K, N=N, N_pad=npad, x=T["x"].data_ptr(), x_stride=xs, w_packed=T["w_packed"].data_ptr(),
                         bias=T["bias"].data_ptr(), residual=T["residual"].data_ptr() if with_res else None, y=T["y"].data_ptr())
        L.check(lib.pd_linear(C.byref(a), stream()), "pd_linear")

    def check(O):
        ref = F.linear(x, w, bias) + (res if with_res else 0)
        assert rel(O["y"].float(), ref) < ROW_OP_TOL[mode]

    return Case(ins, outs, launch, check, nsamples=M, environ=environ)


LINEAR_GEGLU_CASES = {"plain-300x64x256": ((300, 64, 256), {}), "plain-130x96x32": ((130, 96, 32), {}), "plain-515x320x1280": ((515, 320, 1280), {}),
                      "p8-300x64x256": ((300, 64, 256), {"PD_LIN_P8": "1"}), "p8-515x320x1280": ((515, 320, 1280), {"PD_LIN_P8": "1"})}


def linear_geglu_case(env_, mode, key):
    """pd_linear(glu = 1): weights packed as in test_linear_gemm_fused_geglu (value / gate tiles interleaved)."""
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    (M, K, inner), environ = LINEAR_GEGLU_CASES[key]
    g = torch.Generator().manual_seed(164)
    x = bf16_round(torch.randn(M, K, generator=g), mode)
    w = bf16_round(torch.randn(2 * inner, K, generator=g) / K ** 0.5, mode)
    bias = torch.randn(2 * inner, generator=g)
    W = w.to(dev)
    tile = (K // 32) * 2 * 512
    wp = torch.full((2 * inner // 32, tile), float("nan"), dtype=tdt, device=dev)
    for half in (0, 1):
        src = W[half * inner:(half + 1) * inner].contiguous()
        a = L.PackWeightArgs(dtype=code, cout=inner, cin=K, cout_pad=inner, cin_pad=K, ksize=1, src_in=K, dgrad=0,
                             src=src.data_ptr(), dst=wp.data_ptr() + half * tile * wp.element_size(), dst_ct_stride=2 * tile)
        L.check(lib.pd_pack_weight(C.byref(a), stream()), "pd_pack_weight")
    torch.cuda.synchronize()
    ins = {"x": Op(x.to(tdt), guard_size(256, K, tdt), sample_dim=0), "w_packed": Op(wp), "bias": Op(bias)}
    outs = {"y": out_op((M, inner), tdt, guard=guard_size(256, inner, tdt), sample_dim=0)}

    def launch(T):
        a = L.LinearArgs(dtype=code, M=M, K=K, N=2 * inner, N_pad=2 * inner, x=T["x"].data_ptr(), x_stride=K, w_packed=T["w_packed"].data_ptr(),
                         bias=T["bias"].data_ptr(), residual=None, y=T["y"].data_ptr(), glu=1)
        L.check(lib.pd_linear(C.byref(a), stream()), "pd_linear")

    def check(O):
        proj = F.linear(x.double(), w.double(), bias.double())
        assert rel(O["y"].float(), proj[:, :inner] * F.gelu(proj[:, inner:])) < ROW_OP_TOL[mode]

    return Case(ins, outs, launch, check, nsamples=M, environ=environ)


# ---- pd_token_wgrad (sums over rows: no P3) ----------------------------------------------------------------------------------------------
TOKEN_WGRAD_CASES = {"231x96x256-strided": (77 * 3, 96, 256, 32), "8200x640x200-strided": (8200, 640, 200, 24), "300x64x64": (300, 64, 64, 0),
                     "dma-2080x96x352-strided": (2048 + 32, 96, 352, 32)}


def token_wgrad_case(env_, mode, key, accumulate):
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    M, K, N, pad = TOKEN_WGRAD_CASES[key]
    g = torch.Generator().manual_seed(162)
    x = bf16_round(torch.randn(M, K, generator=g), mode)
    dy = bf16_round(torch.randn(M, N, generator=g), mode)
    prev = torch.randn(N, K, generator=g)
    a0 = L.TokenWgradArgs(dtype=code, M=M, K=K, N=N, x_stride=K + pad, dy_stride=N + pad, accumulate=accumulate)
    need = int(lib.pd_token_wgrad_workspace(C.byref(a0)))
    ins = {"x": Op(x.to(tdt), guard_size(256, K + pad, tdt), stride=K + pad if pad else None),
           "dy": Op(dy.to(tdt), guard_size(256, N + pad, tdt), stride=N + pad if pad else None)}
    outs = {"dw": Op(prev.clone() if accumulate else torch.full((N, K), float("nan"))),
            "slab": out_op((need // 4,), torch.float32, whole=False)}      # (the workspace is an upper bound: canaried, not necessarily filled)

    def launch(T):
        a = L.TokenWgradArgs(dtype=code, M=M, K=K, N=N, x=T["x"].data_ptr(), x_stride=K + pad, dy=T["dy"].data_ptr(), dy_stride=N + pad,
                             dw=T["dw"].data_ptr(), accumulate=accumulate, slab=T["slab"].data_ptr(), slab_bytes=need)
        L.check(lib.pd_token_wgrad(C.byref(a), stream()), "pd_token_wgrad")

    def check(O):
        ref = dy.double().t() @ x.double()
        got = O["dw"].double() - (prev.double() if accumulate else 0)
        assert rel(got.float(), ref.float()) < TOKEN_WGRAD_TOL[mode]

    return Case(ins, outs, launch, check)


# ---- pd_layernorm, pd_geglu --------------------------------------------------------------------------------------------------------------
def layernorm_case(env_, mode, key):
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    rows, Cc = {"37x64": (37, 64), "301x640": (301, 640), "5x2048": (5, 2048)}[key]
    g = torch.Generator().manual_seed(142)
    x = bf16_round(torch.randn(rows, Cc, generator=g) * 2 + 0.5, mode)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    ins = {"x": Op(x.to(tdt), sample_dim=0), "gamma": Op(gamma), "beta": Op(beta)}
    outs = {"y": out_op((rows, Cc), tdt, sample_dim=0)}

    def launch(T):
        a = L.LayerNormArgs(dtype=code, rows=rows, C=Cc, eps=1e-5, x=T["x"].data_ptr(), gamma=T["gamma"].data_ptr(), beta=T["beta"].data_ptr(),
                            y=T["y"].data_ptr())
        L.check(lib.pd_layernorm(C.byref(a), stream()), "pd_layernorm")

    def check(O):
        assert rel(O["y"].float(), F.layer_norm(x, (Cc,), gamma, beta, 1e-5)) < ROW_OP_TOL[mode]

    return Case(ins, outs, launch, check, nsamples=rows)


def geglu_case(env_, mode, key):
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    rows, inner = {"301x256": (301, 256), "7x1288": (7, 1288)}[key]
    g = torch.Generator().manual_seed(143)
    x = bf16_round(torch.randn(rows, 2 * inner, generator=g) * 2, mode)
    ins = {"x": Op(x.to(tdt), sample_dim=0)}
    outs = {"y": out_op((rows, inner), tdt, sample_dim=0)}

    def launch(T):
        a = L.GegluArgs(dtype=code, rows=rows, inner=inner, x=T["x"].data_ptr(), y=T["y"].data_ptr())
        L.check(lib.pd_geglu(C.byref(a), stream()), "pd_geglu")

    def check(O):
        h, gate = x.chunk(2, -1)
        assert rel(O["y"].float(), h * F.gelu(gate)) < ROW_OP_TOL[mode]

    return Case(ins, outs, launch, check, nsamples=rows)


# ---- pd_conv ---------------------------------------------------------------------------------------------------------------------------
# B, C0, C1, Cout, H, W + options.  gn: GroupNorm-affine + SiLU prologue; temb: a column slice of a wider row (stride 200, gap columns
# guarded); res: residual; stats: per-tile GroupNorm statistics of the output; stack: PD_CONV_STACK=1, two 8 x 8 images per tile.
# Guard: 2 x 64 output pixels' worth of input rows is far below 64 KiB at these widths -> two whole image rows of 2 x W x C, >= 64 KiB.
CONV_CASES = {
    "3x3-5x7": dict(B=2, c0=128, cout=64, h=5, w=7),
    "3x3-9x33": dict(B=3, c0=32, cout=64, h=9, w=33),
    "3x3-20x17-stats": dict(B=3, c0=32, cout=96, h=20, w=17, stats=True),
    "3x3-40x72": dict(B=1, c0=64, cout=128, h=40, w=72),
    "stride2-pad1-9x33": dict(B=3, c0=64, cout=64, h=9, w=33, stride=2, pad=1),
    "stride2-pad0-9x33": dict(B=3, c0=64, cout=64, h=9, w=33, stride=2, pad=0),
    "upsample-5x7": dict(B=3, c0=64, cout=64, h=5, w=7, upsample=1),
    "concat-gn-temb-res-20x17-stats": dict(B=3, c0=64, c1=32, cout=64, h=20, w=17, gn=True, temb=True, res=True, stats=True),
    "1x1-res-9x33": dict(B=3, c0=64, cout=96, h=9, w=33, ksize=1, pad=0, res=True),
    "nchw-f32-cout3-pad32-9x33": dict(B=3, c0=64, cout=3, h=9, w=33, out_mode=1, cout_pad=32),
    "qkv-head-major-16x16": dict(B=3, c0=64, cout=192, h=16, w=16, ksize=1, pad=0, out_mode=2, heads=8),
    "stack-8x8-B5-concat-temb-res-stats": dict(B=5, c0=64, c1=32, cout=96, h=8, w=8, temb=True, res=True, stats=True, environ={"PD_CONV_STACK": "1"}),
    "stack-8x8-B3-stats": dict(B=3, c0=64, cout=64, h=8, w=8, stats=True, environ={"PD_CONV_STACK": "1"}),
}


def conv_case(env_, mode, key):
    from test_gpu_kernels import TOL, nhwc
    L, lib, pack, dev = env_
    code, tdt = DT[mode]
    o = dict(c1=0, ksize=3, stride=1, pad=1, upsample=0, gn=False, temb=False, res=False, stats=False, out_mode=0, heads=0, cout_pad=None, temb_stride=200, environ={})
    o.update(CONV_CASES[key])
    B, c0, c1, cout, h, w_, ks, stride, pad, up = (o[k] for k in ("B", "c0", "c1", "cout", "h", "w", "ksize", "stride", "pad", "upsample"))
    cp = o["cout_pad"] or cout
    g = torch.Generator().manual_seed(171)
    x0 = torch.randn(B, c0, h, w_, generator=g)
    x1 = torch.randn(B, c1, h, w_, generator=g) if c1 else None
    w = torch.randn(cout, c0 + c1, ks, ks, generator=g) / ((c0 + c1) * ks * ks) ** 0.5
    b = torch.randn(cout, generator=g)
    scale, shift = torch.rand(B, c0 + c1, generator=g) + 0.5, torch.randn(B, c0 + c1, generator=g)
    temb = torch.randn(B, cout, generator=g)
    hc, wc = (2 * h, 2 * w_) if up else (h, w_)
    extra = 1 if (ks == 3 and pad == 0) else 0
    ho, wo = (hc + 2 * pad + extra - ks) // stride + 1, (wc + 2 * pad + extra - ks) // stride + 1
    res = torch.randn(B, cout, ho, wo, generator=g)
    bias = torch.zeros(cp)
    bias[:cout] = b
    gin = lambda c: guard_size(2 * w_, c, tdt)
    ins = {"x0": Op(nhwc(x0, tdt), gin(c0), sample_dim=0), "w_packed": Op(pack(w.float(), tdt, cp)), "bias": Op(bias)}
    if c1:
        ins["x1"] = Op(nhwc(x1, tdt), gin(c1), sample_dim=0)
    if o["gn"]:
        ins["scale"], ins["shift"] = Op(scale, sample_dim=0), Op(shift, sample_dim=0)
    if o["temb"]:
        ins["temb"] = Op(temb, stride=o["temb_stride"], sample_dim=0)
    if o["res"]:
        ins["residual"] = Op(nhwc(res, tdt), guard_size(2 * wo, cout, tdt), sample_dim=0)
    if o["out_mode"] == 0:
        outs = {"y": out_op((B, ho, wo, cout), tdt, guard=guard_size(2 * wo, cout, tdt), sample_dim=0)}
    elif o["out_mode"] == 1:
        outs = {"y": out_op((B, cout, ho, wo), torch.float32, sample_dim=0)}          # Cout_pad - Cout padded channels: written nowhere
    else:
        outs = {"y": out_op((3, B, o["heads"], ho * wo, 8), tdt, sample_dim=1)}
    T_ = lib.pd_conv_stat_tiles(ho, wo, ks, stride)
    if o["stats"]:
        outs["stats"] = out_op((B, T_, cout, 2), torch.float32, sample_dim=0)

    def launch(T):
        a = L.ConvArgs(dtype=code, B=B, Hin=h, Win=w_, Hout=ho, Wout=wo, C0=c0, C1=c1, Cout=cout, Cout_pad=cp, ksize=ks, stride=stride, pad=pad,
                       upsample=up, silu=int(o["gn"]), out_mode=o["out_mode"], heads=o["heads"], x0=T["x0"].data_ptr(), x1=L.ptr(T.get("x1")),
                       scale=L.ptr(T.get("scale")), shift=L.ptr(T.get("shift")), w_packed=T["w_packed"].data_ptr(), bias=T["bias"].data_ptr(),
                       temb=L.ptr(T.get("temb")), temb_stride=o["temb_stride"] if o["temb"] else 0, residual=L.ptr(T.get("residual")), y=T["y"].data_ptr(),
                       stats_out=L.ptr(T.get("stats")), im2col3=0)
        L.check(lib.pd_conv(C.byref(a), stream()), "pd_conv")

    def check(O):
        xin = torch.cat([bf16_round(x0, mode)] + ([bf16_round(x1, mode)] if c1 else []), 1)
        if o["gn"]:
            xin = bf16_round(F.silu(xin * scale[:, :, None, None] + shift[:, :, None, None]), mode)
        if up:
            xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
        if extra:
            xin = F.pad(xin, (0, 1, 0, 1))
        ref = F.conv2d(xin, bf16_round(w, mode), b, stride=stride, padding=pad)
        if o["temb"]:
            ref = ref + temb[:, :, None, None]
        if o["res"]:
            ref = ref + bf16_round(res, mode)
        y = O["y"].float()
        if o["out_mode"] == 0:
            y = y.permute(0, 3, 1, 2)
        elif o["out_mode"] == 2:
            ref = ref.view(B, 3, o["heads"], 8, ho * wo).permute(1, 0, 2, 4, 3)
        assert rel(y, ref) < TOL[mode]

    return Case(ins, outs, launch, check, nsamples=B, environ=o["environ"])


# ---- pd_linear behind a GroupNorm prologue: head-major output, kmax2_out, the folded per-sample-weight route ---------------------------------
# staged: x * scale[n] + shift[n] applied while staging (all engines); kmax2: + the key bound (16-bit engines); folded: a fold_ws workspace
# makes pd_linear fold the affine into per-sample weights and run the DMA-staged GEMM (16-bit engines).  Output [3][B][heads][tokens][8].
LINEAR_GN_CASES = {"staged-headmajor": ("staged", False), "staged-headmajor-kmax2": ("staged", True), "folded-headmajor-kmax2": ("folded", True)}


def linear_gn_case(env_, mode, key):
    from phendiff_amd.packing import pack_conv_weight
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    route, with_kmax2 = LINEAR_GN_CASES[key]
    B, Ntok, Cc, heads = 3, 256, 128, 16
    g = torch.Generator().manual_seed(163)
    x = bf16_round(torch.randn(B, Ntok, Cc, generator=g) * 1.5 + 0.3, mode)
    scale, shift = torch.rand(B, Cc, generator=g) + 0.5, torch.randn(B, Cc, generator=g)
    w = bf16_round(torch.randn(3 * Cc, Cc, generator=g) / Cc ** 0.5, mode)
    bias = torch.randn(3 * Cc, generator=g)
    ins = {"x": Op(x.to(tdt), guard_size(256, Cc, tdt), sample_dim=0), "scale": Op(scale, sample_dim=0), "shift": Op(shift, sample_dim=0),
           "w_packed": Op(pack_conv_weight(w[:, :, None, None], tdt)), "bias": Op(bias)}
    outs = {"y": out_op((3, B, heads, Ntok, 8), tdt, guard=guard_size(256, 8, tdt), sample_dim=1)}
    if with_kmax2:
        outs["kmax2"] = Op(torch.zeros(B, heads), sample_dim=0)            # (the plans hand over a zeroed slot)
    a0 = L.LinearArgs(dtype=code, M=B * Ntok, K=Cc, N=3 * Cc, N_pad=3 * Cc, x_stride=Cc, rows_per_sample=Ntok, qkv_heads=heads)
    a0.scale = a0.shift = 1                                                 # (non-null: the workspace query only looks at the shape)
    need = int(lib.pd_linear_fold_workspace(C.byref(a0))) if route == "folded" else 0
    if route == "folded":
        assert need > 0
        outs["fold_ws"] = Op(torch.zeros(need, dtype=torch.uint8), whole=False)

    def launch(T):
        a = L.LinearArgs(dtype=code, M=B * Ntok, K=Cc, N=3 * Cc, N_pad=3 * Cc, x=T["x"].data_ptr(), x_stride=Cc, w_packed=T["w_packed"].data_ptr(),
                         bias=T["bias"].data_ptr(), residual=None, y=T["y"].data_ptr(), scale=T["scale"].data_ptr(), shift=T["shift"].data_ptr(),
                         rows_per_sample=Ntok, qkv_heads=heads, kmax2_out=L.ptr(T.get("kmax2")), fold_ws=L.ptr(T.get("fold_ws")), fold_ws_bytes=need)
        L.check(lib.pd_linear(C.byref(a), stream()), "pd_linear")

    def check(O):
        if route == "folded":
            ref, tol = F.linear(x * scale[:, None, :] + shift[:, None, :], w, bias), LINEAR_FOLD_TOL[mode]
        else:
            ref, tol = F.linear(bf16_round(x * scale[:, None, :] + shift[:, None, :], mode), w, bias), LINEAR_GN_TOL[mode]
        ref = ref.reshape(B, Ntok, 3, heads, 8).permute(2, 0, 3, 1, 4)
        assert rel(O["y"].float(), ref) < tol
        if with_kmax2:
            assert torch.allclose(O["kmax2"], (O["y"][1].float() ** 2).sum(-1).amax(-1), rtol=KMAX2_RTOL, atol=0)

    return Case(ins, outs, launch, check, nsamples=B)


# ---- pd_conv: fused 1x1 tail, sub-pixel phases, im2col3, two output tiles per workgroup -----------------------------------------------------
CONV_TAIL_CASES = {"tail1-gn-20x17": (3, 64, 96, 0, 64, 20, 17, False), "tail2-gn-20x17": (3, 64, 32, 32, 96, 20, 17, False),
                   "tail2-plain-9x33": (3, 32, 32, 32, 96, 9, 33, True)}


def conv_tail_case(env_, mode, key):
    from test_gpu_kernels import TOL, nhwc
    L, lib, pack, dev = env_
    code, tdt = DT[mode]
    B, cm, t0, t1, cout, h, w_, plain = CONV_TAIL_CASES[key]
    g = torch.Generator().manual_seed(113)
    hmid, xa = torch.randn(B, cm, h, w_, generator=g), torch.randn(B, t0, h, w_, generator=g)
    xb = torch.randn(B, t1, h, w_, generator=g) if t1 else None
    w2 = torch.randn(cout, cm, 3, 3, generator=g) / (cm * 9) ** 0.5
    ws = torch.randn(cout, t0 + t1, 1, 1, generator=g) / (t0 + t1) ** 0.5
    b2, bs = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
    scale, shift = torch.rand(B, cm, generator=g) + 0.5, torch.randn(B, cm, generator=g)
    p2, ps = pack(w2, tdt), pack(ws, tdt)
    ct = p2.shape[0]
    wp = torch.cat([p2.reshape(ct, -1, 64, 8), ps.reshape(ct, -1, 64, 8)], 1).contiguous()
    gin = lambda c: guard_size(2 * w_, c, tdt)
    ins = {"x0": Op(nhwc(hmid, tdt), gin(cm), sample_dim=0), "tail_x0": Op(nhwc(xa, tdt), gin(t0), sample_dim=0), "w_packed": Op(wp), "bias": Op(b2 + bs)}
    if t1:
        ins["tail_x1"] = Op(nhwc(xb, tdt), gin(t1), sample_dim=0)
    if not plain:
        ins["scale"], ins["shift"] = Op(scale, sample_dim=0), Op(shift, sample_dim=0)
    outs = {"y": out_op((B, h, w_, cout), tdt, guard=gin(cout), sample_dim=0)}

    def launch(T):
        a = L.ConvArgs(dtype=code, B=B, Hin=h, Win=w_, Hout=h, Wout=w_, C0=cm, C1=0, Cout=cout, Cout_pad=cout, ksize=3, stride=1, pad=1,
                       upsample=0, silu=0 if plain else 1, out_mode=0, heads=0, x0=T["x0"].data_ptr(), x1=None, scale=L.ptr(T.get("scale")),
                       shift=L.ptr(T.get("shift")), w_packed=T["w_packed"].data_ptr(), bias=T["bias"].data_ptr(), temb=None, temb_stride=0,
                       residual=None, y=T["y"].data_ptr(), stats_out=None, tail_x0=T["tail_x0"].data_ptr(), tail_x1=L.ptr(T.get("tail_x1")),
                       tail_C0=t0, tail_C1=t1, im2col3=0)
        L.check(lib.pd_conv(C.byref(a), stream()), "pd_conv")

    def check(O):
        hin = bf16_round(hmid, mode) if plain else bf16_round(F.silu(bf16_round(hmid, mode) * scale[:, :, None, None] + shift[:, :, None, None]), mode)
        xcat = torch.cat([bf16_round(xa, mode)] + ([bf16_round(xb, mode)] if t1 else []), 1)
        ref = F.conv2d(hin, bf16_round(w2, mode), b2, padding=1) + F.conv2d(xcat, bf16_round(ws, mode), bs)
        assert rel(O["y"].float().permute(0, 3, 1, 2), ref) < TOL[mode]

    return Case(ins, outs, launch, check, nsamples=B)


# sub-pixel phases of the upsampler: forward (four launches fill y and its statistic tiles) and phase_in = 1 (the input gradient: four
# launches ACCUMULATE into dx through residual = y = dx); bounds as test_upsample_conv_*_as_four_subpixel_phases state them


def conv_phase_case(env_, mode, key):
    from phendiff_amd.packing import dgrad_weight, upsample_phase_weights
    from test_gpu_kernels import PHASE_FWD_TOL, PHASE_IN_TOL, nhwc
    L, lib, pack, dev = env_
    code, tdt = DT[mode]
    B, cin, cout, h, w_ = {"fwd-9x33": (3, 32, 64, 9, 33), "fwd-20x17": (3, 32, 64, 20, 17), "phase_in-9x33": (3, 64, 32, 9, 33)}[key]
    inward = key.startswith("phase_in")
    g = torch.Generator().manual_seed(141)
    x = torch.randn(B, cin, h, w_, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=g)
    dy = bf16_round(torch.randn(B, cout, 2 * h, 2 * w_, generator=g), mode)
    prev = bf16_round(torch.randn(B, cin, h, w_, generator=g), mode)
    ks = upsample_phase_weights(w)
    if inward:
        ins = {"dy": Op(nhwc(dy, tdt), guard_size(4 * w_, cout, tdt), sample_dim=0), "bias": Op(torch.zeros(cin))}
        for ph, k in enumerate(ks):
            ins[f"w{ph}"] = Op(pack(dgrad_weight(k), tdt))
        outs = {"dx": Op(nhwc(prev, tdt), guard_size(2 * w_, cin, tdt), sample_dim=0)}
    else:
        T_ = lib.pd_conv_stat_tiles(h, w_, 2, 1)
        ins = {"x": Op(nhwc(x, tdt), guard_size(2 * w_, cin, tdt), sample_dim=0), "bias": Op(b)}
        for ph, k in enumerate(ks):
            ins[f"w{ph}"] = Op(pack(k, tdt))
        outs = {"y": out_op((B, 2 * h, 2 * w_, cout), tdt, guard=guard_size(4 * w_, cout, tdt), sample_dim=0),
                "stats": out_op((B, 4 * T_, cout, 2), torch.float32, sample_dim=0)}

    def launch(T):
        for ph in range(4):
            if inward:
                a = L.ConvArgs(dtype=code, B=B, Hin=h, Win=w_, Hout=h, Wout=w_, C0=cout, C1=0, Cout=cin, Cout_pad=cin, ksize=2, stride=1, pad=0,
                               upsample=0, silu=0, out_mode=0, heads=0, x0=T["dy"].data_ptr(), x1=None, scale=None, shift=None,
                               w_packed=T[f"w{ph}"].data_ptr(), bias=T["bias"].data_ptr(), temb=None, temb_stride=0, residual=T["dx"].data_ptr(),
                               y=T["dx"].data_ptr(), stats_out=None, im2col3=0, phase=1 + ph, phase_in=1)
            else:
                a = L.ConvArgs(dtype=code, B=B, Hin=h, Win=w_, Hout=h, Wout=w_, C0=cin, C1=0, Cout=cout, Cout_pad=cout, ksize=2, stride=1, pad=0,
                               upsample=0, silu=0, out_mode=0, heads=0, x0=T["x"].data_ptr(), x1=None, scale=None, shift=None,
                               w_packed=T[f"w{ph}"].data_ptr(), bias=T["bias"].data_ptr(), temb=None, temb_stride=0, residual=None,
                               y=T["y"].data_ptr(), stats_out=T["stats"].data_ptr(), im2col3=0, phase=1 + ph)
            L.check(lib.pd_conv(C.byref(a), stream()), "pd_conv")

    def check(O):
        if inward:
            xl = x.clone().requires_grad_(True)
            F.conv2d(F.interpolate(xl, scale_factor=2.0, mode="nearest"), w, None, padding=1).backward(dy)
            assert rel(O["dx"].float().permute(0, 3, 1, 2), prev + xl.grad) < PHASE_IN_TOL[mode]
        else:
            ref = F.conv2d(F.interpolate(bf16_round(x, mode), scale_factor=2.0, mode="nearest"), w, b, padding=1)
            assert rel(O["y"].float().permute(0, 3, 1, 2), ref) < PHASE_FWD_TOL[mode]

    return Case(ins, outs, launch, check, nsamples=B)


def conv_im2col3_case(env_, mode, key):
    """conv_in as pd_conv(im2col3 = 3): the NCHW fp32 sample is gathered while staging."""
    from test_gpu_kernels import TOL
    L, lib, pack, dev = env_
    code, tdt = DT[mode]
    B, h, w_ = {"9x33": (3, 9, 33), "24x40": (3, 24, 40)}[key]
    g = torch.Generator().manual_seed(112)
    x = torch.randn(B, 3, h, w_, generator=g)
    w = torch.randn(64, 3, 3, 3, generator=g) / 5
    b = torch.randn(64, generator=g)
    wv = torch.zeros(64, 32, 1, 1)
    wv[:, :27, 0, 0] = w.reshape(64, 27)
    ins = {"x": Op(x, sample_dim=0), "w_packed": Op(pack(wv, tdt)), "bias": Op(b)}
    outs = {"y": out_op((B, h, w_, 64), tdt, guard=guard_size(2 * w_, 64, tdt), sample_dim=0)}

    def launch(T):
        a = L.ConvArgs(dtype=code, B=B, Hin=h, Win=w_, Hout=h, Wout=w_, C0=32, C1=0, Cout=64, Cout_pad=64, ksize=1, stride=1, pad=0,
                       upsample=0, silu=0, out_mode=0, heads=0, x0=T["x"].data_ptr(), x1=None, scale=None, shift=None, w_packed=T["w_packed"].data_ptr(),
                       bias=T["bias"].data_ptr(), temb=None, temb_stride=0, residual=None, y=T["y"].data_ptr(), stats_out=None, im2col3=3)
        L.check(lib.pd_conv(C.byref(a), stream()), "pd_conv")

    def check(O):
        ref = F.conv2d(bf16_round(x, mode), bf16_round(w, mode), b, padding=1)
        assert rel(O["y"].float().permute(0, 3, 1, 2), ref) < TOL[mode]

    return Case(ins, outs, launch, check, nsamples=B)


# the NCO = 2 shape of test_conv3x3_two_output_tiles_per_workgroup, as it is (the rounds-of-workgroups estimate needs B = 16 to pick that kernel in
# the 16-bit engines; f32 runs the one-tile form): concat + GroupNorm prologue + temb slice + residual + statistics of both tiles
CONV_CASES["nco2-64x64-B16-concat-gn-temb-res-stats"] = dict(B=16, c0=96, c1=32, cout=256, h=64, w=64, gn=True, temb=True, temb_stride=300, res=True, stats=True)


# ---- pd_conv_wgrad (sums over samples: no P3) ------------------------------------------------------------------------------------------------
CONV_WGRAD_CASES = {"3x3-B2-192to32-20x12": (2, 192, 0, 32, 20, 12, 3, 0), "3x3-B3-128to64-8x8": (3, 128, 0, 64, 8, 8, 3, 0),
                    "3x3-concat-64+32to64-24x16-acc": (2, 64, 32, 64, 24, 16, 3, 1), "1x1-B2-128to384-8x8": (2, 128, 0, 384, 8, 8, 1, 0)}


def conv_wgrad_case(env_, mode, key):
    from test_gpu_backward import CONV_WGRAD_TOL
    from test_gpu_kernels import nhwc
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    B, c0, c1, cout, H, W, ks, acc = CONV_WGRAD_CASES[key]
    pad = 1 if ks == 3 else 0
    g = torch.Generator().manual_seed(121)
    x = bf16_round(torch.randn(B, c0 + c1, H, W, generator=g), mode)
    dy = bf16_round(torch.randn(B, cout, H, W, generator=g), mode)
    prev = torch.randn(cout, c0 + c1, ks, ks, generator=g)
    a0 = L.WgradArgs(dtype=code, B=B, Hin=H, Win=W, Hout=H, Wout=W, C0=c0, C1=c1, Cout=cout, ksize=ks, stride=1, pad=pad, accumulate=acc)
    need = int(lib.pd_conv_wgrad_workspace(C.byref(a0)))
    assert need > 0
    ins = {"x0": Op(nhwc(x[:, :c0], tdt), guard_size(2 * W, c0, tdt)), "dy": Op(nhwc(dy, tdt), guard_size(2 * W, cout, tdt))}
    if c1:
        ins["x1"] = Op(nhwc(x[:, c0:], tdt), guard_size(2 * W, c1, tdt))
    outs = {"dw": Op(prev.clone() if acc else torch.full((cout, c0 + c1, ks, ks), float("nan"))), "slab": out_op((need // 4,), torch.float32, whole=False)}

    def launch(T):
        a = L.WgradArgs(dtype=code, B=B, Hin=H, Win=W, Hout=H, Wout=W, C0=c0, C1=c1, Cout=cout, ksize=ks, stride=1, pad=pad, upsample=0, silu=0,
                        x0=T["x0"].data_ptr(), x1=L.ptr(T.get("x1")), scale=None, shift=None, dy=T["dy"].data_ptr(), dw=T["dw"].data_ptr(),
                        Cout_valid=0, Cin_valid=0, accumulate=acc, slab=T["slab"].data_ptr(), slab_bytes=need)
        L.check(lib.pd_conv_wgrad(C.byref(a), stream()), "pd_conv_wgrad")

    def check(O):
        w = torch.zeros(cout, c0 + c1, ks, ks, requires_grad=True)
        (ref,) = torch.autograd.grad(F.conv2d(x, w, None, padding=pad), w, dy)
        assert rel(O["dw"] - (prev if acc else 0), ref) < CONV_WGRAD_TOL[mode]

    return Case(ins, outs, launch, check)


# ---- pd_attn_d8_bwd ---------------------------------------------------------------------------------------------------------------------------
# (B, heads, N), one-pass form (a workspace for the per-key-block partial dQ: 16-bit engines, N >= 512)
ATTN_D8_BWD_CASES = {"B3-h2-16": ((3, 2, 16), False), "B3-h8-200": ((3, 8, 200), False), "B2-h4-2100": ((2, 4, 2100), False),
                     "B2-h4-2100-onepass-slab": ((2, 4, 2100), True)}


def attn_d8_bwd_case(env_, mode, key):
    from test_gpu_backward import ATTN_D8_BWD_TOL
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    (B, heads, N), onepass = ATTN_D8_BWD_CASES[key]
    Cc = heads * 8
    g = torch.Generator().manual_seed(131)
    q, k, v = (bf16_round(torch.randn(B, heads, N, 8, generator=g) * 1.2, mode).requires_grad_(True) for _ in range(3))
    dout = bf16_round(torch.randn(B, N, Cc, generator=g), mode)
    Q, K, V = (t.detach().to(tdt).to(dev).contiguous() for t in (q, k, v))
    o = torch.empty((B, N, Cc), dtype=tdt, device=dev)
    lse = torch.empty((B, heads, N), device=dev)
    a = L.AttnArgs(dtype=code, B=B, heads=heads, N=N, q=Q.data_ptr(), k=K.data_ptr(), v=V.data_ptr(), out=o.data_ptr(), lse=lse.data_ptr())
    L.check(lib.pd_attn_d8(C.byref(a), stream()), "pd_attn_d8")
    torch.cuda.synchronize()
    ins = {"q": Op(Q, sample_dim=0), "k": Op(K, sample_dim=0), "v": Op(V, sample_dim=0), "o": Op(o, sample_dim=0), "dout": Op(dout.to(tdt), sample_dim=0),
           "lse": Op(lse, sample_dim=0)}
    outs = {"delta": out_op((B, heads, N), torch.float32, sample_dim=0), "dqkv": out_op((B, N, 3 * Cc), tdt, sample_dim=0)}
    need = 0
    if onepass:
        b0 = L.AttnBwdArgs(dtype=code, B=B, heads=heads, N=N)
        need = int(lib.pd_attn_d8_bwd_workspace(C.byref(b0)))
        assert need > 0, "the one-pass form needs a 16-bit engine and N >= 512"
        outs["slab"] = out_op((need // 4,), torch.float32, whole=False)

    def launch(T):
        b = L.AttnBwdArgs(dtype=code, B=B, heads=heads, N=N, q=T["q"].data_ptr(), k=T["k"].data_ptr(), v=T["v"].data_ptr(), o=T["o"].data_ptr(),
                          dout=T["dout"].data_ptr(), lse=T["lse"].data_ptr(), delta=T["delta"].data_ptr(), dqkv=T["dqkv"].data_ptr(),
                          slab=L.ptr(T.get("slab")), slab_bytes=need)
        L.check(lib.pd_attn_d8_bwd(C.byref(b), stream()), "pd_attn_d8_bwd")

    def check(O):
        ref_o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, Cc)
        grads = torch.autograd.grad(ref_o, (q, k, v), dout)
        got = O["dqkv"].float().reshape(B, N, 3, heads, 8).permute(2, 0, 3, 1, 4)
        for i in range(3):
            assert rel(got[i], grads[i]) < ATTN_D8_BWD_TOL[mode], "qkv"[i]

    return Case(ins, outs, launch, check, nsamples=B)


# ---- pd_attn_wide (+ bwd): one fused [B][N][3C] operand, ragged N; out / dq / dk / dv rows wider than what is written ----------------------------
def attn_wide_case(env_, mode, key):
    from test_gpu_vae import ATTN_WIDE_BWD_TOL, ATTN_WIDE_TOL
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    B, heads, D, N = 3, 2, 128, 77
    Cc = heads * D
    bwd = key.startswith("bwd")
    g = torch.Generator().manual_seed(145)
    qkv = bf16_round(torch.randn(B, N, 3 * Cc, generator=g), mode)
    dout = bf16_round(torch.randn(B, N, Cc, generator=g), mode)
    gq = guard_size(64, 3 * Cc, tdt)
    sp = lambda t: t.reshape(B, N, heads, D).transpose(1, 2)
    if not bwd:
        ins = {"qkv": Op(qkv.to(tdt), gq, sample_dim=0)}
        outs = {"out": out_op((B, N, Cc), tdt, guard=guard_size(64, Cc + 64, tdt), stride=Cc + 64, sample_dim=0), "lse": out_op((B, heads, N), torch.float32, sample_dim=0)}

        def launch(T):
            p, esz = T["qkv"].data_ptr(), T["qkv"].element_size()
            a = L.AttnWideArgs(dtype=code, B=B, heads=heads, D=D, Nq=N, Nkv=N, scale=D ** -0.5, q=p, q_stride=3 * Cc, k=p + Cc * esz, v=p + 2 * Cc * esz,
                               kv_stride=3 * Cc, out=T["out"].data_ptr(), out_stride=Cc + 64, lse=T["lse"].data_ptr())
            L.check(lib.pd_attn_wide(C.byref(a), stream()), "pd_attn_wide")

        def check(O):
            ref = F.scaled_dot_product_attention(sp(qkv[..., :Cc]), sp(qkv[..., Cc:2 * Cc]), sp(qkv[..., 2 * Cc:])).transpose(1, 2).reshape(B, N, Cc)
            assert rel(O["out"].float(), ref) < ATTN_WIDE_TOL[mode]

        return Case(ins, outs, launch, check, nsamples=B)
    QKV = qkv.to(tdt).to(dev).contiguous()
    esz = QKV.element_size()
    o = torch.empty((B, N, Cc), dtype=tdt, device=dev)
    lse = torch.empty((B, heads, N), device=dev)
    p0 = QKV.data_ptr()
    a = L.AttnWideArgs(dtype=code, B=B, heads=heads, D=D, Nq=N, Nkv=N, scale=D ** -0.5, q=p0, q_stride=3 * Cc, k=p0 + Cc * esz, v=p0 + 2 * Cc * esz,
                       kv_stride=3 * Cc, out=o.data_ptr(), out_stride=Cc, lse=lse.data_ptr())
    L.check(lib.pd_attn_wide(C.byref(a), stream()), "pd_attn_wide")
    torch.cuda.synchronize()
    gs = 3 * Cc + 64                                     # dq | dk | dv interleaved per token, 64 gap columns behind them
    ins = {"qkv": Op(QKV, gq, sample_dim=0), "o": Op(o, guard_size(64, Cc, tdt), sample_dim=0), "dout": Op(dout.to(tdt), guard_size(64, Cc, tdt), sample_dim=0),
           "lse": Op(lse, sample_dim=0)}
    outs = {"delta": out_op((B, heads, N), torch.float32, sample_dim=0), "dqkv": out_op((B, N, 3 * Cc), tdt, guard=guard_size(64, gs, tdt), stride=gs, sample_dim=0)}

    def launch(T):
        p, dp = T["qkv"].data_ptr(), T["dqkv"].data_ptr()
        b = L.AttnWideBwdArgs(dtype=code, B=B, heads=heads, D=D, Nq=N, Nkv=N, scale=D ** -0.5, q=p, q_stride=3 * Cc, k=p + Cc * esz, v=p + 2 * Cc * esz,
                              kv_stride=3 * Cc, o=T["o"].data_ptr(), dout=T["dout"].data_ptr(), o_stride=Cc, lse=T["lse"].data_ptr(), delta=T["delta"].data_ptr(),
                              dq=dp, dq_stride=gs, dk=dp + Cc * esz, dv=dp + 2 * Cc * esz, dkv_stride=gs)
        L.check(lib.pd_attn_wide_bwd(C.byref(b), stream()), "pd_attn_wide_bwd")

    def check(O):
        leaf = qkv.clone().requires_grad_(True)
        ref = F.scaled_dot_product_attention(sp(leaf[..., :Cc]), sp(leaf[..., Cc:2 * Cc]), sp(leaf[..., 2 * Cc:])).transpose(1, 2).reshape(B, N, Cc)
        ref.backward(dout)
        got = O["dqkv"].float()
        for i in range(3):
            assert rel(got[..., i * Cc:(i + 1) * Cc], leaf.grad[..., i * Cc:(i + 1) * Cc]) < ATTN_WIDE_BWD_TOL[mode], "qkv"[i]

    return Case(ins, outs, launch, check, nsamples=B)


# ---- GroupNorm helpers --------------------------------------------------------------------------------------------------------------------------
def gn_case(env_, mode, key):
    from test_gpu_kernels import GN_FINALIZE_TOL, GN_STATS_TOL
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    B, c0, c1, hw = 3, 128, 64, 64
    Cc = c0 + c1
    g = torch.Generator().manual_seed(106)
    xs = bf16_round(torch.randn(B, Cc, hw, generator=g) * 2 + 0.7, mode)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    X0, X1 = xs[:, :c0].permute(0, 2, 1).contiguous().to(tdt), xs[:, c0:].permute(0, 2, 1).contiguous().to(tdt)
    ref = F.group_norm(xs, 32, gamma, beta, eps=1e-5)
    if key == "stats":
        splits = 4
        ins = {"x0": Op(X0, sample_dim=0), "x1": Op(X1, sample_dim=0), "gamma": Op(gamma), "beta": Op(beta)}
        outs = {"partial": out_op((B, splits, Cc, 2), torch.float64, sample_dim=0), "scale": out_op((B, Cc), torch.float32, sample_dim=0),
                "shift": out_op((B, Cc), torch.float32, sample_dim=0)}

        def launch(T):
            a = L.GnStatsArgs(dtype=code, B=B, HW=hw, C0=c0, C1=c1, groups=32, eps=1e-5, x0=T["x0"].data_ptr(), x1=T["x1"].data_ptr(), gamma=T["gamma"].data_ptr(),
                              beta=T["beta"].data_ptr(), partial=T["partial"].data_ptr(), splits=splits, scale=T["scale"].data_ptr(), shift=T["shift"].data_ptr())
            L.check(lib.pd_gn_stats(C.byref(a), stream()), "pd_gn_stats")

        def check(O):
            assert rel(xs * O["scale"][:, :, None] + O["shift"][:, :, None], ref) < GN_STATS_TOL
    elif key == "finalize":
        T0, T1 = 4, 2                                     # per-tile (sum, sum of squares) of the two producers, as pd_conv(stats_out) leaves them
        tiles = lambda t, n: torch.stack([torch.stack([c.sum(2), (c * c).sum(2)], -1) for c in t.double().chunk(n, 2)], 1).float()
        ins = {"stats0": Op(tiles(xs[:, :c0], T0), sample_dim=0), "stats1": Op(tiles(xs[:, c0:], T1), sample_dim=0), "gamma": Op(gamma), "beta": Op(beta)}
        outs = {"scale": out_op((B, Cc), torch.float32, sample_dim=0), "shift": out_op((B, Cc), torch.float32, sample_dim=0)}

        def launch(T):
            a = L.GnFinalizeArgs(B=B, HW=hw, groups=32, eps=1e-5, C0=c0, T0=T0, stats0=T["stats0"].data_ptr(), C1=c1, T1=T1, stats1=T["stats1"].data_ptr(),
                                 gamma=T["gamma"].data_ptr(), beta=T["beta"].data_ptr(), scale=T["scale"].data_ptr(), shift=T["shift"].data_ptr())
            L.check(lib.pd_gn_finalize(C.byref(a), stream()), "pd_gn_finalize")

        def check(O):
            assert rel(xs * O["scale"][:, :, None] + O["shift"][:, :, None], ref) < GN_FINALIZE_TOL
    else:
        # pd_gn_apply has no parity test of its own: y = silu(x * scale + shift) stored in the engine dtype is one rounding of an elementwise fp32
        # expression, the precision class of pd_layernorm / pd_geglu -> their bound (ROW_OP_TOL)
        scale, shift = torch.rand(B, Cc, generator=g) + 0.5, torch.randn(B, Cc, generator=g)
        ins = {"x0": Op(X0, sample_dim=0), "x1": Op(X1, sample_dim=0), "scale": Op(scale, sample_dim=0), "shift": Op(shift, sample_dim=0)}
        outs = {"y": out_op((B, hw, Cc), tdt, sample_dim=0)}

        def launch(T):
            a = L.GnApplyArgs(dtype=code, B=B, HW=hw, C0=c0, C1=c1, silu=1, x0=T["x0"].data_ptr(), x1=T["x1"].data_ptr(), scale=T["scale"].data_ptr(),
                              shift=T["shift"].data_ptr(), y=T["y"].data_ptr())
            L.check(lib.pd_gn_apply(C.byref(a), stream()), "pd_gn_apply")

        def check(O):
            assert rel(O["y"].float().permute(0, 2, 1), F.silu(xs * scale[:, :, None] + shift[:, :, None])) < ROW_OP_TOL[mode]
    return Case(ins, outs, launch, check, nsamples=B)


# ---- pd_layernorm_bwd, pd_geglu_bwd ---------------------------------------------------------------------------------------------------------------
def layernorm_bwd_case(env_, mode, key):
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    rows, Cc, with_res = {"37x64": (37, 64, False), "513x1280-res": (513, 1280, True)}[key]
    g = torch.Generator().manual_seed(152)
    x = bf16_round(torch.randn(rows, Cc, generator=g) * 2 + 0.5, mode).requires_grad_()
    gamma = torch.randn(Cc, generator=g).requires_grad_()
    beta = torch.randn(Cc, generator=g).requires_grad_()
    dy = bf16_round(torch.randn(rows, Cc, generator=g), mode)
    res = bf16_round(torch.randn(rows, Cc, generator=g), mode)
    nb = lib.pd_layernorm_bwd_blocks(rows)
    ins = {"x": Op(x.detach().to(tdt), sample_dim=0), "dy": Op(dy.to(tdt), sample_dim=0), "gamma": Op(gamma.detach())}
    if with_res:
        ins["res"] = Op(res.to(tdt), sample_dim=0)
    outs = {"dx": out_op((rows, Cc), tdt, sample_dim=0), "dgamma": Op(torch.full((Cc,), 1.0)), "dbeta": Op(torch.full((Cc,), -2.0)),      # accumulate (+=)
            "partial": out_op((nb * 2 * Cc,), torch.float32, whole=False)}

    def launch(T):
        a = L.LayerNormBwdArgs(dtype=code, rows=rows, C=Cc, eps=1e-5, x=T["x"].data_ptr(), dy=T["dy"].data_ptr(), gamma=T["gamma"].data_ptr(),
                               res=L.ptr(T.get("res")), dx=T["dx"].data_ptr(), dgamma=T["dgamma"].data_ptr(), dbeta=T["dbeta"].data_ptr(), partial=T["partial"].data_ptr())
        L.check(lib.pd_layernorm_bwd(C.byref(a), stream()), "pd_layernorm_bwd")

    def check(O):
        F.layer_norm(x, (Cc,), gamma, beta, 1e-5).backward(dy)
        assert rel(O["dx"].float(), x.grad + (res if with_res else 0)) < LN_BWD_TOL[mode]
        assert rel(O["dgamma"] - 1.0, gamma.grad) < LN_BWD_PARAM_TOL and rel(O["dbeta"] + 2.0, beta.grad) < LN_BWD_PARAM_TOL

    return Case(ins, outs, launch, check, nsamples=rows)


def geglu_bwd_case(env_, mode, key):
    L, lib, _, dev = env_
    code, tdt = DT[mode]
    rows, inner, Bs, splits = {"301x264": (301, 264, 0, 0), "333x256-sums-B3-s5": (333, 256, 3, 5)}[key]
    g = torch.Generator().manual_seed(153)
    x = bf16_round(torch.randn(rows, 2 * inner, generator=g) * 1.5, mode).requires_grad_()
    dy = bf16_round(torch.randn(rows, inner, generator=g), mode)
    ins = {"x": Op(x.detach().to(tdt), sample_dim=0), "dy": Op(dy.to(tdt), sample_dim=0)}
    outs = {"dx": out_op((rows, 2 * inner), tdt, sample_dim=0)}
    if Bs:
        outs["sums"] = out_op((Bs * splits * 2 * inner,), torch.float32)

    def launch(T):
        a = L.GegluBwdArgs(dtype=code, rows=rows, inner=inner, x=T["x"].data_ptr(), dy=T["dy"].data_ptr(), dx=T["dx"].data_ptr(), sums=L.ptr(T.get("sums")),
                           sum_splits=splits, B=Bs)
        L.check(lib.pd_geglu_bwd(C.byref(a), stream()), "pd_geglu_bwd")

    def check(O):
        h, gate = x.chunk(2, dim=-1)
        (h * F.gelu(gate)).backward(dy)
        assert rel(O["dx"].float(), x.grad) < GEGLU_BWD_TOL[mode]

    return Case(ins, outs, launch, check, nsamples=rows)


# ---- pd_temb --------------------------------------------------------------------------------------------------------------------------------------
def temb_case(env_, mode, key):
    """pd_temb at SD width (fp32 only: it has one engine), as test_temb_wide_projection_stack; rows = timesteps."""
    import math
    from test_gpu_kernels import TEMB_TOL
    L, lib, _, dev = env_
    rows, with_emb = {"11rows-emb": (11, True), "3rows": (3, False)}[key]
    g = torch.Generator().manual_seed(21)
    c0, tdim, pdim = 320, 1280, 3400
    w1, w2, wp = (torch.randn(i, o, generator=g) / math.sqrt(i) for i, o in ((c0, tdim), (tdim, tdim), (tdim, pdim)))
    b1, b2, bp = (torch.randn(n, generator=g) * 0.1 for n in (tdim, tdim, pdim))
    ts = torch.randint(0, 1000, (rows,), generator=g).float()
    ins = {"w1": Op(w1), "b1": Op(b1), "w2": Op(w2), "b2": Op(b2), "wp": Op(wp), "bp": Op(bp), "ts": Op(ts, sample_dim=0)}
    outs = {"proj": out_op((rows, pdim), torch.float32, sample_dim=0), "z1": out_op((rows, tdim), torch.float32, sample_dim=0),
            "feat": out_op((rows, c0), torch.float32, sample_dim=0)}
    if with_emb:
        outs["emb"] = out_op((rows, tdim), torch.float32, sample_dim=0)

    def launch(T):
        a = L.TembArgs(rows=rows, c0=c0, tdim=tdim, proj_dim=pdim, flip_sin_to_cos=1, freq_shift=0.0, num_classes=0, timesteps=T["ts"].data_ptr(), labels=None,
                       class_emb=None, w1=T["w1"].data_ptr(), b1=T["b1"].data_ptr(), w2=T["w2"].data_ptr(), b2=T["b2"].data_ptr(), class_table=None,
                       wp=T["wp"].data_ptr(), bp=T["bp"].data_ptr(), emb=L.ptr(T.get("emb")), proj=T["proj"].data_ptr(), feat=T["feat"].data_ptr(), z1=T["z1"].data_ptr())
        L.check(lib.pd_temb(C.byref(a), stream()), "pd_temb")

    def check(O):
        half = c0 // 2
        freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
        arg = ts.double()[:, None] * freqs[None]
        se = torch.cat([arg.cos(), arg.sin()], 1)
        emb_ref = F.silu(se @ w1.double() + b1.double()) @ w2.double() + b2.double()
        assert rel(O["proj"].double(), F.silu(emb_ref) @ wp.double() + bp.double()) < TEMB_TOL

    return Case(ins, outs, launch, check, nsamples=rows)


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------
ALL3 = ["f32", "bf16", "fp16"]
PER_SAMPLE = ([("pd_attn_d64", attn_d64_case, k, m) for k in ATTN_D64_CASES for m in ALL3]
              + [("pd_attn_d64_bwd", attn_d64_bwd_case, k, m) for k in ATTN_D64_BWD_CASES for m in ALL3]
              + [("pd_attn_d8", attn_d8_case, k, m) for k, (_, km) in ATTN_D8_CASES.items() for m in (["bf16", "fp16"] if km else ALL3)]
              + [("pd_linear", linear_case, k, m) for k, (_, e) in LINEAR_CASES.items() for m in (ALL3 if not e else ["bf16", "fp16"])]
              + [("pd_linear-glu", linear_geglu_case, k, m) for k, (_, e) in LINEAR_GEGLU_CASES.items() for m in (ALL3 if not e else ["bf16", "fp16"])]
              + [("pd_conv", conv_case, k, m) for k in CONV_CASES for m in ALL3]
              + [("pd_linear-gn", linear_gn_case, k, m) for k, (r, km) in LINEAR_GN_CASES.items() for m in (["bf16", "fp16"] if (km or r == "folded") else ALL3)]
              + [("pd_conv-tail", conv_tail_case, k, m) for k in CONV_TAIL_CASES for m in ALL3]
              + [("pd_conv-phase", conv_phase_case, k, m) for k in ("fwd-9x33", "fwd-20x17", "phase_in-9x33") for m in ALL3]
              + [("pd_conv-im2col3", conv_im2col3_case, k, m) for k in ("9x33", "24x40") for m in ALL3]
              + [("pd_attn_d8_bwd", attn_d8_bwd_case, k, m) for k, (_, op1) in ATTN_D8_BWD_CASES.items() for m in (["bf16", "fp16"] if op1 else ALL3)]
              + [("pd_attn_wide", attn_wide_case, k, m) for k in ("fwd-B3-h2-d128-77-outstrided", "bwd-B3-h2-d128-77-dqkv-strided") for m in ALL3]
              + [("pd_gn", gn_case, k, m) for k in ("stats", "finalize", "apply") for m in ALL3]
              + [("pd_layernorm_bwd", layernorm_bwd_case, k, m) for k in ("37x64", "513x1280-res") for m in ALL3]
              + [("pd_geglu_bwd", geglu_bwd_case, k, m) for k in ("301x264", "333x256-sums-B3-s5") for m in ALL3]
              + [("pd_temb", temb_case, k, "f32") for k in ("11rows-emb", "3rows")]
              + [("pd_layernorm", layernorm_case, k, m) for k in ("37x64", "301x640", "5x2048") for m in ALL3]
              + [("pd_geglu", geglu_case, k, m) for k in ("301x256", "7x1288") for m in ALL3])
SUMMED_CONV = [("pd_conv_wgrad", conv_wgrad_case, k, m) for k in CONV_WGRAD_CASES for m in ALL3]
SUMMED = [("pd_token_wgrad", (lambda e, m, k, acc=acc: token_wgrad_case(e, m, k, acc)), f"{k}-acc{acc}", m)
          for k in TOKEN_WGRAD_CASES for acc in (0, 1) for m in ALL3]
_id = lambda c: f"{c[0]}-{c[2]}-{c[3]}"


def _build(env_, c):
    name, builder, key, mode = c
    return builder(env_, mode, key.rsplit("-acc", 1)[0] if name == "pd_token_wgrad" else key)


@pytest.mark.parametrize("c", PER_SAMPLE + SUMMED + SUMMED_CONV, ids=_id)
def test_p1_poisoned_surroundings(env, c, monkeypatch):
    p1_poisoned_surroundings(_build(env, c), env[3], monkeypatch)


@pytest.mark.parametrize("c", PER_SAMPLE + SUMMED + SUMMED_CONV, ids=_id)
def test_p2_canaried_outputs(env, c, monkeypatch):
    p2_canaried_outputs(_build(env, c), env[3], monkeypatch)


@pytest.mark.parametrize("c", PER_SAMPLE, ids=_id)
def test_p3_sample_isolation(env, c, monkeypatch):
    p3_sample_isolation(_build(env, c), env[3], monkeypatch)
