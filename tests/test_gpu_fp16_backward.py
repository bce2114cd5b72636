"""The fp16 backward kernels in the loss-scaled regime: every kernel runs the cases of tests/fp16_bwd_cases.py twice, with the incoming gradient
at unit scale and multiplied by GAIN = 256.  The kernels are linear in that gradient and the gain is a power of two, so as long as nothing
saturates no rounding changes: the fp64 reference is GAIN times the unit one and the relative-L2 bound is the one of the unit-scale parity
tests (imported, not restated).  tests/test_host_fp16_backward_cases.py shows on the CPU that the reference itself stays inside fp16 at GAIN,
so a non-finite value or a missed bound here is the kernel's.  Where a kernel is documented bit-reproducible, two runs must agree bitwise."""
import ctypes as C

import pytest
import torch

import fp16_bwd_cases as cases
from fp16_bwd_cases import GAIN
from test_gpu_backward import ATTN_D8_BWD_TOL, CONV_WGRAD_FUSED_TOL, CONV_WGRAD_TOL, from_nhwc, run_wgrad
from test_gpu_kernels import DT, TOL, env, nhwc, rel, stream  # noqa: F401  (env is a fixture)
from test_gpu_sd_kernels import ATTN_D64_BWD_TOL, GEGLU_BWD_TOL, LN_BWD_PARAM_TOL, LN_BWD_TOL, TOKEN_WGRAD_TOL

pytestmark = pytest.mark.gpu
MODE = "fp16"
CODE, TDT = DT[MODE]
GAINS = (1.0, GAIN)


def finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


# ---- pd_conv_wgrad ------------------------------------------------------------------------------------------------------------------------------
def wgrad_phases(env, x, dy):
    """The four sub-pixel phase launches of Upsample2D's weight gradient, on top of a zero gradient."""
    L, lib, _, dev = env
    B, cin, h, w_ = x.shape
    cout = dy.shape[1]
    X, DY = nhwc(x.to(dev), TDT), nhwc(dy.to(dev), TDT)
    dw = torch.zeros((cout, cin, 3, 3), device=dev)
    for ph in range(4):
        a = L.WgradArgs(dtype=CODE, B=B, Hin=h, Win=w_, Hout=h, Wout=w_, C0=cin, C1=0, Cout=cout, ksize=2, stride=1, pad=0, upsample=0, silu=0,
                        x0=X.data_ptr(), x1=None, scale=None, shift=None, dy=DY.data_ptr(), dw=dw.data_ptr(), Cout_valid=0, Cin_valid=0,
                        accumulate=1, phase=1 + ph)
        need = lib.pd_conv_wgrad_workspace(C.byref(a))
        assert need > 0
        slab = torch.empty(need // 4, device=dev)
        a.slab, a.slab_bytes = slab.data_ptr(), need
        L.check(lib.pd_conv_wgrad(C.byref(a), stream()), "pd_conv_wgrad")
    torch.cuda.synchronize()
    return dw.cpu()


@pytest.mark.parametrize("key", list(cases.CONV_WGRAD))
def test_conv_weight_gradient_under_the_gain(env, key):
    c = cases.conv_wgrad(key)
    m = c.meta
    tol = (CONV_WGRAD_FUSED_TOL if m.get("fused") else CONV_WGRAD_TOL)[MODE]
    for gain in GAINS:
        t = c.scaled_inputs(gain)
        runs = []
        for _ in range(2):
            if m.get("phases"):
                runs.append(wgrad_phases(env, t["x"], t["dy"]))
            elif m.get("fused"):
                c0 = m["cin"] - m["c1"]
                runs.append(run_wgrad(env, MODE, t["x"][:, :c0], t["dy"], x1=t["x"][:, c0:], silu=1, scale=t["scale"], shift=t["shift"]))
            else:
                runs.append(run_wgrad(env, MODE, t["x"], t["dy"], ksize=m["ksize"], stride=m["stride"], pad=m["ksize"] // 2))
        assert finite(runs[0]), gain
        assert rel(runs[0], c.ref["dw"] * gain) < tol, gain
        assert torch.equal(runs[0], runs[1]), gain            # fixed split and fold order: the same bits


# ---- pd_attn_d8_bwd -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(cases.ATTN_D8_BWD))
def test_attention_d8_backward_under_the_gain(env, key):
    L, lib, _, dev = env
    c = cases.attn_d8_bwd(key)
    B, heads, N, onepass = (c.meta[k] for k in ("B", "heads", "N", "onepass"))
    Cc = heads * 8
    Q, K, V = (c.inputs[n].to(TDT).to(dev).contiguous() for n in ("q", "k", "v"))
    out = torch.empty((B, N, Cc), dtype=TDT, device=dev)
    lse = torch.full((B, heads, N), float("nan"), device=dev)
    a = L.AttnArgs(dtype=CODE, B=B, heads=heads, N=N, q=Q.data_ptr(), k=K.data_ptr(), v=V.data_ptr(), out=out.data_ptr(), lse=lse.data_ptr())
    L.check(lib.pd_attn_d8(C.byref(a), stream()), "pd_attn_d8")
    torch.cuda.synchronize()
    for gain in GAINS:
        DO = c.scaled_inputs(gain)["dout"].to(TDT).to(dev).contiguous()
        delta = torch.empty((B, heads, N), device=dev)
        dqkv = torch.full((B, N, 3 * Cc), float("nan"), dtype=TDT, device=dev)
        b = L.AttnBwdArgs(dtype=CODE, B=B, heads=heads, N=N, q=Q.data_ptr(), k=K.data_ptr(), v=V.data_ptr(), o=out.data_ptr(), dout=DO.data_ptr(),
                          lse=lse.data_ptr(), delta=delta.data_ptr(), dqkv=dqkv.data_ptr())
        need = int(lib.pd_attn_d8_bwd_workspace(C.byref(b)))
        assert (need > 0) == onepass
        if onepass:
            slab = torch.full((need // 4,), float("nan"), device=dev)
            b.slab, b.slab_bytes = slab.data_ptr(), need
        runs = []
        for _ in range(2):
            dqkv.fill_(float("nan"))
            L.check(lib.pd_attn_d8_bwd(C.byref(b), stream()), "pd_attn_d8_bwd")
            torch.cuda.synchronize()
            runs.append(dqkv.clone())
        assert finite(runs[0], delta), gain
        got = runs[0].float().cpu().reshape(B, N, 3, heads, 8).permute(2, 0, 3, 1, 4)          # [which][B][heads][N][8]
        for i, name in enumerate(("dq", "dk", "dv")):
            assert rel(got[i], c.ref[name] * gain) < ATTN_D8_BWD_TOL[MODE], (name, gain)
        if onepass:                                                                          # the one-pass form has no atomics
            assert torch.equal(runs[0], runs[1]), gain


# ---- pd_attn_d64_bwd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(cases.ATTN_D64_BWD))
def test_attention_d64_backward_under_the_gain(env, key):
    L, lib, _, dev = env
    c = cases.attn_d64_bwd(key)
    B, heads, Nq, Nkv = (c.meta[k] for k in ("B", "heads", "Nq", "Nkv"))
    Cc = heads * 64
    Q, KV = c.inputs["q"].to(TDT).to(dev), c.inputs["kv"].to(TDT).to(dev)
    esz = Q.element_size()
    out = torch.empty((B, Nq, Cc), dtype=TDT, device=dev)
    lse = torch.empty((B, heads, Nq), dtype=torch.float32, device=dev)
    a = L.AttnD64Args(dtype=CODE, B=B, heads=heads, Nq=Nq, Nkv=Nkv, q=Q.data_ptr(), q_stride=Cc, k=KV.data_ptr(), v=KV.data_ptr() + Cc * esz,
                      kv_stride=2 * Cc, out=out.data_ptr(), out_stride=Cc, lse=lse.data_ptr())
    L.check(lib.pd_attn_d64(C.byref(a), stream()), "pd_attn_d64")
    torch.cuda.synchronize()
    for gain in GAINS:
        DO = c.scaled_inputs(gain)["dout"].to(TDT).to(dev)
        dq = torch.full((B, Nq, Cc), float("nan"), dtype=TDT, device=dev)
        dkv = torch.full((B, Nkv, 2 * Cc), float("nan"), dtype=TDT, device=dev)
        delta = torch.empty((B, heads, Nq), dtype=torch.float32, device=dev)
        b = L.AttnD64BwdArgs(dtype=CODE, B=B, heads=heads, Nq=Nq, Nkv=Nkv, q=Q.data_ptr(), q_stride=Cc, k=KV.data_ptr(), v=KV.data_ptr() + Cc * esz,
                             kv_stride=2 * Cc, o=out.data_ptr(), dout=DO.data_ptr(), o_stride=Cc, lse=lse.data_ptr(), delta=delta.data_ptr(),
                             dq=dq.data_ptr(), dq_stride=Cc, dk=dkv.data_ptr(), dv=dkv.data_ptr() + Cc * esz, dkv_stride=2 * Cc)
        L.check(lib.pd_attn_d64_bwd(C.byref(b), stream()), "pd_attn_d64_bwd")
        torch.cuda.synchronize()
        assert finite(dq, dkv, delta), gain
        tol = ATTN_D64_BWD_TOL[MODE]
        assert rel(dq.float(), c.ref["dq"] * gain) < tol, ("dq", gain)
        assert rel(dkv.float()[..., :Cc], c.ref["dk"] * gain) < tol, ("dk", gain)
        assert rel(dkv.float()[..., Cc:], c.ref["dv"] * gain) < tol, ("dv", gain)


# ---- pd_gn_silu_bwd -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(cases.GN_SILU_BWD))
def test_groupnorm_silu_backward_under_the_gain(env, key):
    L, lib, _, dev = env
    c = cases.gn_silu_bwd(key)
    B, c0, c1, H, W, silu = (c.meta[k] for k in ("B", "c0", "c1", "H", "W", "silu"))
    Cc, splits = c0 + c1, 4
    x = c.inputs["x"]
    X0, X1 = nhwc(x[:, :c0].to(dev), TDT), nhwc(x[:, c0:].to(dev), TDT)
    mean, rstd = c.meta["stats"]["mean"].to(dev), c.meta["stats"]["rstd"].to(dev)
    gm, bt = c.inputs["gamma"].to(dev), c.inputs["beta"].to(dev)
    for gain in GAINS:
        t = c.scaled_inputs(gain)
        DZ, RES = nhwc(t["dz"].to(dev), TDT), nhwc(t["res"].to(dev), TDT)
        partial = torch.empty((B, splits, Cc, 2), dtype=torch.float64, device=dev)
        coef = torch.empty((B, 32, 2), device=dev)
        dx0 = torch.full((B, H, W, c0), float("nan"), dtype=TDT, device=dev)
        dx1 = torch.full((B, H, W, c1), float("nan"), dtype=TDT, device=dev)
        dgamma, dbeta = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
        b = L.GnBwdArgs(dtype=CODE, B=B, HW=H * W, C0=c0, C1=c1, groups=32, silu=silu, x0=X0.data_ptr(), x1=X1.data_ptr(), dz0=DZ.data_ptr(), dz1=None,
                        mean=mean.data_ptr(), rstd=rstd.data_ptr(), gamma=gm.data_ptr(), beta=bt.data_ptr(), partial=partial.data_ptr(), splits=splits,
                        coef=coef.data_ptr(), dx0=dx0.data_ptr(), dx1=dx1.data_ptr(), accumulate0=0, accumulate1=0, dgamma=dgamma.data_ptr(),
                        dbeta=dbeta.data_ptr(), dz_combined=1, res=RES.data_ptr())
        L.check(lib.pd_gn_silu_bwd(C.byref(b), stream()), "pd_gn_silu_bwd")
        torch.cuda.synchronize()
        assert finite(dx0, dx1, dgamma, dbeta), gain
        assert rel(from_nhwc(dx0), c.ref["dx"][:, :c0] * gain) < TOL[MODE], gain
        assert rel(from_nhwc(dx1), c.ref["dx"][:, c0:] * gain) < TOL[MODE], gain
        assert rel(dgamma.cpu(), c.ref["dgamma"] * gain) < 2e-5 and rel(dbeta.cpu(), c.ref["dbeta"] * gain) < 2e-5, gain


# ---- pd_layernorm_bwd, pd_geglu_bwd, pd_token_wgrad, pd_pool2x2_sum ------------------------------------------------------------------------------
def test_layernorm_backward_under_the_gain(env):
    L, lib, _, dev = env
    c = cases.layernorm_bwd()
    rows, Cc = c.meta["rows"], c.meta["C"]
    X, gm = c.inputs["x"].to(TDT).to(dev), c.inputs["gamma"].to(dev)
    nb = lib.pd_layernorm_bwd_blocks(rows)
    for gain in GAINS:
        t = c.scaled_inputs(gain)
        DY, R = t["dy"].to(TDT).to(dev), t["res"].to(TDT).to(dev)
        dx = torch.full((rows, Cc), float("nan"), dtype=TDT, device=dev)
        dgm, dbt, dxs = (torch.zeros(Cc, dtype=torch.float32, device=dev) for _ in range(3))       # all three accumulate (+=)
        part = torch.empty(nb * 3 * Cc, dtype=torch.float32, device=dev)
        a = L.LayerNormBwdArgs(dtype=CODE, rows=rows, C=Cc, eps=1e-5, x=X.data_ptr(), dy=DY.data_ptr(), gamma=gm.data_ptr(), res=R.data_ptr(),
                               dx=dx.data_ptr(), dgamma=dgm.data_ptr(), dbeta=dbt.data_ptr(), partial=part.data_ptr(), dxsum=dxs.data_ptr())
        L.check(lib.pd_layernorm_bwd(C.byref(a), stream()), "pd_layernorm_bwd")
        torch.cuda.synchronize()
        assert finite(dx, dgm, dbt, dxs), gain
        assert rel(dx.float(), c.ref["dx"] * gain) < LN_BWD_TOL[MODE], gain
        assert rel(dgm, c.ref["dgamma"] * gain) < LN_BWD_PARAM_TOL and rel(dbt, c.ref["dbeta"] * gain) < LN_BWD_PARAM_TOL, gain
        assert rel(dxs, dx.double().sum(0)) < 1e-5, gain                                           # the column sums of dx as stored


def test_geglu_backward_under_the_gain(env):
    L, lib, _, dev = env
    c = cases.geglu_bwd()
    rows, inner, B, splits = (c.meta[k] for k in ("rows", "inner", "B", "splits"))
    X = c.inputs["x"].to(TDT).to(dev)
    for gain in GAINS:
        DY = c.scaled_inputs(gain)["dy"].to(TDT).to(dev)
        dx = torch.full((rows, 2 * inner), float("nan"), dtype=TDT, device=dev)
        ws = torch.full((B * splits * 2 * inner,), float("nan"), dtype=torch.float32, device=dev)
        a = L.GegluBwdArgs(dtype=CODE, rows=rows, inner=inner, x=X.data_ptr(), dy=DY.data_ptr(), dx=dx.data_ptr(), sums=ws.data_ptr(), sum_splits=splits, B=B)
        L.check(lib.pd_geglu_bwd(C.byref(a), stream()), "pd_geglu_bwd")
        torch.cuda.synchronize()
        assert finite(dx, ws), gain
        assert rel(dx.float(), c.ref["dx"] * gain) < GEGLU_BWD_TOL[MODE], gain
        assert rel(ws.reshape(B, splits, 2 * inner).double().sum(1), dx.double().reshape(B, rows // B, 2 * inner).sum(1)) < 1e-5, gain


@pytest.mark.parametrize("key", list(cases.TOKEN_WGRAD))
def test_token_weight_gradient_under_the_gain(env, key):
    L, lib, _, dev = env
    c = cases.token_wgrad(key)
    M, K, N = c.meta["M"], c.meta["K"], c.meta["N"]
    X = c.inputs["x"].to(TDT).to(dev)
    for gain in GAINS:
        DY = c.scaled_inputs(gain)["dy"].to(TDT).to(dev)
        runs = []
        for _ in range(2):
            dw = torch.full((N, K), float("nan"), device=dev)
            a = L.TokenWgradArgs(dtype=CODE, M=M, K=K, N=N, x=X.data_ptr(), x_stride=K, dy=DY.data_ptr(), dy_stride=N, dw=dw.data_ptr(), accumulate=0)
            need = lib.pd_token_wgrad_workspace(C.byref(a))
            slab = torch.empty(need // 4, dtype=torch.float32, device=dev)
            a.slab, a.slab_bytes = slab.data_ptr(), need
            L.check(lib.pd_token_wgrad(C.byref(a), stream()), "pd_token_wgrad")
            torch.cuda.synchronize()
            runs.append(dw)
        assert finite(runs[0]), gain
        assert rel(runs[0], c.ref["dw"] * gain) < TOKEN_WGRAD_TOL[MODE], gain
        assert torch.equal(runs[0], runs[1]), gain                                                 # bitwise reproducible


def test_pool2x2_sum_under_the_gain(env):
    L, lib, _, dev = env
    c = cases.pool2x2_sum()
    B, H, W, Cc = (c.meta[k] for k in ("B", "H", "W", "C"))
    for gain in GAINS:
        DU = nhwc(c.scaled_inputs(gain)["du"].to(dev), TDT)
        dx = torch.full((B, H, W, Cc), float("nan"), dtype=TDT, device=dev)
        a = L.Pool2x2Args(dtype=CODE, B=B, H=H, W=W, C=Cc, du=DU.data_ptr(), dx=dx.data_ptr(), accumulate=0)
        L.check(lib.pd_pool2x2_sum(C.byref(a), stream()), "pd_pool2x2_sum")
        torch.cuda.synchronize()
        assert finite(dx), gain
        assert rel(from_nhwc(dx), c.ref["dx"] * gain) < TOL[MODE], gain
