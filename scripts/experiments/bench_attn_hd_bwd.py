#!/usr/bin/env python3
"""pd_attn_hd and pd_attn_hd_bwd at head_dim 16 / 32 against the zero-padded route through pd_attn_d64 / pd_attn_d64_bwd (docs/LAB_r10.md).

    python scripts/experiments/bench_attn_hd_bwd.py [--B 32] [--C 256] [--N 4096]

Self attention on one fused [B][N][3C] projection output, C / D heads, bf16 (the 64 x 64 level of a 256 x 256 input at B = 32, C = 256,
N = 4096).  Per head dimension ONE child process times, back to back on the same device state,
  native : pd_attn_hd, then pd_attn_hd_bwd writing dq | dk | dv into one fused [B][N][3C] gradient, and
  padded : the only alternative the tree offers -- every head zero-padded to 64 channels (q pre-multiplied so that pd_attn_d64's fixed
           1/8 is the true scale) through pd_attn_d64 / pd_attn_d64_bwd: 64 / D x the matrix work and the q / k / v / dO bytes, plus
           three extra tensors per attention whose construction is NOT timed.
The ratio printed is padded / native (>= 1.0: the native kernel is not slower).  Times are device times between events.  The relative
difference of the two routes' results is a sanity check, not a parity test.
Every child runs under its own time limit; the first one that fails, faults or times out ends the run (nothing is started after it).
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_attn_hd import best_of, box_state  # noqa: E402

DIMS = (16, 32)
STEP_LIMIT_S = 120


def step(B, Cc, N, D):
    import torch
    from phendiff_amd import _lib as L
    code, tdt, es = 1, torch.bfloat16, 2
    dev, lib = "cuda:0", L.lib()
    st = torch.cuda.current_stream().cuda_stream
    heads, DP = Cc // D, 64
    Cp = heads * DP
    scale = float(D) ** -0.5
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B, N, 3 * Cc, device=dev, generator=g).to(tdt)
    do = torch.randn(B, N, Cc, device=dev, generator=g).to(tdt)

    def ptrs(t, c):
        p = t.data_ptr()
        return p, p + c * es, p + 2 * c * es

    out = torch.empty(B, N, Cc, device=dev, dtype=tdt)
    lse = torch.empty(B, heads, N, device=dev, dtype=torch.float32)
    delta = torch.empty_like(lse)
    dqkv = torch.empty_like(qkv)
    qp, kp, vp = ptrs(qkv, Cc)
    dqp, dkp, dvp = ptrs(dqkv, Cc)
    fa = L.AttnHdArgs(dtype=code, B=B, heads=heads, D=D, Nq=N, Nkv=N, scale=scale, q=qp, q_stride=3 * Cc, k=kp, v=vp, kv_stride=3 * Cc,
                      out=out.data_ptr(), out_stride=Cc, lse=lse.data_ptr())
    ba = L.AttnHdBwdArgs(dtype=code, B=B, heads=heads, D=D, Nq=N, Nkv=N, scale=scale, q=qp, q_stride=3 * Cc, k=kp, v=vp, kv_stride=3 * Cc,
                         o=out.data_ptr(), dout=do.data_ptr(), o_stride=Cc, lse=lse.data_ptr(), delta=delta.data_ptr(), dq=dqp,
                         dq_stride=3 * Cc, dk=dkp, dv=dvp, dkv_stride=3 * Cc)
    L.check(lib.pd_attn_hd(C.byref(fa), st), "pd_attn_hd")
    L.check(lib.pd_attn_hd_bwd(C.byref(ba), st), "pd_attn_hd_bwd")
    t_fwd = best_of(lambda: lib.pd_attn_hd(C.byref(fa), st))
    t_bwd = best_of(lambda: lib.pd_attn_hd_bwd(C.byref(ba), st))

    # the padded route: zeros in the pad channels of every head
    def pad(t, mul=1.0):
        p = torch.zeros(B, N, heads, DP, device=dev, dtype=tdt)
        p[..., :D] = (t.reshape(B, N, heads, D).float() * mul).to(tdt)
        return p.reshape(B, N, Cp)
    qmul = scale / 0.125
    pqkv = torch.cat([pad(qkv[..., :Cc], qmul), pad(qkv[..., Cc:2 * Cc]), pad(qkv[..., 2 * Cc:])], -1).contiguous()
    pdo = pad(do).contiguous()
    pout = torch.empty(B, N, Cp, device=dev, dtype=tdt)
    plse, pdelta = torch.empty_like(lse), torch.empty_like(lse)
    pdqkv = torch.empty_like(pqkv)
    pq, pk, pv = ptrs(pqkv, Cp)
    pdq, pdk, pdv = ptrs(pdqkv, Cp)
    pfa = L.AttnD64Args(dtype=code, B=B, heads=heads, Nq=N, Nkv=N, q=pq, q_stride=3 * Cp, k=pk, v=pv, kv_stride=3 * Cp, out=pout.data_ptr(),
                        out_stride=Cp, lse=plse.data_ptr())
    pba = L.AttnD64BwdArgs(dtype=code, B=B, heads=heads, Nq=N, Nkv=N, q=pq, q_stride=3 * Cp, k=pk, v=pv, kv_stride=3 * Cp, o=pout.data_ptr(),
                           dout=pdo.data_ptr(), o_stride=Cp, lse=plse.data_ptr(), delta=pdelta.data_ptr(), dq=pdq, dq_stride=3 * Cp, dk=pdk,
                           dv=pdv, dkv_stride=3 * Cp)
    L.check(lib.pd_attn_d64(C.byref(pfa), st), "pd_attn_d64")
    L.check(lib.pd_attn_d64_bwd(C.byref(pba), st), "pd_attn_d64_bwd")
    t_pfwd = best_of(lambda: lib.pd_attn_d64(C.byref(pfa), st))
    t_pbwd = best_of(lambda: lib.pd_attn_d64_bwd(C.byref(pba), st))
    torch.cuda.synchronize()
    # the two routes compute the same thing (dq of the padded route is the gradient w.r.t. the pre-multiplied q)
    cut = lambda t: t.reshape(B, N, heads, DP)[..., :D].float()
    nat = lambda t: t.reshape(B, N, heads, D).float()
    d_out = float((cut(pout) - nat(out)).norm() / nat(out).norm())
    d_dv = float((cut(pdqkv[..., 2 * Cp:]) - nat(dqkv[..., 2 * Cc:])).norm() / nat(dqkv[..., 2 * Cc:]).norm())
    d_dk = float((cut(pdqkv[..., Cp:2 * Cp]) - nat(dqkv[..., Cc:2 * Cc])).norm() / nat(dqkv[..., Cc:2 * Cc]).norm())
    d_dq = float((cut(pdqkv[..., :Cp]) * qmul - nat(dqkv[..., :Cc])).norm() / nat(dqkv[..., :Cc]).norm())
    print(json.dumps(dict(D=D, heads=heads, B=B, C=Cc, N=N, dtype="bf16",
                          fwd_native_ms=round(t_fwd * 1e3, 4), fwd_padded_ms=round(t_pfwd * 1e3, 4), fwd_ratio=round(t_pfwd / t_fwd, 3),
                          bwd_native_ms=round(t_bwd * 1e3, 4), bwd_padded_ms=round(t_pbwd * 1e3, 4), bwd_ratio=round(t_pbwd / t_bwd, 3),
                          fwd_native_tflops=round(4.0 * B * N * N * Cc / t_fwd / 1e12, 1),
                          bwd_native_tflops=round(10.0 * B * N * N * Cc / t_bwd / 1e12, 1),
                          rel_diff=dict(out=d_out, dq=d_dq, dk=d_dk, dv=d_dv))), flush=True)


def main():
    argv = sys.argv[1:]
    val = lambda flag, dflt: int(argv[argv.index(flag) + 1]) if flag in argv else dflt
    B, Cc, N = val("--B", 32), val("--C", 256), val("--N", 4096)
    if "--step" in argv:
        return step(B, Cc, N, int(argv[argv.index("--step") + 1]))
    print(json.dumps(dict(box_before=box_state())), flush=True)
    for D in DIMS:
        job = ["--B", str(B), "--C", str(Cc), "--N", str(N), "--step", str(D)]
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + job, timeout=STEP_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(stopped_after=job, exit_status=rc)), flush=True)
            return rc
    print(json.dumps(dict(box_after=box_state())), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
