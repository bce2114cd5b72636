#!/usr/bin/env python3
"""pd_attn_hd at the Stable Diffusion 1.x attention shapes against the zero-padded route through the existing kernels (docs/LAB_r9.md).

    python scripts/experiments/bench_attn_hd.py [--B 32] [--unet]

B x 8 heads, (D, Nq, Nkv) = (40, 4096, 4096), (80, 1024, 1024), (160, 256, 256), (40, 4096, 77), (160, 64, 64), bf16 and fp16.  Per
shape and dtype ONE child process times, back to back on the same device state,
  native : pd_attn_hd on q / k / v as slices of the fused projection output (cross attention: q and a fused k|v), and
  padded : the same heads zero-padded to 64 (pd_attn_d64; q pre-multiplied so that its fixed 1/8 is the true scale) resp. to 128 / 256
           (pd_attn_wide with the true scale) -- 1.6 x the matrix work and 1.6 x the q / k / v bytes; building the padded copies is NOT timed.
The ratio printed is padded / native (>= 1.0: the native kernel is not slower).  TF/s counts the true 4 B heads Nq Nkv D.  Times are
device times between events.  The relative difference of the two routes' outputs is a sanity check, not a parity test: at D = 40 it
includes the second 16-bit rounding of the pre-multiplied q.
Every child runs under its own time limit; the first one that fails, faults or times out ends the run (nothing is started after it).
--unet adds one more child: the forward of a random-init SD15_UNET_CONFIG at 64 x 64 latents, 77 tokens (information, not a gate).
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SHAPES = ((40, 4096, 4096), (80, 1024, 1024), (160, 256, 256), (40, 4096, 77), (160, 64, 64))
HEADS = 8
STEP_LIMIT_S = 120


def best_of(fn, reps=None, rounds=5):
    """Seconds per call: device time between two events around `reps` back-to-back launches, best of `rounds`.  `reps` defaults to what
    fills ~20 ms of device time (20 .. 2000), so that a kernel of a few microseconds is not timed by its launch submission."""
    import torch

    def timed(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    for _ in range(3):
        fn()
    if reps is None:
        reps = int(min(2000, max(20, 0.02 / max(timed(20), 1e-7))))
    return min(timed(reps) for _ in range(rounds))


def step(B, D, Nq, Nkv, mode):
    import torch
    from phendiff_amd import _lib as L
    code, tdt = {"bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}[mode]
    dev, lib, es = "cuda:0", L.lib(), 2
    st = torch.cuda.current_stream().cuda_stream
    Cc, DP = HEADS * D, {40: 64, 80: 128, 160: 256}[D]
    Cp = HEADS * DP
    g = torch.Generator(device=dev).manual_seed(0)
    if Nq == Nkv:
        qkv = torch.randn(B, Nq, 3 * Cc, device=dev, generator=g).to(tdt)
        q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        qp, kp, vp, qs, kvs = qkv.data_ptr(), qkv.data_ptr() + Cc * es, qkv.data_ptr() + 2 * Cc * es, 3 * Cc, 3 * Cc
    else:
        q = torch.randn(B, Nq, Cc, device=dev, generator=g).to(tdt)
        kv = torch.randn(B, Nkv, 2 * Cc, device=dev, generator=g).to(tdt)
        k, v = kv[..., :Cc], kv[..., Cc:]
        qp, kp, vp, qs, kvs = q.data_ptr(), kv.data_ptr(), kv.data_ptr() + Cc * es, Cc, 2 * Cc
    out = torch.empty(B, Nq, Cc, device=dev, dtype=tdt)
    scale = float(D) ** -0.5
    a = L.AttnHdArgs(dtype=code, B=B, heads=HEADS, D=D, Nq=Nq, Nkv=Nkv, scale=scale, q=qp, q_stride=qs, k=kp, v=vp, kv_stride=kvs,
                     out=out.data_ptr(), out_stride=Cc)
    L.check(lib.pd_attn_hd(C.byref(a), st), "pd_attn_hd")
    t_native = best_of(lambda: lib.pd_attn_hd(C.byref(a), st))

    # the padded route, in the same layouts (one fused [B][N][3 Cp] resp. q + fused k|v), zeros in the pad channels of every head
    def pad(t, n, mul=1.0):
        p = torch.zeros(B, n, HEADS, DP, device=dev, dtype=tdt)
        p[..., :D] = (t.reshape(B, n, HEADS, D).float() * mul).to(tdt)
        return p.reshape(B, n, Cp)
    qmul = scale / 0.125 if DP == 64 else 1.0
    if Nq == Nkv:
        pq = torch.cat([pad(q, Nq, qmul), pad(k, Nkv), pad(v, Nkv)], -1).contiguous()
        pqp, pkp, pvp, pqs, pkvs = pq.data_ptr(), pq.data_ptr() + Cp * es, pq.data_ptr() + 2 * Cp * es, 3 * Cp, 3 * Cp
    else:
        pq, pkv = pad(q, Nq, qmul).contiguous(), torch.cat([pad(k, Nkv), pad(v, Nkv)], -1).contiguous()
        pqp, pkp, pvp, pqs, pkvs = pq.data_ptr(), pkv.data_ptr(), pkv.data_ptr() + Cp * es, Cp, 2 * Cp
    pout = torch.empty(B, Nq, Cp, device=dev, dtype=tdt)
    common = dict(dtype=code, B=B, heads=HEADS, Nq=Nq, Nkv=Nkv, q=pqp, q_stride=pqs, k=pkp, v=pvp, kv_stride=pkvs, out=pout.data_ptr(), out_stride=Cp)
    if DP == 64:
        fn, pa, what = lib.pd_attn_d64, L.AttnD64Args(**common), "pd_attn_d64"
    else:
        fn, pa, what = lib.pd_attn_wide, L.AttnWideArgs(D=DP, scale=scale, **common), f"pd_attn_wide D={DP}"
    L.check(fn(C.byref(pa), st), what)
    t_padded = best_of(lambda: fn(C.byref(pa), st))
    torch.cuda.synchronize()
    # the two routes compute the same thing
    diff = float((pout.reshape(B, Nq, HEADS, DP)[..., :D].float() - out.reshape(B, Nq, HEADS, D).float()).norm() / out.float().norm())
    fl = 4.0 * B * HEADS * Nq * Nkv * D
    print(json.dumps(dict(D=D, Nq=Nq, Nkv=Nkv, B=B, heads=HEADS, dtype=mode, native_ms=round(t_native * 1e3, 4), padded_ms=round(t_padded * 1e3, 4),
                          padded_kernel=what, ratio=round(t_padded / t_native, 3), native_tflops=round(fl / t_native / 1e12, 1),
                          padded_vs_native_rel_diff=diff)), flush=True)


def unet_step(B):
    import torch
    import phendiff_amd as P
    torch.manual_seed(0)
    m = P.SDUNet2DConditionModel(compute_dtype="bf16", **P.SD15_UNET_CONFIG).to("cuda:0")
    x, ts = torch.randn(B, 4, 64, 64, device="cuda:0"), torch.full((B,), 500.0, device="cuda:0")
    ehs = torch.randn(B, 77, 768, device="cuda:0")
    t = best_of(lambda: m(x, ts, ehs), reps=5, rounds=3)
    plan = next(iter(m._plans.values()))
    print(json.dumps(dict(what="SD15_UNET_CONFIG forward, random init, bf16, 64x64 latents, 77 tokens", B=B, forward_ms=round(t * 1e3, 3),
                          attn_hd_launches=sum(op.what == "attn_hd" for op in plan.ops))), flush=True)


def box_state():
    """Clock and power as the box reports them (read-only query; absent tool: empty)."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else {}
    except Exception:
        return {}


def main():
    argv = sys.argv[1:]
    B = int(argv[argv.index("--B") + 1]) if "--B" in argv else 32
    if "--step" in argv:
        i = argv.index("--step")
        return step(B, int(argv[i + 1]), int(argv[i + 2]), int(argv[i + 3]), argv[i + 4])
    if "--unet-step" in argv:
        return unet_step(min(B, 8))
    print(json.dumps(dict(box_before=box_state())), flush=True)
    jobs = [["--step", str(D), str(nq), str(nkv), mode] for (D, nq, nkv) in SHAPES for mode in ("bf16", "fp16")]
    if "--unet" in argv:
        jobs.append(["--unet-step"])
    for job in jobs:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--B", str(B)] + job, timeout=STEP_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(stopped_after=job, exit_status=rc)), flush=True)
            return rc
    print(json.dumps(dict(box_after=box_state())), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
