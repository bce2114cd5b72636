#!/usr/bin/env python3
"""pd_attn_d8 alone at the headline's shape (B = 32, 32 heads, N = 4096, bf16, kmax2 supplied: the DMA-staged kernel, every tile
through its check-free body), for the counter passes of scripts/attn_d8_counters.sh.  Prints the event-timed mean of the launches
(isolated, back to back: NOT the in-situ figure -- bench.py's roofline leg has that one).
    python scripts/attn_d8_launch.py [--launches 6] [--B 32] [--heads 32] [--N 4096]"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phendiff_amd._lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=6)
ap.add_argument("--B", type=int, default=32)
ap.add_argument("--heads", type=int, default=32)
ap.add_argument("--N", type=int, default=4096)
args = ap.parse_args()
lib = L.lib()
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(5)
q, k, v = (torch.randn(args.B, args.heads, args.N, 8, generator=g).to(torch.bfloat16).to(dev) for _ in range(3))
kmax2 = (k.float() ** 2).sum(-1).amax(-1).contiguous()
out = torch.empty((args.B, args.N, args.heads * 8), dtype=torch.bfloat16, device=dev)
a = L.AttnArgs(dtype=1, B=args.B, heads=args.heads, N=args.N, q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), out=out.data_ptr(),
               kmax2=kmax2.data_ptr())
st = torch.cuda.current_stream().cuda_stream
L.check(lib.pd_attn_d8(C.byref(a), st), "pd_attn_d8")
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(args.launches):
    L.check(lib.pd_attn_d8(C.byref(a), st), "pd_attn_d8")
e1.record()
torch.cuda.synchronize()
print(f"pd_attn_d8 B={args.B} heads={args.heads} N={args.N} bf16: {e0.elapsed_time(e1) / args.launches:.4f} ms per launch (isolated), "
      f"out sum {float(out.float().sum()):.6e}")
