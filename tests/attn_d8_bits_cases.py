"""Cases, seeded inputs and launch helpers shared by tests/test_gpu_attn_d8_bits.py and scripts/record_attn_d8_bits.py: pd_attn_d8 /
pd_attn_d8_bwd in bf16, compared BIT FOR BIT with the outputs an earlier build of the kernels left under tests/golden/attn_d8_bits/.

Inputs are built from element-wise operations on seeded CPU draws only (no reduction whose summation order a torch build could
change), and every fixture carries the sha256 of the inputs it was recorded on.

``plain``:  randn * 1.5, the distribution of the parity tests.
``spread``: every q and k row is a signed permutation of ONE multiset of magnitudes (|row| = 15.9 for all of them), queries sit within a
            small perturbation of one of 16 prototype rows and keys 0..31 ARE the prototypes.  So the exact maximum over the first 32 keys
            is within a few units of the Cauchy-Schwarz bound |q| max|k| -- the tile-level decision takes the check-free body from the
            first tile on -- while the log2-domain scores against the other keys spread over about +-65 around 0: probabilities
            p = 2^(s - m) of every exponent from 1 down to the flush below 2^-126 occur, those of 2^-126 .. 2^-119 (a denormal when the
            upper half of the fp32 word is read as an f16) among them: ``band_count``."""
import ctypes as C
import hashlib
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_d8_bits")
QSCALE = 0.35355339059327373 * 1.4426950408889634           # softmax scale and log2(e), folded into q by the kernels
MAGS = torch.tensor([1.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 7.25])       # sum of squares 252.6: |row| = 15.9

# name -> (kind, B, heads, N, kmax2 supplied, inputs, seed)
CASES = {
    # B = 1, 2 heads, N = 1024, kmax2 supplied.  (With 8 query blocks this launch stays on attn_kernel's 4-wave form: the launcher takes
    #  the DMA-staged kernel from 1024 query blocks of 256 on.  The two cases after it are the ones that reach it.)
    "fwd_n1024_plain": ("fwd", 1, 2, 1024, True, "plain", 11),
    "fwd_n1024_spread": ("fwd", 1, 2, 1024, True, "spread", 12),
    # the DMA-staged kernel at its smallest N: 4 tiles of 256 keys, 8 x 32 x 4 = 1024 workgroups
    "fwd_dma_plain": ("fwd", 8, 32, 1024, True, "plain", 13),
    "fwd_dma_spread": ("fwd", 8, 32, 1024, True, "spread", 14),
    # attn_kernel, ragged masked keys, the exact-maximum path
    "fwd_n300_plain": ("fwd", 2, 2, 300, False, "plain", 15),
    "fwd_n300_spread": ("fwd", 2, 2, 300, False, "spread", 16),
    "bwd_n256_plain": ("bwd", 1, 2, 256, False, "plain", 17),
    "bwd_n256_spread": ("bwd", 1, 2, 256, False, "spread", 18),
    "bwd_n300_plain": ("bwd", 1, 2, 300, False, "plain", 19),
    "bwd_n300_spread": ("bwd", 1, 2, 300, False, "spread", 20),
}
SAMPLE_ABOVE = 65536          # outputs with more elements are stored as a fixed sample plus the sha256 of all of them


def _signed_perms(g, shape):
    """Rows that are signed permutations of MAGS: argsort of seeded uniforms (no ties in practice) and seeded signs."""
    order = torch.rand(*shape, 8, generator=g).argsort(-1)
    sign = torch.randint(0, 2, (*shape, 8), generator=g).float() * 2 - 1
    return MAGS[order] * sign


def make_inputs(name):
    """CPU bf16 tensors: q, k, v [B][heads][N][8] (+ dout [B][N][heads * 8] for the backward cases)."""
    kind, B, heads, N, _, inputs, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    if inputs == "plain":
        q, k, v = (torch.randn(B, heads, N, 8, generator=g) * 1.5 for _ in range(3))
    else:
        proto = _signed_perms(g, (B, heads, 16))                                      # [B][heads][16][8]
        which = torch.randint(0, 16, (B, heads, N), generator=g)
        q = torch.gather(proto, 2, which[..., None].expand(B, heads, N, 8)) + 0.125 * torch.randn(B, heads, N, 8, generator=g)
        k = _signed_perms(g, (B, heads, N))
        k[:, :, :32] = torch.cat([proto, proto], 2)
        v = torch.randn(B, heads, N, 8, generator=g)
    t = {"q": q.to(torch.bfloat16), "k": k.to(torch.bfloat16), "v": v.to(torch.bfloat16)}
    if kind == "bwd":
        t["dout"] = torch.randn(B, N, heads * 8, generator=g).to(torch.bfloat16)
    return t


def inputs_sha256(t):
    h = hashlib.sha256()
    for key in sorted(t):
        h.update(t[key].contiguous().view(torch.int16).numpy().tobytes())
    return h.hexdigest()


def kmax2_of(k):
    """max |k|^2 per (sample, head): fp64 sums of squares of bf16 values are exact, so the fp32 slot is the same on every host."""
    return (k.double() ** 2).sum(-1).amax(-1).float().contiguous()


def band_count(name, t):
    """fp64 restatement: how many probabilities of this case lie in 2^-125.5 .. 2^-119.5 whichever reference maximum the kernel holds
    at that key.  Forward: the reference is at least the maximum over keys 0..31 and at most the row maximum; backward: it is the
    log-sum-exp (p = 2^(s - lse))."""
    kind = CASES[name][0]
    qs = (t["q"].float() * QSCALE).to(torch.bfloat16).double()                       # the kernels round the scaled q to bf16
    s = torch.einsum("bhqd,bhkd->bhqk", qs, t["k"].double())
    if kind == "bwd":
        lse = torch.logsumexp(s * 0.6931471805599453, -1, keepdim=True) * 1.4426950408889634
        lo = hi = lse
    else:
        lo, hi = s[..., :32].amax(-1, keepdim=True), s.amax(-1, keepdim=True)
    return int(((s - lo < -119.5) & (s - hi >= -125.5)).sum())


def run_case(L, lib, name, t, dev):
    """Launch the case on ``dev``; returns {array name: CPU integer-view tensor} of everything the kernels wrote."""
    kind, B, heads, N, with_kmax2, _, _ = CASES[name]
    Cc = heads * 8
    st = torch.cuda.current_stream().cuda_stream
    Q, K, V = (t[x].to(dev).contiguous() for x in "qkv")
    out = torch.full((B, N, Cc), float("nan"), dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, heads, N), float("nan"), device=dev)
    km = kmax2_of(t["k"]).to(dev) if with_kmax2 else None
    a = L.AttnArgs(dtype=1, B=B, heads=heads, N=N, q=Q.data_ptr(), k=K.data_ptr(), v=V.data_ptr(), out=out.data_ptr(), lse=lse.data_ptr(),
                   kmax2=L.ptr(km))
    L.check(lib.pd_attn_d8(C.byref(a), st), "pd_attn_d8")
    torch.cuda.synchronize()
    got = {"out": out.view(torch.int16).cpu(), "lse": lse.view(torch.int32).cpu()}
    if kind == "bwd":
        DO = t["dout"].to(dev).contiguous()
        delta = torch.full((B, heads, N), float("nan"), device=dev)
        dqkv = torch.full((B, N, 3 * Cc), float("nan"), dtype=torch.bfloat16, device=dev)
        b = L.AttnBwdArgs(dtype=1, B=B, heads=heads, N=N, q=Q.data_ptr(), k=K.data_ptr(), v=V.data_ptr(), o=out.data_ptr(),
                          dout=DO.data_ptr(), lse=lse.data_ptr(), delta=delta.data_ptr(), dqkv=dqkv.data_ptr())
        L.check(lib.pd_attn_d8_bwd(C.byref(b), st), "pd_attn_d8_bwd")
        torch.cuda.synchronize()
        got["dqkv"] = dqkv.view(torch.int16).cpu()
        got["delta"] = delta.view(torch.int32).cpu()
    return got


def stored_form(got):
    """What a fixture keeps of ``run_case``'s result: small arrays whole; of a large one the sha256 and every 127th element."""
    kept = {}
    for key, v in got.items():
        a = v.contiguous().numpy()
        if a.size > SAMPLE_ABOVE:
            kept[key + "__sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            kept[key + "__sample127"] = a.reshape(-1)[::127].copy()
        else:
            kept[key] = a
    return kept


def fixture_path(name):
    return os.path.join(GOLDEN, name + ".npz")
