"""Cases, seeded inputs, launch helper and fp64 restatements shared by tests/test_gpu_attn_d8_resident3_bits.py and
scripts/record_attn_d8_bits.py (``--cases attn_d8_resident3_cases``): the paths of pd_attn_d8's DMA-staged bf16 kernel that the cases of
tests/attn_d8_bits_cases.py do not pin -- the exact running-maximum path with rescales, its hand-over to the check-free run inside one
wave, the ragged last tile, the ``lse`` output and the safety net behind a wrong ``kmax2`` slot.  Outputs are compared BIT FOR BIT with
what a library built from the revision before the kernel was fitted into 80 registers wrote (tests/golden/attn_d8_resident3_bits/).

All cases: bf16, B = 8, 32 heads, N = 1100 (five query blocks of 256 -> 1280 workgroups of 8 waves, the smallest launch the launcher
gives to attn_glds_kernel with a ragged N: four full key tiles and one of 76 keys, whose third 32-key sub-tile has 12 keys to mask;
queries 1100..1279 of the last block are not stored), ``kmax2`` supplied.

``ragged``      plain inputs (randn * 1.5).  About 40 % of the waves run the four full tiles check-free, the others exact (their bound is
                not met; one rescale at most), all of them the last tile exact with keys masked.
``never``       key norms grow along the sequence (x 1 .. x 4) and the supplied kmax2 is 16 x the true maximum (a valid bound, only a loose
                one): |q| max|k| - m > THR holds to the end for every wave, every tile runs exact, every wave rescales o at least twice.
``transition``  rows of equal norm as in the ``spread`` inputs of attn_d8_bits_cases; the key that matches a query's prototype (score within
                a few units of the bound) sits in tile 0, 1 or 2 depending on the wave (global wave index mod 3), and never among the
                first 32 keys.  A wave runs exact until its prototypes have passed, then check-free, then the ragged tile: loops 1 -> 2 -> 3
                of the kernel in one wave, neighbouring waves of a workgroup switching at different tiles.  ``lse`` requested.
``safety_net``  plain inputs, but the kmax2 slot of (sample 3, head 5) is 0 (a stale slot): the first sub-tile's maximum exceeds the
                "bound", those waves keep the exact path for the whole launch; all other (sample, head) behave as in ``ragged``.
                ``lse`` requested."""
import ctypes as C
import hashlib
import os

import numpy as np
import torch

from attn_d8_bits_cases import MAGS, QSCALE, _signed_perms, inputs_sha256, kmax2_of, stored_form  # noqa: F401  (re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_d8_resident3_bits")
B, HEADS, N = 8, 32, 1100
KT, THR = 256, 16.0                     # keys per staged tile; the bf16 rescale threshold (log2 domain)
NT = (N + KT - 1) // KT                 # 5 tiles, the last one ragged
NQB = (N + 255) // 256                  # query blocks of 8 waves x 32 queries
BAD_SLOT = (3, 5)                       # (sample, head) whose kmax2 slot is zeroed in ``safety_net``
TOL = 8e-3                              # relative L2 against fp64: tests/test_gpu_kernels.py ATTN_D8_TOL["bf16"]

# name -> (inputs, seed, lse requested)
CASES = {
    "ragged": ("plain", 31, False),
    "never": ("ramp", 32, False),
    "transition": ("handover", 33, True),
    "safety_net": ("plain", 34, True),
}


def make_inputs(name):
    """CPU bf16 tensors q, k, v [B][heads][N][8]: element-wise operations on seeded CPU draws only."""
    inputs, seed, _ = CASES[name]
    g = torch.Generator().manual_seed(seed)
    if inputs == "plain":
        q, k, v = (torch.randn(B, HEADS, N, 8, generator=g) * 1.5 for _ in range(3))
    elif inputs == "ramp":
        q, k, v = (torch.randn(B, HEADS, N, 8, generator=g) * 1.5 for _ in range(3))
        k = k * (1.0 + 3.0 * torch.arange(N).float() / (N - 1))[:, None]
    else:
        proto = _signed_perms(g, (B, HEADS, 15))                                         # [B][heads][15][8], |row| = 15.9
        # queries of global wave w (32 consecutive queries) sit near prototypes 5 (w % 3) .. 5 (w % 3) + 4
        group = (torch.arange(N) // 32) % 3
        which = group * 5 + torch.randint(0, 5, (B, HEADS, N), generator=g)
        q = torch.gather(proto, 2, which[..., None].expand(B, HEADS, N, 8)) + 0.125 * torch.randn(B, HEADS, N, 8, generator=g)
        k = _signed_perms(g, (B, HEADS, N))
        for grp in range(3):                                                             # group g's prototypes are keys of tile g
            k[:, :, 256 * grp + 40:256 * grp + 45] = proto[:, :, 5 * grp:5 * grp + 5]
        v = torch.randn(B, HEADS, N, 8, generator=g)
    return {"q": q.to(torch.bfloat16), "k": k.to(torch.bfloat16), "v": v.to(torch.bfloat16)}


def kmax2_slots(name, t):
    """The kmax2 array handed to the kernel."""
    km = kmax2_of(t["k"])
    if name == "never":
        km = km * 16.0
    if name == "safety_net":
        km[BAD_SLOT] = 0.0
    return km.contiguous()


def scores(t, b):
    """fp64 log2-domain scores [heads][N][N] of sample b as the kernel forms them (it rounds the scaled q to bf16)."""
    qs = (t["q"][b].float() * QSCALE).to(torch.bfloat16).double()
    return torch.einsum("hqd,hkd->hqk", qs, t["k"][b].double()), qs


def simulate(name, t, thr=THR):
    """fp64 restatement of the kernel's per-wave decisions.  Returns (fast [B][heads][waves][NT] bool: the tile ran check-free,
    rescales [B][heads][waves]: how often the wave rescaled o, tripped [B][heads][waves]: the safety net fired in the wave)."""
    km = kmax2_slots(name, t).double()
    nw = NQB * 8
    fast = torch.zeros(B, HEADS, nw, NT, dtype=torch.bool)
    rescales = torch.zeros(B, HEADS, nw, dtype=torch.int64)
    tripped = torch.zeros(B, HEADS, nw, dtype=torch.bool)
    qidx = torch.arange(nw * 32).clamp(max=N - 1)                 # lanes past N hold the last query
    for b in range(B):
        s, qs = scores(t, b)
        s = s[:, qidx]                                            # [heads][nw * 32][N]
        qn = qs.pow(2).sum(-1).sqrt()[:, qidx] * 1.00001 + 1e-6
        bound = qn * (km[b].sqrt() * 1.00002)[:, None]
        m = s[..., :32].amax(-1)
        trip = m > bound
        bound = torch.where(trip, torch.full_like(bound, float("inf")), bound)
        tripped[b] = trip.view(HEADS, nw, 32).any(-1)
        for ti in range(NT):
            k0 = ti * KT
            need = (bound - m > thr).view(HEADS, nw, 32).any(-1)
            f = ~need if k0 + KT <= N else torch.zeros_like(need)
            fast[b, :, :, ti] = f
            for kb in range(k0, min(k0 + KT, N), 32):
                need = (bound - m > thr).view(HEADS, nw, 32).any(-1) & ~f
                t2 = s[..., kb:min(kb + 32, N)].amax(-1) - m
                resc = need & (t2 > thr).view(HEADS, nw, 32).any(-1)
                m = torch.where(resc[..., None].expand(HEADS, nw, 32).reshape(HEADS, nw * 32), m + t2.clamp(min=0.0), m)
                rescales[b] += resc
    return fast, rescales, tripped


def check_paths(name, t):
    """Does the case reach the path it is named for?  Asserted at recording time, at the threshold and a hair to either side of it (an fp32
    decision within 0.01 of the threshold could fall the other way on the GPU).  Returns a one-line summary."""
    out = []
    for thr in (THR - 0.01, THR, THR + 0.01):
        fast, resc, trip = simulate(name, t, thr)
        assert not fast[..., NT - 1].any(), "the ragged tile runs exact"
        nv = (N + 31) // 32                      # waves that hold a query below N; the other five of the last block repeat query N - 1
        full, resc = fast[..., :nv, :NT - 1], resc[..., :nv]
        mono = (full[..., 1:] | ~full[..., :-1]).all()
        assert mono, "once check-free, every later full tile is check-free"
        if name == "ragged":
            assert not trip.any()
            share = float(full.all(-1).float().mean())
            assert 0.25 < share < 0.75, f"both kinds of wave: {share:.2f} of them run every full tile check-free, the others exact"
        elif name == "never":
            assert not trip.any()
            assert not full.any(), "no tile of any wave satisfies the bound"
            assert int(resc.min()) >= 2, f"every wave rescales at least twice (min {int(resc.min())})"
        elif name == "transition":
            assert not trip.any()
            first = torch.where(full.any(-1), full.float().argmax(-1), torch.full((), NT - 1))   # index of the first check-free tile
            want = torch.arange(nv) % 3 + 1                                  # group g: tiles 0..g exact, then check-free
            hit = float((first == want).float().mean())
            assert hit > 0.99, f"wave w hands over after tile w % 3: only {hit:.4f} of the waves do"
            assert not full[..., 0].any() and int(resc.min()) >= 1, "every wave starts exact and rescales there"
        elif name == "safety_net":
            bad = torch.zeros(B, HEADS, dtype=torch.bool)
            bad[BAD_SLOT] = True
            assert trip[bad].all() and not trip[~bad].any(), "the safety net fires in every wave of the zeroed slot and nowhere else"
            assert not full[bad].any(), "those waves keep the exact path for the whole launch"
            assert full[~bad].all(-1).float().mean() > 0.25
        out.append(f"thr {thr:.2f}: check-free {int(full.sum())} of {full.numel()} full tiles, rescales per wave {int(resc.min())}..{int(resc.max())}, "
                   f"tripped waves {int(trip.sum())}")
    return "; ".join(out)


def reference(t, dev):
    """fp64 attention of the inputs (exact scale, no rounding of q): out [B][N][heads * 8], lse [B][heads][N] in the log2 domain."""
    outs, lses = [], []
    for b in range(B):
        q, k, v = (t[x][b].to(dev).double() for x in "qkv")
        s = torch.einsum("hqd,hkd->hqk", q, k) * QSCALE
        lse = torch.logsumexp(s * 0.6931471805599453, -1) * 1.4426950408889634
        p = torch.exp2(s - lse[..., None])
        outs.append(torch.einsum("hqk,hkd->qhd", p, v).reshape(N, HEADS * 8))
        lses.append(lse)
    return torch.stack(outs).cpu(), torch.stack(lses).cpu()


def run_case(L, lib, name, t, dev):
    """Launch the case on ``dev``; returns {array name: CPU integer-view tensor} of everything the kernel wrote."""
    want_lse = CASES[name][2]
    st = torch.cuda.current_stream().cuda_stream
    Q, K, V = (t[x].to(dev).contiguous() for x in "qkv")
    out = torch.full((B, N, HEADS * 8), float("nan"), dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, HEADS, N), float("nan"), device=dev) if want_lse else None
    km = kmax2_slots(name, t).to(dev)
    a = L.AttnArgs(dtype=1, B=B, heads=HEADS, N=N, q=Q.data_ptr(), k=K.data_ptr(), v=V.data_ptr(), out=out.data_ptr(), lse=L.ptr(lse),
                   kmax2=L.ptr(km))
    L.check(lib.pd_attn_d8(C.byref(a), st), "pd_attn_d8")
    torch.cuda.synchronize()
    got = {"out": out.view(torch.int16).cpu()}
    if want_lse:
        got["lse"] = lse.view(torch.int32).cpu()
    return got


def fixture_path(name):
    return os.path.join(GOLDEN, name + ".npz")
