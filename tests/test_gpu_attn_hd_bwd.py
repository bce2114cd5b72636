"""pd_attn_hd for head_dim 16 / 32 and its backward pd_attn_hd_bwd on MI355X: parity with F.scaled_dot_product_attention and
torch.autograd over it in fp32 on the CPU (on the engine-rounded inputs), run-to-run determinism, guard bands (tests/guard_bands.py
through the engine of tests/test_gpu_guard_bands.py) and graph capture.

The forward runs the helpers of tests/test_gpu_attn_hd.py over that file's own cases and bounds.  The backward's bounds are the
project's own for this arithmetic (16-bit or exact-fp32 MFMA products, fp32 accumulation, P and dS rounded to the storage type before
the second product): ATTN_D64_BWD_TOL for f32 / bf16, ATTN_WIDE_BWD_TOL for fp16 -- imported, not restated.

A gradient that is mathematically zero has no relative error: with ONE key the softmax is constant, so autograd's dq and dk are exactly
0 while the kernel leaves the fp32 round-off of dP - delta (two sums of the same products in different orders).  Such a tensor is held
to the rule of tests/test_gpu_unet_backward.py::compare: where the reference's norm is below 1e-6 of the whole gradient's norm
(dq, dk, dv together), the absolute error must stay below 1e-5 of that norm (fp32 round-off of a D-term sum is ~1e-7 of it)."""
import ctypes as C

import pytest
import torch

import test_gpu_attn_hd as H
from guard_bands import guard_size
from test_gpu_guard_bands import Case, Op, out_op, p1_poisoned_surroundings, p2_canaried_outputs, p3_sample_isolation
from test_gpu_kernels import DT, bf16_round, env, rel, stream  # noqa: F401
from test_gpu_sd_kernels import ATTN_D64_BWD_TOL
from test_gpu_vae import ATTN_WIDE_BWD_TOL

pytestmark = pytest.mark.gpu

DIMS = (16, 32)
MODES = ("f32", "bf16", "fp16")
BWD_TOL = dict(ATTN_D64_BWD_TOL, fp16=ATTN_WIDE_BWD_TOL["fp16"])
# ragged tiles, one tile and several, more than one workgroup per head, single elements
BWD_CASES = [(2, 2, 256, 256), (2, 3, 200, 77), (1, 1, 16, 16), (2, 2, 130, 4), (1, 2, 1, 1), (1, 2, 333, 517)]


# ---- forward, D = 16 / 32: the helpers of tests/test_gpu_attn_hd.py --------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("cfg", H.PARITY_CASES)
def test_attention_hd_16_32(env, mode, D, cfg):
    H.test_attention_hd(env, mode, D, cfg)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("hazard", ["rising", "late_spike", "all_equal"])
def test_attention_hd_16_32_softmax_hazards(env, mode, D, hazard):
    H.test_attention_hd_softmax_hazards(env, mode, D, hazard)           # N = 320


# ---- backward --------------------------------------------------------------------------------------------------------------------------
def forward(L, lib, code, B, heads, D, Nq, Nkv, qp, qs, kp, vp, kvs, out, out_stride, lse):
    H.launch(L, lib, code, B, heads, D, Nq, Nkv, qp, qs, kp, vp, kvs, out, out_stride, lse)


def backward(L, lib, code, B, heads, D, Nq, Nkv, qp, qs, kp, vp, kvs, o, dout, o_stride, lse, delta, dq, dqs, dk, dv, dkvs):
    a = L.AttnHdBwdArgs(dtype=code, B=B, heads=heads, D=D, Nq=Nq, Nkv=Nkv, scale=float(D) ** -0.5, q=qp, q_stride=qs, k=kp, v=vp,
                        kv_stride=kvs, o=o, dout=dout, o_stride=o_stride, lse=lse, delta=delta, dq=dq, dq_stride=dqs, dk=dk, dv=dv,
                        dkv_stride=dkvs)
    L.check(lib.pd_attn_hd_bwd(C.byref(a), stream()), "pd_attn_hd_bwd")


class Problem:
    """One (engine, D, shape): engine-rounded inputs on the host, the same on the device, and autograd's dq / dk / dv (computed once).
    Self layout (Nq == Nkv): q | k | v are slices of one fused [B][N][3C] tensor and dq | dk | dv of one fused gradient; cross layout:
    q [B][Nq][C], fused k | v [B][Nkv][2C], dq and a fused dk | dv."""

    def __init__(self, mode, D, cfg, dev, seed=51):
        self.mode, self.D, self.cfg = mode, D, cfg
        self.code, self.tdt = DT[mode]
        B, heads, Nq, Nkv = cfg
        Cc = self.Cc = heads * D
        self.self_layout = Nq == Nkv
        g = torch.Generator().manual_seed(seed)
        if self.self_layout:
            qkv = bf16_round(torch.randn(B, Nq, 3 * Cc, generator=g), mode).requires_grad_()
            q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        else:
            q = bf16_round(torch.randn(B, Nq, Cc, generator=g), mode).requires_grad_()
            kv = bf16_round(torch.randn(B, Nkv, 2 * Cc, generator=g), mode).requires_grad_()
            k, v = kv[..., :Cc], kv[..., Cc:]
        self.do = bf16_round(torch.randn(B, Nq, Cc, generator=g), mode)
        H.sdpa(q, k, v, B, heads, D, Nq, Nkv).backward(self.do)
        if self.self_layout:
            self.host = {"qkv": qkv.detach()}
            self.ref = {"dq": qkv.grad[..., :Cc], "dk": qkv.grad[..., Cc:2 * Cc], "dv": qkv.grad[..., 2 * Cc:]}
        else:
            self.host = {"q": q.detach(), "kv": kv.detach()}
            self.ref = {"dq": q.grad, "dk": kv.grad[..., :Cc], "dv": kv.grad[..., Cc:]}
        self.gnorm = float(sum(t.double().pow(2).sum() for t in self.ref.values()) ** 0.5)
        self.dev_in = {n: t.to(self.tdt).to(dev).contiguous() for n, t in self.host.items()}
        self.DO = self.do.to(self.tdt).to(dev)

    def pointers(self, T, pad=0):
        """(q, q_stride, k, v, kv_stride) of the input tensors `T` whose rows are `pad` elements wider than their contents."""
        Cc = self.Cc
        if self.self_layout:
            p, esz = T["qkv"].data_ptr(), T["qkv"].element_size()
            return p, 3 * Cc + pad, p + Cc * esz, p + 2 * Cc * esz, 3 * Cc + pad
        esz = T["kv"].element_size()
        return T["q"].data_ptr(), Cc + pad, T["kv"].data_ptr(), T["kv"].data_ptr() + Cc * esz, 2 * Cc + pad

    def grad_shapes(self):
        B, heads, Nq, Nkv = self.cfg
        return {"dqkv": (B, Nq, 3 * self.Cc)} if self.self_layout else {"dq": (B, Nq, self.Cc), "dkv": (B, Nkv, 2 * self.Cc)}

    def grad_pointers(self, G, pad=0):
        """(dq, dq_stride, dk, dv, dkv_stride) of the gradient tensors `G`."""
        Cc = self.Cc
        if self.self_layout:
            p, esz = G["dqkv"].data_ptr(), G["dqkv"].element_size()
            return p, 3 * Cc + pad, p + Cc * esz, p + 2 * Cc * esz, 3 * Cc + pad
        esz = G["dkv"].element_size()
        return G["dq"].data_ptr(), Cc + pad, G["dkv"].data_ptr(), G["dkv"].data_ptr() + Cc * esz, 2 * Cc + pad

    def split(self, G):
        Cc = self.Cc
        if self.self_layout:
            return {"dq": G["dqkv"][..., :Cc], "dk": G["dqkv"][..., Cc:2 * Cc], "dv": G["dqkv"][..., 2 * Cc:]}
        return {"dq": G["dq"], "dk": G["dkv"][..., :Cc], "dv": G["dkv"][..., Cc:]}

    def run_forward(self, env_):
        L, lib, _, dev = env_
        B, heads, Nq, Nkv = self.cfg
        o = torch.full((B, Nq, self.Cc), float("nan"), dtype=self.tdt, device=dev)
        lse = torch.full((B, heads, Nq), float("nan"), dtype=torch.float32, device=dev)
        forward(L, lib, self.code, B, heads, self.D, Nq, Nkv, *self.pointers(self.dev_in), o, self.Cc, lse)
        return o, lse

    def run_backward(self, env_, o, lse, G, delta):
        L, lib, _, dev = env_
        B, heads, Nq, Nkv = self.cfg
        backward(L, lib, self.code, B, heads, self.D, Nq, Nkv, *self.pointers(self.dev_in), o.data_ptr(), self.DO.data_ptr(), self.Cc,
                 lse.data_ptr(), delta.data_ptr(), *self.grad_pointers(G))

    def new_grads(self, dev):
        B, heads, Nq, _ = self.cfg
        G = {n: torch.full(s, float("nan"), dtype=self.tdt, device=dev) for n, s in self.grad_shapes().items()}
        return G, torch.full((B, heads, Nq), float("nan"), dtype=torch.float32, device=dev)

    def check(self, got, what=""):
        tol = BWD_TOL[self.mode]
        for n, ref in self.ref.items():
            g = got[n].float().cpu()
            assert bool(torch.isfinite(g).all()), (n, what)
            if float(ref.norm()) > 1e-6 * self.gnorm:
                err = rel(g, ref)
                print(f"pd_attn_hd_bwd {self.mode} D={self.D} {self.cfg} {what}{n}: {err:.3e}")
                assert err < tol, (n, err)
            else:           # mathematically zero (one key: the softmax is constant): round-off only -- see the module docstring
                err = float((g - ref).norm()) / self.gnorm
                print(f"pd_attn_hd_bwd {self.mode} D={self.D} {self.cfg} {what}{n}: zero reference, |error| / |gradient| {err:.3e}")
                assert err < 1e-5, (n, err)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("cfg", BWD_CASES)
def test_attention_hd_backward(env, mode, D, cfg):
    dev = env[3]
    pr = Problem(mode, D, cfg, dev)
    o, lse = pr.run_forward(env)
    G, delta = pr.new_grads(dev)
    pr.run_backward(env, o, lse, G, delta)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in G.values()) and bool(torch.isfinite(delta).all())      # every element written
    pr.check(pr.split(G))
    # run-to-run determinism: no atomics, every reduction lane-local
    G2, delta2 = pr.new_grads(dev)
    pr.run_backward(env, o, lse, G2, delta2)
    torch.cuda.synchronize()
    assert all(torch.equal(G[n], G2[n]) for n in G) and torch.equal(delta, delta2)


# ---- guard bands -------------------------------------------------------------------------------------------------------------------------
# Forward: the cases of tests/test_gpu_attn_hd.py (a cross case with Nkv = 77 and a self case; every row 64 elements wider than its contents).
FWD_GUARD_PARAMS = [(D, k, m) for D in DIMS for k in H.GUARD_CASES for m in MODES]


@pytest.mark.parametrize("D,key,mode", FWD_GUARD_PARAMS)
def test_attn_hd_16_32_p1_poisoned_surroundings(env, monkeypatch, D, key, mode):
    p1_poisoned_surroundings(H.attn_hd_case(env, mode, D, key), env[3], monkeypatch)


@pytest.mark.parametrize("D,key,mode", FWD_GUARD_PARAMS)
def test_attn_hd_16_32_p2_canaried_outputs(env, monkeypatch, D, key, mode):
    p2_canaried_outputs(H.attn_hd_case(env, mode, D, key), env[3], monkeypatch)


@pytest.mark.parametrize("D,key,mode", [p for p in FWD_GUARD_PARAMS if H.GUARD_CASES[p[1]][0][0] > 1])
def test_attn_hd_16_32_p3_sample_isolation(env, monkeypatch, D, key, mode):
    p3_sample_isolation(H.attn_hd_case(env, mode, D, key), env[3], monkeypatch)


# Backward.  Every operand with channels (q / kv / qkv, o, dout, dq / dkv / dqkv) has rows 64 elements wider than its contents: the gap
# columns are NaN in P1 (inputs: with D = 16 the pad pieces of the last head would read them) and canary in P2 (outputs: a pad channel
# stored would land there).  Guards: 128 rows (two 64-row tiles) of the operand's row stride, >= 64 KiB, before and after.
BWD_GUARD_CASES = {"cross-B2-h2-130x77": (2, 2, 130, 77), "self-B2-h3-72": (2, 3, 72, 72)}
PAD = 64


def attn_hd_bwd_case(env_, mode, D, key):
    L, lib, _, dev = env_
    cfg = BWD_GUARD_CASES[key]
    B, heads, Nq, Nkv = cfg
    pr = Problem(mode, D, cfg, dev, seed=151)
    Cc, tdt, code = pr.Cc, pr.tdt, pr.code
    o, lse = pr.run_forward(env_)        # o and lse as the forward leaves them (plain allocations: the forward has its own cases above)
    torch.cuda.synchronize()
    ins = {n: Op(t.to(tdt), guard_size(64, t.shape[-1] + PAD, tdt), stride=t.shape[-1] + PAD, sample_dim=0) for n, t in pr.host.items()}
    ins["o"] = Op(o.cpu(), guard_size(64, Cc + PAD, tdt), stride=Cc + PAD, sample_dim=0)
    ins["dout"] = Op(pr.do.to(tdt), guard_size(64, Cc + PAD, tdt), stride=Cc + PAD, sample_dim=0)
    ins["lse"] = Op(lse.cpu(), sample_dim=0)
    outs = {n: out_op(s, tdt, guard=guard_size(64, s[-1] + PAD, tdt), stride=s[-1] + PAD, sample_dim=0) for n, s in pr.grad_shapes().items()}
    outs["delta"] = out_op((B, heads, Nq), torch.float32, sample_dim=0)

    def run(T):
        assert all(T[n].stride(-2) == T[n].shape[-1] + PAD for n in T if n not in ("lse", "delta"))
        backward(L, lib, code, B, heads, D, Nq, Nkv, *pr.pointers(T, PAD), T["o"].data_ptr(), T["dout"].data_ptr(), Cc + PAD,
                 T["lse"].data_ptr(), T["delta"].data_ptr(), *pr.grad_pointers(T, PAD))

    return Case(ins, outs, run, lambda O: pr.check(pr.split(O), "guarded "), nsamples=B)


BWD_GUARD_PARAMS = [(D, k, m) for D in DIMS for k in BWD_GUARD_CASES for m in MODES]


@pytest.mark.parametrize("D,key,mode", BWD_GUARD_PARAMS)
def test_attn_hd_bwd_p1_poisoned_surroundings(env, monkeypatch, D, key, mode):
    p1_poisoned_surroundings(attn_hd_bwd_case(env, mode, D, key), env[3], monkeypatch)


@pytest.mark.parametrize("D,key,mode", BWD_GUARD_PARAMS)
def test_attn_hd_bwd_p2_canaried_outputs(env, monkeypatch, D, key, mode):
    p2_canaried_outputs(attn_hd_bwd_case(env, mode, D, key), env[3], monkeypatch)


@pytest.mark.parametrize("D,key,mode", BWD_GUARD_PARAMS)
def test_attn_hd_bwd_p3_sample_isolation(env, monkeypatch, D, key, mode):
    p3_sample_isolation(attn_hd_bwd_case(env, mode, D, key), env[3], monkeypatch)


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_attn_hd_forward_backward_graph_replay_is_bit_identical(env, D):
    L, lib, _, dev = env
    pr = Problem("bf16", D, (2, 2, 200, 200), dev, seed=5)
    B, heads, Nq, Nkv = pr.cfg

    def buffers():
        o = torch.full((B, Nq, pr.Cc), float("nan"), dtype=pr.tdt, device=dev)
        lse = torch.full((B, heads, Nq), float("nan"), dtype=torch.float32, device=dev)
        return (o, lse) + pr.new_grads(dev)

    def pair(o, lse, G, delta):
        forward(L, lib, pr.code, B, heads, D, Nq, Nkv, *pr.pointers(pr.dev_in), o, pr.Cc, lse)
        pr.run_backward(env, o, lse, G, delta)

    eager = buffers()
    pair(*eager)
    torch.cuda.synchronize()
    got = buffers()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair(*got)
    for t in (got[0], got[1], got[3], *got[2].values()):
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    assert torch.equal(bits(got[0]), bits(eager[0])) and torch.equal(bits(got[1]), bits(eager[1])) and torch.equal(bits(got[3]), bits(eager[3]))
    assert all(torch.equal(bits(got[2][n]), bits(eager[2][n])) for n in eager[2])
    assert bool(torch.isfinite(got[2]["dqkv"]).all())
