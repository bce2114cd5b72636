"""Case generators for the fp16 backward kernels under the loss scale: seeded inputs (exact in fp16) and a plain-torch fp64 reference, one
function per kernel.  Every kernel here is linear in its incoming gradient(s), so the reference at a gain G is G times the unit one.

A Case holds
  inputs   name -> fp32 tensor holding fp16-exact values, in the layout torch's reference ops use (NCHW, [B][heads][N][d], [rows][C])
  grads    the names in `inputs` that are incoming gradients (multiplied by the gain)
  ref      name -> fp64 reference output at unit gain
  kept     name -> fp64 tensor, at unit gain, of every gain-scaled value the kernel holds in fp16 besides its incoming gradients: the stored
           16-bit outputs and, for the attention backwards, dP - delta per (query, key), which bounds |dS| since p <= 1
  meta     shape parameters the launcher needs

tests/test_host_fp16_backward_cases.py checks on the CPU that nothing of this reaches 2^15 at GAIN (so the gain cannot hide a saturation the
reference itself would have); tests/test_gpu_fp16_backward.py runs the kernels at gain 1 and GAIN."""
import torch
import torch.nn.functional as F

GAIN = 256.0
FP16_LIMIT = 2.0 ** 15


class Case:
    def __init__(self, name, inputs, grads, ref, kept, **meta):
        self.name, self.inputs, self.grads, self.ref, self.kept, self.meta = name, inputs, tuple(grads), ref, kept, meta

    def scaled_inputs(self, gain):
        """The inputs with every incoming gradient multiplied by `gain` (a power of two: still exact in fp16 unless it overflows)."""
        return {k: (v * gain if k in self.grads else v) for k, v in self.inputs.items()}


def h(t):
    return t.half().float()


def _randn(g, *shape, std=1.0, mean=0.0):
    return h(torch.randn(*shape, generator=g) * std + mean)


# ---- pd_conv_wgrad --------------------------------------------------------------------------------------------------------------------------------
CONV_WGRAD = {"3x3-s1-B2-192to32-20x12": dict(B=2, cin=192, cout=32, H=20, W=12, ksize=3, stride=1),
              "3x3-s2-B2-64to96-16x48": dict(B=2, cin=64, cout=96, H=16, W=48, ksize=3, stride=2),
              "1x1-B2-128to384-8x8": dict(B=2, cin=128, cout=384, H=8, W=8, ksize=1, stride=1),
              "phases-B1-96to128-33x40": dict(B=1, cin=96, cout=128, H=33, W=40, ksize=3, stride=1, phases=True),
              "fused-silu-affine-concat-B2-64+32to64-24x16": dict(B=2, cin=96, c1=32, cout=64, H=24, W=16, ksize=3, stride=1, fused=True)}


def conv_wgrad(key):
    m = CONV_WGRAD[key]
    B, cin, cout, H, W, ks, stride = (m[k] for k in ("B", "cin", "cout", "H", "W", "ksize", "stride"))
    g = torch.Generator().manual_seed(201)
    x = _randn(g, B, cin, H, W)
    inputs = {"x": x}
    z = x.double()
    if m.get("fused"):        # the staged operand silu(x * scale_n + shift_n) is rounded to fp16 before the MFMA (the kernel's documented rounding point)
        inputs["scale"], inputs["shift"] = torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g) * 0.3
        z = F.silu(z * inputs["scale"].double()[:, :, None, None] + inputs["shift"].double()[:, :, None, None]).half().double()
    if m.get("phases"):       # Upsample2D: the conv runs on the nearest x2 upsampled tensor
        z = F.interpolate(z, scale_factor=2.0, mode="nearest")
    pad = ks // 2
    ho, wo = (z.shape[2] + 2 * pad - ks) // stride + 1, (z.shape[3] + 2 * pad - ks) // stride + 1
    inputs["dy"] = _randn(g, B, cout, ho, wo)
    w = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    (dw,) = torch.autograd.grad(F.conv2d(z, w, None, stride=stride, padding=pad), w, inputs["dy"].double())
    return Case("pd_conv_wgrad-" + key, inputs, ["dy"], {"dw": dw}, {}, **m)


# ---- attention backward ---------------------------------------------------------------------------------------------------------------------------
def _attention_reference(q, k, v, dout):
    """q [B][h][Nq][d], k / v [B][h][Nkv][d], dout [B][h][Nq][d], all fp64 -> dq, dk, dv, dP - delta."""
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    p = torch.softmax(q @ k.transpose(-1, -2) / q.shape[-1] ** 0.5, -1)
    o = p @ v
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), dout)
    ds_bound = dout @ v.detach().transpose(-1, -2) - (dout * o.detach()).sum(-1, keepdim=True)
    return dq, dk, dv, ds_bound


ATTN_D8_BWD = {"two-kernel-B1-h3-300": dict(B=1, heads=3, N=300, onepass=False),
               "one-pass-B1-h2-1300-slab": dict(B=1, heads=2, N=1300, onepass=True)}       # three ragged key blocks


def attn_d8_bwd(key):
    m = ATTN_D8_BWD[key]
    B, heads, N = m["B"], m["heads"], m["N"]
    g = torch.Generator().manual_seed(202)
    q, k, v = (_randn(g, B, heads, N, 8, std=1.2) for _ in range(3))
    dout = _randn(g, B, N, heads * 8)
    dq, dk, dv, dsb = _attention_reference(q.double(), k.double(), v.double(), dout.double().reshape(B, N, heads, 8).transpose(1, 2))
    return Case("pd_attn_d8_bwd-" + key, {"q": q, "k": k, "v": v, "dout": dout}, ["dout"], {"dq": dq, "dk": dk, "dv": dv},
                {"dq": dq, "dk": dk, "dv": dv, "dP-delta": dsb}, **m)


ATTN_D64_BWD = {"B2-h3-200x77": dict(B=2, heads=3, Nq=200, Nkv=77), "B1-h2-70x200": dict(B=1, heads=2, Nq=70, Nkv=200)}


def attn_d64_bwd(key):
    m = ATTN_D64_BWD[key]
    B, heads, Nq, Nkv = m["B"], m["heads"], m["Nq"], m["Nkv"]
    Cc = heads * 64
    g = torch.Generator().manual_seed(203)
    q, kv, dout = _randn(g, B, Nq, Cc), _randn(g, B, Nkv, 2 * Cc), _randn(g, B, Nq, Cc)
    sp = lambda t, n: t.double().reshape(B, n, heads, 64).transpose(1, 2)
    dq, dk, dv, dsb = _attention_reference(sp(q, Nq), sp(kv[..., :Cc], Nkv), sp(kv[..., Cc:], Nkv), sp(dout, Nq))
    back = lambda t, n: t.transpose(1, 2).reshape(B, n, Cc)                      # -> the [B][N][C] layout of the tensors
    ref = {"dq": back(dq, Nq), "dk": back(dk, Nkv), "dv": back(dv, Nkv)}
    return Case("pd_attn_d64_bwd-" + key, {"q": q, "kv": kv, "dout": dout}, ["dout"], ref, dict(ref, **{"dP-delta": dsb}), **m)


# ---- pd_gn_silu_bwd: dz as one tensor over both sources + the skip gradient `res` -------------------------------------------------------------------
GN_SILU_BWD = {"B2-128+64-8x8": dict(B=2, c0=128, c1=64, H=8, W=8, silu=1), "B1-1280+640-8x4": dict(B=1, c0=1280, c1=640, H=8, W=4, silu=1)}


def gn_silu_bwd(key):
    m = GN_SILU_BWD[key]
    B, c0, c1, H, W = m["B"], m["c0"], m["c1"], m["H"], m["W"]
    Cc = c0 + c1
    g = torch.Generator().manual_seed(204)
    x = _randn(g, B, Cc, H, W, std=1.5, mean=0.3)
    gamma, beta = torch.randn(Cc, generator=g) * 0.5 + 1.0, torch.randn(Cc, generator=g) * 0.3
    dz, res = _randn(g, B, Cc, H, W), _randn(g, B, Cc, H, W)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = F.group_norm(xd, 32, gd, bd, eps=1e-5)
    dx, dg, db = torch.autograd.grad(F.silu(y) if m["silu"] else y, (xd, gd, bd), dz.double())
    dx = dx + res.double()
    xg = x.double().reshape(B, 32, -1)
    stats = {"mean": xg.mean(-1).float(), "rstd": (1.0 / torch.sqrt(xg.var(-1, unbiased=False) + 1e-5)).float()}
    return Case("pd_gn_silu_bwd-" + key, {"x": x, "gamma": gamma, "beta": beta, "dz": dz, "res": res}, ["dz", "res"],
                {"dx": dx, "dgamma": dg, "dbeta": db}, {"dx": dx}, stats=stats, **m)


# ---- row kernels of the transformer blocks -------------------------------------------------------------------------------------------------------
def layernorm_bwd(key="513x1280-res-dxsum"):
    rows, Cc = 513, 1280
    g = torch.Generator().manual_seed(205)
    x = _randn(g, rows, Cc, std=2.0, mean=0.5)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    dy, res = _randn(g, rows, Cc), _randn(g, rows, Cc)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    dx, dg, db = torch.autograd.grad(F.layer_norm(xd, (Cc,), gd, bd, 1e-5), (xd, gd, bd), dy.double())
    dx = dx + res.double()
    return Case("pd_layernorm_bwd-" + key, {"x": x, "gamma": gamma, "dy": dy, "res": res}, ["dy", "res"], {"dx": dx, "dgamma": dg, "dbeta": db},
                {"dx": dx}, rows=rows, C=Cc)


def geglu_bwd(key="333x1280-sums-B3-s5"):
    rows, inner = 333, 1280
    g = torch.Generator().manual_seed(206)
    x, dy = _randn(g, rows, 2 * inner, std=1.5), _randn(g, rows, inner)
    xd = x.double().requires_grad_(True)
    hh, gate = xd.chunk(2, dim=-1)
    (dx,) = torch.autograd.grad(hh * F.gelu(gate), xd, dy.double())
    return Case("pd_geglu_bwd-" + key, {"x": x, "dy": dy}, ["dy"], {"dx": dx}, {"dx": dx}, rows=rows, inner=inner, B=3, splits=5)


TOKEN_WGRAD = {"300x64x64": (300, 64, 64), "231x96x256": (77 * 3, 96, 256)}


def token_wgrad(key):
    M, K, N = TOKEN_WGRAD[key]
    g = torch.Generator().manual_seed(207)
    x, dy = _randn(g, M, K), _randn(g, M, N)
    return Case("pd_token_wgrad-" + key, {"x": x, "dy": dy}, ["dy"], {"dw": dy.double().t() @ x.double()}, {}, M=M, K=K, N=N)


def pool2x2_sum(key="B2-8x16-64"):
    B, H, W, Cc = 2, 8, 16, 64
    g = torch.Generator().manual_seed(208)
    du = _randn(g, B, Cc, 2 * H, 2 * W)
    dx = F.avg_pool2d(du.double(), 2) * 4
    return Case("pd_pool2x2_sum-" + key, {"du": du}, ["du"], {"dx": dx}, {"dx": dx}, B=B, H=H, W=W, C=Cc)


ALL_CASES = ([(conv_wgrad, k) for k in CONV_WGRAD] + [(attn_d8_bwd, k) for k in ATTN_D8_BWD] + [(attn_d64_bwd, k) for k in ATTN_D64_BWD]
             + [(gn_silu_bwd, k) for k in GN_SILU_BWD] + [(layernorm_bwd, "513x1280-res-dxsum"), (geglu_bwd, "333x1280-sums-B3-s5")]
             + [(token_wgrad, k) for k in TOKEN_WGRAD] + [(pool2x2_sum, "B2-8x16-64")])
