"""SD-tier AutoencoderKL on MI355X: pd_attn_wide / pd_latent_sample against plain PyTorch fp32 of the same ops, and
encode / decode against the CPU oracle on identical seeded weights and inputs."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import DT, bf16_round, env, rel, stream  # noqa: F401

pytestmark = pytest.mark.gpu


# relative L2 bounds of the two parity tests below (named: tests/test_gpu_guard_bands.py asserts the same numbers)
ATTN_WIDE_TOL = {"f32": 2e-5, "bf16": 1.5e-2, "fp16": 1.5e-2}
ATTN_WIDE_BWD_TOL = {"f32": 3e-5, "bf16": 2e-2, "fp16": 4e-3}


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("cfg", [(2, 1, 512, 256), (1, 1, 512, 1000), (2, 2, 128, 77), (1, 1, 256, 16), (1, 3, 256, 130), (1, 1, 512, 4096)])
def test_attention_wide(env, mode, cfg):
    L, lib, _, dev = env
    code, tdt = DT[mode]
    B, heads, D, N = cfg
    Cc = heads * D
    g = torch.Generator().manual_seed(43)
    qkv = bf16_round(torch.randn(B, N, 3 * Cc, generator=g), mode)
    q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
    QKV = qkv.to(tdt).to(dev).contiguous()
    esz = QKV.element_size()
    out = torch.full((B, N, Cc), float("nan"), dtype=tdt, device=dev)
    a = L.AttnWideArgs(dtype=code, B=B, heads=heads, D=D, Nq=N, Nkv=N, scale=D ** -0.5, q=QKV.data_ptr(), q_stride=3 * Cc,
                       k=QKV.data_ptr() + Cc * esz, v=QKV.data_ptr() + 2 * Cc * esz, kv_stride=3 * Cc, out=out.data_ptr(), out_stride=Cc)
    L.check(lib.pd_attn_wide(C.byref(a), stream()), "pd_attn_wide")
    torch.cuda.synchronize()
    sp = lambda t: t.reshape(B, N, heads, D).transpose(1, 2)
    ref = F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).reshape(B, N, Cc)
    assert rel(out.float(), ref) < ATTN_WIDE_TOL[mode]


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])       # fp16: round 5 (training under a loss scale)
@pytest.mark.parametrize("cfg", [(2, 1, 512, 16), (1, 1, 512, 256), (2, 2, 128, 77), (1, 3, 256, 130), (1, 1, 512, 4)])
def test_attention_wide_backward(env, mode, cfg):
    """pd_attn_wide_bwd (dQ pass + dK / dV pass, P recomputed from the forward's log-sum-exp) against torch.autograd of
    F.scaled_dot_product_attention on the same (storage-rounded) q, k, v and upstream gradient: the attention of
    orig_google_ddpm_model_denoiser.json under accelerator.backward (utils_training.py:436), sequence lengths incl. partial tiles."""
    L, lib, _, dev = env
    code, tdt = DT[mode]
    B, heads, D, N = cfg
    Cc = heads * D
    g = torch.Generator().manual_seed(45)
    qkv = bf16_round(torch.randn(B, N, 3 * Cc, generator=g), mode)
    dout = bf16_round(torch.randn(B, N, Cc, generator=g), mode)
    sp = lambda t: t.reshape(B, N, heads, D).transpose(1, 2)
    leaf = qkv.clone().requires_grad_(True)
    ref = F.scaled_dot_product_attention(sp(leaf[..., :Cc]), sp(leaf[..., Cc:2 * Cc]), sp(leaf[..., 2 * Cc:])).transpose(1, 2).reshape(B, N, Cc)
    ref.backward(dout)
    QKV, DO = qkv.to(tdt).to(dev).contiguous(), dout.to(tdt).to(dev).contiguous()
    esz = QKV.element_size()
    out = torch.empty((B, N, Cc), dtype=tdt, device=dev)
    lse = torch.empty((B, heads, N), device=dev)
    p = QKV.data_ptr()
    a = L.AttnWideArgs(dtype=code, B=B, heads=heads, D=D, Nq=N, Nkv=N, scale=D ** -0.5, q=p, q_stride=3 * Cc, k=p + Cc * esz,
                       v=p + 2 * Cc * esz, kv_stride=3 * Cc, out=out.data_ptr(), out_stride=Cc, lse=lse.data_ptr())
    L.check(lib.pd_attn_wide(C.byref(a), stream()), "pd_attn_wide")
    dqkv = torch.full((B, N, 3 * Cc), float("nan"), dtype=tdt, device=dev)
    delta = torch.empty((B, heads, N), device=dev)
    dp = dqkv.data_ptr()
    b = L.AttnWideBwdArgs(dtype=code, B=B, heads=heads, D=D, Nq=N, Nkv=N, scale=D ** -0.5, q=p, q_stride=3 * Cc, k=p + Cc * esz,
                          v=p + 2 * Cc * esz, kv_stride=3 * Cc, o=out.data_ptr(), dout=DO.data_ptr(), o_stride=Cc, lse=lse.data_ptr(),
                          delta=delta.data_ptr(), dq=dp, dq_stride=3 * Cc, dk=dp + Cc * esz, dv=dp + 2 * Cc * esz, dkv_stride=3 * Cc)
    L.check(lib.pd_attn_wide_bwd(C.byref(b), stream()), "pd_attn_wide_bwd")
    torch.cuda.synchronize()
    # the log-sum-exp the forward kept (log2 domain) and delta = rowsum(O dO)
    s = (sp(qkv[..., :Cc]) @ sp(qkv[..., Cc:2 * Cc]).transpose(-1, -2)) * D ** -0.5
    assert float((lse.cpu() - torch.logsumexp(s, -1) * 1.4426950408889634).abs().max()) < (1e-4 if mode == "f32" else 3e-2)
    tol = ATTN_WIDE_BWD_TOL[mode]
    got = dqkv.float().cpu()
    for i, name in enumerate("qkv"):
        assert rel(got[..., i * Cc:(i + 1) * Cc], leaf.grad[..., i * Cc:(i + 1) * Cc]) < tol, (name, mode, cfg)


def test_attention_wide_rejects_unbuilt_dim(env):
    L, lib, _, dev = env
    t = torch.zeros(1, 32, 3 * 96, device=dev)
    a = L.AttnWideArgs(dtype=L.PD_F32, B=1, heads=1, D=96, Nq=32, Nkv=32, scale=1.0, q=t.data_ptr(), q_stride=288, k=t.data_ptr(),
                       v=t.data_ptr(), kv_stride=288, out=t.data_ptr(), out_stride=288)
    assert lib.pd_attn_wide(C.byref(a), stream()) == -4


def test_latent_sample(env):
    import phendiff_amd as P
    g = torch.Generator().manual_seed(44)
    mom = torch.randn(3, 8, 5, 7, generator=g) * 3
    mom[0, 4:] = 50.0        # clamp to 20
    mom[1, 4:] = -50.0       # clamp to -30
    noise = torch.randn(3, 4, 5, 7, generator=g)
    d = P.DiagonalGaussianDistribution(mom.cuda())
    ref = mom[:, :4] + torch.exp(0.5 * mom[:, 4:].clamp(-30, 20)) * noise
    assert rel(d.sample(noise=noise.cuda()), ref) < 1e-6
    assert rel(d.sample(noise=noise.cuda(), scale=0.18215), 0.18215 * ref) < 1e-6
    assert torch.equal(d.mode().cpu(), mom[:, :4])
    assert torch.equal(d.mean.cpu(), mom[:, :4]) and float(d.logvar.max()) == 20.0
    # CPU generator: the draw happens on the CPU like diffusers' randn_tensor, so it matches the oracle's draw
    z = d.sample(torch.Generator().manual_seed(7))
    n7 = torch.randn(3, 4, 5, 7, generator=torch.Generator().manual_seed(7))
    assert rel(z, mom[:, :4] + torch.exp(0.5 * mom[:, 4:].clamp(-30, 20)) * n7) < 1e-6


CFGS = {
    "d64": (dict(block_out_channels=(32, 64), layers_per_block=1), (32, 32)),
    "d128": (dict(block_out_channels=(32, 64, 128), layers_per_block=2), (64, 48)),
    "d256": (dict(block_out_channels=(64, 128, 256, 256), layers_per_block=1), (64, 64)),
}


def make_pair(cfg, mode, seed=0):
    import phendiff_amd as P
    from oracle import AutoencoderKLRef
    torch.manual_seed(seed)
    r = AutoencoderKLRef(**cfg).eval()
    m = P.AutoencoderKL(compute_dtype=mode, **cfg)
    m.load_state_dict(r.state_dict())
    return r, m.to("cuda:0")


# measured maxima (profiles/r2_parity_errors.json): f32 7.1e-6, bf16 2.9e-2, fp16 3.5e-3
@pytest.mark.parametrize("mode,tol", [("f32", 3e-5), ("bf16", 5e-2), ("fp16", 8e-3)])
@pytest.mark.parametrize("name", list(CFGS))
def test_vae_encode_decode(mode, tol, name):
    cfg, (H, W) = CFGS[name]
    r, m = make_pair(cfg, mode)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, H, W, generator=g) * 2 - 1
    with torch.no_grad():
        rd = r.encode(x).latent_dist
        noise = torch.randn(rd.mean.shape, generator=g)
        rz = rd.sample(noise=noise)
        ry = r.decode(rz, return_dict=False)[0]
    d = m.encode(x.cuda()).latent_dist
    assert d.parameters.shape == (2, 8, H >> (len(cfg["block_out_channels"]) - 1), W >> (len(cfg["block_out_channels"]) - 1))
    assert rel(d.mean, rd.mean) < tol, rel(d.mean, rd.mean)
    assert rel(d.parameters[:, 4:], rd.logvar) < tol          # unclamped region with random init
    # decode the ORACLE's latents so the decoder is checked on its own
    y = m.decode(rz.cuda(), return_dict=False)[0]
    assert y.shape == x.shape and y.dtype == torch.float32
    assert rel(y, ry) < tol, rel(y, ry)
    assert torch.equal(m.decode(rz.cuda()).sample, y)
    # full round trip on the engine
    y2 = m.decode(d.sample(noise=noise.cuda())).sample
    assert rel(y2, ry) < 2 * tol


def test_sd_vae_full_config_f32_small_image():
    """The exact SD-VAE structure (83.7 M parameters; 512-channel one-head attention -> pd_attn_wide D=512) on a 64x64 image."""
    r, m = make_pair({}, "f32")
    assert sum(p.numel() for p in m.parameters()) == 83_653_863
    g = torch.Generator().manual_seed(4)
    x = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    with torch.no_grad():
        rd = r.encode(x).latent_dist
        ry = r.decode(rd.mean).sample
    d = m.encode(x.cuda()).latent_dist
    assert rel(d.parameters, torch.cat([rd.mean, r.quant_conv(r.encoder(x)).detach()[:, 4:]], 1)) < 5e-5
    assert rel(m.decode(rd.mean.cuda()).sample, ry) < 5e-5


def test_vae_batch_chunking_and_errors():
    import phendiff_amd as P
    cfg, _ = CFGS["d64"]
    r, m = make_pair(cfg, "f32")
    x = torch.rand(5, 3, 16, 16) * 2 - 1
    with torch.no_grad():
        ref = r.quant_conv(r.encoder(x))
    m._max_batch = lambda H, W, kind="dec": 2                 # force 3 chunks (2 + 2 + 1)
    assert rel(m.encode(x.cuda()).latent_dist.parameters, ref) < 5e-5
    with pytest.raises(P.PhenDiffHipError):
        m.encode(x)
    with pytest.raises(ValueError):
        m.decode(torch.zeros(1, 3, 4, 4, device="cuda"))
    with pytest.raises(NotImplementedError):
        P.AutoencoderKL(block_out_channels=(32, 96))


def test_vae_chunk_size_respects_the_2gib_source_limit():
    """SD VAE at 512x512: the decoder's last stage reads 256 channels at full resolution (134 MB / sample in bf16), so a batch of
    16 must be split (it overflowed pd_conv's 32-bit source offsets before the limit accounted for that tensor)."""
    import phendiff_amd as P
    m = P.AutoencoderKL(compute_dtype="bf16")
    assert m._max_batch(512, 512, "enc") == 31 and m._max_batch(512, 512, "dec") == 15
    f = P.AutoencoderKL(compute_dtype="f32")
    assert f._max_batch(512, 512, "dec") == 7


def test_image_processor():
    import phendiff_amd as P
    from oracle import vae_postprocess_ref, vae_preprocess_ref
    ip = P.VaeImageProcessor(vae_scale_factor=8)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 8, 8, generator=g)
    assert torch.equal(ip.preprocess(x.cuda()).cpu(), vae_preprocess_ref(x))
    xn = x * 2 - 1
    assert torch.equal(ip.preprocess(xn.cuda()).cpu(), vae_preprocess_ref(xn))
    lat = torch.randn(2, 4, 4, 4, generator=g).cuda()
    assert ip.preprocess(lat) is lat and ip.postprocess(lat, "latent") is lat
    y = torch.randn(2, 3, 8, 8, generator=g) * 2
    assert np.array_equal(ip.postprocess(y.cuda(), "np"), vae_postprocess_ref(y, "np"))
    assert torch.equal(ip.postprocess(y.cuda(), "pt").cpu(), vae_postprocess_ref(y, "pt"))
    pil = ip.postprocess(y.cuda(), "pil")
    assert len(pil) == 2 and pil[0].size == (8, 8)
