"""The restatement ``pd_guidance_rescale`` is tested against: diffusers' ``rescale_noise_cfg`` (StableDiffusionPipeline's
``guidance_rescale``; arXiv 2305.08891 section 3.4) evaluated in float64 from the fp32 guided prediction, with that prediction built by
fp32 torch operations in the kernel's order (``pd_ddim_step``'s combine).  Plus the inputs, the shapes and the ulp measure of
tests/test_gpu_guidance_rescale.py; tests/test_host_guidance_rescale.py proves the restatement's own properties on the CPU.

``phi`` is taken as the C ABI carries it (``float rescale``): the fp32 value nearest to the number given.

A plain module: no fixtures, no pytest hooks."""
import numpy as np
import torch

PHIS = (0.3, 1.0)
# (cfg equation?, weights): scalar and per-sample w, both equations; strong guidance (w >= 2-3) is where the rescale matters
GUIDANCE = ((0, (3.0,)), (1, (2.0,)), (0, (1.5, 0.0, 3.0, 2.0, 7.5)), (1, (1.5, 0.0, 3.0, 2.0, 7.5)))


def shapes(chunk: int):
    """(B, n): rows that start unaligned (n % 4 == 1, three rows: offsets 0, 1, 2 mod 4); whole vectors; the smallest sample that has
    a standard deviation; one reduction chunk plus one element (a second chunk of one element); several chunks with a ragged last one
    in a batch of 5 (n % 4 == 3)."""
    return ((3, 105), (2, 256), (1, 2), (2, chunk + 1), (5, 2 * chunk + 1003))


def inputs(B: int, n: int, seed: int = 0):
    """(cond, uncond): fp32 [B][n].  Per row its own mean and scale (a model output is not centred), the unconditional prediction
    correlated with the conditional one (as two evaluations of one model are)."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + n)
    scale = 0.5 + torch.rand(B, 1, generator=g)
    mean = 0.3 * torch.randn(B, 1, generator=g)
    cond = (mean + scale * torch.randn(B, n, generator=g)).float()
    uncond = (0.8 * cond + 0.1 + 0.4 * scale * torch.randn(B, n, generator=g)).float()
    return cond.contiguous(), uncond.contiguous()


def weights(B: int, w):
    """The (1,) or (B,) fp32 weights of a GUIDANCE entry for a batch of B."""
    return torch.tensor(w if len(w) == 1 else [w[b % len(w)] for b in range(B)], dtype=torch.float32)


def combine_f32(cond: torch.Tensor, uncond: torch.Tensor, w: torch.Tensor, guidance_cfg) -> torch.Tensor:
    """The guided prediction in fp32, one rounding per operation in the kernel's order: d = cond - uncond; m = w * d; base + m."""
    assert cond.dtype == uncond.dtype == w.dtype == torch.float32
    wv = w.reshape(-1, *([1] * (cond.dim() - 1)))
    d = cond - uncond
    m = wv * d
    return (cond if guidance_cfg else uncond) + m


def rescale_noise_cfg(noise_cfg: torch.Tensor, noise_pred_text: torch.Tensor, guidance_rescale: float) -> torch.Tensor:
    """diffusers' function, in the dtype of its inputs (float64 here)."""
    dims = list(range(1, noise_pred_text.ndim))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg


def rescale_factored(noise_cfg: torch.Tensor, noise_pred_text: torch.Tensor, guidance_rescale: float) -> torch.Tensor:
    """The same, factored as the kernel evaluates it: cfg * (phi * std_text / std_cfg + (1 - phi))."""
    dims = list(range(1, noise_pred_text.ndim))
    ratio = noise_pred_text.std(dim=dims, keepdim=True) / noise_cfg.std(dim=dims, keepdim=True)
    return noise_cfg * (guidance_rescale * ratio + (1 - guidance_rescale))


def abi_phi(phi: float) -> float:
    return float(np.float32(phi))


def reference(cond: torch.Tensor, uncond: torch.Tensor, w: torch.Tensor, phi: float, guidance_cfg) -> torch.Tensor:
    """float64 [B][...]: rescale_noise_cfg of the fp32 guided prediction and the fp32 conditional prediction, both widened to float64."""
    cfg = combine_f32(cond, uncond, w, guidance_cfg)
    return rescale_noise_cfg(cfg.double(), cond.double(), abi_phi(phi))


def ulps(got: torch.Tensor, want64: torch.Tensor) -> torch.Tensor:
    """|got - want| in units of the fp32 spacing at want (the spacing of the fp32 value nearest to it; never below the smallest normal's)."""
    want32 = want64.float()
    spacing = torch.from_numpy(np.spacing(np.maximum(np.abs(want32.numpy()), np.float32(np.finfo(np.float32).tiny)))).double()
    return (got.double() - want64).abs() / spacing


MAX_ULPS = 2.0      # one rounding of g to fp32, one of the product (tests/test_gpu_guidance_rescale.py says why it is 2 and not 1)
