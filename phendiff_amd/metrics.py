"""FID / IS / KID of generated images, as the reference computes them with ``torch_fidelity.calculate_metrics`` at evaluation time
(``src/utils_training.py:948-1001``: per class, generated folder vs the class's real images, ``isc`` / ``fid`` / ``kid`` /
``kid_subset_size`` from the arguments) and after a class-transfer experiment (``src/utils_Img2Img.py:462-563``).

torch-fidelity's defaults are what the reference runs with: the ``inception-v3-compat`` feature extractor (the TF-Slim InceptionV3 of the
original FID code: uint8 image -> TF1-style bilinear resize to 299 x 299 -> (x - 128) / 128 -> 94 conv + BatchNorm + ReLU layers, FID's two
pooling quirks -> 2048-d pool3 features -> fc to 1008 logits), FID and KID on the 2048-d features, IS on the un-biased logits, 10 IS
splits, 100 KID subsets, polynomial kernel (degree 3, gamma 1/d, coef0 1), RNG seed 2020.

Here the network runs on the HIP engine (``csrc/metric_kernels.hip``: ``pd_resize_tf1``, ``pd_conv_rect`` with the BatchNorm folded into
weights and bias at pack time and the branch concatenations written in place, ``pd_pool2d``, ``pd_fc_f32``); the statistics are fp64 on the
host, like the library's (numpy / scipy) -- or, with ``device_statistics=True``, fp64 on the device for the heavy part (``csrc/metric_stats.hip``:
``pd_kid_mmd``, ``pd_feature_moments``) with the matrix square root and the Inception score still on the host.  Deviation, stated: the reference writes PNG files and torch-fidelity reads them back; this module
takes the uint8 arrays themselves (``round(255 x)`` of the pipeline's float output -- the bytes the PNGs would hold), so there is no file
round trip.  The module tree carries torch-fidelity's state_dict names: its published ``pt_inception-2015-12-05`` weights load with
``load_state_dict``.  They are not obtainable here (no network), so tests and examples run the structure on seeded random weights.

Beyond what the reference logs: improved precision / recall and density / coverage over the same 2048-d features (``prc=`` / ``dc=``, off by
default; ``csrc/manifold_stats.hip`` on the device path) -- see the section below the KID / FID device statistics."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from .packing import pack_conv_weight

_DT = {"f32": (L.PD_F32 if hasattr(L, "PD_F32") else 0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}


def _c32(c: int) -> int:
    return (c + 31) // 32 * 32


class BasicConv2d(nn.Module):
    """conv (no bias) + BatchNorm(eps 1e-3, inference statistics) + ReLU: torch-fidelity / torchvision ``BasicConv2d``."""

    def __init__(self, cin, cout, kernel_size, stride=1, padding=0):
        super().__init__()
        kh, kw = (kernel_size, kernel_size) if isinstance(kernel_size, int) else kernel_size
        ph, pw = (padding, padding) if isinstance(padding, int) else padding
        self.geom = (cin, cout, kh, kw, stride, ph, pw)
        self.conv = nn.Conv2d(cin, cout, (kh, kw), stride, (ph, pw), bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)


# block tables: every entry of a branch is (attribute name, cin, cout, kernel, stride, padding) or a pooling marker; a branch's LAST
# convolutions (one, or the two of InceptionE's split) are written into the block's concatenated output in table order
def _A(cin, pf):
    return [[("branch1x1", cin, 64, 1, 1, 0)],
            [("branch5x5_1", cin, 48, 1, 1, 0), ("branch5x5_2", 48, 64, 5, 1, 2)],
            [("branch3x3dbl_1", cin, 64, 1, 1, 0), ("branch3x3dbl_2", 64, 96, 3, 1, 1), ("branch3x3dbl_3", 96, 96, 3, 1, 1)],
            ["avg311", ("branch_pool", cin, pf, 1, 1, 0)]]


def _B(cin):
    return [[("branch3x3", cin, 384, 3, 2, 0)],
            [("branch3x3dbl_1", cin, 64, 1, 1, 0), ("branch3x3dbl_2", 64, 96, 3, 1, 1), ("branch3x3dbl_3", 96, 96, 3, 2, 0)],
            ["max320"]]


def _C(cin, c7):
    return [[("branch1x1", cin, 192, 1, 1, 0)],
            [("branch7x7_1", cin, c7, 1, 1, 0), ("branch7x7_2", c7, c7, (1, 7), 1, (0, 3)), ("branch7x7_3", c7, 192, (7, 1), 1, (3, 0))],
            [("branch7x7dbl_1", cin, c7, 1, 1, 0), ("branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)), ("branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)),
             ("branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)), ("branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))],
            ["avg311", ("branch_pool", cin, 192, 1, 1, 0)]]


def _D(cin):
    return [[("branch3x3_1", cin, 192, 1, 1, 0), ("branch3x3_2", 192, 320, 3, 2, 0)],
            [("branch7x7x3_1", cin, 192, 1, 1, 0), ("branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)), ("branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)),
             ("branch7x7x3_4", 192, 192, 3, 2, 0)],
            ["max320"]]


def _E(cin, pool):
    return [[("branch1x1", cin, 320, 1, 1, 0)],
            [("branch3x3_1", cin, 384, 1, 1, 0), [("branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)), ("branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))]],
            [("branch3x3dbl_1", cin, 448, 1, 1, 0), ("branch3x3dbl_2", 448, 384, 3, 1, 1),
             [("branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), ("branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))]],
            [pool, ("branch_pool", cin, 192, 1, 1, 0)]]


STEM = [("Conv2d_1a_3x3", 3, 32, 3, 2, 0), ("Conv2d_2a_3x3", 32, 32, 3, 1, 0), ("Conv2d_2b_3x3", 32, 64, 3, 1, 1), "max320",
        ("Conv2d_3b_1x1", 64, 80, 1, 1, 0), ("Conv2d_4a_3x3", 80, 192, 3, 1, 0), "max320"]
BLOCKS = [("Mixed_5b", _A(192, 32)), ("Mixed_5c", _A(256, 64)), ("Mixed_5d", _A(288, 64)), ("Mixed_6a", _B(288)),
          ("Mixed_6b", _C(768, 128)), ("Mixed_6c", _C(768, 160)), ("Mixed_6d", _C(768, 160)), ("Mixed_6e", _C(768, 192)),
          ("Mixed_7a", _D(768)), ("Mixed_7b", _E(1280, "avg311")), ("Mixed_7c", _E(2048, "max311"))]
_POOLS = {"max320": (0, 3, 2, 0), "avg311": (1, 3, 1, 1), "max311": (0, 3, 1, 1)}      # marker -> (mode, k, stride, pad)


def _flat(entries):
    for e in entries:
        if isinstance(e, list):
            yield from _flat(e)
        elif isinstance(e, tuple):
            yield e


class InceptionV3Features(nn.Module):
    """torch-fidelity ``FeatureExtractorInceptionV3`` ("inception-v3-compat") on the HIP engine.  ``forward(images)``: uint8 images,
    NHWC (N, H, W, 3) or NCHW (N, 3, H, W), on the GPU -> {"2048": pool3 features, "logits_unbiased", "logits"} (fp32, on the device)."""

    def __init__(self, compute_dtype: str = "bf16", num_logits: int = 1008):
        super().__init__()
        if compute_dtype not in _DT:
            raise ValueError(f"compute_dtype {compute_dtype!r} not in {sorted(_DT)}")
        self.compute_dtype = compute_dtype
        for e in STEM:
            if isinstance(e, tuple):
                setattr(self, e[0], BasicConv2d(*e[1:]))
        for name, branches in BLOCKS:
            blk = nn.Module()
            for e in _flat(branches):
                setattr(blk, e[0], BasicConv2d(*e[1:]))
            setattr(self, name, blk)
        self.fc = nn.Linear(2048, num_logits)
        self._packed = None
        self._plans: Dict[tuple, "_Plan"] = {}
        self.eval()

    def invalidate(self):
        """Drop the packed weights and plans (after loading / changing parameters)."""
        self._packed, self._plans = None, {}

    def load_state_dict(self, *a, **k):
        self.invalidate()
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self.invalidate()
        return super()._apply(fn, *a, **k)

    @property
    def device(self):
        return self.fc.weight.device

    # ---- weights: BatchNorm folded, channels padded to multiples of 32, MFMA fragment order -------------------------------------------
    def _pack(self):
        tdt = _DT[self.compute_dtype][1]
        out = {}
        for prefix, mod in self.named_modules():
            if not isinstance(mod, BasicConv2d):
                continue
            cin, cout, kh, kw, stride, ph, pw = mod.geom
            bn = mod.bn
            g = (bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps))
            w = mod.conv.weight.detach().double() * g.view(-1, 1, 1, 1)
            b = bn.bias.detach().double() - bn.running_mean.detach().double() * g
            cip, cop = _c32(cin), _c32(cout)
            wp = torch.zeros((cout, cip, kh, kw), dtype=torch.float32, device=w.device)
            wp[:, :cin] = w.float()
            bp = torch.zeros(cop, dtype=torch.float32, device=w.device)
            bp[:cout] = b.float()
            out[prefix] = (pack_conv_weight(wp, tdt, cop).contiguous(), bp.contiguous(), (cip, cop, kh, kw, stride, ph, pw))
        out["fc"] = (self.fc.weight.detach().float().t().contiguous(), self.fc.bias.detach().float().contiguous())
        return out

    @torch.no_grad()
    def forward(self, images: torch.Tensor):
        if not images.is_cuda:
            raise L.PhenDiffHipError("phendiff_amd runs on MI355X only (no CPU fallback): move the images to 'cuda'")
        if images.dtype != torch.uint8 or images.ndim != 4:
            raise ValueError("Expecting uint8 images of shape (N, H, W, 3) or (N, 3, H, W)")
        if images.shape[-1] != 3:
            if images.shape[1] != 3:
                raise ValueError(f"Expecting 3-channel images, got {tuple(images.shape)}")
            images = images.permute(0, 2, 3, 1)
        images = images.contiguous()
        if self._packed is None:
            self._packed = self._pack()
        N, H, W, _ = images.shape
        key = (N, H, W)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = _Plan(self, N, H, W)
        return plan.run(images)


class _Plan:
    """Static launch plan for N images of H x W: every activation buffer (NHWC, channels padded to 32) and pre-filled argument struct."""

    def __init__(self, net: InceptionV3Features, N: int, H: int, W: int):
        self.lib = L.lib()
        self.code, self.tdt = _DT[net.compute_dtype]
        self.dev, self.N = net.device, N
        self.ops, self.bufs = [], []
        P = net._packed
        x = self._buf(299, 299, 32)
        self.resize = L.ResizeTf1Args(dtype=self.code, N=N, H=H, W=W, OH=299, OW=299, scale_y=float(np.float32(H / 299)),
                                      scale_x=float(np.float32(W / 299)), sub=128.0, div=128.0, x=None, y=x.data_ptr())
        for e in STEM:
            x = self._conv(P, e[0], x) if isinstance(e, tuple) else self._pool(x, e)
        for name, branches in BLOCKS:
            x = self._block(P, name, branches, x)
        self.pool = torch.empty((N, 2048), dtype=torch.float32, device=self.dev)
        h, w, c = x.shape[1:]
        self.ops.append((self.lib.pd_pool2d, L.Pool2dArgs(dtype=self.code, B=N, Hin=h, Win=w, C=c, Hout=1, Wout=1, k=h, stride=1, pad=0, mode=2,
                                                          x=x.data_ptr(), x_cs=c, y=self.pool.data_ptr(), y_cs=c, y_co=0), "pd_pool2d"))
        wt, bias = P["fc"]
        self.logits_u = torch.empty((N, wt.shape[1]), dtype=torch.float32, device=self.dev)
        self.logits = torch.empty_like(self.logits_u)
        for y, b in ((self.logits_u, None), (self.logits, bias)):
            self.ops.append((self.lib.pd_fc_f32, L.FcF32Args(rows=N, in_dim=wt.shape[0], out_dim=wt.shape[1], x=self.pool.data_ptr(), wt=wt.data_ptr(),
                                                             bias=L.ptr(b), y=y.data_ptr()), "pd_fc_f32"))

    def _buf(self, h, w, c):
        t = torch.empty((self.N, h, w, c), dtype=self.tdt, device=self.dev)
        self.bufs.append(t)
        return t

    def _conv(self, P, name, x, out=None, co=0):
        wp, bp, (cip, cop, kh, kw, stride, ph, pw) = P[name]
        _, hin, win, cs = x.shape
        assert cs == cip, (name, cs, cip)
        hout, wout = (hin + 2 * ph - kh) // stride + 1, (win + 2 * pw - kw) // stride + 1
        if out is None:
            out = self._buf(hout, wout, cop)
        a = L.ConvRectArgs(dtype=self.code, B=self.N, Hin=hin, Win=win, Cin=cip, Hout=hout, Wout=wout, Cout_pad=cop, KH=kh, KW=kw, stride=stride,
                           pad_h=ph, pad_w=pw, relu=1, x=x.data_ptr(), x_cs=cs, w_packed=wp.data_ptr(), bias=bp.data_ptr(), y=out.data_ptr(),
                           y_cs=out.shape[3], y_co=co)
        self.ops.append((self.lib.pd_conv_rect, a, f"pd_conv_rect {name}"))
        return out

    def _pool(self, x, marker, out=None, co=0):
        mode, k, stride, pad = _POOLS[marker]
        _, hin, win, c = x.shape
        hout, wout = (hin + 2 * pad - k) // stride + 1, (win + 2 * pad - k) // stride + 1
        if out is None:
            out = self._buf(hout, wout, c)
        a = L.Pool2dArgs(dtype=self.code, B=self.N, Hin=hin, Win=win, C=c, Hout=hout, Wout=wout, k=k, stride=stride, pad=pad, mode=mode,
                         x=x.data_ptr(), x_cs=c, y=out.data_ptr(), y_cs=out.shape[3], y_co=co)
        self.ops.append((self.lib.pd_pool2d, a, f"pd_pool2d {marker}"))
        return out

    def _block(self, P, name, branches, x):
        """One Inception block: each branch's last layer(s) write their channel slice of the concatenated output directly."""
        def heads(br):
            last = br[-1]
            return last if isinstance(last, list) else [last]
        widths = []
        for br in branches:
            for hd in heads(br):
                widths.append(x.shape[3] if isinstance(hd, str) else _c32(hd[2]))
        first = branches[0][0]
        stride = 2 if any(isinstance(e, tuple) and e[4] == 2 for br in branches for e in _flat(br)) else 1
        h = (x.shape[1] - 3) // 2 + 1 if stride == 2 else x.shape[1]
        w = (x.shape[2] - 3) // 2 + 1 if stride == 2 else x.shape[2]
        out = self._buf(h, w, sum(widths))
        co = 0
        for br in branches:
            t = x
            for e in br[:-1]:
                t = self._pool(t, e) if isinstance(e, str) else self._conv(P, f"{name}.{e[0]}", t)
            for hd in heads(br):
                if isinstance(hd, str):
                    self._pool(t, hd, out, co)
                    co += t.shape[3]
                else:
                    self._conv(P, f"{name}.{hd[0]}", t, out, co)
                    co += _c32(hd[2])
        assert co == out.shape[3] and first is not None
        return out

    def run(self, images_u8: torch.Tensor):
        st = torch.cuda.current_stream(self.dev).cuda_stream
        self.resize.x = images_u8.data_ptr()
        L.check(self.lib.pd_resize_tf1(C.byref(self.resize), st), "pd_resize_tf1")
        for fn, a, what in self.ops:
            L.check(fn(C.byref(a), st), what)
        self._keep = images_u8
        return {"2048": self.pool.clone(), "logits_unbiased": self.logits_u.clone(), "logits": self.logits.clone()}


# ---- the three metrics, fp64 on the host (torch_fidelity metric_fid.py / metric_isc.py / metric_kid.py) ---------------------------------
KEY_FID, KEY_ISC_MEAN, KEY_ISC_STD = "frechet_inception_distance", "inception_score_mean", "inception_score_std"
KEY_KID_MEAN, KEY_KID_STD = "kernel_inception_distance_mean", "kernel_inception_distance_std"


def fid_statistics(features) -> tuple:
    f = np.asarray(features, dtype=np.float64)
    return np.mean(f, axis=0), np.cov(f, rowvar=False)


def fid_from_statistics(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """||mu1 - mu2||^2 + Tr(S1) + Tr(S2) - 2 Tr(sqrtm(S1 S2)); a singular product is retried with eps on both diagonals."""
    import scipy.linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    diff = mu1 - mu2
    covmean, _ = scipy.linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = scipy.linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError("FID: the matrix square root has an imaginary component")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def inception_score(logits_unbiased, splits: int = 10, shuffle: bool = True, rng_seed: int = 2020) -> dict:
    """exp(mean_x KL(p(y|x) || p(y))) per split of the (shuffled) samples; mean and std over the splits."""
    f = np.asarray(logits_unbiased, dtype=np.float64)
    N = f.shape[0]
    if shuffle:
        f = f[np.random.RandomState(rng_seed).permutation(N), :]
    z = f - f.max(axis=1, keepdims=True)
    log_p = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    p = np.exp(log_p)
    scores = []
    for i in range(splits):
        sl = slice(i * N // splits, (i + 1) * N // splits)
        q = p[sl].mean(axis=0, keepdims=True)
        scores.append(float(np.exp((p[sl] * (log_p[sl] - np.log(q))).sum(axis=1).mean())))
    return {KEY_ISC_MEAN: float(np.mean(scores)), KEY_ISC_STD: float(np.std(scores))}


def kernel_inception_distance(features_1, features_2, kid_subsets: int = 100, kid_subset_size: int = 1000, degree: int = 3,
                              gamma: Optional[float] = None, coef0: float = 1, rng_seed: int = 2020) -> dict:
    """Unbiased MMD^2 under the polynomial kernel (x . y / d + 1)^3 over ``kid_subsets`` random subsets of ``kid_subset_size`` samples."""
    f1, f2 = np.asarray(features_1, dtype=np.float64), np.asarray(features_2, dtype=np.float64)
    if kid_subset_size > len(f1) or kid_subset_size > len(f2):
        raise ValueError(f"kid_subset_size {kid_subset_size} exceeds the number of samples ({len(f1)}, {len(f2)})")
    rng = np.random.RandomState(rng_seed)
    gam = gamma if gamma is not None else 1.0 / f1.shape[1]
    mmds = np.zeros(kid_subsets)
    for i in range(kid_subsets):
        a = f1[rng.choice(len(f1), kid_subset_size, replace=False)]
        b = f2[rng.choice(len(f2), kid_subset_size, replace=False)]
        kxx, kxy, kyy = (a @ a.T * gam + coef0) ** degree, (a @ b.T * gam + coef0) ** degree, (b @ b.T * gam + coef0) ** degree
        m = kid_subset_size
        mmds[i] = ((kxx.sum() - np.trace(kxx)) + (kyy.sum() - np.trace(kyy))) / (m * (m - 1)) - 2 * kxy.sum() / (m * m)
    return {KEY_KID_MEAN: float(np.mean(mmds)), KEY_KID_STD: float(np.std(mmds))}


def kid_subset_indices(n1: int, n2: int, kid_subsets: int = 100, kid_subset_size: int = 1000, rng_seed: int = 2020):
    """The rows :func:`kernel_inception_distance` draws, as two int32 tables [kid_subsets][kid_subset_size]: per subset
    ``rng.choice(n1, m, replace=False)`` and then ``rng.choice(n2, m, replace=False)`` from one ``RandomState(rng_seed)``."""
    if kid_subset_size > n1 or kid_subset_size > n2:
        raise ValueError(f"kid_subset_size {kid_subset_size} exceeds the number of samples ({n1}, {n2})")
    rng = np.random.RandomState(rng_seed)
    i1 = np.empty((kid_subsets, kid_subset_size), dtype=np.int32)
    i2 = np.empty((kid_subsets, kid_subset_size), dtype=np.int32)
    for i in range(kid_subsets):
        i1[i] = rng.choice(n1, kid_subset_size, replace=False)
        i2[i] = rng.choice(n2, kid_subset_size, replace=False)
    return i1, i2


# ---- the statistics of KID and FID on the device (csrc/metric_stats.hip: fp64 MFMA over the fp32 features; no host fallback) -----------
def _device_features(f, what: str) -> torch.Tensor:
    if not torch.is_tensor(f) or not f.is_cuda:
        raise L.PhenDiffHipError(f"{what}: phendiff_amd runs on MI355X only (no CPU fallback): pass the features as a 'cuda' tensor")
    if f.dtype != torch.float32 or f.ndim != 2:
        raise ValueError(f"{what}: expecting fp32 features of shape (N, D), got {f.dtype} {tuple(f.shape)}")
    if f.stride(1) != 1 or f.stride(0) % 4 or f.stride(0) < f.shape[1] or f.data_ptr() % 16:
        f = f.contiguous()
    return f


def kid_mmd_device(f1: torch.Tensor, f2: torch.Tensor, idx1, idx2, degree: int = 3, gamma: Optional[float] = None, coef0: float = 1):
    """One ``pd_kid_mmd`` call: ``(sums, mmd)`` ON THE DEVICE -- fp64 [S][3] (the off-diagonal sums of k(a, a) and k(b, b) and the whole
    sum of k(a, b)) and fp64 [S] (the unbiased MMD^2) of the subsets ``a = f1[idx1[s]]``, ``b = f2[idx2[s]]``.  The index tables
    (int32 [S][m], host arrays or tensors) are checked against the row counts here, on the host: the kernel cannot."""
    f1, f2 = _device_features(f1, "kid_mmd_device"), _device_features(f2, "kid_mmd_device")
    if f1.device != f2.device or f1.shape[1] != f2.shape[1]:
        raise ValueError("kid_mmd_device: the two feature sets must share a device and a width")
    i1 = np.ascontiguousarray(idx1.cpu().numpy() if torch.is_tensor(idx1) else idx1, dtype=np.int32)
    i2 = np.ascontiguousarray(idx2.cpu().numpy() if torch.is_tensor(idx2) else idx2, dtype=np.int32)
    if i1.ndim != 2 or i1.shape != i2.shape:
        raise ValueError(f"kid_mmd_device: index tables of shapes {i1.shape} and {i2.shape} (two [S][m] tables)")
    S, m = i1.shape
    for tab, n in ((i1, f1.shape[0]), (i2, f2.shape[0])):
        if tab.size and (tab.min() < 0 or tab.max() >= n):
            raise ValueError(f"kid_mmd_device: a subset index outside 0 .. {n - 1}")
    dev, D = f1.device, f1.shape[1]
    lib = L.lib()
    with torch.cuda.device(dev):
        d1, d2 = torch.from_numpy(i1).to(dev), torch.from_numpy(i2).to(dev)
        sums = torch.empty((S, 3), dtype=torch.float64, device=dev)
        mmd = torch.empty((S,), dtype=torch.float64, device=dev)
        ws_bytes = lib.pd_kid_mmd_workspace(S, m)
        ws = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=dev)
        a = L.KidMmdArgs(D=D, S=S, m=m, degree=int(degree), N1=f1.shape[0], N2=f2.shape[0], f1_stride=f1.stride(0), f2_stride=f2.stride(0),
                         idx_stride=m, gamma=float(gamma if gamma is not None else 1.0 / D), coef0=float(coef0), f1=f1.data_ptr(),
                         f2=f2.data_ptr(), idx1=d1.data_ptr(), idx2=d2.data_ptr(), sums=sums.data_ptr(), mmd=mmd.data_ptr(),
                         workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
        L.check(lib.pd_kid_mmd(C.byref(a), torch.cuda.current_stream(dev).cuda_stream), "pd_kid_mmd")
    return sums, mmd


def kernel_inception_distance_device(features_1: torch.Tensor, features_2: torch.Tensor, kid_subsets: int = 100, kid_subset_size: int = 1000,
                                     degree: int = 3, gamma: Optional[float] = None, coef0: float = 1, rng_seed: int = 2020) -> dict:
    """:func:`kernel_inception_distance` over fp32 features that stay on the device: the same subsets (:func:`kid_subset_indices`), the
    per-subset MMD^2 from ``pd_kid_mmd`` in fp64; the mean and ``np.std`` of the ``kid_subsets`` values are taken on the host."""
    f1, f2 = _device_features(features_1, "kernel_inception_distance_device"), _device_features(features_2, "kernel_inception_distance_device")
    i1, i2 = kid_subset_indices(f1.shape[0], f2.shape[0], kid_subsets, kid_subset_size, rng_seed)
    _, mmd = kid_mmd_device(f1, f2, i1, i2, degree, gamma, coef0)
    mmds = mmd.cpu().numpy()
    return {KEY_KID_MEAN: float(np.mean(mmds)), KEY_KID_STD: float(np.std(mmds))}


def fid_statistics_device(features: torch.Tensor) -> tuple:
    """:func:`fid_statistics` over fp32 features that stay on the device (``pd_feature_moments``): ``(mu [D], sigma [D][D])`` as fp64 device
    tensors; :func:`fid_from_statistics` takes their ``.cpu().numpy()`` (the matrix square root stays on the host)."""
    f = _device_features(features, "fid_statistics_device")
    dev, (N, D) = f.device, f.shape
    lib = L.lib()
    with torch.cuda.device(dev):
        mu = torch.empty((D,), dtype=torch.float64, device=dev)
        sigma = torch.empty((D, D), dtype=torch.float64, device=dev)
        ws_bytes = lib.pd_feature_moments_workspace(N, D)
        ws = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=dev)
        a = L.FeatureMomentsArgs(D=D, N=N, f_stride=f.stride(0), cov_stride=D, f=f.data_ptr(), mean=mu.data_ptr(), cov=sigma.data_ptr(),
                                 workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
        L.check(lib.pd_feature_moments(C.byref(a), torch.cuda.current_stream(dev).cuda_stream), "pd_feature_moments")
    return mu, sigma


# ---- precision / recall / density / coverage: k-nearest-neighbour manifold estimates over the 2048-d features ----------------------------
# Improved precision and recall (Kynkaanniemi et al. 2019; torch-fidelity's `prc`) and density / coverage (Naeem et al. 2020; the `prdc`
# package), by their published definitions, everything in SQUARED distances:
#     d2(a, b)       = max(0, |a|^2 + |b|^2 - 2 a.b), a NaN counted as +inf (never a neighbour, never counted)
#     rad2_k(F)[i]   = the (k + 1)-th smallest of row i of d2(F, F), the diagonal exactly 0 (the row's own entry takes one place)
#     precision      = mean_j [ exists i: d2(y_j, x_i) <= rad2_k(X)[i] ]          recall = mean_i [ exists j: d2(x_i, y_j) <= rad2_k(Y)[j] ]
#     density        = sum_j #{ i: d2(y_j, x_i) <= rad2_k(X)[i] } / (k Ng)        coverage = mean_i [ min_j d2(x_i, y_j) <= rad2_k(X)[i] ]
# with X the real and Y the generated features.  Deviation, stated: torch-fidelity's default extractor for `prc` is VGG-16; here both pairs
# run over the 2048-d Inception pool features the other metrics use (as users of `prdc` commonly do).  No parity with torch-fidelity's code
# is claimed (it is not available to test against): the definitions above are the contract.
KEY_PRECISION, KEY_RECALL, KEY_F_SCORE, KEY_DENSITY, KEY_COVERAGE = "precision", "recall", "f_score", "density", "coverage"
_MANIFOLD_BLOCK_ROWS = 2048


def _f64_rows(f, what: str) -> np.ndarray:
    f = np.asarray(f, dtype=np.float64)
    if f.ndim != 2 or f.shape[0] < 1:
        raise ValueError(f"{what}: expecting features of shape (N, D), got {f.shape}")
    return f


def _d2_rows(a, na, b, nb):
    """[len(a)][len(b)] squared distances in the Gram form; NaN -> +inf."""
    d = (na[:, None] + nb[None, :]) - 2.0 * (a @ b.T)
    with np.errstate(invalid="ignore"):
        return np.where(d > 0, d, np.where(d <= 0, 0.0, np.inf))


def knn_radii(features, k: int, block_rows: int = _MANIFOLD_BLOCK_ROWS) -> np.ndarray:
    """``rad2_k(features)``: fp64 [N], the squared distance of every row to its k-th nearest other row (``kthvalue(k + 1)`` of a row of the
    distance matrix that includes the row itself, at exactly 0).  ``block_rows`` rows at a time: no N x N array."""
    f = _f64_rows(features, "knn_radii")
    n = len(f)
    if not 1 <= k <= L.CONSTANTS["PD_MANIFOLD_MAX_K"] or k + 1 > n:
        raise ValueError(f"knn_radii: k = {k} (1 .. {L.CONSTANTS['PD_MANIFOLD_MAX_K']}, and k + 1 <= N = {n})")
    nf = np.einsum("ij,ij->i", f, f)
    out = np.empty(n)
    for i in range(0, n, block_rows):
        d = _d2_rows(f[i:i + block_rows], nf[i:i + block_rows], f, nf)
        r = np.arange(len(d))
        d[r, i + r] = 0.0
        out[i:i + block_rows] = np.partition(d, k, axis=1)[:, k]
    return out


def manifold_query(queries, refs, rad2=None, block_rows: int = _MANIFOLD_BLOCK_ROWS):
    """``(count | None, dmin2)`` per query row: ``count[j] = #{i: d2(q_j, r_i) <= rad2[i]}`` (int64; None without ``rad2``) and
    ``dmin2[j] = min_i d2(q_j, r_i)``."""
    q, r = _f64_rows(queries, "manifold_query"), _f64_rows(refs, "manifold_query")
    if q.shape[1] != r.shape[1]:
        raise ValueError("manifold_query: the two feature sets must share a width")
    nq, nr = np.einsum("ij,ij->i", q, q), np.einsum("ij,ij->i", r, r)
    rad2 = None if rad2 is None else np.asarray(rad2, dtype=np.float64)
    count = None if rad2 is None else np.empty(len(q), dtype=np.int64)
    dmin2 = np.empty(len(q))
    for i in range(0, len(q), block_rows):
        d = _d2_rows(q[i:i + block_rows], nq[i:i + block_rows], r, nr)
        dmin2[i:i + block_rows] = d.min(axis=1)
        if count is not None:
            count[i:i + block_rows] = (np.isfinite(d) & (d <= rad2[None, :])).sum(axis=1)
    return count, dmin2


def _f_score(p: float, r: float) -> float:
    return 2.0 * p * r / (p + r) if p + r > 0 else 0.0


def precision_recall(features_1, features_2, neighborhood: int = 3, block_rows: int = _MANIFOLD_BLOCK_ROWS) -> dict:
    """Improved precision / recall of the generated ``features_1`` against the real ``features_2``, fp64 on the host."""
    gen, real = _f64_rows(features_1, "precision_recall"), _f64_rows(features_2, "precision_recall")
    in_real, _ = manifold_query(gen, real, knn_radii(real, neighborhood, block_rows), block_rows)
    in_gen, _ = manifold_query(real, gen, knn_radii(gen, neighborhood, block_rows), block_rows)
    p, r = float((in_real > 0).mean()), float((in_gen > 0).mean())
    return {KEY_PRECISION: p, KEY_RECALL: r, KEY_F_SCORE: _f_score(p, r)}


def density_coverage(features_1, features_2, nearest_k: int = 5, block_rows: int = _MANIFOLD_BLOCK_ROWS) -> dict:
    """Density / coverage of the generated ``features_1`` against the real ``features_2``, fp64 on the host."""
    gen, real = _f64_rows(features_1, "density_coverage"), _f64_rows(features_2, "density_coverage")
    rad2 = knn_radii(real, nearest_k, block_rows)
    count, _ = manifold_query(gen, real, rad2, block_rows)
    _, dmin2 = manifold_query(real, gen, None, block_rows)
    return {KEY_DENSITY: float(count.sum() / (nearest_k * len(gen))), KEY_COVERAGE: float((np.isfinite(dmin2) & (dmin2 <= rad2)).mean())}


def knn_radii_device(features: torch.Tensor, k: int, splits: int = 0) -> torch.Tensor:
    """:func:`knn_radii` over fp32 features that stay on the device (``pd_knn_radii``): fp64 [N] ON THE DEVICE.  ``splits``: column ranges
    per block of 64 rows (0: the library's default; the result does not depend on it)."""
    f = _device_features(features, "knn_radii_device")
    dev, (N, D) = f.device, f.shape
    lib = L.lib()
    with torch.cuda.device(dev):
        rad2 = torch.empty((N,), dtype=torch.float64, device=dev)
        ws_bytes = lib.pd_knn_radii_workspace(N, int(k), int(splits))
        ws = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=dev)
        a = L.KnnRadiiArgs(D=D, k=int(k), splits=int(splits), N=N, f_stride=f.stride(0), f=f.data_ptr(), rad2=rad2.data_ptr(),
                           workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
        L.check(lib.pd_knn_radii(C.byref(a), torch.cuda.current_stream(dev).cuda_stream), "pd_knn_radii")
    return rad2


def manifold_query_device(queries: torch.Tensor, refs: torch.Tensor, rad2: Optional[torch.Tensor] = None, splits: int = 0):
    """:func:`manifold_query` over fp32 features that stay on the device (``pd_manifold_query``): ``(count | None, dmin2)`` ON THE DEVICE,
    int32 [Nq] (None without ``rad2``, an fp64 device tensor [Nr]) and fp64 [Nq]."""
    q, r = _device_features(queries, "manifold_query_device"), _device_features(refs, "manifold_query_device")
    if q.device != r.device or q.shape[1] != r.shape[1]:
        raise ValueError("manifold_query_device: the two feature sets must share a device and a width")
    if rad2 is not None:
        if not torch.is_tensor(rad2) or rad2.device != r.device or rad2.dtype != torch.float64 or rad2.shape != (r.shape[0],):
            raise ValueError(f"manifold_query_device: rad2 must be an fp64 tensor of shape ({r.shape[0]},) on the features' device")
        rad2 = rad2.contiguous()
    dev, (Nq, D), Nr = q.device, q.shape, r.shape[0]
    lib = L.lib()
    with torch.cuda.device(dev):
        count = None if rad2 is None else torch.empty((Nq,), dtype=torch.int32, device=dev)
        dmin2 = torch.empty((Nq,), dtype=torch.float64, device=dev)
        ws_bytes = lib.pd_manifold_query_workspace(Nq, Nr, int(splits))
        ws = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=dev)
        a = L.ManifoldQueryArgs(D=D, splits=int(splits), Nq=Nq, Nr=Nr, q_stride=q.stride(0), r_stride=r.stride(0), q=q.data_ptr(), r=r.data_ptr(),
                                rad2=L.ptr(rad2), count=L.ptr(count), dmin2=dmin2.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws_bytes)
        L.check(lib.pd_manifold_query(C.byref(a), torch.cuda.current_stream(dev).cuda_stream), "pd_manifold_query")
    return count, dmin2


def _precision_recall_on_device(gen, real, k):
    in_real, _ = manifold_query_device(gen, real, knn_radii_device(real, k))
    in_gen, _ = manifold_query_device(real, gen, knn_radii_device(gen, k))
    return [(in_real > 0).sum(), (in_gen > 0).sum()]


def _density_coverage_on_device(gen, real, k):
    rad2 = knn_radii_device(real, k)
    count, _ = manifold_query_device(gen, real, rad2)
    _, dmin2 = manifold_query_device(real, gen)
    return [count.sum(dtype=torch.int64), (torch.isfinite(dmin2) & (dmin2 <= rad2)).sum()]


def manifold_metrics_device(features_1: torch.Tensor, features_2: torch.Tensor, neighborhood: Optional[int] = None,
                            nearest_k: Optional[int] = None) -> dict:
    """Either pair or both over fp32 features that stay on the device: precision / recall / f_score with ``neighborhood``, density / coverage
    with ``nearest_k`` (None: that pair is left out).  Radii, counts and minima come from ``pd_knn_radii`` / ``pd_manifold_query``; the rows
    inside a manifold are counted on the device and two integers per pair reach the host in ONE transfer, where they are divided (exact
    integer sums and one correctly rounded division each, like the host twins' means: the same bits)."""
    gen, real = _device_features(features_1, "manifold_metrics_device"), _device_features(features_2, "manifold_metrics_device")
    parts = (_precision_recall_on_device(gen, real, neighborhood) if neighborhood is not None else []) + \
            (_density_coverage_on_device(gen, real, nearest_k) if nearest_k is not None else [])
    if not parts:
        return {}
    n = [int(v) for v in torch.stack(parts).cpu()]
    ng, nr, out = gen.shape[0], real.shape[0], {}
    if neighborhood is not None:
        p, r = n[0] / ng, n[1] / nr
        out.update({KEY_PRECISION: p, KEY_RECALL: r, KEY_F_SCORE: _f_score(p, r)})
    if nearest_k is not None:
        out.update({KEY_DENSITY: n[-2] / (nearest_k * ng), KEY_COVERAGE: n[-1] / nr})
    return out


def precision_recall_device(features_1: torch.Tensor, features_2: torch.Tensor, neighborhood: int = 3) -> dict:
    """:func:`precision_recall` over fp32 features that stay on the device (:func:`manifold_metrics_device`)."""
    return manifold_metrics_device(features_1, features_2, neighborhood=neighborhood)


def density_coverage_device(features_1: torch.Tensor, features_2: torch.Tensor, nearest_k: int = 5) -> dict:
    """:func:`density_coverage` over fp32 features that stay on the device (:func:`manifold_metrics_device`)."""
    return manifold_metrics_device(features_1, features_2, nearest_k=nearest_k)


def to_uint8(images) -> np.ndarray:
    """What the reference's PNG files hold: ``(images * 255).round().astype("uint8")`` of the pipeline's float NHWC output in [0, 1]
    (utils_training.py:829,915); uint8 arrays pass through."""
    a = images.detach().cpu().numpy() if torch.is_tensor(images) else np.asarray(images)
    if a.dtype == np.uint8:
        return a
    return (a * 255).round().astype("uint8")


def extract_features(net: InceptionV3Features, images, batch_size: int = 64) -> dict:
    """All three feature sets of a set of images (uint8 or float NHWC in [0, 1]), fp64 on the host."""
    u8 = to_uint8(images)
    outs = []
    for i in range(0, len(u8), batch_size):
        o = net(torch.from_numpy(np.ascontiguousarray(u8[i:i + batch_size])).to(net.device))
        outs.append({k: v.double().cpu().numpy() for k, v in o.items()})
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}


def extract_features_device(net: InceptionV3Features, images, batch_size: int = 64) -> dict:
    """:func:`extract_features` without the trip to the host: all three feature sets as fp32 tensors on ``net.device``.  ``images``: what
    :func:`extract_features` takes, or a uint8 tensor already on the device (then nothing passes through the host)."""
    if torch.is_tensor(images) and images.is_cuda and images.dtype == torch.uint8:
        u8 = images
    else:
        u8 = torch.from_numpy(np.ascontiguousarray(to_uint8(images)))
    outs = [net(u8[i:i + batch_size].to(net.device)) for i in range(0, len(u8), batch_size)]
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


def _calculate_metrics_device(net, input1, input2, isc, fid, kid, kid_subset_size, batch_size, input2_features, prc=False,
                              prc_neighborhood=3, dc=False, dc_nearest_k=5) -> dict:
    f1 = extract_features_device(net, input1, batch_size)
    out = {}
    if isc:
        out.update(inception_score(f1["logits_unbiased"].double().cpu().numpy()))
    if fid or kid or prc or dc:
        f2 = input2_features if input2_features is not None else extract_features_device(net, input2, batch_size)
        g1, g2 = f1["2048"], f2["2048"]
        if not torch.is_tensor(g2):      # features cached on the host: fp32 features widened to fp64, so the way back is exact
            g2 = torch.from_numpy(np.ascontiguousarray(g2, dtype=np.float32))
        g2 = g2.to(g1.device)
        if fid:
            out[KEY_FID] = fid_from_statistics(*(t.cpu().numpy() for t in fid_statistics_device(g1)),
                                               *(t.cpu().numpy() for t in fid_statistics_device(g2)))
        if kid:
            out.update(kernel_inception_distance_device(g1, g2, kid_subset_size=kid_subset_size))
        if prc or dc:      # (one transfer of the counts for both pairs)
            out.update(manifold_metrics_device(g1, g2, prc_neighborhood if prc else None, dc_nearest_k if dc else None))
    return out


def calculate_metrics(net: InceptionV3Features, input1, input2=None, *, isc: bool = True, fid: bool = True, kid: bool = False,
                      kid_subset_size: int = 1000, batch_size: int = 64, input2_features: Optional[dict] = None,
                      device_statistics: bool = False, prc: bool = False, prc_neighborhood: int = 3, dc: bool = False,
                      dc_nearest_k: int = 5) -> dict:
    """``torch_fidelity.calculate_metrics(input1=generated, input2=real, isc=, fid=, kid=, kid_subset_size=)`` on image arrays: IS of
    ``input1``; FID / KID between ``input1`` and ``input2``.  ``input2_features``: features of the real images extracted once (what the
    reference gets from ``cache_root`` / ``input2_cache_name``).  ``device_statistics``: the 2048-d features stay on the device and the
    statistics of FID (mean, covariance) and KID (per-subset MMD^2) come from ``pd_feature_moments`` / ``pd_kid_mmd``; the logits go to
    the host for the Inception score, the covariances for the matrix square root; ``input2_features`` may then hold device tensors.
    ``prc`` (``prc_neighborhood``): improved precision / recall / f_score; ``dc`` (``dc_nearest_k``): density / coverage -- both over the
    2048-d features (:func:`precision_recall`, :func:`density_coverage`; ``pd_knn_radii`` / ``pd_manifold_query`` with
    ``device_statistics``).  Both default to off, and nothing of them runs then."""
    if device_statistics:
        return _calculate_metrics_device(net, input1, input2, isc, fid, kid, kid_subset_size, batch_size, input2_features, prc,
                                         prc_neighborhood, dc, dc_nearest_k)
    f1 = extract_features(net, input1, batch_size)
    out = {}
    if isc:
        out.update(inception_score(f1["logits_unbiased"]))
    if fid or kid or prc or dc:
        f2 = input2_features if input2_features is not None else extract_features(net, input2, batch_size)
        if fid:
            out[KEY_FID] = fid_from_statistics(*fid_statistics(f1["2048"]), *fid_statistics(f2["2048"]))
        if kid:
            out.update(kernel_inception_distance(f1["2048"], f2["2048"], kid_subset_size=kid_subset_size))
        if prc:
            out.update(precision_recall(f1["2048"], f2["2048"], prc_neighborhood))
        if dc:
            out.update(density_coverage(f1["2048"], f2["2048"], dc_nearest_k))
    return out


def class_metrics_hook(net: InceptionV3Features, real_images_by_class: Dict[int, Sequence], results: dict, *, isc: bool = True,
                       fid: bool = True, kid: bool = False, kid_subset_size: int = 1000, batch_size: int = 64,
                       device_statistics: bool = False, prc: bool = False, prc_neighborhood: int = 3, dc: bool = False,
                       dc_nearest_k: int = 5):
    """``on_class_done`` callback for :func:`phendiff_amd.eval_generation.generate_samples`: what ``_compute_log_metrics`` does after a
    class's images were generated (utils_training.py:948-1001) -- metrics of that class's generated images against its real images
    (their features cached per class, like ``input2_cache_name``), stored as ``results[f"{metric}/{class_name}"]``.
    ``device_statistics``: as in :func:`calculate_metrics` (the cached features are device tensors then); ``prc`` / ``dc`` and their
    neighbourhood sizes likewise."""
    cache: Dict[int, dict] = {}
    extract = extract_features_device if device_statistics else extract_features

    def done(class_label: int, class_name: str, batches):
        on_device = [getattr(b, "images_u8_device", None) for b in batches]
        if device_statistics and batches and all(t is not None for t in on_device):
            gen = torch.cat(on_device)      # generated on the device (generate_samples(device_noise=...)): the pixels never leave it
        else:
            gen = np.concatenate([to_uint8(b.images) for b in batches])
        if class_label not in cache:
            cache[class_label] = extract(net, real_images_by_class[class_label], batch_size)
        m = calculate_metrics(net, gen, isc=isc, fid=fid, kid=kid, kid_subset_size=kid_subset_size, batch_size=batch_size,
                              input2_features=cache[class_label], device_statistics=device_statistics, prc=prc,
                              prc_neighborhood=prc_neighborhood, dc=dc, dc_nearest_k=dc_nearest_k)
        for k, v in m.items():
            results[f"{k}/{class_name}"] = v
    return done
