"""The re-pack after an optimizer step, replayed on the host (no GPU): for the three trainable families the pack jobs, the
``pre`` steps and the small copies of the re-packer must leave exactly what freshly constructed forward and input-gradient
weight sets hold -- every tensor, bit for bit -- and must write every packed tensor of the training set.

``pd_pack_weight`` itself is replaced by a torch reference written here (``replay``); the kernel is compared against
``packing.py`` by the GPU tests (``test_device_repack_equals_host_packing`` and its SD / VAE counterparts)."""
from types import SimpleNamespace

import pytest
import torch


def lay_out(order):
    """One flat fp32 buffer in the given parameter order, the parameters re-pointed to views of it (as ``FlatAdamWEMA`` does;
    that class needs a device)."""
    flat = torch.empty(sum(p.numel() for _, p in order), dtype=torch.float32)
    off = 0
    for _, p in order:
        k = p.numel()
        flat[off:off + k].copy_(p.detach().reshape(-1))
        p.data = flat[off:off + k].view_as(p)
        off += k
    return flat


def tensors(obj, path):
    """(path, tensor) of every tensor a weight set holds: attributes, dicts of entries, entries, tuples."""
    for k, v in (obj.items() if isinstance(obj, dict) else vars(obj).items()):
        if torch.is_tensor(v):
            yield f"{path}.{k}", v
        elif isinstance(v, (dict, SimpleNamespace)):
            yield from tensors(v, f"{path}.{k}")
        elif isinstance(v, tuple):
            for i, vv in enumerate(v):
                if torch.is_tensor(vv):
                    yield f"{path}.{k}[{i}]", vv


def replay(a, src, dst):
    """Reference of one ``pd_pack_weight`` job: ``pack_conv_weight`` of the source (``src_in`` input channels per row; through
    ``dgrad_weight`` when ``dgrad``) zero-padded to (cout_pad, cin_pad), each 32-row tile written at ``dst + ct * dst_ct_stride``."""
    from phendiff_amd.packing import dgrad_weight, pack_conv_weight
    assert a.src == src.data_ptr() and not a.dst2
    k, rows = a.ksize, (a.cin if a.dgrad else a.cout)
    # (a fused q | k | v source continues behind the first parameter: read the storage, not the view)
    s = torch.as_strided(src.detach(), (rows, a.src_in, k, k), (a.src_in * k * k, k * k, k, 1), src.storage_offset())
    wt = dgrad_weight(s) if a.dgrad else s
    assert tuple(wt.shape[:2]) == (a.cout, a.cin)
    full = torch.zeros((a.cout_pad, a.cin_pad, k, k), dtype=torch.float32)
    full[:a.cout, :a.cin] = wt
    packed = pack_conv_weight(full, dst.dtype)
    off, rem = divmod(a.dst - dst.data_ptr(), dst.element_size())
    assert rem == 0 and off >= 0 and dst.is_contiguous()
    flat, per = dst.view(-1), packed[0].numel()
    assert off + (packed.shape[0] - 1) * a.dst_ct_stride + per <= flat.numel(), "a tile past the end of the destination"
    torch.as_strided(flat, (packed.shape[0], per), (a.dst_ct_stride, 1), off).copy_(packed.reshape(packed.shape[0], per))


def pixel(mode):
    import phendiff_amd as P
    from phendiff_amd.unet import _PackedWeights
    from phendiff_amd.unet_train import TrainWeights, _Repacker, training_param_order
    m = P.CustomCondUNet2DModel(compute_dtype=mode, **dict(P.UNET_CONFIGS["super_small"], sample_size=32))
    sets = lambda: (_PackedWeights(m, "cpu"), TrainWeights(m, "cpu", P.unet._DT[mode][1]))
    return m, training_param_order(m), sets, _Repacker, lambda n: True, lambda path: True


def sd(mode):
    import phendiff_amd as P
    from phendiff_amd.sd_unet import _SDPackedWeights
    from phendiff_amd.sd_unet_train import SDTrainWeights, _SDRepacker, sd_training_param_order
    from test_gpu_sd_unet import TINY
    m = P.SDUNet2DConditionModel(compute_dtype=mode, **TINY)
    sets = lambda: (_SDPackedWeights(m, "cpu"), SDTrainWeights(m, "cpu", P.unet._DT[mode][1]))
    return m, sd_training_param_order(m), sets, _SDRepacker, lambda n: True, lambda path: not path.endswith(".zero_bias")


def vae(mode):
    import phendiff_amd as P
    from phendiff_amd.vae import _VaeWeights
    from phendiff_amd.vae_train import VaeTrainWeights, _VaeRepacker, vae_never_graded, vae_training_param_order
    from test_gpu_vae import CFGS
    m = P.AutoencoderKL(compute_dtype=mode, **CFGS["d64"][0])      # the tiny configuration tests/test_gpu_vae.py encodes / decodes with
    never = vae_never_graded(m)
    sets = lambda: (_VaeWeights(m, "cpu"), VaeTrainWeights(m, "cpu", P.unet._DT[mode][1]))
    # only encoder.* and quant_conv train: the decoder's and post_quant_conv's entries are never re-packed
    trained = lambda path: path.startswith("tw.") or ".encoder." in path or path.split(".")[1].startswith(("enc_", "quant_"))
    return m, vae_training_param_order(m), sets, _VaeRepacker, lambda n: n not in never, trained


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("family", [pixel, sd, vae])
def test_host_replay_of_the_repack_equals_fresh_packing(family, mode):
    torch.manual_seed(0)
    m, order, sets, repacker, trains, trained = family(mode)
    flat = lay_out(order)
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    master = lambda t: lo <= t.data_ptr() < hi          # a view of the flat buffer: a master parameter the kernels read directly
    w, tw = sets()
    rp = repacker(m, w, tw)
    assert len(rp.job_tensors) == len(rp.jobs) > 0
    # 1. perturb every master parameter that trains
    g = torch.Generator().manual_seed(1)
    for n, p in order:
        if trains(n):
            p.data.add_(0.05 * torch.randn(p.shape, generator=g) + 0.01)
    # 2. zero every packed tensor of the training set
    packed = [(path, t) for root, s in (("w", w), ("tw", tw)) for path, t in tensors(s, root) if not master(t) and trained(path)]
    untouched = {path: t.clone() for root, s in (("w", w), ("tw", tw)) for path, t in tensors(s, root) if not master(t) and not trained(path)}
    assert len(packed) > len(rp.jobs) // 2
    for _, t in packed:
        t.zero_()
    # 3. the re-pack, on the host
    with torch.no_grad():
        for f in rp.pre:
            f()
        for a, (src, dst) in zip(rp.jobs, rp.job_tensors):
            replay(a, src, dst)
        for f in rp.small:
            f()
    # 4. exactly what packing.py builds from the new parameters; nothing skipped
    fw, ftw = sets()
    fresh = dict(list(tensors(fw, "w")) + list(tensors(ftw, "tw")))
    have = dict(list(tensors(w, "w")) + list(tensors(tw, "tw")))
    assert set(fresh) == set(have)
    for path, t in have.items():
        if trained(path):
            assert torch.equal(t, fresh[path]), path
    for path, t in packed:
        assert bool(t.count_nonzero()), f"{path}: no pack job or small copy writes it"
    for path, t in untouched.items():
        assert torch.equal(have[path], t), f"{path}: not in the training set, yet the re-pack wrote it"


def test_pack_jobs_pair_up_into_fused_jobs():
    """``fuse_pack_jobs`` folds the input-gradient job of a weight into its forward job (``dst2``); the re-exports of
    ``unet_train`` are the shared functions."""
    from phendiff_amd import unet_train, weight_layout
    assert unet_train.fuse_pack_jobs is weight_layout.fuse_pack_jobs and unet_train.run_pack_jobs is weight_layout.run_pack_jobs
    torch.manual_seed(0)
    m, order, sets, repacker, _, _ = vae("bf16")
    lay_out(order)
    rp = repacker(m, *sets())
    owner = {a.dst: i for i, a in enumerate(rp.jobs)}
    n, ndgrad = len(rp.jobs), sum(1 for a in rp.jobs if a.dgrad)
    fused = weight_layout.fuse_pack_jobs(rp.jobs)
    assert len(fused) == n - ndgrad and all(not a.dgrad for a in fused)          # every dgrad job of the VAE has a forward partner
    for a in fused:
        if a.dst2:
            b = rp.jobs[owner[a.dst2]]
            assert b.dgrad and b.src == a.src and (b.cout, b.cin, b.cout_pad, b.cin_pad) == (a.cin, a.cout, a.cin_pad, a.cout_pad)
            assert a.dst2_ct_stride == b.dst_ct_stride          # the input-gradient copy lands where its own job would have put it
