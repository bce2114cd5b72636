"""`components_to_train autoencoder` (train.py:189-199, 268-285) on the engine -- what needs no GPU: the C ABI of
pd_latent_chain_bwd, the layout of the trainer's flat buffers with a training / frozen autoencoder, accelerate's checkpoint
numbering, and the argument guards of `step_images`."""
import pytest
import torch

from abi_header import define, header_fields

TINY_VAE = dict(block_out_channels=(32, 64), layers_per_block=1)      # the tiny configuration of tests/test_gpu_vae.py


def models():
    import phendiff_amd as P
    from test_gpu_sd_unet import TINY
    torch.manual_seed(0)
    return P.SDUNet2DConditionModel(compute_dtype="f32", **TINY), P.CustomEmbedding(2, TINY["cross_attention_dim"]), \
        P.AutoencoderKL(compute_dtype="f32", **TINY_VAE)


def test_latent_chain_bwd_struct_matches_header_and_is_bound():
    import phendiff_amd._lib as L
    assert header_fields("pd_latent_chain_bwd_args") == [f[0] for f in L.LatentChainBwdArgs._fields_]
    assert "pd_latent_chain_bwd" in L.SYMBOLS and hasattr(L.lib(), "pd_latent_chain_bwd")
    assert define("PD_ABI_VERSION") == L.ABI_VERSION == 8


def test_latent_chain_bwd_validates_before_launching():
    import ctypes as C
    import phendiff_amd._lib as L
    lib = L.lib()
    assert lib.pd_latent_chain_bwd(None, None) == -2
    assert lib.pd_latent_chain_bwd(C.byref(L.LatentChainBwdArgs(dtype=1, B=1, C=4, HW=16, Cpad=4)), None) == -2 and b"Cpad" in lib.pd_last_error()
    assert lib.pd_latent_chain_bwd(C.byref(L.LatentChainBwdArgs(dtype=1, B=1, C=4, HW=16, Cpad=32, pred_type=3)), None) == -1
    assert lib.pd_latent_chain_bwd(C.byref(L.LatentChainBwdArgs(dtype=1, B=1, C=4, HW=16, Cpad=32, pred_type=2)), None) == -1
    assert b"null pointer" in lib.pd_last_error()


def test_flat_layout_vae_denoiser_and_class_embedding():
    """params_to_optimize walks pipeline.components = (vae, unet, class_embedding): VAE first, the class table stays the tail."""
    import phendiff_amd as P
    unet, emb, vae = models()
    order, flags, never, vae_trains = P.sd_training_layout(unet, emb, vae)
    names = [n for n, _ in order]
    nv, nu = len(list(vae.parameters())), len(list(unet.parameters()))
    assert vae_trains and len(names) == nv + nu + 1 and len(set(names)) == len(names)
    assert all(n.startswith("vae.") for n in names[:nv]) and not any(n.startswith("vae.") for n in names[nv:])
    assert names[nv:nv + nu] == [n for n, _ in P.sd_training_param_order(unet)]
    assert names[-1] == "class_embedding.inner_module.weight"
    assert sorted(n[4:] for n in names[:nv]) == sorted(n for n, _ in vae.named_parameters())
    # the fused q | k | v projection of every attention: weights adjacent, then biases
    a = "vae.encoder.mid_block.attentions.0."
    i = names.index(a + "to_q.weight")
    assert names[i:i + 6] == [a + f"{w}.{s}" for s in ("weight", "bias") for w in ("to_q", "to_k", "to_v")]
    assert all(flags)
    assert never == {n for n in names[:nv] if n.startswith("vae.decoder.") or n.startswith("vae.post_quant_conv.")}
    assert never and not any(n.startswith("vae.encoder.") or n.startswith("vae.quant_conv.") for n in never)


def test_flat_layout_vae_only():
    import phendiff_amd as P
    unet, emb, vae = models()
    unet.requires_grad_(False)
    emb.requires_grad_(False)
    order, flags, never, vae_trains = P.sd_training_layout(unet, emb, vae)
    assert vae_trains
    for (n, _), f in zip(order, flags):
        assert f == n.startswith("vae."), n
    assert "vae.decoder.conv_in.weight" in never and "vae.quant_conv.weight" not in never


def test_flat_layout_frozen_vae_is_todays_layout():
    import phendiff_amd as P
    unet, emb, vae = models()
    base = P.sd_training_layout(unet, emb, None)
    vae.requires_grad_(False)                       # train.py:189-191
    order, flags, never, vae_trains = P.sd_training_layout(unet, emb, vae)
    assert not vae_trains and never == frozenset()
    assert [n for n, _ in order] == [n for n, _ in base[0]] and flags == base[1]
    assert not any(n.startswith("vae.") for n, _ in order)
    # an explicit choice that names only decoder parameters cannot train anything of the autoencoder
    with pytest.raises(ValueError, match="never receive a gradient"):
        P.sd_training_layout(unet, emb, vae, trainable=["vae.decoder.conv_in.weight"])


def test_checkpoint_modules_numbering():
    """accelerate numbers the prepared models unet 0, vae 1, class_embedding 2 (train.py:318-326)."""
    import phendiff_amd as P
    from phendiff_amd.sd_unet_train import sd_checkpoint_modules
    unet, emb, vae = models()
    names = [n for n, _ in P.sd_training_layout(unet, emb, vae)[0]]
    mods = sd_checkpoint_modules(unet, emb, vae, names)
    assert {i: (m, p) for i, m, p in mods} == {0: (unet, ""), 1: (vae, "vae."), 2: (emb, "class_embedding.")}
    assert [i for i, _, _ in mods] == [1, 0, 2]      # the optimizer's parameter order: vae, unet, class embedding
    covered = [p + n for _, m, p in mods for n, _ in m.named_parameters()]
    assert sorted(covered) == sorted(names)
    vae.requires_grad_(False)
    names = [n for n, _ in P.sd_training_layout(unet, emb, vae)[0]]
    assert [i for i, _, _ in sd_checkpoint_modules(unet, emb, vae, names)] == [0, 2]
    assert [i for i, _, _ in sd_checkpoint_modules(unet, emb, None, names)] == [0, 2]


def test_step_images_argument_guards():
    import phendiff_amd as P
    from phendiff_amd.sd_unet_train import check_training_images
    unet, emb, vae = models()
    with pytest.raises(P.PhenDiffHipError, match="MI355X"):
        check_training_images(vae, torch.zeros(2, 3, 32, 32))               # a CPU tensor: there is no CPU fallback
    with pytest.raises(ValueError, match=r"\(B, 3, H, W\)"):
        check_training_images(vae, torch.zeros(2, 4, 32, 32))
    with pytest.raises(ValueError, match="multiple of 2"):
        check_training_images(vae, torch.zeros(2, 3, 33, 32))
    tr = P.SDUNetTrainer.__new__(P.SDUNetTrainer)                            # (a trainer cannot be built without a device)
    tr.vae = None
    with pytest.raises(ValueError, match="vae=pipeline.vae"):
        tr.step_images(torch.zeros(2, 3, 32, 32), None, None, None)
    with pytest.raises(TypeError):
        P.AutoencoderKL(compute_dtype="f32", nonsense=1)
