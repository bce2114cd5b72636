"""Signature of the launch plans the training code lays out: every op of ``plan.ops`` and ``plan.bwd_ops`` field for field, plus the
gradient-ready schedule.  Nothing is launched.  Two revisions lay out the same program iff their outputs are byte-identical:

   python scripts/plan_signature.py > head.json        (and the same file, unchanged, on a checkout of the other revision)
   diff parent.json head.json

Per op: ``what`` / ``side`` / ``ctx`` / FLOPs / bytes, the entry point's name, the ctypes struct's type name and every field in
``_fields_`` order.  Pointer fields are recorded as null or a canonical ordinal (the first distinct address met while walking the plan is 0,
the next 1, ...): the aliasing structure is compared, allocator addresses are not.  ``--check`` only verifies that the fp32 ``super_small``
plan reaches the emitter branches a change of the backward emitters has to cover."""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phendiff_amd as P  # noqa: E402
from phendiff_amd.unet_train import UNetTrainer  # noqa: E402

DEV = "cuda:0"
SD_TINY = dict(in_channels=4, out_channels=4, block_out_channels=(64, 128), layers_per_block=1,
               down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
               attention_head_dim=(1, 2), cross_attention_dim=96, norm_num_groups=32)
VAE_TINY = dict(block_out_channels=(32, 64), layers_per_block=1)


def op_record(op, ordinals):
    fields = []
    for name, ctype in op.args._fields_:
        v = getattr(op.args, name)
        if ctype is C.c_void_p:
            v = None if not v else ordinals.setdefault(v, len(ordinals))
        fields.append([name, v])
    return dict(what=op.what, side=bool(op.side), ctx=bool(op.ctx), flops=op.flops, bytes=op.bytes, fn=getattr(op.fn, "__name__", None),
                struct=type(op.args).__name__, fields=fields)


def plan_record(plan):
    ordinals = {}
    return dict(ops=[op_record(op, ordinals) for op in plan.ops], bwd_ops=[op_record(op, ordinals) for op in plan.bwd_ops],
                grad_ready=dict(sorted(plan.grad_ready.items())), class_mlp_ops=list(getattr(plan, "_class_mlp_ops", (0, 0))),
                emb_grad_at=getattr(plan, "_emb_grad_at", -1))


def pixel_model(mode, size=32, **over):
    torch.manual_seed(0)
    return P.CustomCondUNet2DModel(compute_dtype=mode, **dict(P.UNET_CONFIGS["super_small"], sample_size=size, **over)).to(DEV)


def pixel_plan(mode, attention_only=False, **over):
    m = pixel_model(mode, **over)
    if attention_only:        # --attention_fine_tuning: freeze everything, re-enable the blocks' attentions
        m.requires_grad_(False)
        for mod in m.modules():
            if hasattr(mod, "attentions"):
                mod.attentions.requires_grad_(True)
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"])
    return UNetTrainer(m, sched, lr=1e-4, use_ema=False).plan_for(2, 32, 32)


def sd_plans(train_class_embedding=True, vae=False):
    torch.manual_seed(0)
    m = P.SDUNet2DConditionModel(compute_dtype="f32", **SD_TINY).to(DEV)
    emb = P.CustomEmbedding(2, SD_TINY["cross_attention_dim"]).to(DEV)
    v = P.AutoencoderKL(compute_dtype="f32", **VAE_TINY).to(DEV) if vae else None
    sched = P.DDIMScheduler(**P.SCHEDULER_CONFIGS["SD_orig_config"])
    tr = P.SDUNetTrainer(m, emb, sched, lr=1e-4, use_ema=False, train_class_embedding=train_class_embedding, vae=v)
    plans = [tr.plan_for(2, 16, 16)]
    if vae:
        plans.append(tr.vae_plan_for(2, 32, 32))
    return plans


def vae_encoder_plan():
    from phendiff_amd.training import FlatAdamWEMA
    from phendiff_amd.vae import _VaeWeights
    from phendiff_amd.vae_train import VaeEncodeTrainPlan, VaeTrainWeights, vae_never_graded
    torch.manual_seed(0)
    m = P.AutoencoderKL(compute_dtype="f32", **VAE_TINY).to(DEV)
    order = P.vae_training_param_order(m)
    FlatAdamWEMA([p for _, p in order], 0.0, use_ema=False)
    params, grads = {n: p.data for n, p in order}, {n: p.grad for n, p in order}
    m.invalidate()
    m._weights = _VaeWeights(m, m.device)
    tw = VaeTrainWeights(m, m.device, m._weights.tdt)
    return VaeEncodeTrainPlan(m, m._weights, tw, 2, 32, 32, m.device, params, grads, frozen=vae_never_graded(m))


def check_branches(plan):
    """The fp32 ``super_small`` backward at 32 x 32 holds every branch of the weight-gradient / bias-gradient emitters."""
    kinds = [op.what for op in plan.bwd_ops]
    missing = [k for k in ("gn_apply_bwd", "channel_sum_fused", "pool2x2") if k not in kinds]
    if not any(k.endswith("_fold") and op.side for k, op in zip(kinds, plan.bwd_ops)):
        missing.append("*_fold side ops")
    if not any(kinds[i:i + 8] == ["wgrad2x2", "wgrad2x2_fold"] * 4 for i in range(len(kinds))):
        missing.append("four consecutive wgrad2x2 pairs")
    if missing:
        raise SystemExit(f"plan_signature: the fp32 super_small plan does not reach {missing}")


def main():
    full = pixel_plan("f32")
    check_branches(full)
    if "--check" in sys.argv[1:]:
        print("branches ok")
        return
    variant = dict(center_input_sample=True, resnet_time_scale_shift="scale_shift", class_embed_type="timestep")
    plans = {
        "pixel_f32": full,
        "pixel_bf16": pixel_plan("bf16"),
        "pixel_f32_attention_only": pixel_plan("f32", attention_only=True),
        "pixel_f32_input_grad": pixel_model("f32").input_grad_plan(2, 32, 32, torch.device(DEV)),
        "pixel_f32_head_dim_16": pixel_plan("f32", attention_head_dim=16),
        "pixel_f32_one_wide_head": pixel_plan("f32", attention_head_dim=None),
        "pixel_f32_centered_scale_shift_class_mlp": pixel_plan("f32", **variant),
        "pixel_f32_centered_input_grad": pixel_model("f32", **variant).input_grad_plan(2, 32, 32, torch.device(DEV)),
        "sd_tiny": sd_plans()[0],
        "sd_tiny_no_class_table": sd_plans(train_class_embedding=False)[0],
        "vae_encoder": vae_encoder_plan(),
    }
    plans["sd_tiny_training_vae"], plans["sd_tiny_training_vae_encoder"] = sd_plans(vae=True)
    json.dump({name: plan_record(p) for name, p in plans.items()}, sys.stdout, indent=0, sort_keys=False)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
