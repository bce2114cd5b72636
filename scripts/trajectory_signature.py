"""Signature of what the captured-trajectory runners (``DDIBGraph``, ``CFGForwardStartGraph``, ``SDDDIBGraph``, ``GuidedTransferGraph``,
``SDGuidedTransferGraph``) enqueue: every call into the HIP library, in order, argument for argument, from the construction of the model
to the end of two ``run`` calls, plus the sha256 of the runners' outputs.  Two revisions enqueue the same program iff their outputs are
byte-identical:

   python scripts/trajectory_signature.py > head.txt
   python scripts/trajectory_signature.py --tree <export of the other revision, holding a built library> > parent.txt
   cmp parent.txt head.txt

``--tree``: the directory to import ``phendiff_amd`` from (default: this checkout), so that one script file signs both revisions.

A recording proxy stands in for the loaded library (``phendiff_amd._lib._lib``) before any model, plan or runner exists, so every entry
point a plan stores or a runner calls goes through it.  Every runner is built with ``use_graph=False`` (the launches a capture would
record, enqueued on the runner's stream) and run twice, the second time with other labels and inputs.  Per call: the symbol, and per
argument the ctypes struct's type name with every field in ``_fields_`` order.  Pointers (fields, streams, handles) are recorded as null or
a canonical ordinal (the first distinct address met in a case is 0, the next 1, ...), as ``plan_signature.py`` does: the aliasing structure
is compared, allocator addresses are not.  Tiny seeded models and inputs; a few seconds on the GPU."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
_ap.add_argument("--tree", default=ROOT, help="directory to import phendiff_amd from (default: this checkout)")
sys.path.insert(0, os.path.abspath(_ap.parse_args().tree))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import phendiff_amd as P  # noqa: E402
import phendiff_amd._lib as L  # noqa: E402

DEV = "cuda:0"


class RecordingLib:
    """The loaded library with every entry point wrapped: a call is appended to ``self.calls`` and forwarded."""

    def __init__(self, real):
        self._real, self._fns = real, {}
        self.calls, self.ordinals = [], {}

    def reset(self):
        self.calls, self.ordinals = [], {}

    def _pointer(self, v):
        return None if not v else self.ordinals.setdefault(int(v), len(self.ordinals))

    def _argument(self, a):
        if a is None or isinstance(a, int):
            return self._pointer(a)
        obj = getattr(a, "_obj", a)                      # C.byref(struct)
        if isinstance(obj, C.Structure):
            fields = []
            for name, ctype in obj._fields_:
                v = getattr(obj, name)
                fields.append([name, self._pointer(v) if ctype is C.c_void_p else v])
            return [type(obj).__name__, fields]
        if isinstance(obj, C.c_void_p):                  # an out-handle
            return ["c_void_p", self._pointer(obj.value)]
        return [type(obj).__name__]

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            real = getattr(self._real, name)

            def fn(*args):
                if name != "pd_last_error":
                    self.calls.append([name] + [self._argument(a) for a in args])
                return real(*args)
            fn.__name__ = name
            self._fns[name] = fn
        return fn


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def emit(name, rec, runner=None):
    """Flush what was recorded since the last flush under ``name``, with the runner's output hashes."""
    torch.cuda.synchronize()
    print(f"== {name}: {len(rec.calls)} calls")
    for c in rec.calls:
        print(json.dumps(c, separators=(",", ":")))
    if runner is not None:
        for attr in ("images", "inverted", "images_u8", "guided", "guided_latents", "losses"):
            if getattr(runner, attr, None) is not None:
                print(f"sha256 {attr} {sha(getattr(runner, attr))}")
    rec.calls = []


def pixel_pipe(mode, **over):
    torch.manual_seed(0)
    unet = P.CustomCondUNet2DModel(compute_dtype=mode, **dict(P.UNET_CONFIGS["super_small"], sample_size=32, **over)).to(DEV)
    return P.ConditionalDDIMPipeline(unet, P.DDIMScheduler(**P.SCHEDULER_CONFIGS["3k_steps_clipping_rescaling"]))


def images(B, seed, size=32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, size, size, generator=g) * 2 - 1).to(DEV)


def conditioning(kind, B, tdim, seed):
    """Two different conditionings of a batch for the pixel UNet's ``class_embed_type``."""
    g = torch.Generator().manual_seed(seed)
    if kind == "identity":
        return torch.randn(B, tdim, generator=g).to(DEV), torch.randn(B, tdim, generator=g).to(DEV)
    if kind == "timestep":
        a = torch.randint(0, 8, (B,), generator=g).float()
        return a.to(DEV), (a + 1).to(DEV)
    a = torch.randint(0, 2, (B,), generator=g)
    return a.to(DEV), (1 - a).to(DEV)


def ddib_case(name, rec, mode, B, max_batch=None, **over):
    rec.reset()
    pipe = pixel_pipe(mode, **over)
    cls = type(pipe.unet)
    saved = cls.max_batch
    if max_batch is not None:
        cls.max_batch = lambda self, H, W: max_batch
    try:
        runner = P.DDIBGraph(pipe, batch_size=B, num_inference_steps=2, height=32, width=32, use_graph=False)
        emit(f"{name} construct", rec)
        orig, target = conditioning(over.get("class_embed_type"), B, pipe.unet.time_embed_dim, 11)
        for i, cond in enumerate(((orig, target), (target, orig))):
            runner.run(images(B, 1 + i), *cond)
            emit(f"{name} run {i}", rec, runner)
    finally:
        cls.max_batch = saved


def cfg_case(name, rec, eqn, w):
    rec.reset()
    pipe = pixel_pipe("f32")
    B = 3
    runner = P.CFGForwardStartGraph(pipe, batch_size=B, num_inference_steps=4, guidance_scale=w, frac_diffusion_skipped=0.5,
                                    guidance_eqn=eqn, height=32, width=32, use_graph=False)
    emit(f"{name} construct", rec)
    for i, labels in enumerate(conditioning(None, B, 0, 21)):
        noise = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(31 + i)).to(DEV)
        runner.run(images(B, 1 + i), labels, noise)
        emit(f"{name} run {i}", rec, runner)


def guided_case(name, rec, mode, **over):
    """fp16 takes the device-scale path (``pd_lp_guidance_scaled``, the overflow flag of ``pd_guided_step``) and ``settle``."""
    rec.reset()
    pipe = pixel_pipe(mode, **over)
    B = 3
    runner = P.GuidedTransferGraph(pipe, B, 2, 2, 0.5, height=32, width=32, use_graph=False)
    emit(f"{name} construct", rec)
    orig, target = conditioning(over.get("class_embed_type"), B, pipe.unet.time_embed_dim, 61)
    for i, cond in enumerate(((orig, target), (target, orig))):
        runner.run(images(B, 1 + i), *cond)
        emit(f"{name} run {i}", rec, runner)


def sd_pipe(mode):
    from make_golden import SD_SCHED, SD_TINY_UNET, SD_TINY_VAE, sd_tiny_pipe
    ref = sd_tiny_pipe()
    unet = P.SDUNet2DConditionModel(compute_dtype=mode, **SD_TINY_UNET)
    unet.load_state_dict(ref.unet.state_dict())
    vae = P.AutoencoderKL(compute_dtype=mode, **SD_TINY_VAE)
    vae.load_state_dict(ref.vae.state_dict())
    emb = P.CustomEmbedding(2, SD_TINY_UNET["cross_attention_dim"])
    emb.load_state_dict(ref.class_embedding.state_dict())
    return P.CustomStableDiffusionImg2ImgPipeline(vae.to(DEV), unet.to(DEV), P.DDIMScheduler(**SD_SCHED), emb.to(DEV))


def sd_case(name, rec, mode, guided=False):
    rec.reset()
    pipe = sd_pipe(mode)
    B = 2
    if guided:
        runner = P.SDGuidedTransferGraph(pipe, B, 2, 2, 0.5, 32, 32, use_graph=False)
    else:
        runner = P.SDDDIBGraph(pipe, batch_size=B, num_inference_steps=2, height=32, width=32, use_graph=False)
    emit(f"{name} construct", rec)
    orig, target = conditioning(None, B, 0, 41)
    for i, cond in enumerate(((orig, target), (target, orig))):
        noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(51 + i)).to(DEV)
        runner.run(images(B, 1 + i), *cond, noise=noise)
        emit(f"{name} run {i}", rec, runner)


def main():
    print(f"phendiff_amd from {os.path.dirname(P.__file__)}", file=sys.stderr)
    rec = RecordingLib(L.lib())
    L._lib = rec
    ddib_case("ddib_f32", rec, "f32", 3)
    ddib_case("ddib_bf16", rec, "bf16", 3)
    ddib_case("ddib_f32_class_timestep", rec, "f32", 3, class_embed_type="timestep")
    ddib_case("ddib_f32_class_identity", rec, "f32", 3, class_embed_type="identity", num_class_embeds=None)
    ddib_case("ddib_f32_sliced_7_by_3", rec, "f32", 7, max_batch=3)
    cfg_case("cfg_imagen_w2.5", rec, "imagen", 2.5)
    cfg_case("cfg_imagen_w1.0_no_uncond", rec, "imagen", 1.0)
    cfg_case("cfg_CFG_w2.5", rec, "CFG", 2.5)
    sd_case("sd_ddib_f32", rec, "f32")
    sd_case("sd_ddib_bf16", rec, "bf16")
    guided_case("guided_f32", rec, "f32")
    guided_case("guided_fp16", rec, "fp16")
    guided_case("guided_f32_class_identity", rec, "f32", class_embed_type="identity", num_class_embeds=None)
    guided_case("guided_f32_class_timestep", rec, "f32", class_embed_type="timestep")
    sd_case("sd_guided_f32", rec, "f32", guided=True)
    sd_case("sd_guided_bf16", rec, "bf16", guided=True)


if __name__ == "__main__":
    main()
