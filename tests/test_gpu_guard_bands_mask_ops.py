"""Guard bands (tests/guard_bands.py) around the operands of the four mask-refinement entry points: pd_mask_distance, pd_mask_morph,
pd_mask_components, pd_mask_filter.  Shapes 37 x 53 and 1 x 53 at B = 3: the last partial row or column and the sample boundary are what
can go wrong.  Masks and results are integers, so the properties of tests/test_gpu_guard_bands.py read:

  P2 canaried outputs    every output AND every workspace sits between two 64 KiB canaries; the bodies are pre-filled with a byte pattern
                         (0xA5, then 0x5A).  The canaries survive, and the outputs equal the reference under both fills -- so every element
                         is written.
  P1 / P3 for masks      the mask's surroundings (0xFF instead of zeros) and a neighbouring sample (0xFF bytes: all set) change nothing
                         in the other samples' results.
Guard size: 64 KiB before and after every operand -- more than two whole samples of 37 x 53 int32 words."""
import ctypes as C

import numpy as np
import pytest
import torch

import phendiff_amd._lib as L
from guard_bands import MIN_GUARD_BYTES, guarded
from mask_ops_cases import CASES, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"37x53": "shapes_37x53", "random_37x53": "random_37x53", "1x53": "random_1x53", "extremes_1x53": "extremes_1x53"}
assert 2 * 37 * 53 * 4 < MIN_GUARD_BYTES


def st():
    return torch.cuda.current_stream().cuda_stream


class Run:
    """One entry point over guarded operands: `outs` name -> (shape, dtype); call(T) launches with the guarded views T."""

    def __init__(self, mask_np, outs, call):
        self.T, self.H, self.outs, self.call = {}, {}, outs, call
        self.T["mask"], self.H["mask"] = guarded(torch.from_numpy(mask_np.copy()), MIN_GUARD_BYTES, DEV, "mask")
        for name, (shape, dtype) in outs.items():
            self.T[name], self.H[name] = guarded(torch.zeros(shape, dtype=dtype), MIN_GUARD_BYTES, DEV, name)

    def run(self, fill=0xA5):
        for name in self.outs:
            self.T[name].view(torch.uint8).fill_(fill)
            self.H[name].canary()
        self.call(self.T)
        torch.cuda.synchronize()
        for name in self.outs:
            assert self.H[name].intact()
        return {name: self.T[name].cpu().numpy().copy() for name in self.outs}


def entry_points(name):
    """(id, outputs, launch, expected results by output name) for every entry point over case `name`."""
    from phendiff_amd import mask_ops as M
    m = CASES[name]
    B, H, W = m.shape
    lib = L.lib()
    i32, u8 = torch.int32, torch.uint8
    full = (B, H, W)
    out = []

    def distance(T):
        L.check(lib.pd_mask_distance(C.byref(M.mask_distance_args(T["mask"], T["d2"], True, 0, B, H, W)), st()), "pd_mask_distance")
    out.append(("distance", {"d2": (full, i32)}, distance, {"d2": reference(name, "d2", True)}))

    def distance_limit(T):
        L.check(lib.pd_mask_distance(C.byref(M.mask_distance_args(T["mask"], T["d2"], False, 4, B, H, W)), st()), "pd_mask_distance")
    ref = reference(name, "d2", False)
    out.append(("distance_limit", {"d2": (full, i32)}, distance_limit, {"d2": np.where(ref > 4, 5, ref)}))

    for op, what in ((M.DILATE, "dilate"), (M.ERODE, "erode")):
        def morph(T, op=op):
            a = M.mask_morph_args(T["mask"], T["out"], op, 8, T["workspace"], B, H, W, stats=T["stats"], stats_stride=5, stats_mode=M.STATS_IN | M.STATS_OUT)
            L.check(lib.pd_mask_morph(C.byref(a), st()), "pd_mask_morph")
        want = reference(name, what, 8)
        stats = np.zeros((B, 5), np.int32)
        stats[:, 0], stats[:, 1] = (m != 0).reshape(B, -1).sum(1), want.reshape(B, -1).sum(1)
        out.append((what, {"out": (full, u8), "workspace": (full, i32), "stats": ((B, 5), i32)}, morph, {"out": want, "stats": stats}))

    for conn, phase in ((8, 1), (4, 0)):
        def components(T, conn=conn, phase=phase):
            a = M.mask_components_args(T["mask"], phase, conn, T["workspace"], B, H, W, T["label"], T["area"], T["border"], T["count"], T["status"])
            L.check(lib.pd_mask_components(C.byref(a), st()), "pd_mask_components")
        label, area, border, count = reference(name, "label", conn, phase)
        out.append((f"components{conn}{phase}", {"label": (full, i32), "area": (full, i32), "border": (full, u8), "count": ((B,), i32), "status": ((B,), i32),
                                                 "workspace": ((2, B, H * W), i32)}, components,
                    {"label": label, "area": area, "border": border, "count": count, "status": np.zeros((B,), np.int32)}))

    for rule, phase, conn, limit, what, args in ((M.DROP_SMALL, 1, 8, 3, "drop_small", (3, 8)), (M.FILL_HOLES, 0, 4, -1, "fill_holes", (None, 8))):
        label, area, border, _ = reference(name, "label", conn, phase)
        lab = [torch.from_numpy(v.copy()).to(DEV) for v in (label, area, border)]

        def filt(T, rule=rule, limit=limit, lab=lab):
            a = M.mask_filter_args(T["mask"], lab[0], lab[1], lab[2], rule, limit, T["out"], B, H, W, stats=T["stats"], stats_stride=5)
            L.check(lib.pd_mask_filter(C.byref(a), st()), "pd_mask_filter")
        want, stats = reference(name, what, *args)
        out.append((what, {"out": (full, u8), "stats": ((B, 5), i32)}, filt, {"out": want, "stats": stats}))
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
def test_p2_canaried_outputs(shape):
    name = SHAPES[shape]
    for ident, outs, call, want in entry_points(name):
        r = Run(CASES[name], outs, call)
        for fill in (0xA5, 0x5A):
            got = r.run(fill)
            for k, ref in want.items():
                assert np.array_equal(got[k], ref), (ident, k, hex(fill), int((got[k] != ref).sum()))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_p3_a_neighbouring_sample_of_ff_bytes_changes_nothing(shape):
    name = SHAPES[shape]
    m = CASES[name]
    B = m.shape[0]
    for ident, outs, call, want in entry_points(name):
        if ident in ("drop_small", "fill_holes"):
            continue      # (their label / area / border inputs belong to the mask: the filter is elementwise; P2 covers it)
        r = Run(m, outs, call)
        r.H["mask"].clear()
        base = r.run()
        r.H["mask"].poison()      # 0xFF all around the mask
        poisoned = r.run()
        for k in want:
            assert np.array_equal(base[k], poisoned[k]), (ident, k)
        for i in range(B):
            saved = r.T["mask"][i].clone()
            r.T["mask"][i].fill_(0xFF)
            got = r.run()
            r.T["mask"][i].copy_(saved)
            for k in want:
                others = [j for j in range(B) if j != i]
                assert np.array_equal(got[k][others], base[k][others]), (ident, k, i)
