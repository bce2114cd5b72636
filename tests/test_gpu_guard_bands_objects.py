"""Guard bands (tests/guard_bands.py) around the operands of the three per-object entry points: pd_object_index, pd_object_geometry,
pd_object_intensity.  Shapes 37 x 53 and 1 x 53 at B = 3 with K = 13 table rows (a multiple of nothing; the checkerboard overflows it):
the last partial tile, row or wave and the sample boundary are what can go wrong.

  P2 canaried outputs    every output AND the workspace sits between two 64 KiB canaries; the bodies are pre-filled with a byte pattern
                         (0xA5, then 0x5A).  The canaries survive, and the outputs equal the reference under both fills -- so every
                         element is written.
  P1 / P3 for inputs     the inputs' surroundings (0xFF bytes around integers, NaN around the images, instead of zeros) change no output
                         bit; a neighbouring sample of 0xFF bytes (labels and indices of -1: followed nowhere) or of NaN changes nothing
                         in the other samples' results."""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_ops_cases as MC
import objects_ref as O
import phendiff_amd._lib as L
from guard_bands import MIN_GUARD_BYTES, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 13
SHAPES = {"37x53_conn4": ("shapes_37x53", 4), "37x53_conn8": ("random_37x53", 8), "1x53": ("random_1x53", 8), "extremes_1x53": ("extremes_1x53", 4)}
assert 2 * 37 * 53 * 4 < MIN_GUARD_BYTES


def st():
    return torch.cuda.current_stream().cuda_stream


class Run:
    """One entry point over guarded operands: `ins` name -> array, `outs` name -> (shape, dtype); call(T) launches with the guarded views."""

    def __init__(self, ins, outs, call):
        self.T, self.H, self.ins, self.outs, self.call = {}, {}, ins, outs, call
        for name, arr in ins.items():
            self.T[name], self.H[name] = guarded(torch.from_numpy(arr.copy()), MIN_GUARD_BYTES, DEV, name)
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


def entry_points(name, conn):
    """(id, inputs, outputs, launch, expected by output name, the input a sample of which is overwritten) per entry point."""
    from phendiff_amd import objects as M
    B, H, W = MC.CASES[name].shape
    lib = L.lib()
    label = MC.reference(name, "label", conn, 1)[0]
    index, count, status, geom = O.reference(name, conn, K)
    img = O.images(name, "f32")
    table, bound = O.reference(name, conn, K, "f32")
    Cn = img.shape[1]
    i32 = torch.int32
    assert (count > K).any() or name != "shapes_37x53"
    out = []

    def do_index(T):
        a = M.object_index_args(T["label"], T["index"], T["count"], T["status"], T["workspace"], K, B, H, W)
        L.check(lib.pd_object_index(C.byref(a), st()), "pd_object_index")
    ws = lib.pd_object_index_workspace(B, H, W) // 4
    out.append(("index", {"label": label}, {"index": ((B, H, W), i32), "count": ((B,), i32), "status": ((B,), i32), "workspace": ((ws,), i32)}, do_index,
                {"index": index, "count": count, "status": status}, "label"))

    def do_geometry(T):
        L.check(lib.pd_object_geometry(C.byref(M.object_geometry_args(T["index"], T["geometry"], K, B, H, W)), st()), "pd_object_geometry")
    out.append(("geometry", {"index": index}, {"geometry": ((B, K, 12), torch.int64)}, do_geometry, {"geometry": geom}, "index"))

    def do_intensity(T):
        a = M.object_intensity_args(T["index"], T["geometry"], T["images"], T["out"], K, B, H, W, Cn, torch.float32)
        L.check(lib.pd_object_intensity(C.byref(a), st()), "pd_object_intensity")
    out.append(("intensity", {"index": index, "geometry": geom, "images": img}, {"out": ((B, K, Cn, 4), torch.float64)}, do_intensity,
                {"out": (table, bound)}, "images"))
    return out


def agrees(got, ref):
    if isinstance(ref, tuple):      # the intensity table: min and max exact, the two sums within the summation bound
        table, bound = ref
        return np.array_equal(got[..., 2:], table[..., 2:]) and bool((np.abs(got[..., :2] - table[..., :2]) <= bound).all())
    return got.dtype == ref.dtype and np.array_equal(got, ref)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_p2_canaried_outputs(shape):
    for ident, ins, outs, call, want, _ in entry_points(*SHAPES[shape]):
        r = Run(ins, outs, call)
        first = None
        for fill in (0xA5, 0x5A):
            got = r.run(fill)
            for k, ref in want.items():
                assert agrees(got[k], ref), (ident, k, hex(fill))
                assert first is None or got[k].tobytes() == first[k].tobytes(), (ident, k)      # every element is written: no fill byte survives
            first = got


@pytest.mark.parametrize("shape", list(SHAPES))
def test_p1_p3_poisoned_surroundings_and_neighbouring_samples_change_nothing(shape):
    name, conn = SHAPES[shape]
    B = MC.CASES[name].shape[0]
    for ident, ins, outs, call, want, victim in entry_points(name, conn):
        r = Run(ins, outs, call)
        for n in ins:
            r.H[n].clear()
        base = r.run()
        for n in ins:
            r.H[n].poison()      # 0xFF around the integer inputs, NaN around the images
        poisoned = r.run()
        for k in want:
            assert base[k].tobytes() == poisoned[k].tobytes(), (ident, k)
        for i in range(B):
            saved = r.T[victim][i].clone()
            r.T[victim][i].view(torch.uint8).fill_(0xFF)      # labels / indices of -1, or NaN values
            got = r.run()
            r.T[victim][i].copy_(saved)
            others = [j for j in range(B) if j != i]
            for k in want:
                assert got[k][others].tobytes() == base[k][others].tobytes(), (ident, k, i)
            if ident == "index":      # a label of -1 is followed nowhere: index 0 and the flag, the count is that of the roots (none)
                assert not got["index"][i].any() and got["count"][i] == 0 and got["status"][i] == L.CONSTANTS["PD_OBJ_BAD_LABEL"]
            if ident == "geometry":   # an index outside 0..K is read as 0
                assert not got["geometry"][i].any()
