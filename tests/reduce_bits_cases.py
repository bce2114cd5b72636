"""Cases, seeded inputs and launch helpers shared by tests/test_gpu_reduce_bits.py and scripts/record_reduce_bits.py: the entry points
whose fp64 (and integer) reductions run through csrc/pd_reduce.h -- pd_sample_stats, pd_guidance_rescale, pd_contrast_mask, pd_ssim,
pd_object_intensity, pd_kid_mmd and the statistics rows of pd_mask_morph / pd_mask_filter -- compared BIT FOR BIT with what the kernels
of the revision before they were put on that header wrote under tests/golden/reduce_bits/.

Inputs are element-wise operations on seeded numpy draws, row b scaled by ROW_SCALE[b % 3] (step_bits_cases) so that rows differ; every
fixture carries the sha256 of the inputs it was recorded on.  The shapes are the smallest at which the shared pieces can go wrong: one
element, a tail only, one chunk exactly, a chunk plus one element, odd row lengths at B >= 2 (slots taken by the 16-byte access and by
element accesses), and per entry point samples of more than 256 partial records, where the run fold takes runs of two records: 256 chunks
and 5 (or 3) elements = 257 records = 128 runs and a last one of a single record, 257 chunks and 5 elements = 258 records = 129 whole
runs; 17 x 16 = 272 tiles = 136 whole runs, 17 x 17 = 289 tiles = 144 runs and a last one of a single tile."""
import ctypes as C
import hashlib
import os

import numpy as np
import torch

from step_bits_cases import ROW_SCALE, SAMPLE_ABOVE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduce_bits")
KINDS = ("sample_stats", "guidance_rescale", "contrast_mask", "ssim", "object_intensity", "kid_mmd", "mask_stats")
CHUNK = {"sample_stats": 8192, "guidance_rescale": 8192, "contrast_mask": 2048}      # checked against the library's in run_case
SSIM_TILE = (16, 32)                             # valid positions per workgroup
F32 = np.float32
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "u8": torch.uint8, "u16": torch.uint16}
EDGES100 = np.linspace(-3.0, 3.0, 101)
PHI, RATIO = 0.7, 3.0
W1, W3 = (2.5,), (0.5, 1.7, 3.0)
SSIM_SIGMA = {3: 0.5, 7: 1.0, 11: 1.5}
K_OBJECTS = 1024


def run_split(count):
    """pd_reduce.h's run fold, restated: (per, runs, records in the last run) of ``count`` partial records."""
    per = (count + 255) // 256
    runs = (count + per - 1) // per
    return per, runs, count - (runs - 1) * per


def records_of(name):
    """Partial records per sample of a case that has them (chunks, or tiles of scale 0), else None."""
    kind, s = CASES[name]
    if kind in CHUNK:
        return (s["n"] + CHUNK[kind] - 1) // CHUNK[kind]
    if kind == "ssim":
        return -(-(s["H"] - s["win"] + 1) // SSIM_TILE[0]) * -(-(s["W"] - s["win"] + 1) // SSIM_TILE[1])
    return None


def slot_accesses(B, n, chunk, vec, itemsize):
    """load_slot / store_slot restated: (slots taken by the 16-byte access, slots taken by element accesses) over a [B][n] tensor whose
    base is 16-byte aligned: a slot of ``vec`` elements starts at every multiple of ``vec`` within a chunk of a row."""
    wide = narrow = 0
    for b in range(B):
        for j0 in range(0, n, chunk):
            e0 = np.arange(0, min(chunk, n - j0), vec)
            whole = (min(chunk, n - j0) - e0 >= vec) & (((b * n + j0 + e0) * itemsize) % 16 == 0)
            wide += int(whole.sum())
            narrow += int((~whole).sum())
    return wide, narrow


def _build_cases():
    """name -> (kind, settings)."""
    cases = {}
    ck = CHUNK["sample_stats"]
    for B, n in [(1, 1), (1, 3), (1, 1023), (1, ck), (1, ck + 1), (3, 75), (3, 2 * ck + 5), (2, 256 * ck + 5), (2, 257 * ck + 5)]:
        for y, bins in ((None, 0), ("per", 100)):
            cases[f"ss_{B}x{n}_f32_y{y}_b{bins}"] = ("sample_stats", dict(B=B, n=n, dtype="f32", y=y, bins=bins, special=False))
    for n in (75, 2 * ck + 5):
        cases[f"ss_3x{n}_f32_yshared_b100"] = ("sample_stats", dict(B=3, n=n, dtype="f32", y="shared", bins=100, special=False))
        cases[f"ss_3x{n}_f32_yper_b100_special"] = ("sample_stats", dict(B=3, n=n, dtype="f32", y="per", bins=100, special=True))
        for dt in ("bf16", "f16"):
            cases[f"ss_3x{n}_{dt}_yNone_b0"] = ("sample_stats", dict(B=3, n=n, dtype=dt, y=None, bins=0, special=False))
            cases[f"ss_3x{n}_{dt}_yper_b100"] = ("sample_stats", dict(B=3, n=n, dtype=dt, y="per", bins=100, special=False))
    ck = CHUNK["guidance_rescale"]
    for B, n in [(1, 2), (1, 3), (3, 75), (1, ck), (3, ck + 1), (2, 256 * ck + 5), (2, 257 * ck + 5)]:
        cases[f"gr_{B}x{n}"] = ("guidance_rescale", dict(B=B, n=n, constant_row=None))
    for n in (75, ck + 1):
        cases[f"gr_3x{n}_constant_row"] = ("guidance_rescale", dict(B=3, n=n, constant_row=1))
    ck = CHUNK["contrast_mask"]
    for B, n in [(1, 1), (1, 5), (1, ck), (1, ck + 1), (1, 4087), (2, 256 * ck + 3), (2, 257 * ck + 3), (3, 67 * 61)]:
        cases[f"cm_{B}x{n}"] = ("contrast_mask", dict(B=B, n=n, zero_row=None))
    cases["cm_3x4087_zero_sample"] = ("contrast_mask", dict(B=3, n=67 * 61, zero_row=1))
    ssim = lambda B, Cc, H, W, win, levels, dtype="f32", shared=False: ("ssim", dict(B=B, C=Cc, H=H, W=W, win=win, levels=levels, dtype=dtype, shared=shared))  # noqa: E731
    cases["ssim_1x1x11x11_w11"] = ssim(1, 1, 11, 11, 11, 1)      # one position
    for dt in ("f32", "bf16", "f16"):
        cases[f"ssim_2x3x37x53_w11_l1_{dt}"] = ssim(2, 3, 37, 53, 11, 1, dt)
        cases[f"ssim_2x3x37x53_w7_l3_{dt}"] = ssim(2, 3, 37, 53, 7, 3, dt)      # (three scales leave 9 x 13: the 11-tap window does not fit)
    cases["ssim_2x3x37x53_w3_l3"] = ssim(2, 3, 37, 53, 3, 3)
    cases["ssim_2x3x37x53_w11_shared"] = ssim(2, 3, 37, 53, 11, 1, shared=True)
    cases["ssim_1x1x282x522_w11"] = ssim(1, 1, 282, 522, 11, 1)      # 17 x 16 = 272 tiles
    cases["ssim_1x1x282x554_w11"] = ssim(1, 1, 282, 554, 11, 1)      # 17 x 17 = 289 tiles: the last run is a single tile
    for mask in ("shapes_37x53", "speckled_64x64", "hand_40x48"):
        for conn in (4, 8):
            for img in ("f32", "u8", "u16"):
                cases[f"oi_{mask}_c{conn}_{img}"] = ("object_intensity", dict(mask=mask, conn=conn, img=img, K=K_OBJECTS, nan=False))
    cases["oi_hand_40x48_c8_f32_nan"] = ("object_intensity", dict(mask="hand_40x48", conn=8, img="f32", K=K_OBJECTS, nan=True))
    cases["oi_speckled_64x64_c8_f32_K3"] = ("object_intensity", dict(mask="speckled_64x64", conn=8, img="f32", K=3, nan=False))
    for i in (0, 1):
        cases[f"kid_{i}"] = ("kid_mmd", dict(index=i))
    cases["ms_speckled_64x64_recipe0"] = ("mask_stats", dict(mask="speckled_64x64", recipe=0))
    return cases


CASES = _build_cases()
LONG_FOLD = [n for n in CASES if records_of(n) is not None and records_of(n) > 256]      # the cases whose run fold takes per >= 2


def cases_of(kind):
    return [n for n, c in CASES.items() if c[0] == kind]


def _rng(*key):
    return np.random.default_rng([20250, *key])


def _rows(B):
    return np.array([ROW_SCALE[b % 3] for b in range(B)], dtype=F32)[:, None]


HAND_OBJECTS = ((3, 8, 5, 12), (15, 35, 10, 40))      # (y0, y1, x0, x1) of a 5 x 7 box (35 pixels) and a 20 x 30 one (600)
HAND_NAN_INSIDE, HAND_NAN_OUTSIDE = (0, 1, 20, 20), (1, 0, 15, 10)      # (sample, channel, y, x): in the large object; in its box's cut corner


def hand_mask():
    """(2, 40, 48) uint8: a bounding box of fewer than 256 pixels (lanes see 0 or 1 of them) and one of more (lanes see several); the
    second sample holds the first one's boxes with a corner cut off each, so that its boxes hold pixels of no object."""
    m = np.zeros((2, 40, 48), np.uint8)
    for y0, y1, x0, x1 in HAND_OBJECTS:
        m[:, y0:y1, x0:x1] = 1
        m[1, y0:y0 + 2, x0:x0 + 3] = 0
    return m


def mask_of(name):
    from mask_ops_cases import CASES as MASKS
    return hand_mask() if name == "hand_40x48" else MASKS[name]


def make_inputs(name):
    """The case's CPU arrays (float operands as fp32: a bf16 / f16 case rounds them on the way to the device)."""
    kind, s = CASES[name]
    if kind == "sample_stats":
        B, n = s["B"], s["n"]
        g = _rng(1, B, n)
        t = {"x": (g.standard_normal((B, n)) * _rows(B)).astype(F32)}
        if s["y"]:
            noise = (0.1 * g.standard_normal((B, n))).astype(F32)
            t["y"] = (t["x"][0] + noise[0]) if s["y"] == "shared" else (t["x"] + noise)
        if s["special"]:
            t["x"][1, n // 3], t["x"][1, n // 2] = np.nan, np.inf
            t["x"][2] = -0.0
        return t
    if kind == "guidance_rescale":
        B, n = s["B"], s["n"]
        g = _rng(2, B, n)
        cond = ((0.2 + g.standard_normal((B, n))) * _rows(B)).astype(F32)
        uncond = (F32(0.8) * cond + F32(0.1) + (0.4 * g.standard_normal((B, n))).astype(F32) * _rows(B)).astype(F32)
        if s["constant_row"] is not None:
            cond[s["constant_row"]], uncond[s["constant_row"]] = F32(0.3), F32(0.1)
        return {"cond": cond, "uncond": uncond}
    if kind == "contrast_mask":
        B, n = s["B"], s["n"]
        acc = (np.abs(_rng(3, B, n).standard_normal((B, n))) * _rows(B)).astype(F32)
        if s["zero_row"] is not None:
            acc[s["zero_row"]] = 0.0
        return {"acc": acc}
    if kind == "ssim":
        shape = (s["B"], s["C"], s["H"], s["W"])
        g = _rng(4, *shape)
        x = (0.4 * g.standard_normal(shape)).astype(F32) * _rows(s["B"])[:, :, None, None]
        y = x + (0.15 * g.standard_normal(shape)).astype(F32)
        return {"x": x.astype(F32), "y": (y[-1] if s["shared"] else y).astype(F32)}
    if kind == "object_intensity":
        m = mask_of(s["mask"])
        shape = (m.shape[0], 3, *m.shape[1:])
        g = _rng(5, *shape, len(s["img"]))
        if s["img"] == "f32":
            img = ((g.standard_normal(shape) + np.array([0.0, 1000.0, -3.0])[None, :, None, None]) * _rows(shape[0])[:, :, None, None]).astype(F32)
            if s["nan"]:
                img[HAND_NAN_INSIDE] = img[HAND_NAN_OUTSIDE] = np.nan
        else:
            img = g.integers(0, 256 if s["img"] == "u8" else 65536, shape).astype(np.uint8 if s["img"] == "u8" else np.uint16)
        return {"mask": np.ascontiguousarray(m), "images": img}
    if kind == "kid_mmd":
        from test_gpu_metric_stats import KID_CASES, features, tables
        n1, n2, m, D, S = KID_CASES[s["index"]][:5]
        i1, i2 = tables(n1, n2, S, m, 13)
        return {"f1": features(n1, D, 11), "f2": features(n2, D, 12) + F32(0.05), "i1": i1, "i2": i2}
    return {"mask": np.ascontiguousarray(mask_of(s["mask"]))}


def inputs_sha256(t):
    h = hashlib.sha256()
    for key in sorted(t):
        h.update(key.encode())
        h.update(np.ascontiguousarray(t[key]).tobytes())
    return h.hexdigest()


def _bits(v):
    """A CPU tensor of the integer type of v's element size: the comparison is ``torch.equal`` on it."""
    v = v.contiguous().cpu()
    return v if not v.dtype.is_floating_point else v.view({4: torch.int32, 8: torch.int64}[v.element_size()])


def _dev(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def run_guidance(L, lib, cond, uncond, w, eqn, in_place):
    """One pd_guidance_rescale call on device tensors; returns out (``cond`` itself when in place)."""
    B, n = cond.shape
    out = cond if in_place else torch.full_like(cond, float("nan"))
    ws = torch.full((lib.pd_guidance_rescale_workspace(B, n) // 8,), float("nan"), dtype=torch.float64, device=cond.device)
    a = L.GuidanceRescaleArgs(numel=B * n, per_sample=n, model_out=cond.data_ptr(), uncond_out=uncond.data_ptr(), w=w.data_ptr(),
                              w_per_sample=int(w.numel() > 1), guidance_cfg=eqn, rescale=PHI, out=out.data_ptr(), workspace=ws.data_ptr())
    L.check(lib.pd_guidance_rescale(C.byref(a), torch.cuda.current_stream().cuda_stream), "pd_guidance_rescale")
    return out


def run_contrast_mask(L, lib, acc, given):
    """One pd_contrast_mask call on a device [B][n] tensor: (mask, map, stats), the last two None where not ``given``."""
    B, n = acc.shape
    mask = torch.full((B, n), 7, dtype=torch.uint8, device=acc.device)
    cmap = torch.full((B, n), float("nan"), device=acc.device) if given else None
    stats = torch.full((B, 3), float("nan"), device=acc.device) if given else None
    ws = torch.full((lib.pd_contrast_mask_workspace(B, n) // 8,), float("nan"), dtype=torch.float64, device=acc.device)
    a = L.ContrastMaskArgs(B=B, per_pixel=n, acc=acc.data_ptr(), ratio=RATIO, mask=mask.data_ptr(), map=L.ptr(cmap), stats=L.ptr(stats),
                           workspace=ws.data_ptr())
    L.check(lib.pd_contrast_mask(C.byref(a), torch.cuda.current_stream().cuda_stream), "pd_contrast_mask")
    return mask, cmap, stats


def run_case(L, lib, name, t, dev, rows=None):
    """Launch the case on ``dev``; returns {array name: CPU integer-view tensor} of everything recorded.  ``rows``: run on these samples
    of the batch alone (the batch-independence check of the long folds)."""
    import phendiff_amd as P
    from phendiff_amd import diagnostics as D
    kind, s = CASES[name]
    for k, v in CHUNK.items():
        assert L.CONSTANTS[f"PD_{k.upper()}_CHUNK"] == v, k
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    got = {}
    if kind == "sample_stats":
        x = _dev(pick(t["x"]), dev, TORCH[s["dtype"]])
        y = None if "y" not in t else _dev(t["y"] if s["y"] == "shared" else pick(t["y"]), dev, TORCH[s["dtype"]])
        stats, hist = D.sample_stats(x, y=y, edges=EDGES100 if s["bins"] else None)
        got["stats"] = stats
        if hist is not None:
            got["hist"] = hist
    elif kind == "guidance_rescale":
        for eqn in (0, 1):
            for w in (W1, W3):      # one weight; one per sample (a sample run alone keeps its own)
                wt = _dev(np.array(w, F32) if len(w) == 1 else pick(np.array([w[b % len(w)] for b in range(s["B"])], F32)), dev)
                for in_place in (True, False):
                    cond, uncond = _dev(pick(t["cond"]), dev), _dev(pick(t["uncond"]), dev)
                    got[f"e{eqn}_w{len(w)}_{'in' if in_place else 'out_of'}_place"] = run_guidance(L, lib, cond, uncond, wt, eqn, in_place)
    elif kind == "contrast_mask":
        acc = _dev(pick(t["acc"]), dev)
        for given in (True, False):
            mask, cmap, stats = run_contrast_mask(L, lib, acc, given)
            got[f"{'given' if given else 'null'}_mask"] = mask
            if given:
                got.update(given_map=cmap, given_stats=stats)
    elif kind == "ssim":
        x = _dev(pick(t["x"]), dev, TORCH[s["dtype"]])
        y = _dev(t["y"] if s["shared"] else pick(t["y"]), dev, TORCH[s["dtype"]])
        got["means"] = D.ssim_maps_means(x, y, levels=s["levels"], win_size=s["win"], sigma=SSIM_SIGMA[s["win"]])
    elif kind == "object_intensity":
        lab = P.label_objects(_dev(t["mask"], dev), connectivity=s["conn"], max_objects=s["K"])
        got.update(geometry=lab.geometry, count=lab.count, table=P.measure_intensity(lab, _dev(t["images"], dev)).raw)
    elif kind == "kid_mmd":
        from test_gpu_metric_stats import KID_CASES, kid_raw
        _, _, m, _, _, degree, gamma, coef0 = KID_CASES[s["index"]]
        sums, mmd = kid_raw((L, lib, None, dev), *(_dev(t[k], dev) for k in ("f1", "f2", "i1", "i2")), m, degree, gamma, coef0)
        got.update(sums=sums, mmd=mmd)
    else:
        from mask_ops_cases import RECIPES
        m = _dev(t["mask"], dev)
        r = P.MaskRefine(*m.shape, dev, **RECIPES[s["recipe"]])
        r.enqueue(torch.cuda.current_stream().cuda_stream, m)
        got["stats"] = r.stats
    torch.cuda.synchronize()
    return {k: _bits(v) for k, v in got.items()}


# pd_guidance_rescale records eight outputs a case (two equations x two weight forms x in / out of place), random fp32 that does not
# compress: whole up to 4096 elements there, and of the 4 M-element outputs of the long folds the every-127th-element sample for two of
# the eight (33 K elements each) and the sha256 alone for the other six, so that the fixture stays small.  The sha256 covers every bit.
WHOLE_UP_TO = {"guidance_rescale": 4096}
SAMPLED_LONG_GUIDANCE = ("e0_w1_in_place", "e1_w3_out_of_place")


def stored_form(name, got):
    """What a fixture keeps of ``run_case``'s result: small arrays whole; of a large one the sha256 and every 127th element."""
    kind = CASES[name][0]
    kept = {}
    for key, v in got.items():
        a = v.contiguous().numpy()
        if a.size > WHOLE_UP_TO.get(kind, SAMPLE_ABOVE):
            kept[key + "__sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            if not (kind == "guidance_rescale" and name in LONG_FOLD and key not in SAMPLED_LONG_GUIDANCE):
                kept[key + "__sample127"] = a.reshape(-1)[::127].copy()
        else:
            kept[key] = a
    return kept


def fixture_path(kind):
    """One file per entry point (kind): its arrays are named ``<case>--<array>``."""
    return os.path.join(GOLDEN, kind + ".npz")
