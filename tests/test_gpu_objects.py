"""The per-object measurements on MI355X (``phendiff_amd.objects`` / ``csrc/object_stats.hip``) against the numpy references of
``tests/objects_ref.py`` over the masks of ``tests/mask_ops_cases.py`` (every SMALL case and the 256 x 256 one) at connectivity 4 and 8.
Integer tables are compared exactly; floating-point sums against ``math.fsum`` within the worst-case error of an fp64 sum in any order,
``n * 2^-52 * sum|v|``.  A reference is computed once per request and shared (``objects_ref.reference``)."""
import numpy as np
import pytest
import torch

import objects_ref as O
from mask_ops_cases import BIG, CASES, SMALL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = SMALL + [BIG]
TORCH = {"f32": torch.float32, "u8": torch.uint8, "u16": torch.uint16}


def dev(name):
    return torch.from_numpy(CASES[name].copy()).to(DEV)


def dev_images(name, kind):
    return torch.from_numpy(O.images(name, kind).copy()).to(DEV)


def same(t, ref):
    got = t.cpu().numpy()
    return got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(got, ref)


def raw_bytes(t):
    return t.contiguous().cpu().numpy().tobytes()


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_exact_tables_and_shape_numbers(name, conn):
    import phendiff_amd as P
    m = dev(name)
    index, count, status, g = O.reference(name, conn)
    lab = P.label_objects(m, connectivity=conn)
    assert isinstance(lab, P.ObjectLabels) and lab.geometry.dtype == torch.int64 and tuple(lab.geometry.shape) == (m.shape[0], O.K_DEFAULT, 12)
    assert same(lab.index, index) and same(lab.count, count) and same(lab.status, status) and same(lab.geometry, g)
    assert torch.equal(m, dev(name))      # the mask is never written
    want = O.shape_ref(g)
    for k, ref in want.items():
        got = getattr(lab, k)
        assert got.dtype == torch.float64 and tuple(got.shape) == ref.shape, k
        if k == "orientation":      # defined where the two axes differ
            sel = want["major_axis_length"] - want["minor_axis_length"] > 1e-6
            assert np.allclose(got.cpu().numpy()[sel], ref[sel], rtol=1e-12, atol=1e-9), k
        else:
            assert np.allclose(got.cpu().numpy(), ref, rtol=1e-12, atol=1e-9), k
    assert same(lab.valid, g[..., 0] > 0)
    as_bool = (m != 0)[:, None]      # (B, 1, H, W) bool: the same numbers, the index in the input's shape
    lab4 = P.label_objects(as_bool, connectivity=conn)
    assert tuple(lab4.index.shape) == tuple(as_bool.shape) and same(lab4.index[:, 0], index) and same(lab4.geometry, g)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_intensity(name, conn):
    import phendiff_amd as P
    lab = P.label_objects(dev(name), connectivity=conn)
    area = O.reference(name, conn)[3][..., 0]
    for kind in O.KINDS:
        img = dev_images(name, kind)
        table, bound = O.reference(name, conn, O.K_DEFAULT, kind)
        t = P.measure_intensity(lab, img)
        got = t.raw.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == table.shape == (img.shape[0], O.K_DEFAULT, img.shape[1], 4)
        assert np.array_equal(got[..., 2], table[..., 2]) and np.array_equal(got[..., 3], table[..., 3]), kind
        for f in (0, 1):
            err = np.abs(got[..., f] - table[..., f])
            print(f"{name} conn {conn} {kind} field {f}: largest error / bound = {float((err / np.maximum(bound[..., f], 1e-300)).max()):.3g}")
            assert (err <= bound[..., f]).all(), (kind, f)
            if kind != "f32":      # integers below 2^53: exact
                assert np.array_equal(got[..., f], table[..., f]) and float(table[..., f].max(initial=0.0)) < 2.0 ** 53, (kind, f)
        assert same(t.valid, area > 0) and not got[area == 0].any()
        n = np.maximum(area, 1)[..., None].astype(np.float64)
        assert np.array_equal(t.sum.cpu().numpy(), got[..., 0]) and np.array_equal(t.min.cpu().numpy(), got[..., 2])
        assert np.allclose(t.mean.cpu().numpy(), got[..., 0] / n, rtol=1e-15, atol=0)
        var = np.maximum(got[..., 1] / n - (got[..., 0] / n) ** 2, 0.0)
        assert np.allclose(t.std.cpu().numpy(), np.sqrt(var), rtol=1e-12, atol=1e-12)
        assert torch.equal(img.view(torch.uint8), dev_images(name, kind).view(torch.uint8))      # the images are never written


def everything(m, img, conn=8, K=O.K_DEFAULT):
    """Every output over one batch as bytes-comparable CPU tensors."""
    import phendiff_amd as P
    lab = P.label_objects(m, connectivity=conn, max_objects=K)
    t = P.measure_intensity(lab, img)
    torch.cuda.synchronize()
    return {"index": lab.index.cpu(), "count": lab.count.cpu(), "status": lab.status.cpu(), "geometry": lab.geometry.cpu(),
            "intensity": t.raw.cpu().view(torch.int64), "major": lab.major_axis_length.cpu().view(torch.int64), "mean": t.mean.cpu().view(torch.int64)}


@pytest.mark.parametrize("name", [n for n in SMALL if "1x1" not in n] + [BIG])
def test_a_sample_does_not_see_its_batch(name):
    """Two runs give equal bytes; a sample measured alone equals its rows in the batch, bit for bit; samples permuted gives rows permuted."""
    m, img = dev(name), dev_images(name, "f32")
    whole, again = everything(m, img), everything(m, img)
    perm = [2, 0, 1]
    moved = everything(m[perm].contiguous(), img[perm].contiguous())
    for k, v in whole.items():
        assert torch.equal(v, again[k]), k
        assert torch.equal(v[perm], moved[k]), k
    for s in range(m.shape[0]) if name != BIG else (1,):
        alone = everything(m[s:s + 1].contiguous(), img[s:s + 1].contiguous())
        for k, v in whole.items():
            assert torch.equal(v[s:s + 1], alone[k]), (k, s)


@pytest.mark.parametrize("name,conn,K", [("shapes_37x53", 4, 7), ("shapes_37x53", 4, 1), ("speckled_64x64", 8, 3), ("random_37x53", 8, 11)])
def test_overflow(name, conn, K):
    import phendiff_amd as P
    m, img = dev(name), dev_images(name, "f32")
    full, cut = everything(m, img, conn), everything(m, img, conn, K)
    index, count, status, g = O.reference(name, conn, K)
    assert (count > K).any() and same(cut["index"], index) and same(cut["geometry"], g) and same(cut["status"], status)
    assert torch.equal(cut["count"], full["count"]) and same(cut["count"], O.reference(name, conn)[1])      # the true number
    over = full["count"] > K
    assert torch.equal(cut["status"] != 0, over) and bool((cut["status"][over] == P.objects.OBJ_OVERFLOW).all()) and not bool(full["status"].any())
    assert torch.equal(cut["geometry"], full["geometry"][:, :K]) and torch.equal(cut["intensity"], full["intensity"][:, :K])      # rows 1..K
    kept = full["index"] <= K
    assert torch.equal(cut["index"][kept], full["index"][kept]) and not bool(cut["index"][~kept].any())      # dropped objects: index 0


def test_nan_isolation():
    import phendiff_amd as P
    name = "speckled_64x64"
    m, img = dev(name), dev_images(name, "f32")
    lab = P.label_objects(m)
    base = P.measure_intensity(lab, img).raw.cpu().view(torch.int64)
    index = O.reference(name, 8)[0]
    B, K = index.shape[0], O.K_DEFAULT
    # a NaN on background pixels changes nothing
    bg = img.clone()
    bg[(lab.index == 0)[:, None].expand_as(bg)] = float("nan")
    assert torch.equal(P.measure_intensity(lab, bg).raw.cpu().view(torch.int64), base)
    # a NaN in one object (sample 1, its largest object, channel 2, one pixel) changes that object's row of that channel and no other bit
    k = int(np.bincount(index[1].ravel())[1:].argmax()) + 1
    y, x = (int(v[0]) for v in np.nonzero(index[1] == k))
    one = img.clone()
    one[1, 2, y, x] = float("nan")
    got = P.measure_intensity(lab, one)
    raw = got.raw.cpu()
    assert bool(torch.isnan(raw[1, k - 1, 2]).all()) and bool(torch.isnan(got.mean[1, k - 1, 2])) and bool(torch.isnan(got.std[1, k - 1, 2]))
    touched = torch.zeros((B, K, img.shape[1]), dtype=torch.bool)
    touched[1, k - 1, 2] = True
    assert torch.equal(raw.view(torch.int64)[~touched], base[~touched])
    # a sample full of NaN changes no other sample
    whole = img.clone()
    whole[0] = float("nan")
    raw = P.measure_intensity(lab, whole).raw.cpu()
    assert torch.equal(raw.view(torch.int64)[1:], base[1:]) and bool(torch.isnan(raw[0][O.reference(name, 8)[3][0, :, 0] > 0]).all())


@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_captured_measure_equals_eager(kind):
    """ObjectMeasure captured in a graph and replayed on a second mask and image equals the eager calls, bit for bit."""
    import phendiff_amd as P
    names = ("speckled_64x64", "random_64x64")
    Cn = O.KINDS[kind][1]
    B, H, W = CASES[names[0]].shape
    K = 37
    eager = {n: everything(dev(n), dev_images(n, kind), 8, K) for n in names}
    om = P.ObjectMeasure(B, H, W, Cn, DEV, connectivity=8, max_objects=K, dtype=TORCH[kind])
    src, img = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV), torch.zeros((B, Cn, H, W), dtype=TORCH[kind], device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # a warm-up outside the capture
        om.enqueue(side.cuda_stream, src, img)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        om.enqueue(torch.cuda.current_stream().cuda_stream, src, img)
    for replay, n in enumerate((names[0], names[1], names[0])):
        src.copy_(dev(n))
        img.copy_(dev_images(n, kind))
        for t in (om.index, om.count, om.status, om.geometry):
            t.fill_(-7)
        om.intensity.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        want = eager[n]
        assert torch.equal(om.index.cpu(), want["index"]) and torch.equal(om.count.cpu(), want["count"]) and torch.equal(om.status.cpu(), want["status"]), replay
        assert torch.equal(om.geometry.cpu(), want["geometry"]) and torch.equal(om.intensity.cpu().view(torch.int64), want["intensity"]), replay
        tab = om.tables()
        assert torch.equal(tab.labels.major_axis_length.cpu().view(torch.int64), want["major"]) and torch.equal(tab.intensity.mean.cpu().view(torch.int64), want["mean"])
    assert same(om.index, O.reference(names[0], 8, K)[0]) and same(om.geometry, O.reference(names[0], 8, K)[3])
    with pytest.raises(ValueError, match="ObjectMeasure.enqueue"):
        om.enqueue(torch.cuda.current_stream().cuda_stream, src, img[:, :, :-1])
    with pytest.raises(ValueError, match="ObjectMeasure.enqueue"):
        om.enqueue(torch.cuda.current_stream().cuda_stream, src.to(torch.int32), img)


def changed_pair(name, kind):
    """(labels' reference index, source, result, expected changed pixel counts [B][K][C]): the pair differs inside two chosen objects only --
    object 1 of sample 0 in every pixel of channel 0, the largest object of sample 2 in every third of its pixels in the last channel."""
    index = O.reference(name, 8)[0]
    src = O.images(name, kind).copy()
    res = src.copy()
    counts = np.zeros((index.shape[0], O.K_DEFAULT, src.shape[1]), np.int64)
    sel = index[0] == 1
    res[0, 0][sel] += 1
    counts[0, 0, 0] = int(sel.sum())
    k = int(np.bincount(index[2].ravel())[1:].argmax()) + 1
    ys, xs = np.nonzero(index[2] == k)
    ys, xs = ys[::3], xs[::3]
    res[2, -1, ys, xs] += 1
    counts[2, k - 1, -1] = ys.size
    return index, src, res, counts


@pytest.mark.parametrize("kind", ["f32", "u8", "u16"])
def test_object_change(kind):
    import phendiff_amd as P
    name = "speckled_64x64"
    index, src, res, counts = changed_pair(name, kind)
    area = O.reference(name, 8)[3][..., 0]
    lab = P.label_objects(dev(name))
    ch = P.object_change(lab, torch.from_numpy(src).to(DEV), torch.from_numpy(res).to(DEV))
    want = counts / np.maximum(area, 1)[..., None]
    got = ch.changed_fraction.cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, want)      # 0 elsewhere, exact where it changed (one division of two integers)
    assert want[0, 0, 0] == 1.0 and 0.0 < want.max(axis=(1, 2))[2] < 1.0 and int((want != 0).sum()) == 2
    ts, tr = O.intensity_ref(index, src)[0], O.intensity_ref(index, res)[0]
    n = np.maximum(area, 1)[..., None].astype(np.float64)
    assert np.allclose(ch.mean_source.cpu().numpy(), ts[..., 0] / n, rtol=1e-12, atol=1e-12) and np.allclose(ch.mean_result.cpu().numpy(), tr[..., 0] / n, rtol=1e-12, atol=1e-12)
    assert torch.equal(ch.delta_mean, ch.mean_result - ch.mean_source) and torch.equal(ch.delta_std, ch.result.std - ch.source.std)
    unchanged = counts == 0
    assert not ch.delta_mean.cpu().numpy()[unchanged].any() and not ch.delta_std.cpu().numpy()[unchanged].any()
    assert same(ch.valid, area > 0)
    if kind == "f32":      # bit-wise: 0.0 against -0.0 counts as changed
        a = torch.zeros(3, 1, 64, 64, device=DEV)
        assert bool((P.object_change(lab, a, -a).changed_fraction[lab.valid] == 1.0).all())


def test_measure_transfer_on_a_hand_built_output():
    import phendiff_amd as P
    name = "speckled_64x64"
    index, src, res, counts = changed_pair(name, "f32")
    area = O.reference(name, 8)[3][..., 0]
    mask = dev(name)[:, None]
    source, result = torch.from_numpy(src).to(DEV), torch.from_numpy(res).to(DEV)
    out = P.MaskedTransferOutput(images=result.permute(0, 2, 3, 1).contiguous(), mask=mask, inverted=None, sample=None)      # (B, H, W, C), as masked_ddib returns
    ch = P.measure_transfer(out, source)
    assert same(ch.labels.index[:, 0], index) and same(ch.labels.geometry, O.reference(name, 8)[3])
    assert np.array_equal(ch.changed_fraction.cpu().numpy(), counts / np.maximum(area, 1)[..., None])
    direct = P.object_change(P.label_objects(mask), source, result)
    for k in ("mean_source", "mean_result", "delta_mean", "delta_std", "changed_fraction"):
        assert torch.equal(getattr(ch, k).view(torch.int64), getattr(direct, k).view(torch.int64)), k
    nhwc = P.measure_transfer(out, source.permute(0, 2, 3, 1).contiguous(), connectivity=4, max_objects=5)      # source in the images' layout
    assert tuple(nhwc.changed_fraction.shape) == (3, 5, 3) and same(nhwc.labels.index[:, 0], O.reference(name, 4, 5)[0])
