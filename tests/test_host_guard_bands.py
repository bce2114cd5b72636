"""tests/guard_bands.py proved on the CPU: fake "kernels" written in torch that step outside the tensor they were given must each be
reported, a well-behaved one must pass.  (The fakes reach outside through as_strided on the view's own storage -- the way a kernel
reaches outside through pointer arithmetic.)"""
import pytest
import torch

from guard_bands import ALIGN, MIN_GUARD_BYTES, guard_size, guarded, guarded_rows

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _flat(view, extra_before=0, extra_after=0):
    """The `numel + extras` elements around a dense view, straight from its storage."""
    return view.as_strided((view.numel() + extra_before + extra_after,), (1,), view.storage_offset() - extra_before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_alignment_and_contents(dtype):
    t = torch.randn(7, 33).to(dtype)
    v, h = guarded(t, 1024, "cpu")
    assert v.data_ptr() % ALIGN == 0 and v.shape == t.shape and v.dtype == dtype and torch.equal(v, t)
    assert h.front.numel() == h.back.numel() == 1024
    assert h.front.data_ptr() + 1024 == v.data_ptr() and h.back.data_ptr() == v.data_ptr() + t.numel() * t.element_size()
    assert int(h.front.sum()) == 0 and int(h.back.sum()) == 0                     # guards start cleared
    h.poison()
    assert torch.isnan(_flat(v, 5, 5)[:5]).all() and torch.isnan(_flat(v, 5, 5)[-5:]).all() and torch.equal(v, t)
    h.canary()
    assert h.intact() and torch.equal(v, t)
    h.clear()
    assert float(_flat(v, 3, 3)[:3].float().abs().sum()) == 0
    assert guard_size(64, 128, dtype) == max(MIN_GUARD_BYTES, 2 * 64 * 128 * t.element_size())
    assert guard_size(128, 3 * 320, torch.float32) == 2 * 128 * 960 * 4


def test_integer_tensors_are_poisoned_with_all_ones():
    v, h = guarded(torch.arange(10, dtype=torch.int32), 256, "cpu")
    h.poison()
    assert int(_flat(v, 1, 1)[0]) == -1 and int(_flat(v, 1, 1)[-1]) == -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_one_element_past_the_end_is_reported(dtype):
    y, h = guarded(torch.full((5, 8), float("nan"), dtype=dtype), 512, "cpu", name="y")
    h.canary()
    _flat(y, 0, 1).fill_(1.0)                    # the "kernel": 41 elements instead of 40
    assert torch.isfinite(y).all()
    with pytest.raises(AssertionError, match=r"y: guard overwritten 0 bytes past the END"):
        h.intact()


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_one_element_before_the_start_is_reported(dtype):
    y, h = guarded(torch.full((5, 8), float("nan"), dtype=dtype), 512, "cpu", name="y")
    h.canary()
    _flat(y, 1, 0).fill_(1.0)
    esz = y.element_size()
    with pytest.raises(AssertionError, match=rf"y: guard overwritten before the START of the tensor: first differing byte at -{esz} "):
        h.intact()


def test_a_write_far_into_the_band_reports_its_offset():
    y, h = guarded(torch.zeros(16), 1024, "cpu", name="y")
    h.canary()
    _flat(y, 0, 101)[-1] = 3.0                   # element 116: 100 floats past the end
    with pytest.raises(AssertionError, match=r"400 bytes past the END"):
        h.intact()


@pytest.mark.parametrize("dtype", DTYPES)
def test_summing_one_row_too_many_of_a_poisoned_input_is_reported(dtype):
    x, h = guarded(torch.randn(6, 16).to(dtype), 512, "cpu")
    rowsum = lambda rows: _flat(x, 0, 16 * (rows - 6)).view(rows, 16).float().sum(0)      # the "kernel": column sums over `rows` rows
    h.clear()
    clean_good, clean_bad = rowsum(6), rowsum(7)
    assert torch.equal(clean_good, clean_bad)            # the over-read is INVISIBLE next to zeros (and next to finite data it is merely wrong) ...
    h.poison()
    assert torch.equal(rowsum(6), clean_good)            # ... a well-behaved kernel does not care what surrounds its input ...
    assert not torch.equal(rowsum(7), clean_bad)         # ... the over-reading one returns other bits (NaN) once the surroundings are poisoned
    assert torch.isnan(rowsum(7)).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_well_behaved_kernel_passes(dtype):
    x, hx = guarded(torch.randn(9, 24).to(dtype), 512, "cpu", name="x")
    y, hy = guarded(torch.full((9, 24), float("nan"), dtype=dtype), 512, "cpu", name="y")
    hy.canary()
    outs = []
    for fill in (hx.clear, hx.poison):
        fill()
        y.fill_(float("nan"))
        y.copy_(x * 2)
        assert hy.intact() and torch.isfinite(y).all()
        outs.append(y.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_rows_gap_columns_are_guard(dtype):
    t = torch.randn(5, 24).to(dtype)
    v, h = guarded_rows(t, 40, 512, "cpu", name="y")
    assert v.shape == (5, 24) and v.stride() == (40, 1) and v.data_ptr() % ALIGN == 0 and torch.equal(v, t)
    assert h.gap.shape == (5, 16 * t.element_size())
    wide = v.as_strided((5, 40), (40, 1), v.storage_offset())      # every row with its gap columns
    h.poison()
    assert torch.isnan(wide[:, 24:]).all() and torch.equal(wide[:, :24], t)
    h.clear()
    assert float(wide[:, 24:].float().abs().sum()) == 0
    h.canary()
    v.copy_(t * 3)                                                 # a well-behaved strided store
    assert h.intact()
    wide[3, 26] = 1.0                                              # row 3, two elements into the gap
    with pytest.raises(AssertionError, match=rf"y: gap column overwritten in row 3, {2 * t.element_size()} bytes past"):
        h.intact()
    h.canary()
    wide[4, 39] = 1.0                                              # the last row's gap is guard too
    with pytest.raises(AssertionError, match=r"gap column overwritten in row 4"):
        h.intact()


def test_strided_rows_keep_leading_dimensions():
    t = torch.randn(2, 3, 8)
    v, h = guarded_rows(t, 16, 256, "cpu")
    assert v.shape == (2, 3, 8) and v.stride() == (48, 16, 1) and torch.equal(v, t) and h.gap.shape == (6, 32)


def test_poisoned_and_clean_runs_share_one_allocation():
    v, h = guarded(torch.zeros(4), 256, "cpu")
    p = v.data_ptr()
    h.poison(); h.clear(); h.canary()
    assert v.data_ptr() == p and h.intact()
