"""Guard bands around kernel operands: a tensor is placed in the middle of ONE larger allocation, so that whatever a kernel reads or
writes a little outside the tensor it was given stays inside memory the test owns -- and can be seen.

    view, h = guarded(t, guard_bytes, device)      # `view` (256-byte aligned) goes to the kernel, `h` watches its surroundings
    h.clear() / h.poison()                         # input operands: zeros / NaN around the tensor (refilled IN PLACE: same pointers)
    h.canary(); ...kernel...; h.intact()           # output operands: a fixed byte pattern that must still be there afterwards

`guarded_rows(t2d, row_stride, ...)` lays the rows out with a stride larger than their width; the gap columns of every row belong to
the guard as well (slices of a fused projection, `x_stride` / `dy_stride` / `kv_stride` operands).

A plain module (no fixtures, no pytest hooks): imported by tests/test_host_guard_bands.py (which proves it on the CPU) and by
tests/test_gpu_guard_bands.py."""
import torch

ALIGN = 256
MIN_GUARD_BYTES = 64 * 1024


def _pattern(n, start, device):
    """The canary: byte i of a region holds (start + i) % 251 + 1 -- never zero, period prime (no power-of-two stride maps onto itself)."""
    return ((torch.arange(n, dtype=torch.int64, device=device) + start) % 251 + 1).to(torch.uint8)


class Guards:
    """Handle to the surroundings of one guarded tensor: `front` and `back` (uint8, `guard_bytes` each) and, for the strided layout,
    `gap` (uint8 [rows][gap bytes], a strided view)."""

    def __init__(self, raw, start, nbytes, guard_bytes, dtype, name, gap=None):
        self.raw, self.dtype, self.name, self.guard_bytes = raw, dtype, name, guard_bytes
        self.front = raw[start - guard_bytes:start]
        self.back = raw[start + nbytes:start + nbytes + guard_bytes]
        self.gap = gap
        self.clear()

    def _regions(self):
        return [r for r in (self.front, self.back, self.gap) if r is not None and r.numel()]

    def clear(self):
        for r in self._regions():
            r.zero_()
        return self

    def poison(self):
        """NaN of the tensor's dtype all around (all-ones bytes for an integer tensor)."""
        if not self.dtype.is_floating_point:
            for r in self._regions():
                r.fill_(0xFF)
            return self
        esz = torch.empty((), dtype=self.dtype).element_size()
        unit = torch.full((1,), float("nan"), dtype=self.dtype).view(torch.uint8).to(self.raw.device)
        for r in self._regions():
            assert r.shape[-1] % esz == 0
            r.copy_(unit.repeat(r.shape[-1] // esz).expand_as(r))
        return self

    def canary(self):
        dev = self.raw.device
        self.front.copy_(_pattern(self.front.numel(), 0, dev))
        self.back.copy_(_pattern(self.back.numel(), 7, dev))
        if self.gap is not None and self.gap.numel():
            self.gap.copy_(_pattern(self.gap.numel(), 13, dev).view(self.gap.shape))
        return self

    def intact(self):
        """Integer comparison of the guards with the canary; raises AssertionError naming the first byte that differs, relative to the
        tensor's start (front), its end (back) or the row's last valid byte (gap).  Returns True otherwise."""
        dev = self.raw.device
        bad = (self.back != _pattern(self.back.numel(), 7, dev)).nonzero()
        if bad.numel():
            i = int(bad[0])
            raise AssertionError(f"{self.name}: guard overwritten {i} bytes past the END of the tensor "
                                 f"({int(bad.numel())} bytes of the back guard differ, the last one at +{int(bad[-1])})")
        bad = (self.front != _pattern(self.front.numel(), 0, dev)).nonzero()
        if bad.numel():
            n = self.front.numel()
            raise AssertionError(f"{self.name}: guard overwritten before the START of the tensor: first differing byte at -{n - int(bad[0])} "
                                 f"({int(bad.numel())} bytes of the front guard differ, the nearest one at -{n - int(bad[-1])})")
        if self.gap is not None and self.gap.numel():
            bad = (self.gap != _pattern(self.gap.numel(), 13, dev).view(self.gap.shape)).nonzero()
            if bad.numel():
                row, col = int(bad[0][0]), int(bad[0][1])
                raise AssertionError(f"{self.name}: gap column overwritten in row {row}, {col} bytes past the end of the row's valid part "
                                     f"({int(bad.shape[0])} gap bytes differ)")
        return True


def guard_size(tile_rows, row_elems, dtype):
    """Two full tiles of the consuming kernel along its streamed dimension, never less than 64 KiB, in whole 256-byte units."""
    esz = torch.empty((), dtype=dtype).element_size()
    need = max(MIN_GUARD_BYTES, 2 * tile_rows * row_elems * esz)
    return (need + ALIGN - 1) // ALIGN * ALIGN


def _place(nbytes, guard_bytes, device):
    assert guard_bytes > 0 and guard_bytes % ALIGN == 0, "guard_bytes: a positive multiple of 256"
    raw = torch.empty(2 * guard_bytes + nbytes + 2 * ALIGN, dtype=torch.uint8, device=device)
    start = guard_bytes + (-(raw.data_ptr() + guard_bytes)) % ALIGN
    assert (raw.data_ptr() + start) % ALIGN == 0
    return raw, start


def guarded(t, guard_bytes=MIN_GUARD_BYTES, device=None, name="tensor"):
    """Copy `t` into the middle of one larger allocation on `device` (256-byte aligned start, `guard_bytes` before and after).
    Returns (view, Guards); the guards start cleared."""
    device = torch.device(device) if device is not None else t.device
    t = t.contiguous()
    esz = t.element_size()
    nbytes = t.numel() * esz
    raw, start = _place(nbytes, guard_bytes, device)
    assert start % esz == 0
    view = raw[start:start + nbytes].view(t.dtype).view(t.shape)
    view.copy_(t)
    return view, Guards(raw, start, nbytes, guard_bytes, t.dtype, name)


def guarded_rows(t2d, row_stride, guard_bytes=MIN_GUARD_BYTES, device=None, name="tensor"):
    """As `guarded`, rows `row_stride` elements apart (> their width): returns the strided [rows][width] view (leading dimensions of `t2d`
    are kept; they must be dense) and Guards whose `gap` covers columns width..row_stride-1 of EVERY row, the last one included."""
    device = torch.device(device) if device is not None else t2d.device
    width = t2d.shape[-1]
    assert row_stride > width, "guarded_rows: row_stride must exceed the row width (use guarded otherwise)"
    rows = t2d.numel() // width
    esz = t2d.element_size()
    nbytes = rows * row_stride * esz
    raw, start = _place(nbytes, guard_bytes, device)
    assert start % esz == 0
    full = raw[start:start + nbytes].view(t2d.dtype).view(rows, row_stride)
    view = full[:, :width].view(*t2d.shape[:-1], width) if t2d.dim() != 2 else full[:, :width]
    view.copy_(t2d)
    gap = raw[start:start + nbytes].view(rows, row_stride * esz)[:, width * esz:]
    return view, Guards(raw, start, nbytes, guard_bytes, t2d.dtype, name, gap=gap)
