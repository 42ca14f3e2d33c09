"""Guarded buffers for the op-level tests: what a kernel writes is poisoned and fenced, what it reads is followed by
poison, what it borrows as scratch starts out as garbage.

  Out     a strided output [batch][rows][cols] (row stride ld >= cols, batch stride >= rows * ld) carved out of one
          larger allocation.  The payload starts as NaN; a band in front, a band behind, every padding column
          [cols, ld) and every gap between batches hold SENTINEL.  check() asserts, on the buffer's own device with one
          transfer of a few flags, that no payload element is still NaN and that every sentinel element has the bits it
          had before the call; a failure names the first offending flat index as (batch, row, col).
  inp     a copy of an operand followed by a NaN tail: a kernel may read past the end and discard what it read, but
          input data are finite, so a NaN in a checked payload is unwritten poison or a dependence on that tail.
  ws      a workspace of 0xFF bytes: no launcher may depend on what a caller's workspace held before the call.
  twice8  uint8 outputs have no NaN: the call runs on a 0x00-filled and on a 0xFF-filled payload, and the two
          results must be byte-identical.

The front band is a multiple of 256 bytes, so a payload is aligned as a fresh allocation is (the planners pick
kernels by the alignment of C).  The back band is one full 256-row tile of ld elements and never less than 4 KiB.
Everything works on CPU tensors as well (tests/test_guard_host.py drives it with fake kernels).

ENABLED = False (set by the timing scripts under scripts/, never by a test) turns all of it off: plain allocations, no
copies, no fills, no synchronisation, so a timed loop over a wrapper of tests/opref.py measures the kernel.
"""
from __future__ import annotations

import numpy as np
import torch

SENTINEL = 1234.0
SENTINEL_U8 = 0x3C
FRONT_BYTES = 1024          # a multiple of 256
BACK_ROWS = 256             # one BM tile, the furthest a ragged last tile could overrun
BACK_MIN_BYTES = 4096
_INT = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}

ENABLED = True

assert FRONT_BYTES % 256 == 0


class GuardError(AssertionError):
    pass


def bits(t):
    """The elements of a contiguous tensor as integers of the same width (flat)."""
    return t.contiguous().view(-1).view(_INT[t.element_size()])


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got).cpu(), bits(want).cpu())


def back_elems(ld, esize):
    """Elements of the band behind a buffer of row stride ld."""
    return max(BACK_ROWS * max(int(ld), 1), -(-BACK_MIN_BYTES // esize))


def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize(t.device)


class Out:
    """A guarded output.  `.t` is the [batch][rows][cols] view ([rows][cols] when batch is None) a kernel writes
    through data_ptr() / `.ld` / `.stride`; `view(shape)` reshapes a dense one (ld == cols)."""

    def __init__(self, device, dtype, rows, cols, ld=None, batch=None, stride=None, fill=None):
        nb = 1 if batch is None else int(batch)
        rows, cols = int(rows), int(cols)
        ld = cols if ld is None else int(ld)
        stride = rows * ld if stride is None else int(stride)
        assert rows >= 0 and cols >= 1 and ld >= cols and nb >= 1 and stride >= rows * ld
        es = torch.empty((), dtype=dtype).element_size()
        self.dtype, self.es, self.nb, self.rows, self.cols, self.ld, self.stride = dtype, es, nb, rows, cols, ld, stride
        self.batched = batch is not None
        self.front = FRONT_BYTES // es if ENABLED else 0
        self.span = (nb - 1) * stride + rows * ld
        self.back = back_elems(ld, es) if ENABLED else 0
        self.is_float = dtype.is_floating_point
        self.buf = torch.empty(self.front + self.span + self.back, dtype=dtype, device=device)
        if not ENABLED:
            pass
        elif self.is_float:
            assert fill is None
            self.buf.fill_(SENTINEL)
        else:
            assert dtype == torch.uint8 and fill in (0x00, 0xFF), "uint8 payloads take fill 0x00 or 0xFF (see twice8)"
            self.buf.fill_(SENTINEL_U8)
        if ENABLED:
            self.sent_bits = int(bits(self.buf[:1])[0])
            self._payload(self.buf).fill_(float("nan") if self.is_float else fill)
        self.ibuf = self.buf.view(_INT[es])
        self.t3 = self._payload(self.buf)
        self.t = self.t3 if self.batched else self.t3[0]

    # views of a flat buffer laid out as this one
    def _payload(self, flat):
        return flat.as_strided((self.nb, self.rows, self.cols), (self.stride, self.ld, 1), self.front)

    def _pads(self, flat):
        return flat.as_strided((self.nb, self.rows, self.ld - self.cols), (self.stride, self.ld, 1),
                               self.front + self.cols)

    def _gaps(self, flat):
        return flat.as_strided((self.nb - 1, self.stride - self.rows * self.ld), (self.stride, 1),
                               self.front + self.rows * self.ld)

    def _sentinels(self, flat):
        hi = self.front + self.span
        parts = [flat[:self.front], flat[hi:]]
        if self.ld > self.cols and self.rows:
            parts.append(self._pads(flat))
        if self.nb > 1 and self.stride > self.rows * self.ld:
            parts.append(self._gaps(flat))
        return parts

    def ptr(self):
        return self.t.data_ptr()

    def view(self, *shape):
        assert self.ld == self.cols and self.stride == self.rows * self.ld, "view() needs a dense buffer"
        return self.buf[self.front:self.front + self.span].view(*shape)

    def where(self, flat):
        """(batch, row, col) of a flat index of the whole allocation; col >= cols is a pad column, batch / row outside
        the payload are reported as such."""
        i = flat - self.front
        if i < 0:
            return f"{-i} elements in front of the payload"
        if i >= self.span:
            k = i - self.span
            return f"{k} elements past the end (row {self.rows + k // self.ld} col {k % self.ld} of the last batch)"
        b, r = divmod(i, self.stride) if self.nb > 1 else (0, i)
        if r >= self.rows * self.ld:
            return f"(batch {b}, gap element {r - self.rows * self.ld} after its last row)"
        return f"(batch {b}, row {r // self.ld}, col {r % self.ld})" + (" [pad column]" if r % self.ld >= self.cols else "")

    def check(self, what="output", poison_ok=False):
        """After the call: every payload element written, every sentinel intact.  Returns `.t`.  poison_ok: the caller
        itself asserts which payload elements were to be written and which still hold their NaN."""
        if not ENABLED:
            return self.t
        flags = [(s != self.sent_bits).any().view(1) for s in self._sentinels(self.ibuf)]
        if self.is_float and not poison_ok:
            flags.append(torch.isnan(self.t3).any().view(1))
        _sync(self.buf)
        if bool(torch.cat(flags).any().cpu()):      # the one transfer; the slow path below only runs on a failure
            self._fail(what)
        return self.t

    def _fail(self, what):
        clean = torch.zeros_like(self.ibuf, dtype=torch.bool)
        for s in self._sentinels(clean):
            s.fill_(True)
        bad = ((self.ibuf != self.sent_bits) & clean).nonzero().view(-1)
        if bad.numel():
            i = int(bad[0])
            raise GuardError(f"{what}: wrote outside its output: {bad.numel()} sentinel elements changed, first at "
                             f"flat index {i}: {self.where(i)}, now {self.buf[i].item()!r}")
        nan = torch.isnan(self.t3)
        idx = nan.nonzero()
        b, r, c = (int(v) for v in idx[0])
        i = self.front + b * self.stride + r * self.ld + c
        raise GuardError(f"{what}: {idx.shape[0]} of {nan.numel()} payload elements are NaN (never written, or computed "
                         f"from memory past the end of an operand), first at flat index {i}: {self.where(i)}")


def out(device, dtype, *shape, ld_pad=0):
    """A guarded dense output of `shape` (the last dimension is the columns, the rest the rows); ld_pad > 0 adds that
    many sentinel columns to every row."""
    cols = int(shape[-1])
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    return Out(device, dtype, rows, cols, ld=cols + ld_pad)


def done(o, shape, what="output"):
    """check() and the payload in `shape` (a strided view when the buffer has pad columns)."""
    o.check(what)
    assert o.nb == 1 and int(np.prod(shape)) == o.rows * o.cols
    if o.ld == o.cols:
        return o.view(*shape)
    assert shape[-1] == o.cols
    return o.buf.as_strided(tuple(shape), _strides(shape, o.ld), o.front)


def _strides(shape, ld):
    st = [1] * len(shape)
    st[-2] = ld
    for i in range(len(shape) - 3, -1, -1):
        st[i] = st[i + 1] * shape[i + 1]
    return tuple(st)


def inp(t, device=None):
    """A copy of a floating-point operand (same shape and strides, so slices of a wider row stay slices) followed by
    a NaN tail; elements of the original's storage between the view's own (another tensor's columns) are NaN too.
    None and integer tensors pass through."""
    if t is None:
        return None
    device = t.device if device is None else device
    if not ENABLED:
        return t.to(device)
    if not t.dtype.is_floating_point:
        return t.to(device)
    if t.numel() == 0:
        return t.to(device)
    span = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    assert all(s >= 0 for s in t.stride())
    ld = t.stride(-2) if t.dim() >= 2 else 1
    flat = torch.full((span + back_elems(ld, t.element_size()),), float("nan"), dtype=t.dtype, device=device)
    g = flat.as_strided(t.shape, t.stride(), 0)
    g.copy_(t)
    return g


def ws(nbytes, device):
    """A workspace of `nbytes` (at least 16) 0xFF bytes."""
    if not ENABLED:
        return torch.empty(max(16, int(nbytes)), dtype=torch.uint8, device=device)
    return torch.full((max(16, int(nbytes)),), 0xFF, dtype=torch.uint8, device=device)


def twice8(device, rows, cols, run, ld=None, batch=None, stride=None, what="output"):
    """A uint8 output: run(Out) on a 0x00-filled and on a 0xFF-filled payload; both pass check() and agree byte for
    byte.  Returns the payload of the second run."""
    res = []
    for fill in (0x00, 0xFF):
        o = Out(device, torch.uint8, rows, cols, ld=ld, batch=batch, stride=stride, fill=fill)
        run(o)
        res.append(o.check(what))
    if not torch.equal(res[0], res[1]):
        d = (res[0] != res[1]).nonzero()
        raise GuardError(f"{what}: {d.shape[0]} bytes depend on what the output held before the call (never written), "
                         f"first at (batch, row, col) {tuple(int(v) for v in d[0])}")
    return res[1]
