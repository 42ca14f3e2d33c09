"""tests/guard.py on CPU tensors, driven by fake "kernels": Python functions that write a guarded output the way a
broken kernel would.  The helper must raise on each fault, say where, and pass the correct fake."""
import pytest
import torch

from tests import guard as G

CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (batch, rows, cols, ld, stride): dense, padded rows, batches with a gap
LAYOUTS = [(None, 5, 16, 16, None), (None, 7, 10, 16, None), (3, 4, 6, 8, 40)]


def _good(o, a):
    """The correct fake: out[b][r][c] = a[r][c] + b."""
    for b in range(o.nb):
        o.t3[b].copy_(a[:o.rows, :o.cols] + b)


def _mk(dt, layout):
    batch, rows, cols, ld, stride = layout
    o = G.Out(CPU, dt, rows, cols, ld=ld, batch=batch, stride=stride)
    a = G.inp(torch.arange(rows * cols, dtype=torch.float32).view(rows, cols).to(dt))
    return o, a


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES)
def test_correct_fake_passes(dt, layout):
    o, a = _mk(dt, layout)
    _good(o, a)
    t = o.check("good")
    assert t.shape == ((o.nb, o.rows, o.cols) if layout[0] else (o.rows, o.cols))
    assert G.same(o.t3[o.nb - 1], a + (o.nb - 1))


def test_layout():
    """Front band a multiple of 256 bytes, back band a full 256-row tile and at least 4 KiB, payload NaN, rest
    sentinel."""
    for dt in DTYPES:
        for ld in (1, 8, 24):
            o = G.Out(CPU, dt, 3, min(ld, 5), ld=ld)
            assert (o.front * o.es) % 256 == 0 and o.front > 0
            assert o.back >= 256 * ld and o.back * o.es >= 4096
            assert o.t.data_ptr() - o.buf.data_ptr() == o.front * o.es
            assert bool(torch.isnan(o.t).all())
            assert int((o.buf == G.SENTINEL).sum()) == o.buf.numel() - o.rows * o.cols
    x = G.inp(torch.ones(4, 6))
    tail = torch.as_strided(x, (G.back_elems(6, 4),), (1,), x.storage_offset() + 24)
    assert bool(torch.isnan(tail).all()) and tail.numel() * 4 >= 4096 and tail.numel() >= 256 * 6
    w = G.ws(3, CPU)
    assert w.numel() == 16 and bool((w == 0xFF).all())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES)
def test_unwritten_row(dt, layout):
    o, a = _mk(dt, layout)
    _good(o, a)
    o.t3[o.nb - 1, 2].fill_(float("nan"))                     # (a) one row left as the poison it was
    with pytest.raises(G.GuardError, match=rf"{o.cols} of .* NaN.*\(batch {o.nb - 1}, row 2, col 0\)"):
        o.check("skip")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES)
def test_write_past_last_row(dt, layout):
    o, a = _mk(dt, layout)
    _good(o, a)
    o.buf[o.front + o.span] = 1.0                             # (b) first element of the row after the last
    with pytest.raises(G.GuardError, match=rf"outside.*0 elements past the end \(row {o.rows} col 0"):
        o.check("overrun")


def test_write_far_past_last_row():
    o, a = _mk(torch.float32, LAYOUTS[1])
    _good(o, a)
    o.buf[-1] = 1.0                                           # the last element of the 256-row band
    with pytest.raises(G.GuardError, match="outside"):
        o.check("overrun")


@pytest.mark.parametrize("layout", LAYOUTS[1:])
@pytest.mark.parametrize("dt", DTYPES)
def test_write_pad_column(dt, layout):
    o, a = _mk(dt, layout)
    _good(o, a)
    o.buf[o.front + 1 * o.ld + o.cols] = 0.0                  # (c) row 1's first pad column
    with pytest.raises(G.GuardError, match=rf"\(batch 0, row 1, col {o.cols}\) \[pad column\]"):
        o.check("pad")


def test_write_batch_gap():
    o, a = _mk(torch.float16, LAYOUTS[2])
    _good(o, a)
    o.buf[o.front + o.stride + o.rows * o.ld + 3] = 0.0
    with pytest.raises(G.GuardError, match=r"\(batch 1, gap element 3"):
        o.check("gap")


@pytest.mark.parametrize("dt", DTYPES)
def test_write_in_front(dt):
    o, a = _mk(dt, LAYOUTS[0])
    _good(o, a)
    o.buf[o.front - 1] = 0.0                                  # (d)
    with pytest.raises(G.GuardError, match="1 elements in front of the payload"):
        o.check("front")


def test_sentinel_rewritten_with_other_bits():
    """The compare is of bits: -1234.0 or a NaN over a sentinel counts, and so does rewriting 1234.0 as 1234.0 not."""
    o, a = _mk(torch.float32, LAYOUTS[0])
    _good(o, a)
    o.buf[o.front + o.span + 5] = G.SENTINEL                  # the same bits: intact
    o.check("same bits")
    o.buf[o.front + o.span + 5] = float("nan")
    with pytest.raises(G.GuardError, match="5 elements past the end"):
        o.check("nan over sentinel")


@pytest.mark.parametrize("dt", DTYPES)
def test_input_tail_reaches_output(dt):
    o, a = _mk(dt, LAYOUTS[0])
    _good(o, a)
    tail = torch.as_strided(a, (o.cols,), (1,), a.storage_offset() + a.numel())
    o.t3[0, o.rows - 1].copy_(tail)                           # (e) the last row computed from the operand's tail
    with pytest.raises(G.GuardError, match=rf"\(batch 0, row {o.rows - 1}, col 0\)"):
        o.check("tail")


def test_input_slice_keeps_strides():
    qkv = torch.arange(2 * 5 * 12, dtype=torch.float32).view(2, 5, 12)
    k = qkv[:, :, 4:8]
    g = G.inp(k)
    assert g.shape == k.shape and g.stride() == k.stride() and torch.equal(g, k)
    between = torch.as_strided(g, (4,), (1,), g.storage_offset() + 4)      # v's columns of the first row
    assert bool(torch.isnan(between).all())
    ids = torch.arange(4, dtype=torch.int32)
    assert G.inp(ids) is ids and G.inp(None) is None


def test_uint8_twice():
    def good(o):
        o.t.copy_(torch.arange(o.rows * o.cols, dtype=torch.uint8).view(o.rows, o.cols))

    def lazy(o):
        o.t[:2].copy_(torch.arange(2 * o.cols, dtype=torch.uint8).view(2, o.cols))      # the last row keeps its fill

    def overrun(o):
        good(o)
        o.buf[o.front + o.span] = 0

    got = G.twice8(CPU, 3, 7, good, ld=8)
    assert got.shape == (3, 7) and int(got[2, 6]) == 20
    with pytest.raises(G.GuardError, match=r"depend on what the output held.*\(2, 0\)"):
        G.twice8(CPU, 3, 7, lazy, ld=8)
    with pytest.raises(G.GuardError, match="outside"):
        G.twice8(CPU, 3, 7, overrun, ld=8)
    with pytest.raises(AssertionError):
        G.Out(CPU, torch.uint8, 3, 7)


def test_poison_ok_still_checks_sentinels():
    """check(poison_ok=True): the caller asserts itself which payload elements keep their NaN (pad channels inside a
    row the kernel partly owns); the bands are checked all the same."""
    o = G.Out(CPU, torch.float32, 4, 8)
    o.t[:, :3] = 1.0
    o.check("partly written", poison_ok=True)
    with pytest.raises(G.GuardError, match="NaN"):
        o.check("partly written")
    o.buf[o.front + o.span + 1] = 0.0
    with pytest.raises(G.GuardError, match="outside"):
        o.check("overrun", poison_ok=True)


def test_disabled_is_plain(monkeypatch):
    """ENABLED = False (the timing scripts): no bands, no copies, no checks."""
    monkeypatch.setattr(G, "ENABLED", False)
    o = G.Out(CPU, torch.float32, 4, 8, ld=16)
    assert o.front == 0 and o.back == 0 and o.buf.numel() == 4 * 16
    assert o.check("plain") is o.t
    x = torch.ones(3, 3)
    assert G.inp(x) is x and G.ws(100, CPU).numel() == 100
