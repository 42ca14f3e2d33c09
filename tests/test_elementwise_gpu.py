"""The four kernels of csrc/elementwise.hip the models call between GEMMs, each through its own C entry point on
guarded buffers (tests/guard.py) against a plain high-precision reference: irx_op_softmax_rows, irx_op_transpose2d,
irx_op_timestep_embed, irx_op_embed_tokens.  softmax_rows and transpose2d carry the layout contract of the fp32 VAE
attention: the padded key columns [cols, ldo) of the probabilities are zero, and V^T lands in a buffer whose pad
columns the kernel leaves alone.
"""
import math

import pytest
import torch

from tests import guard as G
from tests import opref as O

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2, torch.float16: 5e-3}     # the project's (tests/test_ops_gpu.py)
DTS = [torch.float32, torch.bfloat16, torch.float16]
EPS = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}     # one ulp at 1.0
PREC = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}                            # significand bits
MIN_EXP = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}


def _r(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _up8(n):
    return (n + 7) // 8 * 8


def half_ulp(x, dt):
    """Half an ulp of dt at |x| (float64 tensor), subnormals included."""
    ex = torch.frexp(x.abs().clamp_min(1e-300))[1] - 1                 # floor(log2 |x|)
    return torch.pow(2.0, (ex.clamp_min(MIN_EXP[dt]) - PREC[dt]).double())


# ------------------------------------------------------------------ softmax_rows
def _softmax_input(cols):
    x = torch.zeros(5, cols)
    x[0] = _r(cols, seed=cols) * 3
    x[1] = 0.731                                     # all entries equal
    x[2] = _r(cols, seed=cols + 1)
    x[2, cols - 1] = x[2].max() + 80.0               # one entry 80 above the rest, in the last 256-stride
    x[3] = -1e4 + _r(cols, seed=cols + 2) * 2        # large negative values
    x[4] = _r(cols, seed=cols + 3) * 12
    return x


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cols", [1, 7, 77, 255, 256, 257, 1000])
def test_softmax_rows(device, dt, cols):
    """float64 softmax of the fp32 input, rounded to the output type: per element within TOL[dt] (abs / max); each
    row sums to 1 within `cols` half-ulps of the output type (half an ulp at 1.0, the largest a probability's can be);
    the pad columns [cols, ldo) are exactly zero; the sentinels past the rows and the NaN poison are checked by the
    guarded buffer."""
    ld = _up8(cols) + 8
    x = _softmax_input(cols)
    xin = torch.zeros(5, ld)                         # (the wrapper's guarded copy holds NaN in the pad columns:
    xin[:, :cols] = x                                #  the kernel must not read them either)
    got = O.softmax_rows(xin.to(device), cols, ld, dt).cpu()
    assert got.shape == (5, ld)
    ref = torch.softmax(x.double(), -1)
    want = ref.to(dt)
    err = (got[:, :cols].double() - want.double()).abs().max() / want.double().abs().max()
    print(f"softmax_rows {dt} cols {cols}: err {float(err):.3e}")
    assert float(err) < TOL[dt]
    sums = got[:, :cols].double().sum(-1)
    print(f"  row sums - 1: {[f'{float(v):.3e}' for v in sums - 1]}, bound {cols * EPS[dt] / 2:.3e}")
    assert bool(((sums - 1).abs() <= cols * EPS[dt] / 2).all()), sums
    assert bool((G.bits(got[:, cols:]) == 0).all()), "padded key columns are not +0"
    assert int(got[2, :cols].argmax()) == cols - 1 and (cols == 1 or float(got[2, :cols - 1].max()) < 1e-30)


# ------------------------------------------------------------------ transpose2d
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (32, 32), (33, 65), (77, 512), (100, 3)])
def test_transpose2d(device, dt, rows, cols):
    """The V slice of fused q|k|v rows (ldi = 3 cols, third slice; batch stride past the rows) into [cols][ldo]:
    bit for bit torch.transpose; the pad columns [rows, ldo) keep their sentinels."""
    batch, ldi = 3, 3 * cols
    s_in = rows * ldi + 24
    base = _r(batch * s_in, seed=rows * 1000 + cols).to(dt).to(device)
    v = base.as_strided((batch, rows, cols), (s_in, ldi, 1), 2 * cols)
    got = O.transpose2d(v, _up8(rows))
    assert got.shape == (batch, cols, rows)
    assert G.same(got, v.transpose(1, 2))


# ------------------------------------------------------------------ timestep_embed
TS = (0.0, 1.0, 500.5, 999.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("flip", [0, 1])
def test_timestep_embed(device, dt, flip, shift, t, B):
    """dim 320 against the float64 sinusoid.  fp32 bound |err| <= t 2^-21 + 2^-22: the argument is t * expf(e); expf is
    good to a couple of ulp and two fp32 roundings are added (relative 2^-21 of an argument <= t), sin' and cos' are
    at most 1, and sinf / cosf with the final rounding stay within 2^-22.  16-bit outputs add half an ulp of the
    output.  Measured on an MI355X: fp32 max |err| 5.9e-5 (t = 999), at most 0.123 of the bound; fp16 2.6e-4 and
    bf16 1.9e-3, up to 0.997 of the bound (the output's own half ulp is nearly all of it)."""
    dim = 320
    i = TS.index(t)
    ts = torch.tensor([TS[(i + j) % 4] for j in range(B)], dtype=torch.float32)
    got = O.timestep_embed(ts.to(device), dim, flip, shift, dt).cpu().double()
    ref = O.ref_timestep_embed(ts, dim, flip, shift)
    bound = ts.double()[:, None] * 2.0 ** -21 + 2.0 ** -22
    if dt != torch.float32:
        bound = bound + half_ulp(ref.abs() + bound, dt)
    err = (got - ref).abs()
    print(f"timestep_embed {dt} flip {flip} shift {shift} t {ts.tolist()}: max err {float(err.max()):.3e}, "
          f"max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------ embed_tokens
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D,V", [(24, 49408), (768, 1000)])
def test_embed_tokens(device, dt, D, V):
    """CLIP's token + position embedding, summed in fp32 and rounded once: bit for bit."""
    B, Lt = 2, 77
    tok, pos = _r(V, D, seed=D).to(dt), (_r(Lt, D, seed=D + 1) * 0.1).to(dt)
    ids = torch.randint(0, V, (B, Lt), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    ids[0, 0], ids[0, 1], ids[1, Lt - 1], ids[1, 0] = 0, V - 1, V - 1, 0
    got = O.embed_tokens(ids.to(device), tok.to(device), pos.to(device))
    want = (tok[ids.long()].float() + pos.float()).to(dt)
    assert G.same(got.cpu(), want)
