"""The ping-pong loop on 256x128 / 128x256 tiles, two resident 8-wave blocks per CU (option gemm_pp2; csrc/gemm2.hip).

The tiles run the K steps of every output element in the order of every other large-tile loop (32-deep MFMA steps,
ascending, one accumulator) and the same epilogue arithmetic, so the outputs must be bit for bit what the library gives
with the option off.  Each case runs with the option off (0) and with the 256x128 (2) and 128x256 (3) tiles forced, and
compares the raw 16-bit tensors; the planner query confirms that the forced runs really took the new tiles.

Covered: K of 1, 2, 3 and 5 ring steps of 32 (the prologue's clamped re-issue, the unroll-by-3 tail) on plain GEMMs
(a K that is no multiple of 64 runs on the 4-wave kernel with the option off: it adds a residual before the 16-bit
rounding, the large tiles after it, so those cases carry no residual; the fused GEGLU and the LayerNorm fold exist on
the large tiles only, so those take K = 64 / 128 / 192 = 2, 4 and 6 steps); one tile; 2 x 3 tiles in the
grouped tile order; M = 512 with N = 256 / 768; GEGLU at N = 256 / 512; with and without the LayerNorm fold; an M that
is no multiple of the tile, which the planner must decline.
"""
import ctypes as C
import math

import pytest
import torch

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd.engine import geglu64_order
from tests import opref as O

pytestmark = pytest.mark.gpu

DT16 = [torch.bfloat16, torch.float16]
TILES = {2: (256, 128), 3: (128, 256)}


def _r(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def _dev(x, dt, device):
    return x.to(dt).to(device).contiguous()


def plan_tile(dt, M, N, K, geglu=False, imgs=0):
    """(BM, BN, ping-pong, blocks per CU, group_m) of the large-tile plan under the current options, zeros otherwise."""
    t = (C.c_int * 5)()
    assert L.load().irx_debug_gemm_tile(O.DT[dt], M, N, K, int(geglu), imgs, t) == 0
    return tuple(t)


def run_modes(fn, dt, M, N, K, geglu=False, imgs=0, expect_pair=True):
    """fn() with the option off, then with each tile forced; the forced runs must plan the new tile (or decline it)."""
    outs = {}
    for mode in (0, 2, 3):
        with L.option(gemm_pp2=mode, op_imgs=imgs):
            t = plan_tile(dt, M, N, K, geglu, imgs)
            if mode == 0:
                assert t[3] != 2 or not t[2], t
            elif expect_pair:
                assert t[:4] == (*TILES[mode], 1, 2), (mode, t)
            else:
                assert not (t[2] and t[3] == 2), (mode, t)
            outs[mode] = fn()
    torch.cuda.synchronize()
    return outs


def check(outs):
    assert torch.isfinite(outs[0].float()).all()
    for mode in (2, 3):
        assert torch.equal(outs[0].view(torch.int16), outs[mode].view(torch.int16)), mode


def _plain(dt, device, M, N, K, res):
    A = _dev(_r(M, K, seed=1), dt, device)
    Bw = _dev(_r(N, K, seed=2, scale=1 / math.sqrt(K)), dt, device)
    bias = _r(N, seed=3).to(device).contiguous()
    R = _dev(_r(M, N, seed=4), dt, device) if res else None
    return lambda: O.gemm(A, Bw, bias=bias, residual=R)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("K", [32, 64, 96, 160])
@pytest.mark.parametrize("N,res", [(256, False), (768, True)])
def test_pair_plain_ring_steps(device, dt, K, N, res):
    M = 512
    check(run_modes(_plain(dt, device, M, N, K, res and K % 64 == 0), dt, M, N, K))


@pytest.mark.parametrize("dt", DT16)
def test_pair_one_tile(device, dt):
    """One tile per launch: rows of one image of 16 (the canonical row count keeps the call on the large tiles)."""
    for mode, (bm, bn) in TILES.items():
        fn = _plain(dt, device, bm, bn, 192, False)
        outs = {}
        for m in (0, mode):
            with L.option(gemm_pp2=m, op_imgs=1):
                if m:
                    assert plan_tile(dt, bm, bn, 192, imgs=1)[:4] == (bm, bn, 1, 2)
                outs[m] = fn()
        torch.cuda.synchronize()
        assert torch.equal(outs[0].view(torch.int16), outs[mode].view(torch.int16)), mode


@pytest.mark.parametrize("dt", DT16)
def test_pair_grouped_order(device, dt):
    """2 x 3 tiles of each form in the grouped tile order (six tiles are too few for the cost model to group them, so
    option gemm_group 2 asks for groups of two M tiles)."""
    K = 192
    for mode, (bm, bn) in TILES.items():
        M, N = 2 * bm, 3 * bn
        fn = _plain(dt, device, M, N, K, True)
        outs = {}
        for m in (0, mode):
            with L.option(gemm_pp2=m, gemm_group=2, op_imgs=1):   # (rows of one image of 16, as in the one-tile case)
                if m:
                    t = plan_tile(dt, M, N, K, imgs=1)
                    assert t == (bm, bn, 1, 2, 2), t
                outs[m] = fn()
        torch.cuda.synchronize()
        assert torch.equal(outs[0].view(torch.int16), outs[mode].view(torch.int16)), mode


def _fold_operands(dt, device, M, N, K, geglu):
    x = _dev(_r(M, K, seed=10, shift=0.3), dt, device)
    W = _r(N, K, seed=11, scale=1 / math.sqrt(K))
    gamma, beta, b = _r(K, seed=12, scale=0.2, shift=1.0), _r(K, seed=13, scale=0.1), _r(N, seed=14, scale=0.3)
    perm = geglu64_order(N) if geglu else torch.arange(N)
    Wg = (W * gamma)[perm].to(dt)
    u = Wg.double().sum(1).float().to(device).contiguous()
    v = (W.double() @ beta.double() + b.double()).float()[perm].to(device).contiguous()
    xf = x.float()
    mean = xf.mean(-1)
    rstd = torch.rsqrt(xf.var(-1, unbiased=False) + 1e-5)
    rs = torch.stack([rstd, rstd * mean], -1).contiguous()
    return x, Wg.to(device).contiguous(), u, v, rs


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("K", [64, 128, 192])
@pytest.mark.parametrize("N", [256, 512])
def test_pair_geglu(device, dt, N, K):
    M = 512
    A = _dev(_r(M, K, seed=20), dt, device)
    W = _dev(_r(N, K, seed=21, scale=1 / math.sqrt(K))[geglu64_order(N)], dt, device)
    b = _r(N, seed=22).to(device).contiguous()

    def fn():
        return O.gemm_geglu(A, W, b)
    check(run_modes(fn, dt, M, N, K, geglu=True))


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("N,geglu", [(256, False), (768, False), (256, True), (512, True)])
def test_pair_ln_fold(device, dt, N, geglu, K):
    M = 512
    x, Wg, u, v, rs = _fold_operands(dt, device, M, N, K, geglu)

    def fn():
        return O.gemm_ln_fold(x, Wg, u, v, rs=rs, geglu=geglu)
    check(run_modes(fn, dt, M, N, K, geglu=geglu))


@pytest.mark.parametrize("dt", DT16)
def test_pair_declined_on_partial_tiles(device, dt):
    """M = 576 is no multiple of 256 or 128: the planner keeps the parent's kernel and the result is unchanged."""
    M, N, K = 576, 256, 128
    check(run_modes(_plain(dt, device, M, N, K, True), dt, M, N, K, expect_pair=False))
