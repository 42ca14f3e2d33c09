"""The tile-order remaps at ragged tile counts: xcd_remap (irx_common.h), GemmArgs::nmajor and GemmArgs::group_m of
the dense and the halo large-tile kernels (gemm2.hip), AttnArgs::xcd (attention.hip) and the gemm_sk grid
(per_xcd / n_slices groups, gemm_sk.hip).  They are "scheduling only" exactly as long as each map is a bijection:
a map that is not computes one tile twice and another not at all.  Every case runs one shape under each order on
guarded outputs (tests/guard.py: an unwritten tile is NaN, a tile written twice past the edge hits a sentinel), asserts
the outputs bit-identical to each other and within the project's tolerance of the fp32 CPU reference, and ASSERTS the
ragged condition it is there for from the plan queries (irx_debug_gemm_tile / irx_debug_conv_plan) or, where no query
exists (attention, gemm_sk), from the launcher's own arithmetic restated next to the assertion.
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from image_restoration_and_enhancement_amd import _lib as L
from tests import opref as O
from tests.guard import same

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 2e-2, torch.float16: 5e-3}        # tests/test_ops_gpu.py
DT16 = [torch.bfloat16, torch.float16]
GEMM_SK, GEMM_HALO, GEMM_LARGE = 2, 3, 4                  # GemmPath (csrc/gemm_plan.h)


def _r(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _dev(x, dt, device):
    return x.to(dt).to(device).contiguous()


def _q(x, dt):
    return x.to(dt).float()


def gemm_tile(dt, M, N, K, geglu=False):
    t = (C.c_int * 5)()
    L.call("irx_debug_gemm_tile", O.DT[dt], M, N, K, int(geglu), 0, t)
    return dict(zip(("BM", "BN", "pp", "bpc", "group_m"), t))


def conv_plan(dt, n, h, w, cin, cout):
    t = (C.c_int * 7)()
    L.call("irx_debug_conv_plan", O.DT[dt], cin, 0, n, h, w, h, w, cout, 3, 3, 1, 1, 1, h, w, 0, t)
    return dict(zip(("path", "BM", "BN", "group_m", "splits", "tiles_m", "tiles_n"), t))


def _all_same(outs):
    first = next(iter(outs))
    for k, v in outs.items():
        assert same(v, outs[first]), f"order {k} changes bits against {first}"


# ------------------------------------------------------------------ B.1 dense large-tile GEMM
GM, GN, GK = 1297, 768, 640          # 128 x 128 tiles: 11 x 6 = 66 tiles (66 % 8 = 2), 11 % 2 = 1, 11 % 4 = 3


@functools.lru_cache(maxsize=None)
def _gemm_case(dt, res):
    A, Bw = _r(GM, GK, seed=500), _r(GN, GK, seed=501, scale=1 / math.sqrt(GK))
    bias, R = _r(GN, seed=502), (_r(GM, GN, seed=503) if res else None)
    ref = _q(A, dt) @ _q(Bw, dt).T + bias + (_q(R, dt) if res else 0)
    return A, Bw, bias, R, ref


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("dt", DT16)
def test_dense_gemm_orders(device, dt, res):
    A, Bw, bias, R, ref = _gemm_case(dt, res)
    a_d, b_d, bias_d = _dev(A, dt, device), _dev(Bw, dt, device), bias.to(device)
    r_d = _dev(R, dt, device) if res else None
    outs = {}
    for name, opts, want_g in [("m_major", dict(gemm_group=0, gemm_nmajor=0), 0),
                               ("n_major", dict(gemm_group=0, gemm_nmajor=2), 0),
                               ("group_2", dict(gemm_group=2), 2), ("group_4", dict(gemm_group=4), 4)]:
        with L.option(**opts):
            t = gemm_tile(dt, GM, GN, GK)
            assert t["BM"] > 0, f"{name}: not on the large-tile kernel: {t}"
            tiles_m, tiles_n = -(-GM // t["BM"]), -(-GN // t["BN"])
            assert (tiles_m * tiles_n) % 8 != 0, (name, tiles_m, tiles_n)          # ragged xcd_remap ranges
            assert GM % t["BM"] != 0                                               # a ragged last M tile
            assert t["group_m"] == want_g, (name, t)
            assert want_g == 0 or tiles_m % want_g != 0, (name, tiles_m)           # a partial last group
            outs[name] = O.gemm(a_d, b_d, bias=bias_d, residual=r_d)
    _all_same(outs)
    assert O.rel_err(outs["m_major"], ref) < TOL[dt]


# ------------------------------------------------------------------ B.2 halo 3x3 convs
HALO_CASES = {
    # (n, h, w, cin, cout, residual): 5 M tiles in groups of 4 -> a last group of one; 5 x 8 tiles
    "partial_group": (5, 16, 16, 1280, 1280, False),
    # 12 x 3 = 36 tiles (36 % 8 = 4), tiles_n odd, groups of 8 M tiles -> a last group of four, 2 K splits
    "ragged_xcd_odd_n": (3, 32, 32, 640, 480, True),
}


@functools.lru_cache(maxsize=None)
def _conv_case(name, dt):
    n, h, w, ci, co, res = HALO_CASES[name]
    x = _r(n, ci, h, w, seed=510)
    wt = _r(co, ci, 3, 3, seed=511, scale=1 / math.sqrt(ci * 9))
    b = _r(co, seed=512)
    R = _r(n, h, w, co, seed=513) if res else None
    ref = F.conv2d(_q(x, dt), _q(wt, dt), b, padding=1).permute(0, 2, 3, 1)
    if res:
        ref = ref + _q(R, dt)
    return x, wt, b, R, ref


@pytest.mark.parametrize("name", list(HALO_CASES))
@pytest.mark.parametrize("dt", DT16)
def test_halo_conv_orders(device, dt, name):
    n, h, w, ci, co, res = HALO_CASES[name]
    x, wt, b, R, ref = _conv_case(name, dt)
    x_d = _dev(x.permute(0, 2, 3, 1), dt, device)
    r_d = _dev(R, dt, device) if res else None
    outs = {}
    for hg in (0, 1):
        with L.option(halo_group=hg):
            p = conv_plan(dt, n, h, w, ci, co)
            assert p["path"] == GEMM_HALO and p["tiles_n"] >= 2, p
            if hg == 0:
                assert p["group_m"] == 0, p
            else:
                assert p["group_m"] > 0 and p["tiles_m"] % p["group_m"] != 0, p      # the gm = min(...) branch
                if name == "ragged_xcd_odd_n":
                    assert (p["tiles_m"] * p["tiles_n"]) % 8 != 0 and p["tiles_n"] % 2 == 1, p
            outs[hg] = O.conv2d(x_d, wt.to(dt).float(), b, residual=r_d)
    _all_same(outs)
    assert O.rel_err(outs[0], ref) < TOL[dt]


# ------------------------------------------------------------------ B.3 attention
# AttnArgs::xcd is read by attn3_kernel (128 queries per group; d = 40 cross-attention with resident K/V, d = 64, 80
# and 160) and by attn3q_kernel (256 queries per block; d = 40 self-attention).  launch3_cfg's grid restated:
def _attn_blocks(d, B, H, Lq, Lk, qrep_opt):
    if d == 40 and (Lk > 128 or qrep_opt == 0):
        return -(-Lq // 256) * H * B                      # attn3q (every d = 40 call without resident K/V)
    qrep = 1
    if Lk <= 128 and qrep_opt >= 2:
        qrep = qrep_opt                                   # resident K/V, a forced group count
    elif Lk <= 128 and qrep_opt == 1:
        while qrep < 8 and -(-Lq // (256 * qrep)) * H * B >= (1024 if d <= 40 else 512):
            qrep *= 2
    return -(-Lq // (128 * qrep)) * H * B


@functools.lru_cache(maxsize=None)
def _attn_case(d, Lk, dt):
    B, H, Lq = 1, 5, 333
    q, k, v = _r(B, Lq, H * d, seed=520), _r(B, Lk, H * d, seed=521), _r(B, Lk, H * d, seed=522)
    return q, k, v, O.ref_attention(_q(q, dt), _q(k, dt), _q(v, dt), H)


@pytest.mark.parametrize("Lk", [190, 77], ids=["self", "cross"])
@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("dt", DT16)
def test_attention_xcd_orders(device, dt, d, Lk):
    """B = 1, 5 heads, Lq = 333: 15 blocks of 128 queries, 10 of 256.  attn_qrep at its default (1: the launcher
    chooses the query groups per block), at 0 (cross-attention on the streaming kernel) and at 2 (two groups forced);
    at each, attn_xcd 0 against 1."""
    B, H, Lq = 1, 5, 333
    q, k, v, ref = _attn_case(d, Lk, dt)
    qd, kd, vd = _dev(q, dt, device), _dev(k, dt, device), _dev(v, dt, device)
    for qrep in (1, 0, 2):
        assert _attn_blocks(d, B, H, Lq, Lk, qrep) % 8 != 0
        outs = {}
        for xcd in (0, 1):
            with L.option(attn_xcd=xcd, attn_qrep=qrep):
                outs[xcd] = O.attention(qd, kd, vd, H)
        _all_same(outs)
        assert O.rel_err(outs[0], ref) < 2 * TOL[dt]      # (test_ops_gpu.test_attention's bound for 16-bit types)


# ------------------------------------------------------------------ B.4 gemm_sk
def _sk_grid(N, blocks_opt, geglu=False, bpc=1):
    """launch_sk restated: weight slices of 320 columns (GEGLU: 128 outputs), per_xcd blocks per XCD in groups."""
    n_slices = (N // 2) // 128 if geglu else N // 320
    per_xcd = max(n_slices, blocks_opt if blocks_opt > 0 else 32 * bpc)
    return n_slices, per_xcd


@functools.lru_cache(maxsize=None)
def _sk_case(M, N, dt):
    K = 320
    A, Bw = _r(M, K, seed=530), _r(N, K, seed=531, scale=1 / math.sqrt(K))
    bias, R = _r(N, seed=532), _r(M, N, seed=533)
    return A, Bw, bias, R, _q(A, dt) @ _q(Bw, dt).T + bias + _q(R, dt)


@pytest.mark.parametrize("N", [320, 960])
@pytest.mark.parametrize("M", [777, 1025])
@pytest.mark.parametrize("dt", DT16)
def test_gemm_sk_grids(device, dt, M, N):
    """gemm_sk_blocks default, 1 (per_xcd clamps to n_slices: the minimum grid, one group) and 7 (N = 960: three
    slices, 7 % 3 = 1, so one block per XCD has no group and must do nothing)."""
    A, Bw, bias, R, ref = _sk_case(M, N, dt)
    a_d, b_d, r_d, bias_d = _dev(A, dt, device), _dev(Bw, dt, device), _dev(R, dt, device), bias.to(device)
    assert _sk_grid(N, 1) == (N // 320, N // 320)
    assert N != 960 or _sk_grid(N, 7)[1] % _sk_grid(N, 7)[0] != 0
    outs = {}
    for blocks in (0, 1, 7):
        with L.option(gemm_sk=3, gemm_sk_blocks=blocks):
            assert gemm_tile(dt, M, N, 320)["BM"] == 0          # not the large-tile kernel: gemm_sk takes K = 320
            outs[blocks] = O.gemm(a_d, b_d, bias=bias_d, residual=r_d)
    with L.option(gemm_sk=0):
        assert gemm_tile(dt, M, N, 320)["BM"] > 0
        outs["large_tile"] = O.gemm(a_d, b_d, bias=bias_d, residual=r_d)     # (bit for bit: test_ops_gpu.test_gemm_sk)
    _all_same(outs)
    assert O.rel_err(outs[0], ref) < TOL[dt]


@pytest.mark.parametrize("dt", DT16)
def test_gemm_sk_geglu_grids(device, dt):
    from image_restoration_and_enhancement_amd.engine import geglu64_order
    M, Cc = 1025, 320
    A, Wt, bias = _r(M, Cc, seed=540), _r(8 * Cc, Cc, seed=541, scale=1 / math.sqrt(Cc)), _r(8 * Cc, seed=542)
    perm = geglu64_order(8 * Cc)
    a_d, w_d, b_d = _dev(A, dt, device), _dev(Wt[perm], dt, device), bias[perm].to(device).contiguous()
    assert _sk_grid(8 * Cc, 7, geglu=True) == (10, 10) and _sk_grid(8 * Cc, 0, geglu=True, bpc=2) == (10, 64)
    outs = {}
    for blocks in (0, 1, 7):
        with L.option(gemm_sk=1, gemm_sk_blocks=blocks):
            assert gemm_tile(dt, M, 8 * Cc, Cc, geglu=True)["BM"] == 0
            outs[blocks] = O.gemm_geglu(a_d, w_d, b_d)
    _all_same(outs)
    pr = _q(A, dt) @ _q(Wt, dt).T + bias
    h, g = pr.chunk(2, dim=-1)
    assert O.rel_err(outs[0], h * F.gelu(g)) < TOL[dt]
