"""LayerNorm statistics from the producers at C = 640 and 1280 (GemmArgs::ln_W; option ln_parts 2).

tests/test_ln_parts_gpu.py covers the C = 320 form (final pairs) and the two-partial form at 320 columns.  Here:
  * producers whose partial group is their tile's width: C = 1280 on the 8-wave 128x128 tile (10 partials of 128
    columns per row), C = 640 on the 128x320 tile (2 of 320) — ragged last tiles, with / without a residual, and a
    residual that wraps (GemmArgs::res_rows).  The stored output equals the plain GEMM's bit for bit, the partials
    match an fp64 two-pass over the stored rows within the bars of test_ln_out_partials;
  * folded consumers on every large-tile family, which merge their block's rows once into an LDS table before the
    main loop: against the same call handed (rstd, rstd * mean) rows computed on the host from the partials in the
    merge's order (2 ulp, the bar test_ln_fold_from_partials holds the per-row epilogue merge to) and against fp32
    LayerNorm + projection (TOL);
  * the table form against the per-row merge in the epilogue (what every tile ran before; the 256x320 tile, whose
    staging tile leaves no LDS for a table, still does): bit for bit at T = 2, width 320;
  * the UNet with ln_parts 2 against the statistics pass (0) and the C = 320-only form (1), and its batch invariance.
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd.engine import geglu64_order
from tests import opref as O

pytestmark = pytest.mark.gpu

DT16 = [torch.bfloat16, torch.float16]
TOL = {torch.bfloat16: 2e-2, torch.float16: 5e-3}
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
# C -> (partial width, images that make M = 1024 rows plan like the bench's level: 32x32 / 16x16 at 16 images)
LEVEL = {640: (320, 1), 1280: (128, 4)}


def _r(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def _dev(x, dt, device):
    return x.to(dt).to(device).contiguous()


def _tile(dt, M, N, K, geglu=False, imgs=0):
    """(BM, BN, ping-pong, blocks per CU) of the large-tile plan of a dense GEMM (zeros: another path)."""
    t = (C.c_int * 5)()
    L.load().irx_debug_gemm_tile(O.DT[dt], M, N, K, int(geglu), imgs, t)
    return t[0], t[1], t[2], t[3]


def gemm_ln_out_w(A, W, bias, R, width, res_rows=0, final_rs=False, eps=1e-5):
    """tests/opref.py's gemm_ln_out with the partial width and a wrapping residual (irx_op_gemm_ln_out_w), on guarded
    buffers like it -> (C [M, N], partials [M][N / width][2] fp32, NaN before the call)."""
    M, K = A.shape
    N = W.shape[0]
    out = O.G.out(A.device, A.dtype, M, N)
    parts = O.G.out(A.device, torch.float32, M, N // width * 2)
    A, W, bias, R = (O.G.inp(t) for t in (A, W, bias, R))
    L.call("irx_op_gemm_ln_out_w", O.S(), O.DT[A.dtype], M, N, K, O.P(A), O.P(W), O.P(bias), O.P(R), int(res_rows),
           out.ptr(), parts.ptr(), int(width), int(final_rs), float(eps))
    return (O.G.done(out, (M, N), "irx_op_gemm_ln_out_w"),
            O.G.done(parts, (M, N // width, 2), "irx_op_gemm_ln_out_w parts"))


def gemm_ln_fold_w(x, Wg, u, v, parts, T, width, geglu=False):
    """tests/opref.py's gemm_ln_fold fed partials of `width` columns (irx_op_gemm_ln_fold_w) -> [M, N] or [M, N/2]."""
    M, K = x.shape
    N = Wg.shape[0]
    No = N // 2 if geglu else N
    out = O.G.out(x.device, x.dtype, M, No)
    x, Wg, u, v, parts = (O.G.inp(t) for t in (x, Wg, u, v, parts))
    L.call("irx_op_gemm_ln_fold_w", O.S(), O.DT[x.dtype], M, N, K, O.P(x), O.P(Wg), O.P(u), O.P(v), None, O.P(parts), T,
           int(width), int(geglu), out.ptr())
    return O.G.done(out, (M, No), "irx_op_gemm_ln_fold_w")


def two_pass(x, width):   # fp64 (mean, M2) per `width`-column group
    g = x.double().view(x.shape[0], -1, width)
    mean = g.mean(-1)
    return mean, ((g - mean[..., None]) ** 2).sum(-1)


def _producer_operands(M, Cn, dt, device, rrows):
    A = _dev(_r(M, Cn, seed=1), dt, device)
    W = _dev(_r(Cn, Cn, seed=2, scale=1 / math.sqrt(Cn)), dt, device)
    bias = _r(Cn, seed=3, scale=0.5).to(device)
    R = _dev(_r(rrows, Cn, seed=4, shift=0.7), dt, device) if rrows else None
    return A, W, bias, R


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M,res", [(128, False), (128, True), (1024, False), (1024, True), (1000, False), (1000, True),
                                   (1024, "wrap")])
@pytest.mark.parametrize("Cn,tile", [(1280, (128, 128)), (640, (128, 320))])
def test_ln_out_partials_wide(device, dt, Cn, tile, M, res):
    width, imgs = LEVEL[Cn]
    wrap = res == "wrap"
    A, W, bias, R = _producer_operands(M, Cn, dt, device, (M // 2 if wrap else M) if res else 0)
    # (M = 128: a single row tile; forced onto the level's tile, which the planner picks from 512 canonical rows on)
    force = {"gemm_force": tile[0] * 100000 + tile[1] * 100 + 1} if M == 128 else {}
    with L.option(op_imgs=imgs, **force):
        assert _tile(dt, M, Cn, Cn, imgs=imgs)[:3] == (tile[0], tile[1], 0)
        out, parts = gemm_ln_out_w(A, W, bias, R, width, res_rows=M // 2 if wrap else 0)
        plain = O.gemm(A, W, bias=bias, residual=torch.cat([R, R]) if wrap else R)
    torch.cuda.synchronize()
    assert torch.equal(out, plain)                      # the emission does not change what is stored
    mean, m2 = two_pass(out.float(), width)
    scale = out.float().abs().amax(-1, keepdim=True).double()
    assert parts.shape == (M, Cn // width, 2) and torch.isfinite(parts).all()
    dm = float(((parts[..., 0].double() - mean).abs() / scale).max())
    dq = float(((parts[..., 1].double() - m2).abs() / m2).max())
    print(f"\nln_out C {Cn} M {M} res {res} {dt}: mean {dm:.2e} of max |x|, M2 rel {dq:.2e}")
    assert dm < 1e-5
    assert dq < 5e-5                                    # (one shifted fp32 pass)


@functools.lru_cache(maxsize=None)
def _stream(M, Cn, dt, device):
    """The residual stream h [M, Cn] a producer of the level wrote, with its partials (shared, read only)."""
    width, imgs = LEVEL[Cn]
    A = _dev(_r(M, Cn, seed=10), dt, device)
    Wp = _dev(_r(Cn, Cn, seed=11, scale=1 / math.sqrt(Cn)), dt, device)
    with L.option(op_imgs=imgs):
        h, parts = gemm_ln_out_w(A, Wp, _r(Cn, seed=12).to(device), _dev(_r(M, Cn, seed=13, shift=0.5), dt, device),
                                 width)
    torch.cuda.synchronize()
    return h, parts


def _ln_fold_operands(Cn, N, seed):
    W = _r(N, Cn, seed=seed, scale=1 / math.sqrt(Cn))
    b = _r(N, seed=seed + 1, scale=0.3)
    gamma = _r(Cn, seed=seed + 2, scale=0.2, shift=1.0)
    beta = _r(Cn, seed=seed + 3, scale=0.1)
    return W, b, gamma, beta


def _fold(W, b, gamma, beta, dt, device, geglu):
    perm = geglu64_order(W.shape[0]) if geglu else torch.arange(W.shape[0])
    Wg = (W * gamma)[perm].to(dt)                       # W diag(gamma) as stored
    u = Wg.double().sum(1).float()                      # row sums of the stored matrix
    v = (W.double() @ beta.double() + b.double()).float()[perm]
    return Wg.to(device).contiguous(), u.to(device).contiguous(), v.to(device).contiguous()


def _rs_from_parts(parts, width):
    """(rstd, rstd * mean) rows from the partials in the merge's order (ops.h ln_merge / ln_fin), in fp64."""
    pm, pq = parts[..., 0].double(), parts[..., 1].double()
    Cn = parts.shape[1] * width
    mean = pm.mean(-1)
    m2 = (pq + float(width) * (pm - mean[:, None]) ** 2).sum(-1)
    rstd = torch.rsqrt(m2 / Cn + 1e-5)
    mean, rstd = mean.float(), rstd.float()
    return torch.stack([rstd, rstd * mean], -1).contiguous()


# (N, K, GEGLU, the tile of the M = 1024 call: BM, BN, ping-pong, blocks per CU)
CONSUMERS = [(640, 640, False, (128, 320, 0)), (1280, 1280, False, (128, 128, 0)),
             (1920, 640, False, (256, 128, 1)), (3840, 1280, False, (256, 256, 1)),
             (5120, 640, True, (256, 128, 1)), (10240, 1280, True, (256, 128, 1))]


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("M", [1024, 1000])
@pytest.mark.parametrize("N,K,geglu,tile", CONSUMERS)
def test_ln_fold_from_wide_partials(device, dt, N, K, geglu, tile, M):
    width, imgs = LEVEL[K]
    h, parts = _stream(M, K, dt, device)
    W, b, gamma, beta = _ln_fold_operands(K, N, 20)
    Wg, u, v = _fold(W, b, gamma, beta, dt, device, geglu)
    rs = _rs_from_parts(parts, width)
    with L.option(op_imgs=imgs):
        got_tile = _tile(dt, M, N, K, geglu, imgs)
        print(f"\nln_fold N {N} K {K} M {M} geglu {geglu}: tile {got_tile}")
        assert got_tile[0] > 0                          # a large tile (whole-tile forms need M % BM == 0: M = 1024)
        if M == 1024:
            assert got_tile[:3] == tile
        got = gemm_ln_fold_w(h, Wg, u, v, parts, K // width, width, geglu=geglu)
        via_rs = O.gemm_ln_fold(h, Wg, u, v, rs=rs, geglu=geglu)
    torch.cuda.synchronize()
    d = (got.float() - via_rs.float()).abs() / via_rs.float().abs().clamp_min(1.0)
    assert float(d.max()) <= 2 * ULP[dt], float(d.max())
    ref = F.layer_norm(h.float().cpu(), (K,), gamma, beta, 1e-5) @ W.t() + b
    if geglu:
        hv, gt = ref.chunk(2, dim=-1)
        ref = hv * F.gelu(gt)
    assert O.rel_err(got, ref) < TOL[dt]


@pytest.mark.parametrize("dt", DT16)
def test_ln_table_equals_epilogue_merge(device, dt):
    """T = 2 at width 320: the 128x320 tile (rows merged once per block into the LDS table) against the 256x320 tile
    (the per-row merge in the epilogue, unchanged) — the same accumulation order and the same merge arithmetic, so the
    same bits."""
    M, K, N = 1024, 640, 640
    h, parts = _stream(M, K, dt, device)
    W, b, gamma, beta = _ln_fold_operands(K, N, 20)
    Wg, u, v = _fold(W, b, gamma, beta, dt, device, False)
    outs = []
    for bm in (128, 256):
        with L.option(op_imgs=1, tile_256x320=1, gemm_force=bm * 100000 + 320 * 100 + 1):
            assert _tile(dt, M, N, K, False, 1)[:2] == (bm, 320)
            outs.append(O.gemm_ln_fold(h, Wg, u, v, parts=parts, T=2))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])


@functools.lru_cache(maxsize=None)
def _unet(dtype, device):
    from tests import models_common as MC
    from image_restoration_and_enhancement_amd.engine import UNet
    pc, sd = MC.state_dicts("denoise")
    u = UNet(pc.unet, dtype, device)
    u.load_state_dict(sd["unet"])
    return u


def _unet_inputs(u, B, dtype, device, hw=32):
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 4, hw, hw, generator=g)
    ctx = torch.randn(B, 77, 768, generator=g)
    xin = torch.zeros(B, hw, hw, u.cin_pad)
    xin[..., :4] = x.permute(0, 2, 3, 1)
    return xin.to(tdt).to(device).contiguous(), ctx.to(tdt).to(device).contiguous()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_unet_ln_parts_wide(device, dtype):
    """32x32 latents reach the 32^2 (C 320), 16^2 (640), 8^2 and 4^2 (1280) levels: every width's producers against
    the statistics pass and against the C = 320-only form — the same LayerNorm up to the summation order."""
    u = _unet(dtype, device)
    B = 2
    xin, ctx = _unet_inputs(u, B, dtype, device)
    kv = u.prepare_context(ctx)
    outs = {}
    for v in (2, 1, 0):
        with L.option(ln_parts=v):
            outs[v] = u.forward(xin, torch.full((B,), 481.0, device=device), kv, 77).float().cpu()
    bar = 1e-2 if dtype == "bf16" else 3e-3
    assert torch.isfinite(outs[2]).all()
    for other in (0, 1):
        rel = float((outs[2] - outs[other]).norm() / outs[other].norm())
        print(f"\nln_parts 2 vs {other} ({dtype}): rel L2 {rel:.2e}")
        assert rel < bar, (other, rel)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_unet_ln_parts_wide_batch_invariant(device, dtype):
    u = _unet(dtype, device)
    xin, ctx = _unet_inputs(u, 5, dtype, device)

    def run(x, c):
        return u.forward(x.contiguous(), torch.full((x.shape[0],), 481.0, device=device),
                         u.prepare_context(c.contiguous()), 77)
    with L.option(ln_parts=2):
        whole = run(xin, ctx)
        split = torch.cat([run(xin[:2], ctx[:2]), run(xin[2:], ctx[2:])])
    torch.cuda.synchronize()
    assert torch.isfinite(whole.float()).all()
    assert torch.equal(whole, split)
