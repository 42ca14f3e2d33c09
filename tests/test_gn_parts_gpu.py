"""GroupNorm statistics from producer partials (GemmArgs::gn_part), op by op against tests/gnref.py (fp64).

Every 16-bit UNet / VAE GroupNorm reads (sum, sum of squares) blocks written by the kernel that stored the tensor.
Checked here through the C ABI, the producers as the models call them (irx_op_conv2d_gn_parts, irx_op_gemm_gn_parts,
irx_op_upsample_conv_gn_parts) and the consumers on host-made partials (irx_op_group_norm_parts,
irx_op_group_norm_parts_ab), so neither side can hide the other's mistake:

  producers, per emitter (asserted from the plan's answer: rows per partial R, K splits, halo main loop):
    (a) the stored output is bit-identical with and without the emission;
    (b) it matches the fp32 CPU reference of the op within test_ops_gpu.TOL;
    (c) the partials are finite and equal the fp64 block sums of the stored output: with mean = A / R and
        M2 = B - A^2 / R per block and channel, |d mean| <= 1e-5 max|x| of the block column and M2 relative 5e-5 (the
        bounds test_ln_parts_gpu takes for the same arithmetic: one fp32 pass of sums shifted by the thread's first
        value, merged in fp64) — per image always, per block wherever a block is a run of consecutive rows;
    (d) the partials of an image do not depend on the batch it ran in (3 images vs each alone, torch.equal).
  consumers: output vs gnref within TOL, bit-identical between the fused kernel (gn_fa) and finalize + apply,
    (mean, rstd) and the scale / shift pairs vs fp64, and within one 16-bit ulp of the statistics-pass GroupNorm.

The inputs give image i an offset that grows with i, one 8-channel chunk a mean of 40 with standard deviation 0.3
(where an unshifted fp32 sum of squares fails), and every column real spread; partial buffers start as NaN.
Small forced-halo shapes run under option conv_halo = 2 like test_ops_gpu.test_conv_halo: the planner gives halo
tiles to grids that fill the chip, which no few-second test reaches.

Measured on an MI355X: the partials sit at |d mean| / max|x| <= 2e-9 and M2 relative <= 2.5e-7, the finalize at
3.4e-8 / 5.9e-8, two to three orders below the bounds.  Two mutations of gemm2.hip, tried once and not kept: swapping
two parities in the sub-pixel block remap fails test_upsampler_parity_convs alone (per block: mean off by 4e-2, M2 by
0.4) while every model-level comparison still passes, since an image's totals do not move; dropping the cross term
2 x sd of the epilogue's shifted-sum expansion fails every large-tile / halo producer case here (and is gross enough
for the model-level tests to see as well)."""
import math

import pytest
import torch
import torch.nn.functional as F

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd.engine import conv_up2
from tests import gnref as R
from tests import opref as O
from tests.test_ops_gpu import TOL

pytestmark = pytest.mark.gpu

DT16 = [torch.bfloat16, torch.float16]
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
G, EPS = 32, 1e-5
NB = 3          # images every producer input is made for (the batch-invariance runs take all three)


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _dev(x, dt, device):
    return x.to(dt).to(device).contiguous()


def _q(x, dt):
    return x.to(dt).float()


def _shift(n):   # image i's offset 3 i, broadcast over an [n][...] tensor's trailing dimensions
    return 3.0 * torch.arange(n, dtype=torch.float32)


def _hard_weights(Co, K, seed):
    """[Co][K] weights and a bias whose output has spread ~1 in every column, but mean 40 / deviation 0.3 in columns
    8 .. 16."""
    w = _r(Co, K, seed=seed, scale=1 / math.sqrt(K))
    b = _r(Co, seed=seed + 1)
    w[8:16] *= 0.3
    b[8:16] = 40.0
    return w, b


def _kernels(fn):
    """fn() and the names of the kernels it launched (the in-process profile), namespaces dropped."""
    L.profile_begin()
    try:
        out = fn()
    finally:
        names = {p[0].split("::")[-1] for p in L.profile_end()}
    return out, names


# ------------------------------------------------------------------ the checks every producer case runs
def _cmp_sums(got, want, cnt, amax, what):
    """(sum, sum of squares) pairs `got` vs fp64 `want` over `cnt` values each; amax = max |x| of the same values."""
    gm, wm = got[..., 0] / cnt, want[..., 0] / cnt
    g2, w2 = got[..., 1] - got[..., 0] ** 2 / cnt, want[..., 1] - want[..., 0] ** 2 / cnt
    assert float(w2.min()) > 1e-3 * cnt, "a column without spread: M2 near zero checks nothing"
    dmean = float(((gm - wm).abs() / amax).max())
    dm2 = float(((g2 - w2).abs() / w2).max())
    print(f"\n  {what}: |d mean| / max|x| {dmean:.2e} (bound 1e-5), M2 relative {dm2:.2e} (bound 5e-5)")
    assert dmean <= 1e-5, (what, dmean)
    assert dm2 <= 5e-5, (what, dm2)


def _check_parts(parts, stored, n, R_, per_block, up2=False):
    """parts [blocks][C][2] (device, float64) against the stored [n][...][C] output."""
    got = parts.cpu()
    assert torch.isfinite(got).all(), "a partial block was never written"
    C = stored.shape[-1]
    s = stored.double().cpu()
    want = R.block_sums_up2(s, R_) if up2 else R.block_sums(s.reshape(-1, C), R_)
    assert got.shape == want.shape
    hw = s.reshape(n, -1, C).shape[1]
    amax_img = s.reshape(n, hw, C).abs().amax(1)
    _cmp_sums(R.image_sums(got, n), R.image_sums(want, n), hw, amax_img, "per image")
    if per_block:
        if up2:
            rows = torch.cat([s[i, a::2, b::2].reshape(-1, C) for i in range(n) for a in (0, 1) for b in (0, 1)])
        else:
            rows = s.reshape(-1, C)
        _cmp_sums(got, want, R_, rows.reshape(-1, R_, C).abs().amax(1), "per block")


def _producer(run, plain, ref, n, dt, expect, per_block=True, up2=False):
    """run(sel) -> (out, parts, info) and plain(sel) -> out over the images `sel`; ref(sel) -> fp32 CPU reference."""
    sel = list(range(n))
    (out, parts, info), kernels = _kernels(lambda: run(sel))
    reduce = info["R"] == 64 and info.get("splits", 1) > 2      # (the only emitter with a kernel of its own)
    assert any(k.startswith("splitk_reduce_gn_kernel") for k in kernels) == reduce, kernels
    for k, v in expect.items():
        assert (v(info[k]) if callable(v) else info[k] == v), f"the planner chose another emitter: {info}"
    print(f"\n  emitter: {info}")
    base = plain(sel)
    torch.cuda.synchronize()
    assert torch.equal(out, base)                                   # (a)
    assert O.rel_err(out, ref(sel)) < TOL[dt]                       # (b)
    _check_parts(parts, out, n, info["R"], per_block, up2)          # (c)
    all3 = parts if n == NB else run(list(range(NB)))[1]            # (d)
    all3 = all3.cpu()
    bpi = all3.shape[0] // NB
    for i in range(NB):
        alone = run([i])[1].cpu()
        assert alone.shape[0] == bpi
        assert torch.equal(all3[i * bpi:(i + 1) * bpi], alone), f"image {i}'s partials depend on its batch"


def _conv_case(H, W, C0, C1, Co, k, extra, dt, device, seed):
    """-> run, plain, ref for a stride-1 same-size conv of (x0 | x1) with bias (+ row add + residual)."""
    x = _r(NB, H, W, C0 + C1, seed=seed) + _shift(NB)[:, None, None, None]
    w, b = _hard_weights(Co, (C0 + C1) * k * k, seed + 1)
    w = w.reshape(Co, k, k, C0 + C1).permute(0, 3, 1, 2).contiguous()      # OIHW
    ra = (_r(NB, Co, seed=seed + 3) + _shift(NB)[:, None]) if extra else None
    res = _r(NB, H, W, Co, seed=seed + 4) if extra else None
    x0d = _dev(x[..., :C0], dt, device)
    x1d = _dev(x[..., C0:], dt, device) if C1 else None
    rad = ra.to(device).contiguous() if extra else None
    resd = _dev(res, dt, device) if extra else None
    wq = w.to(dt).float()

    def args(sel):
        return (x0d[sel].contiguous(), wq, b), dict(x1=x1d[sel].contiguous() if C1 else None,
                                                    rowadd=rad[sel].contiguous() if extra else None,
                                                    residual=resd[sel].contiguous() if extra else None)

    def run(sel):
        a, kw = args(sel)
        return O.conv2d_gn_parts(*a, pad=k // 2, **kw)

    def plain(sel):
        a, kw = args(sel)
        return O.conv2d(*a, pad=(k // 2, k // 2), **kw)

    def ref(sel):
        y = F.conv2d(_q(x[sel], dt).permute(0, 3, 1, 2), wq, b, padding=k // 2)
        if extra:
            y = y + ra[sel][:, :, None, None]
        y = y.permute(0, 2, 3, 1)
        return y + _q(res[sel], dt) if extra else y

    return run, plain, ref


@pytest.fixture
def halo_forced():
    with L.option(conv_halo=2):
        yield


# ------------------------------------------------------------------ producers
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("C0,C1,Co,extra", [(64, 0, 160, False), (128, 0, 128, False), (64, 0, 160, True),
                                            (64, 64, 160, False), (64, 64, 128, True)],
                         ids=["64-160", "128-128", "64-160+rowadd+res", "64+64-160", "64+64-128+rowadd+res"])
def test_halo_row_tiles(device, halo_forced, dt, C0, C1, Co, extra):
    """Whole-row halo tiles (HALO 2): 16x16 images, one 256-row tile = one image = one partial block."""
    run, plain, ref = _conv_case(16, 16, C0, C1, Co, 3, extra, dt, device, 100)
    _producer(run, plain, ref, 2, dt, {"R": 256, "splits": 1, "halo": 2})


@pytest.mark.parametrize("dt", DT16)
def test_halo_strip_tiles(device, halo_forced, dt):
    """8 x 32 strip tiles (HALO 5) of an 8x96 image: a block is a strip, not a run of rows — image totals only."""
    run, plain, ref = _conv_case(8, 96, 64, 0, 160, 3, False, dt, device, 110)
    _producer(run, plain, ref, 1, dt, {"R": 256, "splits": 1, "halo": 5}, per_block=False)


@pytest.mark.parametrize("dt", DT16)
def test_halo_two_splits_in_kernel(device, dt):
    """The smallest halo conv the planner gives two K splits under halo_split (32x32, 512 -> 320: 128 tiles at the
    canonical 16 images, 8 slabs): the last-arriving split reduces in the kernel and emits the tile's partials."""
    run, plain, ref = _conv_case(32, 32, 512, 0, 320, 3, True, dt, device, 120)
    _producer(run, plain, ref, 1, dt, {"R": 256, "splits": 2, "halo": 2})


@pytest.mark.parametrize("dt", DT16)
def test_8x8_images_reduce_kernel(device, dt):
    """Four 8x8 images per halo tile (HALO 8; 3 images: a partial last tile), more than two K splits, so
    splitk_reduce_gn_kernel finishes the output and emits one partial per 64 rows = per image."""
    run, plain, ref = _conv_case(8, 8, 320, 0, 320, 3, True, dt, device, 130)
    _producer(run, plain, ref, 3, dt, {"R": 64, "splits": lambda s: s > 2, "halo": 8})


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("H,W,C0,C1,Co,k",
                         [(16, 24, 64, 0, 128, 3), (16, 16, 128, 0, 256, 1), (16, 16, 64, 64, 128, 1)],
                         ids=["3x3-16x24", "1x1-dense", "1x1-two-sources"])
def test_im2col_large_tiles(device, dt, H, W, C0, C1, Co, k):
    """The large-tile epilogue off the halo path: a 3x3 conv whose 24-pixel rows the halo tiles refuse (im2col walk),
    and 1x1 convs rewritten as dense GEMMs (one and two sources)."""
    run, plain, ref = _conv_case(H, W, C0, C1, Co, k, k == 3, dt, device, 140)
    _producer(run, plain, ref, 2, dt, {"R": lambda r: r in (128, 256) and H * W % r == 0, "splits": 1, "halo": 0})


def _dense_case(rows, N, K, dt, device, seed):
    A = _r(NB, rows, K, seed=seed) + _shift(NB)[:, None, None] / 3.0
    w, b = _hard_weights(N, K, seed + 1)
    res = _r(NB, rows, N, seed=seed + 3)
    Ad, wd, bd, resd = _dev(A, dt, device), _dev(w, dt, device), b.to(device), _dev(res, dt, device)

    def run(sel):
        return O.gemm_gn_parts(Ad[sel].reshape(-1, K).contiguous(), wd, bd, resd[sel].reshape(-1, N).contiguous(),
                               len(sel))

    def plain(sel):
        with L.option(op_imgs=len(sel)):
            return O.gemm(Ad[sel].reshape(-1, K).contiguous(), wd, bias=bd,
                          residual=resd[sel].reshape(-1, N).contiguous())

    def ref(sel):
        return (_q(A[sel], dt) @ _q(w, dt).T + b + _q(res[sel], dt)).reshape(-1, N)

    return run, plain, ref


@pytest.mark.parametrize("dt", DT16)
def test_dense_gemm(device, dt):
    """Model::linear's form: 2 x 256 rows, N = K = 320, bias + residual, one K split."""
    run, plain, ref = _dense_case(256, 320, 320, dt, device, 150)
    _producer(run, plain, ref, 2, dt, {"R": lambda r: r in (128, 256), "splits": 1})


@pytest.mark.parametrize("dt", DT16)
def test_dense_gemm_two_splits_in_kernel(device, dt):
    """K = 2048 over few tiles: two K splits, the last arriver reduces in the kernel and emits the 128-row blocks."""
    run, plain, ref = _dense_case(256, 320, 2048, dt, device, 155)
    _producer(run, plain, ref, 2, dt, {"R": 128, "splits": 2})


@pytest.mark.parametrize("dt", DT16)
def test_dense_gemm_reduce_kernel(device, dt):
    """A dense GEMM with a long K and few tiles (test_gemm_splitk_modes' (1024, 1280, 2560) moved by the query to the
    smallest shape with more than two splits: 512 x 320 x 4096, eight): the reduce kernel emits per 64 rows, four
    blocks per 256-row image."""
    run, plain, ref = _dense_case(256, 320, 4096, dt, device, 160)
    _producer(run, plain, ref, 2, dt, {"R": 64, "splits": lambda s: s > 2})


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("forced", [False, True], ids=["large-tiles", "halo-tiles"])
def test_upsampler_parity_convs(device, dt, forced):
    """Nearest-2x + 3x3 conv as four per-parity 2x2 convs (16x16 -> 32x32, 128 channels), on the im2col large tiles
    (two 128-row blocks per image and parity) and on the 4-tap halo tiles: the output against the fp64 per-parity
    reference with the same rounded weights, the partial blocks against the sub-pixel block sums."""
    h, w, c = 16, 16, 128
    x = _r(NB, h, w, c, seed=170) + _shift(NB)[:, None, None, None] / 3.0
    wt, b = _hard_weights(c, c * 9, 171)
    w2 = conv_up2(wt.reshape(c, 3, 3, c).permute(0, 3, 1, 2)).float()
    xd, w2d, bd = _dev(x, dt, device), _dev(w2, dt, device), b.to(device)

    def run(sel):
        out, parts, q = O.upsample_conv_gn_parts(xd[sel].contiguous(), w2d, bd)
        return out, parts, q

    def plain(sel):
        with L.option(gn_parts=0):      # (no entry point runs the parity convs without the request: the option does)
            out, parts, q = O.upsample_conv_gn_parts(xd[sel].contiguous(), w2d, bd)
        assert q["R"] == 0 and torch.isnan(parts).all()
        return out

    def ref(sel):
        return R.up2_conv_ref(_q(x[sel], dt), _q(w2, dt), b).float()

    with L.option(conv_halo=2 if forced else 1):
        _producer(run, plain, ref, 2, dt, {"up2": 1, "R": 256 if forced else 128}, up2=True)


@pytest.mark.parametrize("dt", DT16)
def test_refusals_leave_the_buffer_untouched(device, dt):
    """Calls that cannot emit report R = 0 and never write the partials: rows that are no multiple of the tile
    (13x9 images), an fp32 output, and option gn_parts = 0."""
    x = _dev(_r(2, 13, 9, 64, seed=180), dt, device)
    w = _r(128, 64, 3, 3, seed=181, scale=1 / 24.0).to(dt).float()
    out, parts, q = O.conv2d_gn_parts(x, w, None)
    assert q["R"] == 0 and torch.isnan(parts).all()
    assert torch.equal(out, O.conv2d(x, w, None))
    x = _dev(_r(2, 16, 16, 64, seed=182), dt, device)
    out, parts, q = O.conv2d_gn_parts(x, w, None, out_f32=True)
    assert q["R"] == 0 and torch.isnan(parts).all() and out.dtype == torch.float32
    assert torch.equal(out, O.conv2d(x, w, None, out_f32=True))
    with L.option(gn_parts=0):
        out, parts, q = O.conv2d_gn_parts(x, w, None)
    assert q["R"] == 0 and torch.isnan(parts).all()
    torch.cuda.synchronize()
    assert torch.equal(out, O.conv2d(x, w, None))


# ------------------------------------------------------------------ consumers (partials made on the host)
def _consumer_inputs(C0, C1, HW, r0, r1, N, dt, device):
    x = R.hard_rows(N, HW, C0 + C1, seed=C0 + C1 + HW).to(dt)        # as stored
    x0, x1 = x[..., :C0].contiguous(), (x[..., C0:].contiguous() if C1 else None)
    g = torch.Generator().manual_seed(9)
    gamma = 1.0 + 0.2 * torch.randn(C0 + C1, generator=g)
    beta = 0.1 * torch.randn(C0 + C1, generator=g)
    p0 = R.block_sums(x0.reshape(-1, C0), r0)
    p1 = R.block_sums(x1.reshape(-1, C1), r1) if C1 else None
    return x, x0, x1, gamma, beta, p0, p1


def _consume(x0, x1, p0, p1, r0, r1, gamma, beta, silu, device):
    return O.group_norm_parts(x0.to(device), p0.to(device), r0, gamma.to(device), beta.to(device), EPS, G, silu,
                              x1=x1.to(device) if x1 is not None else None,
                              p1=p1.to(device) if p1 is not None else None, r1=r1)


CONSUMER_CASES = [
    # (C0, C1, HW, r0, r1, N, silu)
    (320, 0, 256, 256, 0, 3, True),
    (320, 160, 256, 256, 64, 2, False),    # groups of 15: group 21 straddles the seam, r1 != r0
    (1280, 640, 64, 64, 64, 2, True),      # groups of 60 across the 1280 | 640 seam
    (960, 0, 256, 128, 0, 2, False),
    (2560, 0, 64, 64, 0, 2, True),         # 8 groups of 80 channels > 256: the finalize kernel's strided branch
                                           # (gn_fa still takes it, one 80-channel group per block)
    (128, 0, 1024, 256, 0, 8, True),       # sliced gn_fa, XCD block map (N S % 8 == 0)
    (128, 0, 1024, 256, 0, 3, False),      # ... and without it when S is small
]


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("case", CONSUMER_CASES, ids=lambda c: "-".join(map(str, c[:6])))
def test_consumers(device, dt, case):
    C0, C1, HW, r0, r1, N, silu = case
    C = C0 + C1
    x, x0, x1, gamma, beta, p0, p1 = _consumer_inputs(C0, C1, HW, r0, r1, N, dt, device)
    mean, rstd, ref = R.gn_from_sums(x0, p0, G, gamma, beta, EPS, silu, x1, p1)
    sliced = HW > 256
    # the fused kernel (every configuration of its grid for the sliced cases) and finalize + apply: one result
    cfgs = [dict(gn_fa=1 << 30, gn_fa_wide=wd, gn_fa_blocks=bl) for wd in (1, 0) for bl in (2048, 64)] if sliced \
        else [dict(gn_fa=4096)]
    with L.option(gn_fa=0):
        two, kernels = _kernels(lambda: _consume(x0, x1, p0, p1, r0, r1, gamma, beta, silu, device))
    assert {k.split("<")[0] for k in kernels} == {"gn_finalize_parts_kernel", "gn_apply_kernel"}, kernels
    torch.cuda.synchronize()
    assert O.rel_err(two, ref) < TOL[dt]
    for cfg in cfgs:
        with L.option(**cfg):
            fused, kernels = _kernels(lambda: _consume(x0, x1, p0, p1, r0, r1, gamma, beta, silu, device))
        assert {k.split("<")[0] for k in kernels} == {"gn_fa_kernel"}, kernels
        torch.cuda.synchronize()
        assert torch.equal(fused, two), cfg
    # the finalize alone, on host-made partials of the whole concat (block size r0): (mean, rstd) against fp64 ...
    pc = R.block_sums(x.reshape(-1, C), r0)
    ab, mr = O.group_norm_parts_ab(pc.to(device), r0, C, N, HW, gamma.to(device), beta.to(device), EPS, G)
    ab, mr = ab.cpu(), mr.cpu()
    assert torch.isfinite(ab).all() and torch.isfinite(mr).all()
    amax = x.double().reshape(N, HW, G, C // G).abs().amax(dim=(1, 3))
    dmean = float(((mr[..., 0].double() - mean).abs() / amax).max())
    drstd = float(((mr[..., 1].double() - rstd).abs() / rstd).max())
    print(f"\n  |d mean| / max|x| {dmean:.2e} (bound 1e-5), rstd relative {drstd:.2e} (bound 5e-5)")
    assert dmean <= 1e-5 and drstd <= 5e-5
    # ... and the scale / shift pairs are exactly what (mean, rstd) give: a = rstd gamma, b = fma(-mean, a, beta)
    cg = C // G
    m32, r32 = mr[..., 0].repeat_interleave(cg, 1), mr[..., 1].repeat_interleave(cg, 1)
    sc = r32 * gamma
    assert torch.equal(ab[..., 0], sc)
    sh = beta.double() - m32.double() * sc.double()
    tol = 2.0 ** -23 * (beta.abs().double() + (m32.double() * sc.double()).abs())    # (one fp32 rounding of the fma)
    assert bool(((ab[..., 1].double() - sh).abs() <= tol).all())
    # the statistics pass over the same tensor: the same GroupNorm up to one 16-bit ulp of each element (of 1, for the
    # elements below it: the two fp32 results differ by ~1e-6 of the normalised magnitude, then round separately)
    sp = O.group_norm(x0.to(device).reshape(N, HW, 1, C0), gamma.to(device), beta.to(device), EPS, G, silu,
                      x1=x1.to(device).reshape(N, HW, 1, C1) if C1 else None).reshape(N, HW, C)
    torch.cuda.synchronize()
    d = (two.float() - sp.float()).abs() / sp.float().abs().clamp_min(1.0)
    assert float(d.max()) <= ULP[dt], float(d.max())


@pytest.mark.parametrize("dt", DT16)
def test_chain_conv_then_group_norm(device, halo_forced, dt):
    """Halo conv producer -> group_norm_parts (two sources: the same tensor twice, as an up-block concat) against the
    fp64 GroupNorm of the stored conv output."""
    run, _, _ = _conv_case(16, 16, 64, 64, 160, 3, True, dt, device, 190)
    y, parts, info = run([0, 1, 2])
    assert info["R"] == 256 and info["halo"] == 2
    g = torch.Generator().manual_seed(11)
    gamma, beta = 1.0 + 0.2 * torch.randn(320, generator=g), 0.1 * torch.randn(320, generator=g)
    y3 = y.reshape(NB, 256, 160)
    got = O.group_norm_parts(y3, parts, 256, gamma.to(device), beta.to(device), EPS, G, True, x1=y3, p1=parts, r1=256)
    torch.cuda.synchronize()
    yc = torch.cat([y3, y3], -1).double().cpu()
    ref = F.silu(F.group_norm(yc.permute(0, 2, 1), G, gamma.double(), beta.double(), EPS).permute(0, 2, 1))
    assert O.rel_err(got, ref) < TOL[dt]
