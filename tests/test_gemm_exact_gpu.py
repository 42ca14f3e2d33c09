"""GEMM and convolution paths on integer operands (tests/exactref.py; conditions proved by tests/test_exact_host.py).

Every product and every partial sum is an integer below 2^24, exact in fp32 in any order, so the output of a right
kernel is the exact integer result rounded once, to nearest even, to the output type — and the assertion is equality:

  "small"  sparse {-1, 0, 1} operands, every exact output within +-128 and so representable in bf16 and fp16: one lost
           or doubled k element, or a split-K partial added twice or not at all, changes an element;
  "wide"   dense operands sized so that, in the tested type, >= 5 % of the exact outputs are not representable and >= 1 %
           are exact ties: a truncating conversion, or an epilogue that rounds before it adds the residual, changes one.

One documented exception to "rounded once": the 16-bit large-tile and gemm_sk epilogues stage alpha acc + bias in the
storage type before a second pass adds row-add and residual (the staged tile fills the LDS), so they round twice.  Both
roundings are of exact values, so the expectation for those kernels is still exact (exactref.expected_staged) and the
assertion still equality; which of the two applies is read off the kernels that ran (staged()).

Bias, residual and (convs) row-add are always present.  Which kernel ran is asserted from the in-process profile (the
kernel's name carries its tile, K depth, stages, halo kind and loop), and split-K from the workspace / plan queries.
Out of scope: activation, GEGLU and norm-folded epilogues (their results are not integers).
"""
import ctypes as C

import pytest
import torch

from image_restoration_and_enhancement_amd import _lib as L
from tests import exactref as X
from tests import opref as O

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# (regime, storage type, fp32 output)
COMBOS16 = [("small", BF16, False), ("small", F16, False), ("wide", BF16, False), ("wide", F16, False)]
COMBOS = COMBOS16 + [("small", F32, False), ("small", BF16, True)]
cid = lambda c: f"{c[0]}-{str(c[1])[6:]}{'-f32out' if c[2] else ''}"          # noqa: E731


def _ran(fn):
    """fn() and the names of the kernels it launched (the in-process profile), namespaces dropped."""
    L.profile_begin()
    try:
        out = fn()
    finally:
        names = {p[0].split("::")[-1] for p in L.profile_end()}
    return out, names


def g2(names):
    """The gemm2_kernel instantiations among `names`, template arguments by name."""
    out = []
    for n in names:
        if n.startswith("gemm2_kernel<"):
            a = n[len("gemm2_kernel<"):n.rindex(">")].split(", ")
            out.append(dict(BM=int(a[1]), BN=int(a[2]), WM=int(a[3]), WN=int(a[4]), BK=int(a[5]), S=int(a[6]),
                            conv=a[7] == "true", HALO=int(a[10]), PP=a[11] == "true"))
    return out


def kinds(names):
    return {n.split("<")[0] for n in names}


def staged(names, out_f32):
    """Whether the launch's epilogue rounds twice (exactref.expected_staged): a 16-bit gemm_sk or gemm2 (large-tile /
    halo) kernel finished the tile itself.  The 4-wave kernel, fp32 outputs and the split-K reduce kernels form the
    whole sum in fp32 and round once."""
    k = kinds(names)
    if out_f32 or k & {"splitk_reduce_kernel", "splitk_reduce_gn_kernel"}:
        return False
    return bool(k & {"gemm_sk_kernel", "gemm2_kernel"})


def run_gemm(device, shape, combo, alpha=1.0, batch=1, expect=None):
    regime, dt, out_f32 = combo
    M, N, K = shape
    c = X.int_gemm_operands(M, N, K, regime, dt, alpha=alpha, batch=batch)
    A, Bw, R = (c[k].to(dt).to(device) for k in ("A", "B", "residual"))
    bias = c["bias"].to(device)
    got, names = _ran(lambda: O.gemm(A, Bw, bias=bias, alpha=alpha, residual=R, out_f32=out_f32, batch=batch))
    msg = X.int_explain(got, c, F32 if out_f32 else dt, staged(names, out_f32))
    assert not msg, f"{shape} {cid(combo)} {sorted(names)}: {msg}"
    if expect is not None and dt != F32 and not out_f32:      # (the named paths are the 16-bit ones)
        expect(names)
    return names


def run_conv(device, geom, combo, expect=None):
    regime, dt, out_f32 = combo
    N, H, W, C0, C1, Co, k, stride, pad, up_hw, asym = geom
    c = X.int_conv_operands(*geom, regime, dt)
    x0 = c["x0"].to(dt).to(device)
    x1 = c["x1"].to(dt).to(device) if C1 else None
    got, names = _ran(lambda: O.conv2d(x0, c["w"], c["bias"], stride=stride, pad=(pad, pad),
                                       out_hw=c["out_hw"] if asym else None, x1=x1, up_hw=up_hw,
                                       rowadd=c["rowadd"].to(device), residual=c["residual"].to(dt).to(device),
                                       out_f32=out_f32))
    msg = X.int_explain(got, c, F32 if out_f32 else dt, staged(names, out_f32))
    assert not msg, f"{geom} {cid(combo)} {sorted(names)}: {msg}"
    if expect is not None and dt != F32 and not out_f32:      # (the named paths are the 16-bit ones)
        expect(names)
    return names


def ws_bytes(dt, M, N, K, out_f32=False):
    return L.load().irx_op_gemm_workspace_bytes(O.DT[dt], M, N, K, 0, int(out_f32), 0)


def conv_plan(dt, geom):
    N, H, W, C0, C1, Co, k, stride, pad, up_hw, asym = geom
    t = (C.c_int * 7)()
    L.call("irx_debug_conv_plan", O.DT[dt], C0, C1, N, H, W, H, W, Co, k, k, stride, pad, pad, H, W, 0, t)
    return dict(zip(("path", "BM", "BN", "group_m", "splits", "tiles_m", "tiles_n"), t))


# ------------------------------------------------------------------ dense: the 4-wave kernel
def _wave4(names):
    assert kinds(names) == {"gemm_kernel"}, names


@pytest.mark.parametrize("combo", COMBOS, ids=cid)
def test_wave4_tiny(device, combo):
    run_gemm(device, X.GEMM_4WAVE[0], combo, expect=_wave4)


@pytest.mark.parametrize("combo", COMBOS, ids=cid)
def test_wave4_large_tiles_off(device, combo):
    with L.option(large_tiles=0):
        run_gemm(device, X.GEMM_4WAVE[1], combo, expect=_wave4)


@pytest.mark.parametrize("combo", COMBOS, ids=cid)
@pytest.mark.parametrize("shape", X.GEMM_SMALL_SPLITK, ids=lambda s: "x".join(map(str, s)))
def test_small_m_split_k(device, shape, combo):
    def expect(names):
        assert ws_bytes(combo[1], *shape, combo[2]) > 0
        assert kinds(names) == {"gemm_kernel", "splitk_reduce_kernel"}, names
    run_gemm(device, shape, combo, expect=expect)


# ------------------------------------------------------------------ dense: each large-tile family (tests/test_ops_gpu.py `tiles`)
FAMILIES = {   # options -> what large_kernel() builds for a 128-row tile: (K depth, stages) or the 4-wave form
    "two_stage": (dict(large_tiles=1, gemm_deep=0, gemm_small=0), lambda k: (k["BK"], k["S"]) == (64, 2)),
    "ring32": (dict(large_tiles=1, gemm_deep=1, gemm_small=0), lambda k: k["BK"] == 32 and k["S"] >= 4),
    "ring64": (dict(large_tiles=1, gemm_deep=2, gemm_small=0), lambda k: k["BK"] == 64 and k["S"] >= 3),
    "small4w": (dict(large_tiles=1, gemm_deep=0, gemm_small=1), lambda k: k["WM"] * k["WN"] == 4),
}


@pytest.mark.parametrize("combo", COMBOS, ids=cid)
@pytest.mark.parametrize("shape", X.GEMM_LARGE, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_large_tile_families(device, fam, shape, combo):
    """Ragged M (1000, 1025 = one valid row in the last tile) at the smallest shapes that plan onto each family."""
    opts, ok = FAMILIES[fam]

    def expect(names):
        ks = g2(names)
        assert kinds(names) == {"gemm2_kernel"} and len(ks) == 1 and not ks[0]["conv"], names
        assert shape[0] % ks[0]["BM"] != 0 and ok(ks[0]), (fam, ks)
    with L.option(**opts):
        run_gemm(device, shape, combo, expect=expect)


@pytest.mark.parametrize("combo", COMBOS16 + [("small", BF16, True)], ids=cid)
@pytest.mark.parametrize("inkernel", [1, 0])
def test_split_k(device, inkernel, combo):
    """Large-tile K splits reduced by the last arriving block (tickets: run twice) and by the reduce kernel."""
    shape = X.GEMM_SPLITK

    def expect(names):
        assert ws_bytes(combo[1], *shape, combo[2]) > 0
        assert ("splitk_reduce_kernel" in kinds(names)) == (not inkernel), names
        assert "gemm2_kernel" in kinds(names)
    with L.option(splitk_inkernel=inkernel):
        for _ in range(2):
            run_gemm(device, shape, combo, expect=expect)


@pytest.mark.parametrize("combo", COMBOS16, ids=cid)
@pytest.mark.parametrize("shape", X.GEMM_SK, ids=lambda s: "x".join(map(str, s)))
def test_gemm_sk(device, shape, combo):
    """The K = 320 streaming kernel (option gemm_sk = 3: every such shape)."""
    def expect(names):
        assert kinds(names) == {"gemm_sk_kernel"}, names
    with L.option(gemm_sk=3):
        run_gemm(device, shape, combo, expect=expect)


@pytest.mark.parametrize("combo", COMBOS16 + [("small", BF16, True)], ids=cid)
@pytest.mark.parametrize("pp", [2, 0])
def test_ping_pong(device, pp, combo):
    """Whole 256 x 256 tiles on the lean ping-pong loop (gemm_pp 2) and on the two-stage loop (0); op_imgs = 1 counts
    the rows as one image of the canonical 16, which is what puts 1024 rows on that tile."""
    def expect(names):
        ks = g2(names)
        assert len(ks) == 1 and (ks[0]["BM"], ks[0]["BN"]) == (256, 256) and ks[0]["PP"] == bool(pp), (pp, names)
    with L.option(gemm_pp=pp, op_imgs=1):
        run_gemm(device, X.GEMM_PP, combo, expect=expect)


@pytest.mark.parametrize("combo", COMBOS, ids=cid)
def test_batched(device, combo):
    b, M, N, K = X.GEMM_BATCHED
    run_gemm(device, (M, N, K), combo, batch=b)


@pytest.mark.parametrize("combo", COMBOS, ids=cid)
def test_alpha_half(device, combo):
    """alpha = 0.5 is exact: half-integers of the same range."""
    run_gemm(device, X.GEMM_ALPHA, combo, alpha=0.5)


@pytest.mark.parametrize("combo", COMBOS16, ids=cid)
def test_conv1x1_two_source_as_dense(device, combo):
    """The 1x1 conv over a channel concat rewritten as a dense GEMM with a second A source (ragged M = 189)."""
    def expect(names):
        ks = g2(names)
        assert ks and not any(k["conv"] for k in ks), names
    run_conv(device, X.CONV_1X1_DENSE, combo, expect=expect)


# ------------------------------------------------------------------ convolutions
@pytest.mark.parametrize("combo", COMBOS, ids=cid)
@pytest.mark.parametrize("name", list(X.CONV_IM2COL))
def test_conv_im2col(device, name, combo):
    """The im2col walk: ragged sizes, stride 2 on odd sizes, the VAE's asymmetric pad, the fused nearest upsample."""
    run_conv(device, X.CONV_IM2COL[name], combo)


def _halo(*want):
    def expect(names):
        ks = g2(names)
        assert len(ks) == 1 and ks[0]["HALO"] in want, (want, names)
    return expect


@pytest.mark.parametrize("combo", COMBOS16, ids=cid)
@pytest.mark.parametrize("pipe", [1, 0])
@pytest.mark.parametrize("name", list(X.CONV_HALO))
def test_conv_halo_rows(device, name, pipe, combo):
    """Whole-row halo tiles (conv_halo = 2 forces them on these small grids): the pipelined loop and the lock-step one."""
    with L.option(conv_halo=2, halo_pipe=pipe):
        run_conv(device, X.CONV_HALO[name], combo, expect=_halo(2 if pipe else 1))


@pytest.mark.parametrize("combo", COMBOS16, ids=cid)
@pytest.mark.parametrize("pipe", [1, 0])
def test_conv_halo_k_split(device, pipe, combo):
    """The 16x16 level: halo tiles in two K splits, reduced in the kernel."""
    with L.option(halo_pipe=pipe):
        assert conv_plan(combo[1], X.CONV_HALO_SPLIT)["splits"] == 2
        run_conv(device, X.CONV_HALO_SPLIT, combo, expect=_halo(2 if pipe else 1))


@pytest.mark.parametrize("combo", COMBOS16, ids=cid)
def test_conv_halo_strips(device, combo):
    with L.option(conv_halo=2):
        run_conv(device, X.CONV_STRIP, combo, expect=_halo(5))


@pytest.mark.parametrize("combo", COMBOS16, ids=cid)
def test_conv_halo_four_images(device, combo):
    """8x8 images four to a tile, N = 5 (a last tile with one image), K splits through the reduce kernel."""
    def expect(names):
        _halo(8)(names)
        assert kinds(names) == {"gemm2_kernel", "splitk_reduce_kernel"}, names
    assert conv_plan(combo[1], X.CONV_MI)["splits"] > 1
    run_conv(device, X.CONV_MI, combo, expect=expect)


@pytest.mark.parametrize("combo", [("small", F32, False), ("small", BF16, True)], ids=cid)
def test_conv_halo_shape_other_types(device, combo):
    """One halo-shaped conv with fp32 storage and with fp32 output (whichever kernel the planner gives those)."""
    with L.option(conv_halo=2):
        run_conv(device, X.CONV_HALO["rows_w16_concat"], combo)
