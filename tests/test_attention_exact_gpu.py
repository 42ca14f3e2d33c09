"""Attention kernels against constructions with a known exact answer (tests/exactref.py; their conditions are proved on
the CPU by tests/test_exact_host.py).  Random q / k make the softmax nearly flat, so one wrong key moves an output by
|v| / Lk — below any relative bar — and the bit-exact A/B tests compare kernels that share their index and mask
arithmetic.  Here every path gets

  one-hot   each query's output must BE the V row of its target key (|got - want| <= 1.0 of entries 16 apart), with
            doubled bait keys in the row that follows a (batch, head)'s last key in memory and (causal) behind the query,
            and once more with every score lowered below zero, so that a zero-filled key row past Lk would win;
  uniform   q = 0, V counts the keys: O[c] = count_c / Lk to 2 ulps, where one key more or less is >= 4;
  ramp      scores that climb or fall along the keys (the running maximum moved on every tile, deferred, or for half
            a wave), against the fp64 softmax of the rounded operands at the project's 2 * TOL of max |ref|.

Which kernel a case ran is asserted from the in-process profile wherever an option or a shape decides it.
"""
import pytest
import torch

from image_restoration_and_enhancement_amd import _lib as L
from tests import exactref as X
from tests import opref as O
from tests.guard import same

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
TOL = {F32: 1e-4, BF16: 2 * 2e-2, F16: 2 * 5e-3}           # tests/test_ops_gpu.py: test_attention's bars
TN = {BF16: "unsigned short", F16: "_Float16", F32: "float"}
DT16 = list(X.DT16)
ids_dt = lambda d: str(d)[6:]                              # noqa: E731


def _ran(fn):
    """fn() and the names of the kernels it launched (the in-process profile), namespaces dropped."""
    L.profile_begin()
    try:
        out = fn()
    finally:
        names = {p[0].split("::")[-1] for p in L.profile_end()}
    return out, names


def attn3(dt, d, causal=False, res=False, pf=0):
    return f"attn3_kernel<{TN[dt]}, {d}, 64, {'true' if causal else 'false'}, {'true' if res else 'false'}, {pf}>"


# ------------------------------------------------------------------ how a [B][H][L][d] case reaches the kernel
def rows(device, ld_pad=0):
    """Row-major [B][L][H d] operands, each contiguous, through irx_op_attention."""
    def run(q, k, v, scale, causal):
        B, H, Lq, d = q.shape
        r = [t.permute(0, 2, 1, 3).reshape(B, t.shape[2], H * d).contiguous().to(device) for t in (q, k, v)]
        o = O.attention(r[0], r[1], r[2], H, causal, ld_pad=ld_pad)
        return o.unflatten(-1, (H, d)).permute(0, 2, 1, 3)
    return run


def fused(device):
    """q | k | v as column blocks of one [B][L][3 H d] buffer (the VAE's fused projection)."""
    def run(q, k, v, scale, causal):
        B, H, Lq, d = q.shape
        C = H * d
        buf = torch.cat([t.permute(0, 2, 1, 3).reshape(B, Lq, C) for t in (q, k, v)], -1).contiguous().to(device)
        o = O.attention(buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:], H, causal)
        return o.unflatten(-1, (H, d)).permute(0, 2, 1, 3)
    return run


def q_offset(device, off=4):
    """Row-major operands with Q placed `off` elements (8 bytes) off a 16-byte boundary."""
    def run(q, k, v, scale, causal):
        B, H, Lq, d = q.shape
        r = [t.permute(0, 2, 1, 3).contiguous().to(device) for t in (q, k, v)]        # [B][L][H][d]
        return O.attention_ex(*(t.permute(0, 2, 1, 3) for t in r), scale, causal, q_off=off)
    return run


def prod_self(device, q_scaled):
    """models.cpp's self-attention: q, k, v and o head-major [B][H][L][d]."""
    def run(q, k, v, scale, causal):
        qq = X.prescale(q, scale, q.dtype) if q_scaled else q
        return O.attention_ex(qq.contiguous().to(device), k.contiguous().to(device), v.contiguous().to(device), scale,
                              causal, q_scaled=q_scaled, o_hm=True)
    return run


def prod_cross(device, q_scaled, extra=24):
    """models.cpp's cross-attention: q head-major, K | V column slices of the packed per-prompt [B Lk][2 C + extra]
    buffer at a column offset, o row-major."""
    def run(q, k, v, scale, causal):
        B, H, Lk, d = k.shape
        C = H * d
        qq = X.prescale(q, scale, q.dtype) if q_scaled else q
        buf = torch.full((B * Lk, 2 * C + extra), 7.0, dtype=q.dtype)
        off = 8                                                      # (a 16-byte aligned column offset)
        buf[:, off:off + C] = k.permute(0, 2, 1, 3).reshape(B * Lk, C)
        buf[:, off + C:off + 2 * C] = v.permute(0, 2, 1, 3).reshape(B * Lk, C)
        buf = buf.to(device)
        kv = [buf[:, o:o + C].unflatten(0, (B, Lk)).unflatten(-1, (H, d)).permute(0, 2, 1, 3) for o in (off, off + C)]
        return O.attention_ex(qq.contiguous().to(device), kv[0], kv[1], scale, causal, q_scaled=q_scaled, ld_pad=8)
    return run


# ------------------------------------------------------------------ the three constructions on one path
def check(run, shape, dt, causal=False, layout="rows", q_scaled=False, kernel=None, seed=0):
    """One-hot (+ baits), uniform and ramp through `run`; `kernel`: the one kernel name every launch must carry."""
    B, H, Lq, Lk, d = shape
    seen = set()

    def go(case):
        out, names = _ran(lambda: run(case["q"], case["k"], case["v"], case["scale"], causal))
        seen.update(names)
        return out

    for floor in (False, True):          # (floor: all scores negative, so a zero-filled key row let in would win)
        case = X.onehot_attention(B, H, Lq, Lk, d, dt, causal, seed, layout, floor)
        msg = X.onehot_explain(go(case), case)
        assert not msg, f"one-hot{' (floor)' if floor else ''}: " + msg

    case = X.uniform_attention(B, H, Lq, Lk, d, dt, causal=causal)
    uni = go(case)
    err = (uni.double().cpu() - case["want"]).abs()
    bad = (err > X.uniform_bar(case["want"], dt)).nonzero()
    assert not len(bad), (f"uniform: {len(bad)} elements off by more than 2 ulps, first (b, h, q, c) = "
                          f"{tuple(int(i) for i in bad[0])}: got {float(uni[tuple(bad[0])])}, want "
                          f"{float(case['want'][tuple(bad[0])])} = count / keys")

    for ramp in X.ramps_for(shape):
        case = X.ramp_attention(B, H, Lq, Lk, d, dt, ramp, causal=causal)
        if q_scaled:             # (the reference of a pre-scaled call is the softmax of the pre-scaled, rounded q)
            qs = X.prescale(case["q"], case["scale"], dt)
            case = dict(case, want=X.softmax_attention64(qs, case["k"], case["v"], case["scale"], causal, q_scaled=True))
        rel = float((go(case).double().cpu() - case["want"]).abs().max() / case["want"].abs().max())
        print(f"\n  ramp {ramp}: max |got - ref| / max |ref| {rel:.2e} (bar {TOL[dt]:.0e})")
        assert rel < TOL[dt], (ramp, rel)
    if kernel is not None:
        assert seen == {kernel}, (seen, kernel)
    return uni


# ------------------------------------------------------------------ d = 40 streamed: attn3q, attn3 PF 3, attn3
D40_OPTS = {"q2": (dict(attn_q2=1), lambda dt: f"attn3q_kernel<{TN[dt]}, 40, 64>"),
            "pf": (dict(attn_q2=0, attn_pf=1), lambda dt: attn3(dt, 40, pf=3)),
            "plain": (dict(attn_q2=0, attn_pf=0), lambda dt: attn3(dt, 40))}


@pytest.mark.parametrize("kind", list(D40_OPTS))
@pytest.mark.parametrize("dt", DT16, ids=ids_dt)
@pytest.mark.parametrize("shape", X.ATTN_D40 + [X.ATTN_D40_BIG], ids=lambda s: "x".join(map(str, s)))
def test_d40_streamed(device, shape, dt, kind):
    """(attn_qrep = 0 keeps Lk <= 128 off the resident-K/V kernel: the streamed kernels at Lk = 1, 64 and 65.)"""
    opts, name = D40_OPTS[kind]
    with L.option(attn_qrep=0, **opts):
        check(rows(device), shape, dt, kernel=name(dt))


# ------------------------------------------------------------------ resident K/V
@pytest.mark.parametrize("qrep", [1, 0, 4])
@pytest.mark.parametrize("dt", DT16, ids=ids_dt)
@pytest.mark.parametrize("shape", X.ATTN_RES, ids=lambda s: "x".join(map(str, s)))
def test_resident_kv(device, shape, dt, qrep):
    """Lk <= 128 against K/V resident in LDS (qrep 1: automatic, one group here; 4: forced, so the one block of 4 x 128
    queries per (batch, head) has two groups past Lq = 200) and, with attn_qrep = 0, the streamed kernels."""
    B, H, Lq, Lk, d = shape
    pf = {160: 1}.get(d, 0)
    with L.option(attn_qrep=qrep):
        if qrep:
            name = attn3(dt, d, res=True, pf=pf)
        else:
            name = {40: f"attn3q_kernel<{TN[dt]}, 40, 64>", 80: attn3(dt, 80, pf=2), 160: attn3(dt, 160, pf=1)}[d]
        if qrep == 4:
            assert -(-Lq // (128 * 4)) * 4 * 128 - Lq >= 2 * 128       # whole query groups past Lq
        check(rows(device), shape, dt, kernel=name)


def test_resident_kv_auto_qrep(device):
    """A grid large enough that the launcher itself picks two query groups per block (launch3_cfg: doubled while
    ceil(Lq / (256 qrep)) H B >= 1024 at d = 40)."""
    B, H, Lq, Lk, d = X.ATTN_RES_AUTO
    qrep = 1
    while qrep < 8 and -(-Lq // (256 * qrep)) * H * B >= 1024:
        qrep *= 2
    assert qrep == 2
    check(rows(device), X.ATTN_RES_AUTO, BF16, kernel=attn3(BF16, 40, res=True))


# ------------------------------------------------------------------ d = 80 / 160 streamed, prefetch on and off
@pytest.mark.parametrize("pf", [2, 0])
@pytest.mark.parametrize("dt", DT16, ids=ids_dt)
@pytest.mark.parametrize("shape", X.ATTN_D80, ids=lambda s: "x".join(map(str, s)))
def test_d80_streamed(device, shape, dt, pf):
    with L.option(attn_pf80=pf):
        check(rows(device), shape, dt, kernel=attn3(dt, 80, pf=pf))


@pytest.mark.parametrize("pf", [1, 0])
@pytest.mark.parametrize("dt", DT16, ids=ids_dt)
@pytest.mark.parametrize("shape", X.ATTN_D160, ids=lambda s: "x".join(map(str, s)))
def test_d160_streamed(device, shape, dt, pf):
    with L.option(attn_pf160=pf):
        check(rows(device), shape, dt, kernel=attn3(dt, 160, pf=pf))


# ------------------------------------------------------------------ d = 64: causal (CLIP) and not
@pytest.mark.parametrize("dt", DT16, ids=ids_dt)
@pytest.mark.parametrize("shape", X.ATTN_D64_CAUSAL, ids=lambda s: "x".join(map(str, s)))
def test_d64_causal(device, shape, dt):
    """L = 77: one query block.  L = 300: three query blocks, key tiles skipped behind a block, the diagonal tile;
    keys behind the query carry doubled codes (exactref.causal_baits)."""
    check(rows(device), shape, dt, causal=True, kernel=attn3(dt, 64, causal=True))


@pytest.mark.parametrize("dt", DT16, ids=ids_dt)
@pytest.mark.parametrize("shape", X.ATTN_D64, ids=lambda s: "x".join(map(str, s)))
def test_d64_full(device, shape, dt):
    check(rows(device), shape, dt, kernel=attn3(dt, 64, res=shape[3] <= 128))


# ------------------------------------------------------------------ d = 512 (attnw), fused q | k | v rows
@pytest.mark.parametrize("dt", DT16, ids=ids_dt)
@pytest.mark.parametrize("shape", X.ATTN_D512, ids=lambda s: "x".join(map(str, s)))
def test_d512_wide(device, shape, dt):
    check(fused(device), shape, dt, kernel=f"attnw_kernel<{TN[dt]}, 512, 1>")


# ------------------------------------------------------------------ fp32 (attn_kernel<float>)
@pytest.mark.parametrize("shape", X.ATTN_F32, ids=lambda s: "x".join(map(str, s)))
def test_f32(device, shape):
    d = shape[4]
    check(rows(device), shape, F32, kernel=f"attn_kernel<float, {(d + 15) // 16 * 16}>")


@pytest.mark.parametrize("shape", X.ATTN_F32_CAUSAL, ids=lambda s: "x".join(map(str, s)))
def test_f32_causal(device, shape):
    check(rows(device), shape, F32, causal=True, kernel="attn_kernel<float, 64>")


# ------------------------------------------------------------------ the bf16 fallback attn_kernel<bf16_t>
def test_bf16_fallback_head_dim(device):
    """A head dim launch3 does not take (48)."""
    check(rows(device), X.ATTN_FALLBACK[0], BF16, kernel="attn_kernel<unsigned short, 48>")


def test_bf16_fallback_unaligned_q(device):
    """d = 40 with Q 8 bytes off a 16-byte boundary: attn3's 16-byte Q loads are not legal, the round-1 kernel runs."""
    check(q_offset(device), X.ATTN_FALLBACK[1], BF16, kernel="attn_kernel<unsigned short, 48>")


# ------------------------------------------------------------------ grids that are no multiple of 8 (xcd_remap's remainder)
@pytest.mark.parametrize("dt", DT16, ids=ids_dt)
@pytest.mark.parametrize("shape", X.ATTN_GRID, ids=lambda s: "x".join(map(str, s)))
def test_ragged_grid(device, shape, dt):
    B, H, Lq, Lk, d = shape
    with L.option(attn_q2=0):
        assert (-(-Lq // 128) * H * B) % 8 != 0
        check(rows(device, ld_pad=8), shape, dt, kernel=attn3(dt, 40, pf=3))
    assert (-(-Lq // 256) * H * B) % 8 != 0
    check(rows(device), shape, dt, kernel=f"attn3q_kernel<{TN[dt]}, 40, 64>")


# ------------------------------------------------------------------ the forms models.cpp launches
@pytest.mark.parametrize("q_scaled", [1, 0])
@pytest.mark.parametrize("dt", DT16, ids=ids_dt)
@pytest.mark.parametrize("case", X.ATTN_PROD, ids=lambda s: "x".join(map(str, s)))
def test_production_self(device, case, dt, q_scaled):
    """Self-attention fully head-major; q_scaled = 1 as every 16-bit model call sets it.  Head-major baits: key Lk of
    head h is key 0 of head h + 1."""
    B, H, Lq, d = case
    shape = (B, H, Lq, Lq, d)
    uni = check(prod_self(device, q_scaled), shape, dt, layout="hm", q_scaled=q_scaled)
    if q_scaled:      # q = 0 pre-scales exactly: the two forms must agree bit for bit
        c = X.uniform_attention(*shape, dt)
        assert same(uni, prod_self(device, 0)(c["q"], c["k"], c["v"], c["scale"], False))


@pytest.mark.parametrize("q_scaled", [1, 0])
@pytest.mark.parametrize("dt", DT16, ids=ids_dt)
@pytest.mark.parametrize("case", X.ATTN_PROD, ids=lambda s: "x".join(map(str, s)))
def test_production_cross(device, case, dt, q_scaled):
    """Cross-attention: Q head-major, K / V column slices (at a column offset) of the packed [B 77][2 C + extra]
    buffer whose other columns are NaN in the guarded copy, O row-major with pad columns."""
    B, H, Lq, d = case
    shape = (B, H, Lq, 77, d)
    uni = check(prod_cross(device, q_scaled), shape, dt, q_scaled=q_scaled,
                kernel=attn3(dt, d, res=True, pf={160: 1}.get(d, 0)))
    if q_scaled:
        c = X.uniform_attention(*shape, dt)
        assert same(uni.contiguous(), prod_cross(device, 0)(c["q"], c["k"], c["v"], c["scale"], False).contiguous())
