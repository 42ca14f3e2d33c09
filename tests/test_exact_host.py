"""The exact-answer constructions (tests/exactref.py) hold their own conditions on the fp64 reference alone, for every
case the GPU tests run — so a failure of tests/test_attention_exact_gpu.py or tests/test_gemm_exact_gpu.py can only be
the kernel.  No GPU, no native library."""
import math

import pytest
import torch

from tests import exactref as X

F32 = torch.float32

ONEHOT = ([(c, dt, False, "rows") for c in X.ATTN_D40 + [X.ATTN_D40_BIG] + X.ATTN_RES + X.ATTN_D80 + X.ATTN_D160
           + X.ATTN_D64 + X.ATTN_D512 + X.ATTN_GRID for dt in X.DT16]
          + [(X.ATTN_RES_AUTO, torch.bfloat16, False, "rows")]
          + [(c, dt, True, "rows") for c in X.ATTN_D64_CAUSAL for dt in X.DT16]
          + [(c, F32, False, "rows") for c in X.ATTN_F32] + [(c, F32, True, "rows") for c in X.ATTN_F32_CAUSAL]
          + [(c, torch.bfloat16, False, "rows") for c in X.ATTN_FALLBACK]
          + [((B, H, lq, lk, d), dt, False, lay) for B, H, lq, d in X.ATTN_PROD for lk, lay in ((lq, "hm"), (77, "rows"))
             for dt in X.DT16])


def _id(p):
    c, dt, causal, layout = p
    return "-".join(map(str, c)) + f"-{str(dt)[6:]}-{'causal' if causal else 'full'}-{layout}"


@pytest.mark.parametrize("floor", [False, True], ids=["plain", "floor"])
@pytest.mark.parametrize("p", ONEHOT, ids=_id)
def test_onehot_conditions(p, floor):
    (B, H, Lq, Lk, d), dt, causal, layout = p
    case = X.onehot_attention(B, H, Lq, Lk, d, dt, causal, 0, layout, floor)
    k, v, perm = case["k"].double(), case["v"].double(), case["perm"]
    # targets exist and, under the mask, are visible
    assert int(perm.min()) >= 0 and int(perm.max()) < Lk
    if causal:
        assert bool((perm <= torch.arange(Lq)).all())
    # no code collisions: no two keys of one (batch, head) point the same way
    for b in range(B):
        for h in range(H):
            sg = torch.sign(k[b, h])
            n_same = int(((sg @ sg.T) == d).sum()) - Lk
            # (a bait key equals its target's code doubled; causal baits live in k itself: one pair each)
            assert n_same == (2 * len(X.causal_baits(Lk)) if causal else 0), (b, h, n_same)
    # V: multiples of 16 in [-112, 112]; key rows of one (b, h) differ; row j differs between heads and batches
    assert bool((v % 16 == 0).all()) and float(v.abs().max()) <= 112
    flat = v.reshape(B * H, Lk, d)
    for i in range(B * H):
        assert len({tuple(r.tolist()) for r in flat[i]}) == Lk
    if B * H > 1:
        for j in range(0, Lk, max(1, Lk // 16)):
            assert len({tuple(r.tolist()) for r in flat[:, j]}) == B * H
    # the softmax sits on the target: off-target mass <= 1e-6, with q as given and with the pre-scaled q
    off = X.onehot_off_target(case)
    off_s = X.onehot_off_target(case, q_scaled=True) if dt != F32 else 0.0
    assert off <= 1e-6 and off_s <= 1e-6, (off, off_s)
    # the expected output is the fp64 softmax's output to well within the bar
    ref = X.softmax_attention64(case["q"], case["k"], case["v"], case["scale"], causal)
    assert float((ref - case["want"]).abs().max()) <= 224 * 1e-6
    # baits: B >= 2 (or H >= 2 head-major) places one behind the last key; the unmasked softmax would pick it
    if causal or B >= 2 or (layout == "hm" and H >= 2):
        assert case["victims"], "no bait in this case"
        assert X.onehot_bait_mass(case) >= 0.99
    # floor: every real score is negative, an all-zero key row would take the softmax (and its zero V row the output)
    if floor:
        assert X.FLOOR_Z[d] ** 2 > 2 * X.CODE_S[d] ** 2 * (d - 1)
        assert X.onehot_zero_key_mass(case) >= 0.99
        assert float(case["want"].abs().amax(-1).min()) >= 16          # no target row is the zero row itself
    # the output's own rounding cannot cross the bar: V entries are exact in dt and 16 apart
    assert X.onehot_bar(dt) < 8


SHAPES = sorted({(c, dt, causal) for c, dt, causal, _ in ONEHOT}, key=str)


@pytest.mark.parametrize("c,dt,causal", SHAPES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_uniform_conditions(c, dt, causal):
    B, H, Lq, Lk, d = c
    case = X.uniform_attention(B, H, Lq, Lk, d, dt, causal=causal)
    assert float(case["count"].max()) <= 32 and float(case["count"].sum()) == Lk
    ref = X.softmax_attention64(case["q"], case["k"], case["v"], case["scale"], causal)
    assert float((ref - case["want"]).abs().max()) <= 1e-12
    # one key more or less moves an element by about 1 / keys: at least twice the 2-ulp bar (count <= 32 against the 8
    # significant bits of bf16: 1 / Lk >= 128 / count ulps >= 4 ulps), so the bar separates count_c from count_c +- 1.
    # Exactly: dropping a counted key gives (n - 1) / (keys - 1), counting one more n / (keys - 1) or (n + 1) / (keys + 1)
    w, keys = case["want"][0, 0], case["keys"][:, None]
    n = w * keys
    bar = X.uniform_bar(w, dt)
    moves = [((n - 1) / (keys - 1).clamp_min(1) - w).abs()[(n >= 1) & (keys > 1)] / bar[(n >= 1) & (keys > 1)],
             ((n + 1) / (keys + 1) - w).abs()[w < 1] / bar[w < 1]]
    for m in moves:
        assert m.numel() == 0 or float(m.min()) >= 2.0, float(m.min())


RAMP = [(c, dt, causal, r) for c, dt, causal in SHAPES for r in X.ramps_for(c)]


@pytest.mark.parametrize("c,dt,causal,ramp", RAMP,
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_ramp_conditions(c, dt, causal, ramp):
    B, H, Lq, Lk, d = c
    case = X.ramp_attention(B, H, Lq, Lk, d, dt, ramp, causal=causal)
    s2 = (case["q"].double() @ case["k"].double().transpose(-1, -2)) * case["scale"] * X.LOG2E     # base-2 scores
    if Lk > 1:
        # per 64-key tile the score moves by 64 * rate (to the operands' rounding): past THR = 8 at 0.5, short of it at 0.1
        step = (s2[..., 64] - s2[..., 0]) if Lk > 64 else (s2[..., Lk - 1] - s2[..., 0]) * 64 / (Lk - 1)
        want = 64 * case["rates"]
        assert float((step - want).abs().max()) <= 0.02 * 64 * 0.5 + 1e-9, float((step - want).abs().max())
        assert bool(((want.abs() > 8) == (case["rates"].abs() == 0.5)).all())
    # every element of a q row has one magnitude (a folded, rounded scale is one common factor)
    qa = case["q"].double().abs()
    assert float((qa.amax(-1) - qa.amin(-1)).max()) == 0.0
    # outputs are O(1) (a weighted mean of unit Gaussians over the few keys next to the maximum): the relative bar bites
    assert float(case["want"].abs().max()) > 0.25


# ------------------------------------------------------------------ integer GEMM / conv
GEMMS = sorted(set(X.GEMM_4WAVE + X.GEMM_SMALL_SPLITK + X.GEMM_LARGE + X.GEMM_SK
                   + [X.GEMM_SPLITK, X.GEMM_PP, X.GEMM_ALPHA]))


@pytest.mark.parametrize("M,N,K", GEMMS)
def test_int_gemm_small(M, N, K):
    for alpha in ((1.0, 0.5) if (M, N, K) == X.GEMM_ALPHA else (1.0,)):
        c = X.int_gemm_operands(M, N, K, "small", torch.bfloat16, alpha=alpha)
        assert float(c["A"].abs().max()) <= 1 and float(c["B"].abs().max()) <= 1
        assert float(c["exact"].abs().max()) <= 128
        for dt in X.DT16:        # every output representable: equality sees a single lost or doubled product
            assert X.int_shares(c["exact"], dt) == (0.0, 0.0)
        assert torch.equal(c["exact"], alpha * (c["A"].double() @ c["B"].double().T) + c["bias"].double()
                           + c["residual"].double())


@pytest.mark.parametrize("dt", X.DT16, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("M,N,K", GEMMS)
def test_int_gemm_wide(M, N, K, dt):
    c = X.int_gemm_operands(M, N, K, "wide", dt)
    for t in (c["A"], c["B"], c["residual"]):
        assert torch.equal(t.to(dt).float(), t)              # operands exact in the storage type
    assert float(c["exact"].abs().max()) < (2 ** 24 if dt == torch.bfloat16 else 60000)
    off, tie = X.int_shares(c["exact"], dt)
    assert off >= 0.05 and tie >= 0.01, (off, tie)
    # the two-pass epilogue's value (expected_staged) is within one ulp (of the larger of the staged value and the
    # result) of the once-rounded one, and not the same thing
    once, twice = X.expected(c["exact"], dt).double(), X.expected_staged(c, dt).double()
    bound = torch.maximum(X.ulp(c["exact"], dt), X.ulp(c["stage"], dt))
    assert bool(((once - twice).abs() <= bound).all()) and not torch.equal(once, twice)
    small = X.int_gemm_operands(M, N, K, "small", dt)
    assert torch.equal(X.expected(small["exact"], dt), X.expected_staged(small, dt))


def test_int_gemm_batched():
    b, M, N, K = X.GEMM_BATCHED
    c = X.int_gemm_operands(M, N, K, "small", torch.bfloat16, batch=b)
    assert c["exact"].shape == (b, M, N) and float(c["exact"].abs().max()) <= 128
    for dt in X.DT16:
        off, tie = X.int_shares(X.int_gemm_operands(M, N, K, "wide", dt, batch=b)["exact"], dt)
        assert off >= 0.05 and tie >= 0.01, (off, tie)


CONVS = dict(X.CONV_IM2COL, **X.CONV_HALO, halo_split=X.CONV_HALO_SPLIT, strip=X.CONV_STRIP, mi=X.CONV_MI,
             dense_1x1=X.CONV_1X1_DENSE)


@pytest.mark.parametrize("name", list(CONVS))
def test_int_conv(name):
    small = X.int_conv_operands(*CONVS[name], "small", torch.bfloat16)
    assert float(small["exact"].abs().max()) <= 128
    for dt in X.DT16:
        assert X.int_shares(small["exact"], dt) == (0.0, 0.0)
        wide = X.int_conv_operands(*CONVS[name], "wide", dt)
        assert float(wide["exact"].abs().max()) < (2 ** 24 if dt == torch.bfloat16 else 60000)
        off, tie = X.int_shares(wide["exact"], dt)
        assert off >= 0.05 and tie >= 0.01, (name, dt, off, tie)


def test_expected_rounds_once_to_nearest_even():
    e = torch.tensor([257.0, 259.0, 258.0, -257.0, 2049.0, 2051.0, 1000.5])
    assert X.expected(e.double(), torch.bfloat16).tolist() == [256.0, 260.0, 258.0, -256.0, 2048.0, 2048.0, 1000.0]
    assert X.expected(e.double(), torch.float16).tolist() == [257.0, 259.0, 258.0, -257.0, 2048.0, 2052.0, 1000.5]
    assert X.int_shares(e.double(), torch.bfloat16) == (6 / 7, 3 / 7)
    assert math.isclose(float(X.ulp(torch.tensor(0.3, dtype=torch.float64), torch.bfloat16)), 2.0 ** -9)
