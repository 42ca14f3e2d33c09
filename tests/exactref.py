"""Exact-answer constructions for the attention and GEMM / conv kernels: operands for which the right result is known
exactly and does not depend on summation order, so one wrong index is an O(1) error at a named element.

  onehot_attention   every query's softmax sits on ONE key (its target), so the output row is that key's V row: pins, per
                     (batch, head, query), which key row the kernel used.  Baits (doubled copies of a target's code) sit
                     where a wrong mask would let them in: in the row that follows a (batch, head)'s last key in memory,
                     and (causal) at keys behind the query.  The reference ignores them by definition.
  uniform_attention  q = 0, V an indicator of key % d: the output counts the keys, O[c] = count_c / Lk.
  ramp_attention     rank-one scores that rise or fall steadily along the keys: drives the online softmax's running
                     maximum (moved on every tile, deferred, never, or for half a wave only).
  int_gemm_operands / int_conv_operands
                     integer operands, bias, residual and row-add: every product and partial sum is an integer below
                     2^24, exact in fp32 in any order, so the output is the exact integer rounded ONCE to the output
                     type ("small": every output representable, equality sees one lost product; "wide": outputs that
                     need rounding, equality sees a truncation or a double rounding) — or, for the epilogues that
                     stage a 16-bit tile before they add the residual, the equally exact expected_staged().

Everything here is CPU-only and deterministic in its seed; tests/test_exact_host.py proves each construction's
conditions on the fp64 reference alone, over the very case lists the GPU tests run (ATTN_* / GEMM_* / CONV_* below).
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634
CODE_S = {40: 4.0, 48: 4.0, 64: 4.0, 80: 2.0, 160: 2.0, 512: 1.0}     # |code element| per head dim (powers of two)
FLOOR_Z = {40: 64.0, 48: 64.0, 64: 64.0, 80: 32.0, 160: 64.0, 512: 64.0}    # powers of two, z^2 well past 2 s^2 (d - 1)
MANT = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}      # significant bits


def ulp(x, dt):
    """Spacing of dt's numbers at |x| (x float64, normal range)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -100)))
    return torch.exp2(e - (MANT[dt] - 1))


def prescale(q, scale, dt):
    """q * scale * log2(e) formed in fp32 and rounded to dt: what a q_scaled = 1 caller hands the kernel."""
    return (q.float() * (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))).to(dt)


def softmax_attention64(q, k, v, scale, causal=False, q_scaled=False, probs=False):
    """fp64 softmax attention on [B][H][L][d] operands as given (already rounded to their type).  q_scaled: the scores
    are q . k in base-2 units (no scale)."""
    s = q.double() @ k.double().transpose(-1, -2)
    s = s * (math.log(2.0) if q_scaled else scale)
    if causal:
        Lq, Lk = s.shape[-2:]
        s = s + torch.full((Lq, Lk), float("-inf"), dtype=torch.float64).triu(1)
    p = torch.softmax(s, -1)
    return p if probs else p @ v.double()


# ------------------------------------------------------------------ one-hot attention
def _succ(layout, B, H):
    """(b, h) -> the (b, h) whose key 0 follows this one's key Lk - 1 in memory (None: nothing of the tensor does)."""
    def rows(b, h):      # [B][Lk][H d]: the next row of the same columns is the next batch's key 0
        return (b + 1, h) if b + 1 < B else None

    def hm(b, h):        # [B][H][Lk][d]: the next head's key 0, then the next batch's head 0
        return (b, h + 1) if h + 1 < H else ((b + 1, 0) if b + 1 < B else None)
    return {"rows": rows, "hm": hm}[layout]


def _codes(n, d, protected, thr, gen, exclude=()):
    """n distinct +-1 codes [n][d] (float64) whose |dot| with every protected code is <= thr and that equal none of
    `exclude`."""
    out, seen = [], {tuple(c.tolist()) for c in exclude}
    P = torch.stack(protected) if protected else None
    while len(out) < n:
        c = torch.randint(0, 2, (4 * n + 64, d), generator=gen).double() * 2 - 1
        if P is not None:
            c = c[((c @ P.T).abs() <= thr).all(1)]
        for row in c:
            t = tuple(row.tolist())
            if t not in seen:
                seen.add(t)
                out.append(row)
                if len(out) == n:
                    break
    return torch.stack(out) if n else torch.zeros(0, d, dtype=torch.float64)


def causal_baits(L):
    """Bait key indices of a causal case: behind query 0's neighbour, at the 32-key sub-tile and 64-key tile edges, the
    diagonal tile of a later query block, and the last key."""
    return sorted({j for j in (2, 33, 64, 65, 128, 129, L - 1) if 2 <= j <= L - 1})


@functools.lru_cache(maxsize=None)
def onehot_attention(B, H, Lq, Lk, d, dt, causal=False, seed=0, layout="rows", floor=False):
    """-> dict: q [B][H][Lq][d], k, v [B][H][Lk][d] (dt, CPU), perm [B][H][Lq], want = V[b, h, perm] (float64),
    victims [(b, h, query, bait)] and bait_k [B][H][d] (the row that follows key Lk - 1 of (b, h) in `layout`, or the
    zero row where nothing follows).  Causal cases carry their baits inside k (victims' bait = the key index).
    floor: the last coordinate of every key is +z and of every query -z (FLOOR_Z), which lowers every score by the
    same z^2 > 2 s^2 (d - 1) — the softmax is unchanged, but every real score is now negative, so a key row of ZEROS
    (what the kernels stage for rows past Lk) would win: the bait for a mask that admits such a row."""
    g = torch.Generator().manual_seed(1000 + seed)
    s, thr = CODE_S[d], d // 8
    K = torch.zeros(B, H, Lk, d, dtype=torch.float64)
    perm = torch.zeros(B, H, Lq, dtype=torch.long)
    victims = []
    succ = _succ(layout, B, H)
    pred = {succ(b, h): (b, h) for b in range(B) for h in range(H)}
    prot = {}                      # (b, h) -> the code of its protected target (the one its successor's key 0 doubles)
    order = [(b, h) for b in range(B) for h in range(H)]     # (a predecessor always comes earlier in this order)
    for b, h in order:
        if causal:
            assert Lq == Lk
            J = causal_baits(Lk)
            T, P = [], []
            for j in J:            # query j - 1 targets t_j <= j - 1; key j > j - 1 carries twice t_j's code
                t = next(t for t in range(1, j) if t not in J and t not in T)
                T.append(t)
                P.append(_codes(1, d, P, thr, g)[0])
            rest = [i for i in range(Lk) if i not in J and i not in T]
            codes = _codes(len(rest), d, P, thr, g, exclude=P)
            K[b, h, rest] = codes
            for j, t, p in zip(J, T, P):
                K[b, h, t] = p
                K[b, h, j] = 2 * p
                victims.append((b, h, j - 1, j))
            free = torch.tensor([i for i in range(Lk) if i not in T])
            for qi in range(Lq):
                ok = free[free <= qi]
                perm[b, h, qi] = ok[int(torch.randint(0, len(ok), (1,), generator=g))]
            for j, t in zip(J, T):
                perm[b, h, j - 1] = t
        else:
            pb = prot.get(pred.get((b, h)))
            pl = [pb] if pb is not None else []
            if Lk == 1:
                own, t = (pb if pb is not None else _codes(1, d, [], thr, g)[0]), 0
                K[b, h, 0] = own * (2 if pb is not None else 1)
            else:
                own, t = _codes(1, d, pl, thr, g)[0], min(Lk - 1, 1 + (b + h) % 3)
                codes = _codes(Lk - 1, d, pl, thr, g, exclude=[own])
                codes[t - 1] = own                         # keys 1 .. Lk - 1; key 0 below
                K[b, h, 1:] = codes
                K[b, h, 0] = 2 * pb if pb is not None else _codes(1, d, [], thr, g, exclude=list(codes))[0]
            prot[(b, h)] = own
            perm[b, h] = torch.randint(0, Lk, (Lq,), generator=g)
            if succ(b, h) is not None:
                for qi in sorted({0, Lq // 2, 63 % Lq, 64 % Lq, Lq - 1}):     # the bait's victims
                    perm[b, h, qi] = t
                    victims.append((b, h, qi, "next"))
    bi = torch.arange(B)[:, None, None]
    hi = torch.arange(H)[None, :, None]
    Q = torch.sign(K)[bi, hi, perm] * s
    K = K * s
    if floor:
        K[..., d - 1], Q[..., d - 1] = FLOOR_Z[d], -FLOOR_Z[d]
    V = torch.randint(-7, 8, (B, H, Lk, d), generator=g).double() * 16
    bait_k = torch.zeros(B, H, d, dtype=torch.float64)
    if not causal:
        for b, h in order:
            if succ(b, h) is not None:
                bait_k[b, h] = K[succ(b, h)][0]
    q, k, v = Q.to(dt), K.to(dt), V.to(dt)
    assert torch.equal(q.double(), Q) and torch.equal(k.double(), K) and torch.equal(v.double(), V)   # all representable
    return dict(q=q, k=k, v=v, perm=perm, want=V[bi, hi, perm], victims=victims, bait_k=bait_k.to(dt), causal=causal,
                scale=1.0 / math.sqrt(d), layout=layout, floor=floor)


def onehot_bar(dt):
    """|got - want| per element.  16-bit: p is stored with relative error <= 2^-9 (bf16) against an fp32 row sum and
    one output rounding adds at most one bf16 ulp at 128 (1.0), while distinct V entries differ by >= 16.  fp32: the
    off-target mass (<= 1e-6) times the V range (224) and fp32 rounding stay below 1e-3."""
    return 1e-3 if dt == torch.float32 else 1.0


def onehot_explain(got, case):
    """'' when got [B][H][Lq][d] meets the bar, else a report of the first failing (b, h, q) and which key row of its
    (batch, head), or of any other, the output equals."""
    want, v = case["want"], case["v"].double()
    err = (got.double().cpu() - want).abs()
    bad = (err > onehot_bar(case["q"].dtype)).any(-1).nonzero()
    if not len(bad):
        return ""
    b, h, qi = (int(x) for x in bad[0])
    row = got[b, h, qi].double().cpu()
    hit = ((v - row).abs() <= 1.0).all(-1).nonzero()
    where = ("the ZERO row (a zero-filled key row past Lk was let in)" if float(row.abs().max()) <= 1.0 else
             "no key row of any (batch, head)") if not len(hit) else \
        "key row (b, h, key) = " + ", ".join(str(tuple(int(x) for x in r)) for r in hit[:4])
    return (f"{len(bad)} of {err.shape[0] * err.shape[1] * err.shape[2]} queries wrong; first (b, h, q) = ({b}, {h}, {qi}): "
            f"target key {int(case['perm'][b, h, qi])}, max |got - want| {float(err[b, h, qi].max())}, output equals {where}")


def onehot_off_target(case, q_scaled=False):
    """Largest softmax mass off the target over all queries (fp64, on the rounded operands)."""
    q = prescale(case["q"], case["scale"], case["q"].dtype) if q_scaled else case["q"]
    p = softmax_attention64(q, case["k"], case["v"], case["scale"], case["causal"], q_scaled, probs=True)
    on = p.gather(-1, case["perm"][..., None])[..., 0]
    return float((1.0 - on).max())


def onehot_bait_mass(case):
    """Smallest mass the victims' UNMASKED softmax puts on their bait (the key row behind the last one appended, or no
    causal mask): the test discriminates only if a kernel that lets the bait in locks onto it."""
    q, k = case["q"], case["k"]
    worst = 1.0
    for b, h, qi, bait in case["victims"]:
        kk = k[b, h].double()
        if bait == "next":
            kk = torch.cat([kk, case["bait_k"][b, h].double()[None]])
            bait = kk.shape[0] - 1
        p = torch.softmax(q[b, h, qi].double() @ kk.T * case["scale"], -1)
        worst = min(worst, float(p[bait]))
    return worst


def onehot_zero_key_mass(case):
    """Smallest mass any query's softmax would put on an all-zero key row appended to its keys."""
    s = case["q"].double() @ case["k"].double().transpose(-1, -2) * case["scale"]
    if case["causal"]:
        s = s + torch.full(s.shape[-2:], float("-inf"), dtype=torch.float64).triu(1)
    p = torch.softmax(torch.cat([s, torch.zeros_like(s[..., :1])], -1), -1)
    return float(p[..., -1].min())


# ------------------------------------------------------------------ uniform attention
@functools.lru_cache(maxsize=None)
def uniform_attention(B, H, Lq, Lk, d, dt, seed=0, causal=False):
    """q = 0 (every score 0, every p = 1), V[j][c] = 1 where j % d == c: O[c] = count_c / Lk (causal: the keys
    j <= q alone, O[q][c] = count_c(q + 1) / (q + 1))."""
    g = torch.Generator().manual_seed(2000 + seed)
    q = torch.zeros(B, H, Lq, d, dtype=dt)
    k = torch.randn(B, H, Lk, d, generator=g).to(dt)
    j = torch.arange(Lk)
    V = (j[:, None] % d == torch.arange(d)[None]).double()
    count = V.sum(0)
    want = (count / Lk).expand(B, H, Lq, d)
    if causal:
        want = (V.cumsum(0) / (j + 1.0)[:, None])[:Lq].expand(B, H, Lq, d)
    return dict(q=q, k=k, v=V.expand(B, H, Lk, d).contiguous().to(dt), want=want, count=count, Lk=Lk,
                scale=1.0 / math.sqrt(d), keys=(j[:Lq] + 1.0) if causal else torch.full((Lq,), float(Lk)))


def uniform_bar(want, dt):
    return 2 * ulp(want, dt)


# ------------------------------------------------------------------ ramp attention
RAMPS = {"rise0.5": (0.5,), "rise0.1": (0.1,), "fall0.5": (-0.5,), "fall0.1": (-0.1,),
         "mixed": (0.5, -0.5, 0.1, -0.1)}          # per query, cycling: one wave holds rising and falling queries


@functools.lru_cache(maxsize=None)
def ramp_attention(B, H, Lq, Lk, d, dt, ramp, seed=0, causal=False):
    """Rank-one scores: k_j = a_j u with a_j = j / 8 and u a +-1 vector, q = c u with c = 8 rate / (d scale log2 e):
    in base-2 units query q's score changes by rate per key.  Every element of a q row has the same magnitude, so a
    kernel that folds scale * log2(e) into q and rounds it perturbs all of the row's scores by one common factor.
    V is Gaussian; want = the fp64 softmax on the rounded operands."""
    g = torch.Generator().manual_seed(3000 + seed)
    scale = 1.0 / math.sqrt(d)
    u = torch.randint(0, 2, (B, H, 1, d), generator=g).double() * 2 - 1
    a = torch.arange(Lk, dtype=torch.float64) / 8
    rates = torch.tensor(RAMPS[ramp], dtype=torch.float64)[torch.arange(Lq) % len(RAMPS[ramp])]
    c = 8 * rates / (d * scale * LOG2E)
    q = (c[None, None, :, None] * u).to(dt)
    k = (a[None, None, :, None] * u).to(dt)
    v = torch.randn(B, H, Lk, d, generator=g).to(dt)
    return dict(q=q, k=k, v=v, scale=scale, want=softmax_attention64(q, k, v, scale, causal), rates=rates)


# ------------------------------------------------------------------ integer GEMM / conv
WIDE_SIGMA = {torch.bfloat16: 300.0, torch.float16: 4000.0}     # spread of the exact outputs of the "wide" regime


def _ints(gen, shape, lim, density=1.0):
    x = torch.randint(-lim, lim + 1, shape, generator=gen).float()
    if density < 1.0:
        x = x * (torch.rand(shape, generator=gen) < density)
    return x


def _regime(regime, K, dt):
    """-> (operand limit L, density, bias / residual limit)."""
    if regime == "small":        # products in {-1, 0, 1}; sum's spread sqrt(K density^2) <= 14
        return 1, min(0.6, math.sqrt(200.0 / K)), 8
    assert regime == "wide" and dt in WIDE_SIGMA
    L = 1
    while L * (L + 1) / 3.0 * math.sqrt(K) < WIDE_SIGMA[dt]:     # E[a^2] = L (L + 1) / 3 of the uniform integers
        L += 1
    return L, 1.0, 64


def _exact_mm(a, b):
    """a @ b^T of integer-valued fp32 matrices, exactly (fp64), batched or not."""
    bound = float(a.abs().max()) * float(b.abs().max()) * a.shape[-1]
    if bound < 2 ** 24:          # every partial sum an integer below 2^24: the fp32 product is exact in any order
        return (a @ b.transpose(-1, -2)).double()
    return a.double() @ b.double().transpose(-1, -2)


@functools.lru_cache(maxsize=None)
def int_gemm_operands(M, N, K, regime, dt, seed=0, alpha=1.0, batch=1):
    """-> dict A [M][K], B [N][K], bias [N], residual [M][N] (fp32, integer-valued; a leading batch dimension on A, B
    and residual when batch > 1) and exact = alpha A B^T + bias + residual (fp64)."""
    g = torch.Generator().manual_seed(4000 + seed)
    L, dens, lb = _regime(regime, K, dt)
    bs = (batch,) if batch > 1 else ()
    A, Bw = _ints(g, bs + (M, K), L, dens), _ints(g, bs + (N, K), L, dens)
    bias, R = _ints(g, (N,), lb), _ints(g, bs + (M, N), lb)
    stage = alpha * _exact_mm(A, Bw) + bias.double()
    return dict(A=A, B=Bw, bias=bias, residual=R, exact=stage + R.double(), stage=stage, post=R.double(), L=L)


@functools.lru_cache(maxsize=None)
def int_conv_operands(N, H, W, C0, C1, Co, k, stride, pad, up_hw, asym, regime, dt, seed=0):
    """NHWC conv operands as integers -> dict x0 [N][H][W][C0], x1 (or None), w [Co][C0 + C1][k][k], bias [Co], rowadd
    [N][Co], residual [N][Ho][Wo][Co] and exact [N][Ho][Wo][Co] (fp64).  asym: the VAE downsampler's pad (0, 1, 0, 1)
    with padding 0."""
    g = torch.Generator().manual_seed(5000 + seed)
    L, dens, lb = _regime(regime, k * k * (C0 + C1), dt)
    x0 = _ints(g, (N, H, W, C0), L, dens)
    x1 = _ints(g, (N, H, W, C1), L, dens) if C1 else None
    w = _ints(g, (Co, C0 + C1, k, k), L, dens)
    xin = (torch.cat([x0, x1], 3) if C1 else x0).permute(0, 3, 1, 2)
    if up_hw is not None:
        xin = F.interpolate(xin, size=up_hw, mode="nearest")
    if asym:
        xin = F.pad(xin, (0, 1, 0, 1))
    big = L * L * k * k * (C0 + C1) >= 2 ** 24
    y = F.conv2d(xin.double() if big else xin, w.double() if big else w, None, stride=stride, padding=0 if asym else pad)
    y = y.permute(0, 2, 3, 1).double()
    bias, rowadd, R = _ints(g, (Co,), lb), _ints(g, (N, Co), lb // 2), _ints(g, tuple(y.shape), lb)
    stage, post = y + bias.double(), rowadd.double()[:, None, None, :] + R.double()
    return dict(x0=x0, x1=x1, w=w, bias=bias, rowadd=rowadd, residual=R, exact=stage + post, stage=stage, post=post,
                L=L, out_hw=(y.shape[1], y.shape[2]))


def expected(exact, odt):
    """The exact result converted once (round to nearest even) to the output type."""
    assert float(exact.abs().max()) < 2 ** 24          # (so the fp64 -> fp32 step of the conversion is exact)
    return exact.to(odt)


def expected_staged(case, dt):
    """What the 16-bit large-tile and gemm_sk epilogues store, exactly: they stage alpha acc + bias in the storage type
    (the staged tile fills the LDS: 256 x 320 x 2 B), then a second pass adds row-add and residual and rounds again
    (gemm2.hip's vec_epilogue passes 1 and 2; gemm_sk.hip's header spells the same arithmetic).  Both roundings are
    to nearest even and both round exact values, so this too is equality, not a bound; it differs from the once-rounded
    result by at most one ulp (of the larger of the staged value and the result), and only where alpha acc + bias is not
    representable."""
    assert float(case["exact"].abs().max()) < 2 ** 24 and float(case["stage"].abs().max()) < 2 ** 24
    return (case["stage"].to(dt).double() + case["post"]).to(dt)


def int_shares(exact, dt):
    """(share of the exact outputs not representable in dt, share that are exact ties between two neighbours)."""
    r = exact.to(dt).double()
    off = (r != exact)
    tie = off & ((exact - r).abs() * 2 == ulp(exact, dt))
    return float(off.double().mean()), float(tie.double().mean())


def int_explain(got, case, odt, staged=False):
    """'' when got equals the exact result rounded once (or, staged, the two-pass epilogue's value), else a report."""
    exact = case["exact"]
    want = expected_staged(case, odt) if staged else expected(exact, odt)
    g = got.detach().cpu()
    if torch.equal(g, want):
        return ""
    bad = (g != want).nonzero()
    i = tuple(int(x) for x in bad[0])
    return (f"{len(bad)} of {want.numel()} elements differ; first at {i}: got {float(g[i])}, want {float(want[i])}, "
            f"exact {float(exact[i])}" + (f" = staged {float(case['stage'][i])} + {float(case['post'][i])}" if staged else ""))


# ------------------------------------------------------------------ the cases the GPU tests run (and the host test proves)
DT16 = (torch.bfloat16, torch.float16)

# (B, H, Lq, Lk, d): streamed d = 40 (attn3q / attn3 PF 3 / attn3), ragged query and key counts, one key
ATTN_D40 = [(2, 2, 130, 64, 40), (2, 2, 130, 65, 40), (2, 2, 64, 129, 40), (2, 3, 333, 190, 40), (2, 2, 300, 1, 40)]
ATTN_D40_BIG = (2, 2, 1024, 1024, 40)
# resident K/V (Lk <= 128)
ATTN_RES = [(2, 2, 200, lk, d) for d in (40, 80, 160) for lk in (1, 20, 64, 65, 77, 128)]
ATTN_RES_AUTO = (16, 8, 2048, 77, 40)        # 16 x 8 x 8 = 1024 blocks of two query groups -> an automatic qrep of 2
ATTN_D80 = [(2, 2, 130, 129, 80), (2, 2, 130, 300, 80)]
ATTN_D160 = [(2, 2, 130, 129, 160), (2, 2, 130, 300, 160)]
ATTN_D64_CAUSAL = [(2, 2, 77, 77, 64), (2, 2, 300, 300, 64)]
ATTN_D64 = [(2, 2, 200, 77, 64), (2, 2, 130, 300, 64)]
ATTN_D512 = [(2, 1, L, L, 512) for L in (77, 256, 333)]
ATTN_F32 = [(2, 2, lq, lk, d) for d in (40, 64, 80, 160) for lq, lk in ((100, 77), (200, 130))]
ATTN_F32_CAUSAL = [(2, 2, 100, 100, 64), (2, 2, 200, 200, 64)]
ATTN_FALLBACK = [(2, 2, 130, 77, 48), (2, 2, 130, 190, 40)]      # (the second with Q offset by 4 elements)
ATTN_GRID = [(1, 5, 200, 190, 40), (3, 3, 200, 190, 40)]         # grids that are no multiple of 8
ATTN_RAMP_ALL = ATTN_D40[3]                  # every ramp runs here (three key tiles, ragged); "mixed" everywhere else


def ramps_for(shape):
    return tuple(RAMPS) if tuple(shape) == ATTN_RAMP_ALL else ("mixed",)


ATTN_PROD = [(2, 8, lq, d) for d in (40, 80, 160) for lq in (256, 100)]      # (B, H, Lq, d): self Lk = Lq, cross Lk = 77

# dense GEMM (M, N, K)
GEMM_4WAVE = [(77, 24, 8), (300, 2560, 320)]
GEMM_SMALL_SPLITK = [(154, 768, 3072), (16, 1280, 1280)]
GEMM_LARGE = [(1000, 256, 512), (1025, 640, 640)]
GEMM_SPLITK = (1024, 1280, 2560)
GEMM_SK = [(1025, 320, 320), (777, 640, 320)]
GEMM_PP = (1024, 1024, 640)           # whole 256 x 256 tiles when its rows count as one image of 16 (op_imgs = 1)
GEMM_BATCHED = (3, 130, 70, 64)
GEMM_ALPHA = (200, 96, 64)
CONV_1X1_DENSE = (3, 7, 9, 320, 1280, 320, 1, 1, 0, None, False)
# convs (N, H, W, C0, C1, Co, k, stride, pad, up_hw, asym)
CONV_IM2COL = {"plain": (1, 13, 9, 32, 0, 40, 3, 1, 1, None, False),
               "stride2_odd": (2, 17, 12, 64, 0, 64, 3, 2, 1, None, False),
               "vae_asym_pad": (2, 18, 14, 64, 0, 64, 3, 2, 0, None, True),
               "upsample": (2, 6, 4, 32, 0, 48, 3, 1, 1, (11, 7), False)}
CONV_HALO = {"rows_w16_concat": (1, 16, 16, 64, 64, 160, 3, 1, 1, None, False),
             "rows_w32": (1, 8, 32, 64, 0, 160, 3, 1, 1, None, False)}
CONV_HALO_SPLIT = (2, 16, 16, 1280, 0, 1280, 3, 1, 1, None, False)
CONV_STRIP = (1, 8, 160, 64, 64, 128, 3, 1, 1, None, False)
CONV_MI = (5, 8, 8, 1280, 0, 1280, 3, 1, 1, None, False)
