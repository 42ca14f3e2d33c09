"""fp64 reference of the GroupNorm producer partials and of GroupNorm computed from them (torch only, no project
code): what a producer must emit for a stored tensor, and what a consumer must make of such partials.

A partial is the (sum, sum of squares) of one output channel over a block of R rows of a stored [M][C] tensor
(row = pixel of an NHWC activation, R dividing the pixels of an image); a consumer only ever reads an image's total
per channel, then pools the channels of a group."""
import torch
import torch.nn.functional as F


def block_sums(y, R):
    """[M][C] -> float64 [M / R][C][2]: (sum, sum of squares) of every channel over blocks of R consecutive rows."""
    y = y.detach().double().cpu()
    M, C = y.shape
    assert M % R == 0
    b = y.reshape(M // R, R, C)
    return torch.stack([b.sum(1), (b * b).sum(1)], -1)


def block_sums_up2(out, R):
    """The sub-pixel layout of a nearest-2x upsampler's four parity convs: out [n][2h][2w][c] -> float64
    [4 n h w / R][c][2].  Block (img * 4 + p) * rpl + j (rpl = h w / R) holds rows j R .. (j + 1) R of the
    low-resolution pixels of parity p = 2a + b, which are out[img, a::2, b::2] flattened."""
    n, H2, W2, c = out.shape
    blocks = []
    for img in range(n):
        for p in range(4):
            a, b = p >> 1, p & 1
            blocks.append(block_sums(out[img, a::2, b::2].reshape(-1, c), R))
    return torch.cat(blocks)


def image_sums(p, N):
    """[N * blocks per image][C][2] -> [N][C][2]: the per-image totals, all a consumer reads."""
    p = p.detach().double().cpu()
    return p.reshape(N, -1, p.shape[-2], 2).sum(1)


def stats_from_sums(N, HW, G, eps, p0, p1=None):
    """(mean, rstd), float64 [N][G] each, of the channel concat (x0 | x1) from the sources' partials.  The sources may
    have different block sizes (the totals do not care), and a group may cross the seam between them."""
    t = image_sums(p0, N)
    if p1 is not None:
        t = torch.cat([t, image_sums(p1, N)], 1)
    C = t.shape[1]
    assert C % G == 0
    g = t.reshape(N, G, C // G, 2).sum(2)
    cnt = float(HW * (C // G))
    mean = g[..., 0] / cnt
    var = (g[..., 1] / cnt - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + eps)


def gn_from_sums(x0, p0, G, gamma, beta, eps, silu=False, x1=None, p1=None):
    """x0 [N][HW][C0] (x1 [N][HW][C1]) with partials p0 (p1) -> (mean [N][G], rstd [N][G], out [N][HW][C0 + C1]),
    float64: the normalised (+SiLU) concat with the statistics taken from the partials alone."""
    x = x0.detach().double().cpu()
    if x1 is not None:
        x = torch.cat([x, x1.detach().double().cpu()], -1)
    N, HW, C = x.shape
    mean, rstd = stats_from_sums(N, HW, G, eps, p0, p1)
    cg = C // G
    m = mean.repeat_interleave(cg, 1)[:, None, :]
    r = rstd.repeat_interleave(cg, 1)[:, None, :]
    y = (x - m) * r * gamma.double().cpu() + beta.double().cpu()
    return mean, rstd, F.silu(y) if silu else y


def up2_conv_ref(x, w2, bias):
    """Nearest-2x upsample + 3x3 / pad-1 conv in its per-parity form, float64: x [n][h][w][c], w2 [4][co][2][2][c] (the
    four 2x2 kernels the 3x3 one collapses to on a pixel-doubled image) -> [n][2h][2w][co].  Output pixel
    (2y + a, 2x + b) sees low-resolution rows y - 1 + a .. y + a and columns x - 1 + b .. x + b."""
    xd = x.detach().double().cpu().permute(0, 3, 1, 2)
    n, c, h, w = xd.shape
    w2 = w2.detach().double().cpu().reshape(4, -1, 2, 2, c)
    out = torch.zeros(n, 2 * h, 2 * w, w2.shape[1], dtype=torch.float64)
    for p in range(4):
        a, b = p >> 1, p & 1
        xp = F.pad(xd, (1 - b, b, 1 - a, a))
        out[:, a::2, b::2] = F.conv2d(xp, w2[p].permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    return out + (bias.double().cpu() if bias is not None else 0.0)


def hard_rows(N, HW, C, seed, chunk=8):
    """fp32 [N][HW][C] that shows the usual mistakes: every column has its own spread (0.5 .. 1.5), image i is shifted
    by 3 i (a block credited to the wrong image moves the mean), and channels chunk .. chunk + 8 have mean 40 and
    standard deviation 0.3 (an unshifted fp32 sum of squares loses their variance)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, HW, C, generator=g) * (0.5 + torch.rand(C, generator=g))
    x[..., chunk:chunk + 8] = 40.0 + 0.3 * torch.randn(N, HW, 8, generator=g)
    return x + 3.0 * torch.arange(N, dtype=torch.float32)[:, None, None]
