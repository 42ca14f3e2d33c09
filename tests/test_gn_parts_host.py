"""CPU checks of tests/gnref.py, the fp64 reference the GroupNorm-partials GPU tests (test_gn_parts_gpu.py) compare
against: GroupNorm rebuilt from block sums equals torch's fp64 GroupNorm of the concatenated tensor, the sub-pixel
block map equals a direct per-parity sum, and the per-parity upsampler reference equals nearest-2x + 3x3 conv."""
import pytest
import torch
import torch.nn.functional as F

from tests import gnref as R


def _affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


@pytest.mark.parametrize("C0,C1,HW,r0,r1,N,silu", [
    (320, 0, 256, 256, 0, 3, False),
    (320, 160, 256, 256, 64, 2, True),     # groups of 15 channels: group 21 straddles the seam; r0 != r1
    (1280, 640, 64, 64, 32, 2, False),     # groups of 60: group 21 again (1260 .. 1320)
    (128, 0, 1024, 128, 0, 2, True),
])
def test_gn_from_sums_is_group_norm(C0, C1, HW, r0, r1, N, silu):
    G, eps = 32, 1e-5
    # (chunk 24: the mean-40 channels never make up a whole group, whose E[x^2] - mean^2 would cancel to 1e-12)
    x = R.hard_rows(N, HW, C0 + C1, seed=C0 + HW, chunk=24 if C0 == 128 else 8).double()
    if C0 == 128:
        x[..., 26:30] -= 40.0
    x0, x1 = x[..., :C0].contiguous(), (x[..., C0:].contiguous() if C1 else None)
    gamma, beta = _affine(C0 + C1, 7)
    p0 = R.block_sums(x0.reshape(N * HW, C0), r0)
    p1 = R.block_sums(x1.reshape(N * HW, C1), r1) if C1 else None
    assert p0.shape == (N * HW // r0, C0, 2) and p0.dtype == torch.float64
    mean, rstd, out = R.gn_from_sums(x0, p0, G, gamma, beta, eps, silu, x1, p1)
    ref = F.group_norm(x.permute(0, 2, 1), G, gamma.double(), beta.double(), eps).permute(0, 2, 1)
    ref = F.silu(ref) if silu else ref
    assert float((out - ref).abs().max()) < 1e-12
    xg = x.reshape(N, HW, G, -1).permute(0, 2, 1, 3).reshape(N, G, -1)
    assert float((mean - xg.mean(-1)).abs().max()) < 1e-12
    assert float((rstd * torch.sqrt(xg.var(-1, unbiased=False) + eps) - 1).abs().max()) < 1e-12
    # image i carries its shift of 3 i: a row block credited to a neighbour would show here
    assert float((mean[1] - mean[0]).min()) > 2.8


def test_block_sums_values():
    y = torch.arange(24, dtype=torch.float32).reshape(6, 4)
    p = R.block_sums(y, 3)
    assert p.shape == (2, 4, 2)
    assert p[1, 2].tolist() == [14.0 + 18.0 + 22.0, 14.0 ** 2 + 18.0 ** 2 + 22.0 ** 2]
    assert torch.equal(R.image_sums(p, 1)[0], p.sum(0))


@pytest.mark.parametrize("n,h,w,c,Rr", [(2, 4, 8, 3, 16), (3, 8, 8, 2, 64), (1, 16, 16, 2, 128)])
def test_sub_pixel_block_map(n, h, w, c, Rr):
    g = torch.Generator().manual_seed(3)
    out = torch.randn(n, 2 * h, 2 * w, c, generator=g, dtype=torch.float64)
    p = R.block_sums_up2(out, Rr)
    rpl = h * w // Rr
    assert p.shape == (4 * n * rpl, c, 2)
    for img in range(n):
        for par in range(4):
            a, b = par >> 1, par & 1
            for j in range(rpl):
                s = torch.zeros(c, dtype=torch.float64)
                q = torch.zeros(c, dtype=torch.float64)
                for m in range(j * Rr, (j + 1) * Rr):     # low-resolution pixel m = y w + x of this image
                    v = out[img, 2 * (m // w) + a, 2 * (m % w) + b]
                    s += v
                    q += v * v
                got = p[(img * 4 + par) * rpl + j]
                assert float((got[:, 0] - s).abs().max()) < 1e-12 and float((got[:, 1] - q).abs().max()) < 1e-12
    # whatever the block size, an image's totals are those of the plain layout
    tot = R.block_sums(out.reshape(n, -1, c).reshape(-1, c), 4 * h * w)
    assert float((R.image_sums(p, n) - R.image_sums(tot, n)).abs().max()) < 1e-10


def test_up2_conv_ref_is_upsample_then_conv():
    from image_restoration_and_enhancement_amd.engine import conv_up2
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 6, 8, generator=g, dtype=torch.float64)
    wt = torch.randn(4, 8, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(4, generator=g, dtype=torch.float64)
    got = R.up2_conv_ref(x, conv_up2(wt), bias)
    up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    ref = F.conv2d(up, wt, bias, padding=1).permute(0, 2, 3, 1)
    assert float((got - ref).abs().max()) < 1e-12
