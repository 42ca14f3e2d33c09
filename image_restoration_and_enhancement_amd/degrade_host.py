"""Host side of the JPEG round-trip and motion-blur degradations (numpy only): the per-image parameters the
kernels in csrc/degrade.hip and csrc/degrade_jpeg.hip consume, and integer / fp32 restatements of both
operations that the kernels are held to bit for bit.

* `motion_kernel_taps`  — the line kernel of add_motion_blur (make_synthetic_pairs.py:51-63) as a tap list.
* `motion_blur_ref`     — cv2.filter2D(img, -1, kernel) for that kernel (:64): correlation, anchor at the
                          centre, BORDER_REFLECT_101, fp32 accumulation in raster tap order, rint, saturate.
                          Parity against cv2 itself is unpinned (OpenCV may take a DFT path for large kernels).
* `jpeg_quant_tables`   — libjpeg's standard tables scaled by a quality (jpeg_set_quality, baseline).
* `jpeg_roundtrip_ref`  — the pixels of cv2.imencode('.jpg') -> cv2.imdecode (:38-43): libjpeg's integer chain
                          (colour conversion, 4:2:0 down-sampling, islow DCT, quantise, dequantise, islow
                          IDCT, fancy up-sampling, colour conversion back).  The entropy coder is lossless and
                          left out.  Pinned bit-exact to Pillow + libjpeg-turbo by tests/test_degrade_artifacts_host.py.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np

MIN_SIDE = 8   # both references (and the kernels' C ABI) refuse H < 8 or W < 8

JPEG_LUMA = (16, 11, 10, 16, 24, 40, 51, 61,
             12, 12, 14, 19, 26, 58, 60, 55,
             14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77,
             24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101,
             72, 92, 95, 98, 112, 100, 103, 99)
JPEG_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99,
               18, 21, 26, 66, 99, 99, 99, 99,
               24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def _check_side(img: np.ndarray) -> None:
    if img.dtype != np.uint8 or img.ndim < 2:
        raise ValueError("expected a uint8 image")
    if img.shape[0] < MIN_SIDE or img.shape[1] < MIN_SIDE:
        raise ValueError(f"H and W must be at least {MIN_SIDE}")


# ---------------------------------------------------------------------------------------- motion blur
def motion_kernel_taps(kernel_size: int, angle_deg: float) -> Tuple[List[Tuple[int, int]], int]:
    """make_synthetic_pairs.py:51-63 -> the distinct non-zero cells as (dy, dx) offsets from the centre, in
    raster order of (y, x), and their count."""
    k = int(kernel_size)
    center = k // 2
    rad = math.radians(angle_deg)
    dx, dy = math.cos(rad), math.sin(rad)
    cells = set()
    for i in range(k):
        x = int(center + (i - center) * dx)
        y = int(center + (i - center) * dy)
        if 0 <= x < k and 0 <= y < k:
            cells.add((y, x))
    taps = [(y - center, x - center) for y, x in sorted(cells)]
    return taps, len(taps)


def _reflect101(i: np.ndarray, n: int) -> np.ndarray:
    period = 2 * n - 2
    i = np.abs(i) % period
    return np.where(i >= n, period - i, i)


def motion_blur_ref(img: np.ndarray, taps) -> np.ndarray:
    """cv2.filter2D(img, -1, kernel), kernel = 1/n on `taps`: per sample acc = acc + coef * src in fp32, one
    rounding per product and per sum, taps in raster order; rint (half to even), clamp to 0..255."""
    _check_side(img)
    if len(taps) == 0:
        raise ValueError("at least one tap")
    H, W = img.shape[:2]
    coef = np.float32(1) / np.float32(len(taps))
    src = img.astype(np.float32)
    acc = np.zeros(img.shape, np.float32)
    ys, xs = np.arange(H), np.arange(W)
    for dy, dx in taps:
        s = src[_reflect101(ys + dy, H)][:, _reflect101(xs + dx, W)]
        acc = acc + coef * s
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------- JPEG
def jpeg_quant_tables(quality: int) -> np.ndarray:
    """int32 [2][64] (luma, chroma; natural row-major order) as jpeg_set_quality(quality, force_baseline)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([JPEG_LUMA, JPEG_CHROMA], dtype=np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.int32)


def _fix(x: float) -> int:
    return int(x * 65536 + 0.5)


_C0298, _C0390, _C0541, _C0765, _C0899, _C1175 = 2446, 3196, 4433, 6270, 7373, 9633
_C1501, _C1847, _C1961, _C2053, _C2562, _C3072 = 12299, 15137, 16069, 16819, 20995, 25172
_CONST_BITS, _PASS1_BITS = 13, 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first: bool):
    """One 1-D pass of jfdctint (islow) along the last axis of d (int64 [..., 8])."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = _CONST_BITS - _PASS1_BITS if first else _CONST_BITS + _PASS1_BITS
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << _PASS1_BITS, (t10 - t11) << _PASS1_BITS
    else:
        out[0], out[4] = _descale(t10 + t11, _PASS1_BITS), _descale(t10 - t11, _PASS1_BITS)
    z1 = (t12 + t13) * _C0541
    out[2] = _descale(z1 + t13 * _C0765, n)
    out[6] = _descale(z1 - t12 * _C1847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _C1175
    t4, t5, t6, t7 = t4 * _C0298, t5 * _C2053, t6 * _C3072, t7 * _C1501
    z1, z2, z3, z4 = -z1 * _C0899, -z2 * _C2562, -z3 * _C1961 + z5, -z4 * _C0390 + z5
    out[7], out[5] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n)
    out[3], out[1] = _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(out, -1)


def _idct_pass(c, n: int):
    """One 1-D pass of jidctint (islow) along the last axis of c, descaled by n bits."""
    z2, z3 = c[..., 2], c[..., 6]
    z1 = (z2 + z3) * _C0541
    t2, t3 = z1 - z3 * _C1847, z1 + z2 * _C0765
    t0, t1 = (c[..., 0] + c[..., 4]) << _CONST_BITS, (c[..., 0] - c[..., 4]) << _CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[..., 7], c[..., 5], c[..., 3], c[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * _C1175
    t0, t1, t2, t3 = t0 * _C0298, t1 * _C2053, t2 * _C3072, t3 * _C1501
    z1, z2, z3, z4 = -z1 * _C0899, -z2 * _C2562, -z3 * _C1961 + z5, -z4 * _C0390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(o, n) for o in out], -1)


def _quantise_plane(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """plane int64 [8a][8b] samples 0..255 -> quantised DCT coefficients [a][b][row][col] (jcdctmgr's division)."""
    Hp, Wp = plane.shape
    blk = (plane - 128).reshape(Hp // 8, 8, Wp // 8, 8).transpose(0, 2, 1, 3)       # [by][bx][row][col]
    c = _fdct_pass(blk, True)                                                         # rows
    c = _fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)                        # columns
    q8 = q.astype(np.int64).reshape(8, 8) * 8
    return np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8)


def _codec_plane(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """plane int64 [8a][8b] samples 0..255 -> reconstructed samples after DCT, quantise, dequantise, IDCT."""
    Hp, Wp = plane.shape
    c = _quantise_plane(plane, q)
    c = c * q.astype(np.int64).reshape(8, 8)
    c = _idct_pass(c.swapaxes(-1, -2), _CONST_BITS - _PASS1_BITS).swapaxes(-1, -2)    # columns
    c = _idct_pass(c, _CONST_BITS + _PASS1_BITS + 3)                                  # rows
    out = np.clip(c + 128, 0, 255)
    return out.transpose(0, 2, 1, 3).reshape(Hp, Wp)


def _pad_edge(p: np.ndarray, h: int, w: int) -> np.ndarray:
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def _upsample_h2v2_fancy(c: np.ndarray, H: int, W: int) -> np.ndarray:
    """c int64 [ceil(H/2)][ceil(W/2)] -> [H][W], libjpeg's triangle filter, neighbours clamped to c's edges."""
    ch, cw = c.shape
    oy, ox = np.arange(H), np.arange(W)
    cy, cx = oy // 2, ox // 2
    ny = np.clip(np.where(oy % 2 == 0, cy - 1, cy + 1), 0, ch - 1)
    s = 3 * c[cy] + c[ny]                                                             # [H][cw]
    nx = np.clip(np.where(ox % 2 == 0, cx - 1, cx + 1), 0, cw - 1)
    bias = np.where(ox % 2 == 0, 8, 7)
    return (3 * s[:, cx] + s[:, nx] + bias) >> 4


def _to_ycbcr(img: np.ndarray, rgb: bool):
    """uint8 [H][W][3] -> int64 Y, Cb, Cr planes (jccolor.c, 16-bit fixed point)."""
    x = img.astype(np.int64)
    R, G, B = (x[..., 0], x[..., 1], x[..., 2]) if rgb else (x[..., 2], x[..., 1], x[..., 0])
    Y = (_fix(.299) * R + _fix(.587) * G + _fix(.114) * B + 32768) >> 16
    Cb = (-_fix(.16874) * R - _fix(.33126) * G + _fix(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (_fix(.5) * R - _fix(.41869) * G - _fix(.08131) * B + (128 << 16) + 32767) >> 16
    return Y, Cb, Cr


def _downsample_h2v2(p: np.ndarray) -> np.ndarray:
    """A full-resolution chroma plane [H][W] -> its 4:2:0 plane padded to whole MCUs [H16 / 2][W16 / 2]: columns
    replicated to W16 before the 2x2 average (bias 1, 2 alternating), rows replicated after it."""
    H, W = p.shape
    H16, W16 = -(-H // 16) * 16, -(-W // 16) * 16
    p = _pad_edge(p, 2 * ((H + 1) // 2), W16)
    bias = np.where(np.arange(W16 // 2) % 2 == 0, 1, 2)
    d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return _pad_edge(d, H16 // 2, W16 // 2)


def jpeg_roundtrip_ref(img: np.ndarray, quality: int, rgb: bool = False) -> np.ndarray:
    """uint8 [H][W][3] (BGR, or RGB with rgb=True) -> the decoded pixels of its quality-`quality` 4:2:0
    baseline JPEG, in the same channel order."""
    _check_side(img)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("expected [H][W][3]")
    H, W = img.shape[:2]
    qt = jpeg_quant_tables(quality)
    Y, Cb, Cr = _to_ycbcr(img, rgb)
    H16, W16 = -(-H // 16) * 16, -(-W // 16) * 16
    CH, CW = (H + 1) // 2, (W + 1) // 2
    Yr = _codec_plane(_pad_edge(Y, H16, W16), qt[0])[:H, :W]

    def chroma(p):
        r = _codec_plane(_downsample_h2v2(p), qt[1])
        return _upsample_h2v2_fancy(r[:CH, :CW], H, W) - 128

    cb, cr = chroma(Cb), chroma(Cr)
    Ro = Yr + ((_fix(1.402) * cr + 32768) >> 16)
    Bo = Yr + ((_fix(1.772) * cb + 32768) >> 16)
    Go = Yr + ((-_fix(.34414) * cb + 32768 - _fix(.71414) * cr) >> 16)
    out = np.stack([Ro, Go, Bo] if rgb else [Bo, Go, Ro], -1)
    return np.clip(out, 0, 255).astype(np.uint8)
