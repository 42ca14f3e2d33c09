"""Synthetic degradations on the GPU: the reference's `scripts/make_synthetic_pairs.py` helpers with the
same names, arguments and RNG draw order, operating on uint8 HWC device tensors (single images or
[B][H][W][C] batches) through `libirx.so` (csrc/degrade.hip, csrc/degrade_jpeg.hip).  Used to build large
synthetic benchmark batches without a host round trip per image.

Every mode of the reference generator is covered, `--denoise_with_artifacts`, `--sr_with_jpeg` and
`--sr_with_motion_blur` included: `add_jpeg_compression` is the decoded pixels of the cv2 JPEG round trip
(libjpeg's integer chain; the entropy coder is lossless and left out) and `add_motion_blur` is
cv2.filter2D with the reference's line kernel.  `jpeg_roundtrip` and `motion_blur` are the same kernels with
per-image parameters and no draws; `degrade_host.py` builds those parameters and holds the host references.

Host-side randomness stays the reference's: `random.uniform / randint / choice / random` for the per-image
parameters and, with `exact_noise=True`, `np.random.randn` for the noise field (bit-identical pixels
to the numpy code).  With `exact_noise=False` the noise is drawn in-kernel (Philox4x32-10, seeded from
numpy's generator) and only its distribution matches.
"""
from __future__ import annotations

import ctypes as C
import random
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import degrade_host as DH


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _u8(img: torch.Tensor) -> torch.Tensor:
    if img.dtype != torch.uint8 or not img.is_cuda:
        raise ValueError("expected a uint8 CUDA tensor")
    return img.contiguous()


def add_gaussian_noise(img: torch.Tensor, sigma_range=(5, 8), exact_noise: bool = True) -> torch.Tensor:
    """make_synthetic_pairs.py:29-35."""
    img = _u8(img)
    sigma = random.uniform(*sigma_range)
    out = torch.empty_like(img)
    if exact_noise:
        z = torch.from_numpy(np.random.randn(*img.shape).astype(np.float32)).to(img.device)
        L.call("irx_degrade_noise", _s(), _p(img), img.numel(), sigma, _p(z), 0, _p(out))
    else:
        seed = int(np.random.randint(0, 2**63 - 1, dtype=np.int64))
        L.call("irx_degrade_noise", _s(), _p(img), img.numel(), sigma, None, seed, _p(out))
    return out


def gaussian_blur_down(img: torch.Tensor, ksizes: Sequence[int], scale: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """cv2.GaussianBlur(k, 0) per image, then cv2.resize(INTER_CUBIC) to (W//scale, H//scale)."""
    img = _u8(img)
    batched = img.dim() == 4
    x = img if batched else img[None]
    B, H, W, Cc = x.shape
    if len(ksizes) != B or any(k not in (1, 3, 5, 7) for k in ksizes):
        raise ValueError("one kernel size in {1, 3, 5, 7} per image")
    ks = torch.tensor(list(ksizes), dtype=torch.int32, device=img.device)
    blur = torch.empty_like(x)
    lr = torch.empty((B, H // scale, W // scale, Cc), dtype=torch.uint8, device=img.device)
    L.call("irx_degrade_blur_down", _s(), _p(x), B, H, W, Cc, _p(ks), scale, _p(blur), _p(lr))
    return (blur, lr) if batched else (blur[0], lr[0])


def jpeg_roundtrip(batch: torch.Tensor, qualities: Sequence[int], rgb: bool = False) -> torch.Tensor:
    """The decoded pixels of a baseline 4:2:0 JPEG of each image ([B][H][W][3] or one [H][W][3]) at its own
    quality; no draws.  Channel order BGR as cv2.imread gives, or RGB with rgb=True."""
    img = _u8(batch)
    batched = img.dim() == 4
    x = img if batched else img[None]
    B, H, W, Cc = x.shape
    if Cc != 3 or len(qualities) != B:
        raise ValueError("expected [B][H][W][3] and one quality per image")
    qt = torch.from_numpy(np.stack([DH.jpeg_quant_tables(q) for q in qualities])).to(img.device)
    nws = L.call("irx_degrade_jpeg_ws_bytes", B, H, W)
    ws = torch.empty(max(int(nws), 8), dtype=torch.uint8, device=img.device)
    out = torch.empty_like(x)
    L.call("irx_degrade_jpeg", _s(), _p(x), B, H, W, _p(qt), int(rgb), _p(ws), _p(out))
    return out if batched else out[0]


def add_jpeg_compression(img: torch.Tensor, quality_range=(30, 90), rgb: bool = False) -> torch.Tensor:
    """make_synthetic_pairs.py:38-43 (one quality draw; a batch shares it)."""
    quality = random.randint(*quality_range)
    return jpeg_roundtrip(img, [quality] * (img.shape[0] if img.dim() == 4 else 1), rgb)


def motion_blur(batch: torch.Tensor, per_image_taps: Sequence[Sequence[Tuple[int, int]]]) -> torch.Tensor:
    """cv2.filter2D with a 1/n kernel on each image's own (dy, dx) taps (`degrade_host.motion_kernel_taps`);
    [B][H][W][C] or one [H][W][C] / [H][W] image with a one-element tap list; no draws."""
    img = _u8(batch)
    x = img if img.dim() == 4 else (img[None] if img.dim() == 3 else img[None, :, :, None])
    B, H, W, Cc = x.shape
    if len(per_image_taps) != B or any(len(t) == 0 for t in per_image_taps):
        raise ValueError("one non-empty tap list per image")
    off = np.cumsum([0] + [len(t) for t in per_image_taps]).astype(np.int32)
    taps = np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1, 2) for t in per_image_taps])
    tp = torch.from_numpy(taps).to(img.device)
    of = torch.from_numpy(off).to(img.device)
    out = torch.empty_like(x)
    L.call("irx_degrade_motion_blur", _s(), _p(x), B, H, W, Cc, _p(tp), _p(of), _p(out))
    return out.reshape(img.shape)


def add_motion_blur(img: torch.Tensor, kernel_size_range=(5, 15), angle_range=(0, 360)) -> torch.Tensor:
    """make_synthetic_pairs.py:46-64 (kernel size, then angle; a batch shares the kernel)."""
    kernel_size = random.randint(*kernel_size_range)
    angle = random.uniform(*angle_range)
    taps, _ = DH.motion_kernel_taps(kernel_size, angle)
    return motion_blur(img, [taps] * (img.shape[0] if img.dim() == 4 else 1))


def degrade_sr(img: torch.Tensor, scale=4, use_jpeg: bool = False, use_motion_blur: bool = False,
               rgb: bool = False) -> torch.Tensor:
    """make_synthetic_pairs.py:67-81: motion blur (30 % of the time, if enabled) or Gaussian blur, cubic
    down-sampling, then optionally a JPEG round trip of the low-resolution image."""
    n = img.shape[0] if img.dim() == 4 else 1
    if use_motion_blur and random.random() < 0.3:
        blur = add_motion_blur(img, kernel_size_range=(5, 12))
        lr = gaussian_blur_down(blur, [1] * n, scale)[1]      # k = 1: identity blur, the cubic resize alone
    else:
        k = random.choice([3, 5, 7])
        lr = gaussian_blur_down(img, [k] * n, scale)[1]
    if use_jpeg:
        lr = add_jpeg_compression(lr, quality_range=(40, 85), rgb=rgb)
    return lr


def to_grayscale(img: torch.Tensor, mode: str = "lab", rgb: bool = False) -> torch.Tensor:
    """make_synthetic_pairs.py:84-90 (input channel order BGR as cv2.imread gives, or RGB with rgb=True)."""
    img = _u8(img)
    out = torch.empty(img.shape[:-1], dtype=torch.uint8, device=img.device)
    L.call("irx_degrade_gray", _s(), _p(img), img.numel() // 3, 1 if mode == "lab" else 0, int(rgb), _p(out))
    return out


def draw_free_form_strokes(h: int, w: int, num_strokes=(5, 15), thickness_range=(10, 40)):
    """The host half of random_free_form_mask (make_synthetic_pairs.py:104-114): the same `random` draws in
    the same order -> [(points, thickness)]."""
    strokes = []
    for _ in range(random.randint(*num_strokes)):
        pts = []
        for _ in range(random.randint(4, 8)):
            pts.append((random.randint(0, w - 1), random.randint(0, h - 1)))
        thickness = random.randint(*thickness_range)
        strokes.append((pts, thickness))
    return strokes


def rasterize_strokes(h: int, w: int, per_image: List[list], device, img: torch.Tensor = None):
    """Stroke lists (one per image) -> mask [B][h][w] (255 inside) and, with `img`, the masked input."""
    segs, thick, off = [], [], [0]
    for strokes in per_image:
        for pts, t in strokes:
            for (x0, y0), (x1, y1) in zip(pts[:-1], pts[1:]):
                segs.append((x0, y0, x1, y1))
                thick.append(t)
        off.append(len(segs))
    B = len(per_image)
    sg = torch.tensor(segs or [(0, 0, 0, 0)], dtype=torch.int32, device=device)
    th = torch.tensor(thick or [0], dtype=torch.int32, device=device)
    of = torch.tensor(off, dtype=torch.int32, device=device)
    mask = torch.empty((B, h, w), dtype=torch.uint8, device=device)
    masked = None
    if img is not None:
        img = _u8(img)
        masked = torch.empty_like(img)
    L.call("irx_degrade_strokes", _s(), B, h, w, _p(sg), _p(th), _p(of), _p(mask), _p(img), _p(masked))
    return mask, masked


def random_free_form_mask(h: int, w: int, num_strokes=(5, 15), thickness_range=(10, 40), device="cuda"):
    """make_synthetic_pairs.py:104-114 -> uint8 [h][w] device mask."""
    return rasterize_strokes(h, w, [draw_free_form_strokes(h, w, num_strokes, thickness_range)], device)[0][0]


def _noise_given(img: torch.Tensor, sigma: float, z: torch.Tensor, out: torch.Tensor) -> None:
    L.call("irx_degrade_noise", _s(), _p(img), img.numel(), sigma, _p(z), 0, _p(out))


def _gather(x: torch.Tensor, idx: List[int]) -> torch.Tensor:
    return x[torch.tensor(idx, dtype=torch.long, device=x.device)]


def _scatter(x: torch.Tensor, idx: List[int], v: torch.Tensor) -> None:
    x[torch.tensor(idx, dtype=torch.long, device=x.device)] = v


def make_pairs(batch: torch.Tensor, sr_scale: int = 4, grayscale_mode: str = "lab",
               inpaint_easy_ratio: float = 0.7, rgb: bool = False, *, denoise_with_artifacts: bool = False,
               sr_with_jpeg: bool = False, sr_with_motion_blur: bool = False) -> dict:
    """process_split's per-image degradations (make_synthetic_pairs.py:155-198) for a [B][H][W][3] batch in
    one set of launches: {task: input tensor} (+ "inpaint_mask").  Per-image parameters are drawn in the
    reference's order (:162-190: denoise sigma + noise [+ JPEG, motion blur], the degrade_sr draws, inpaint
    mask) image by image; the images that take an optional op are gathered, run in one launch with
    per-image parameters, and scattered back."""
    batch = _u8(batch)
    B, H, W, _ = batch.shape
    sigmas, zs, ks, strokes = [], [], [], []
    dn_jpeg, dn_blur, sr_blur, sr_q = {}, {}, {}, []        # image index -> quality / taps
    for b in range(B):
        sigmas.append(random.uniform(3, 15) if denoise_with_artifacts else random.uniform(5, 8))
        zs.append(np.random.randn(H, W, 3).astype(np.float32))
        if denoise_with_artifacts:
            if random.random() < 0.3:
                dn_jpeg[b] = random.randint(40, 85)
            if random.random() < 0.2:
                k = random.randint(3, 8)
                dn_blur[b] = DH.motion_kernel_taps(k, random.uniform(0, 360))[0]
        if sr_with_motion_blur and random.random() < 0.3:
            k = random.randint(5, 12)
            sr_blur[b] = DH.motion_kernel_taps(k, random.uniform(0, 360))[0]
            ks.append(1)                                      # identity blur: the cubic resize alone
        else:
            ks.append(random.choice([3, 5, 7]))
        if sr_with_jpeg:
            sr_q.append(random.randint(40, 85))
        if random.random() < inpaint_easy_ratio:
            strokes.append(draw_free_form_strokes(H, W, (3, 7), (5, 20)))
        else:
            strokes.append(draw_free_form_strokes(H, W, (8, 15), (20, 40)))
    noisy = torch.empty_like(batch)
    z = torch.from_numpy(np.stack(zs)).to(batch.device)
    for b in range(B):
        _noise_given(batch[b], sigmas[b], z[b], noisy[b])
    if dn_jpeg:
        idx = sorted(dn_jpeg)
        _scatter(noisy, idx, jpeg_roundtrip(_gather(noisy, idx), [dn_jpeg[b] for b in idx], rgb))
    if dn_blur:
        idx = sorted(dn_blur)
        _scatter(noisy, idx, motion_blur(_gather(noisy, idx), [dn_blur[b] for b in idx]))
    src = batch
    if sr_blur:
        idx = sorted(sr_blur)
        src = batch.clone()
        _scatter(src, idx, motion_blur(_gather(batch, idx), [sr_blur[b] for b in idx]))
    _, lr = gaussian_blur_down(src, ks, sr_scale)
    if sr_with_jpeg:
        lr = jpeg_roundtrip(lr, sr_q, rgb)
    gray = to_grayscale(batch, grayscale_mode, rgb)
    mask, masked = rasterize_strokes(H, W, strokes, batch.device, batch)
    return {"denoise": noisy, "sr": lr, "colorize": gray, "inpaint": masked, "inpaint_mask": mask}
