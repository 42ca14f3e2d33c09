"""Image preparation — diffusers `VaeImageProcessor` semantics.

The host forms resize with PIL, as the reference does.  On a ROCm device the same resize runs on the GPU, byte for
byte (`resample` / csrc/resample.hip): `images_to_device` / `masks_to_device` upload each source image's bytes and
resize them straight into the engine's batch tensor, and `normalize_mask(..., device=...)` resizes the mask there.
The uint8 -> [-1, 1] conversion and the uint8 post-processing run in `irx_image_to_tensor` /
`irx_tensor_to_image`.
References: img2img preprocess = LANCZOS resize to (W - W%8, H - H%8); inpaint
image/mask processors resize to 512x512 (A.2); `RestorationPipeline._normalize_mask`
(`src/inference.py:778-803`).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
from PIL import Image


def target_size(img: Image.Image, height=None, width=None) -> Tuple[int, int]:
    h = height if height is not None else img.height - img.height % 8
    w = width if width is not None else img.width - img.width % 8
    return h, w


def to_uint8(img: Image.Image, height=None, width=None) -> np.ndarray:
    """PIL -> HWC uint8 (3 channels) at the processor's size (LANCZOS, like the reference)."""
    h, w = target_size(img, height, width)
    img = img.resize((w, h), resample=Image.LANCZOS)
    a = np.asarray(img)
    if a.ndim == 2:
        a = np.repeat(a[..., None], 3, axis=2)
    if a.shape[2] == 4:
        a = a[..., :3]
    return np.ascontiguousarray(a, dtype=np.uint8)


def mask_to_binary(mask: Image.Image, height: int, width: int) -> np.ndarray:
    """mask_processor.preprocess: L, LANCZOS resize, /255, binarize at 0.5 -> float32 HxW of {0,1}."""
    m = mask.convert("L").resize((width, height), resample=Image.LANCZOS)
    a = np.asarray(m).astype(np.float32) / 255.0
    return (a >= 0.5).astype(np.float32)


def nearest_downsample(mask: np.ndarray, h: int, w: int) -> np.ndarray:
    """torch.nn.functional.interpolate(mask, size=(h, w)) in 'nearest' mode."""
    H, W = mask.shape[-2:]
    sy, sx = np.float32(H / h), np.float32(W / w)
    iy = np.minimum((np.arange(h, dtype=np.float32) * sy).astype(np.int64), H - 1)
    ix = np.minimum((np.arange(w, dtype=np.float32) * sx).astype(np.int64), W - 1)
    return np.ascontiguousarray(mask[..., iy[:, None], ix[None, :]])


def images_to_device(images: Sequence[Image.Image], device, height=None, width=None):
    """`to_uint8` of every image as one device tensor [B, h, w, 3] (same bytes): each image's RGB bytes are
    uploaded at their own size and resized on the GPU into their slice of the batch.  The images must share the
    processor's size (h, w); their source sizes may differ when `height` / `width` are given."""
    import torch
    from . import resample
    rgb = [im.convert("RGB") for im in images]
    sizes = {target_size(im, height, width) for im in rgb}
    if len(sizes) != 1:
        raise ValueError(f"images of one batch must share the processed size, got {sorted(sizes)}")
    h, w = sizes.pop()
    if h < 1 or w < 1:
        raise ValueError("height and width must be > 0")
    out = torch.empty((len(rgb), h, w, 3), dtype=torch.uint8, device=device)
    for i, im in enumerate(rgb):
        if resample.supported(im.size, (w, h)):
            resample.resize_u8(resample.upload(im, device), (w, h), "lanczos", out=out[i])
        else:                                       # a ratio beyond the kernel's range: Pillow, then the upload
            out[i].copy_(torch.from_numpy(to_uint8(im, h, w)).to(device))
    return out


def masks_to_device(masks: Sequence[Image.Image], device, height: int, width: int):
    """`mask_to_binary` of every mask as one device tensor fp32 [B, height, width] of {0, 1}: resized as "L" on
    the GPU, then `byte >= 128`, which is `byte / 255 >= 0.5` in fp32 for every byte value."""
    import torch
    from . import resample
    out = torch.empty((len(masks), height, width), dtype=torch.float32, device=device)
    for i, mk in enumerate(masks):
        m = mk.convert("L")
        if resample.supported(m.size, (width, height)):
            u8 = resample.resize_u8(resample.upload(m, device), (width, height), "lanczos")
            out[i].copy_(u8[..., 0] >= 128)
        else:
            out[i].copy_(torch.from_numpy(mask_to_binary(m, height, width)).to(device))
    return out


def normalize_mask(mask: Image.Image, size: Tuple[int, int], device: Optional[str] = None) -> Image.Image:
    """RestorationPipeline._normalize_mask: resize to the image size, invert if < 10 % is white.  With a ROCm
    `device` the resize of an "L" / "RGB" mask runs on the GPU (same bytes); other modes stay with Pillow."""
    if mask.size != size:
        if device is not None and str(device).startswith("cuda"):
            from . import resample
            mask = resample.resize_pil(mask, size, "lanczos", device)
        else:
            mask = mask.resize(size, Image.LANCZOS)
    a = np.array(mask.convert("L"))
    if np.sum(a > 128) / a.size < 0.1:
        a = 255 - a
        mask = Image.fromarray(a).convert("L")
    return mask


def from_uint8(a: np.ndarray) -> Image.Image:
    return Image.fromarray(np.ascontiguousarray(a))
