"""PIL `Image.resize(size, LANCZOS | BICUBIC)` on the GPU, byte for byte (csrc/resample.hip, C ABI
`irx_resample_coeffs` / `irx_resample_u8`): the resize of the LANCZOS super-resolution fallback
(`src/inference.py:593-596`), the SR area cap (:552-559), `_normalize_mask` (:790-801) and the `VaeImageProcessor`
preprocess of the img2img / inpaint calls.

Pillow's 8-bit resampler is integer arithmetic once its coefficient tables exist; the tables are built on the host
with Pillow's own double expressions (csrc/resample_coeffs.cpp) and cached on the device per (in, out, filter).
Covered: modes "RGB" and "L", both filters, ratios down to 1/16 (ksize <= 97).  `box`, `reducing_gap` and modes
with alpha (which Pillow premultiplies) are not: `resize_pil` hands those to Pillow.
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from PIL import Image

from . import _lib as L

logger = logging.getLogger(__name__)

FILTERS = {"lanczos": L.IRX_RESAMPLE_LANCZOS, "bicubic": L.IRX_RESAMPLE_BICUBIC}
_PIL_FILTERS = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC}
MAX_KSIZE = L.IRX_RESAMPLE_MAX_KSIZE
TILE_W = 64          # the kernel's output tile: TILE_W x tile_height(H, h) pixels (csrc/resample.hip)

_TABLES: Dict[Tuple[int, int, str, str], tuple] = {}
_MAX_TABLES = 256    # axis tables kept per process (each is out * (ksize + 2) ints on the device)
_logged_fallback = set()


def tile_height(in_h: int, out_h: int) -> int:
    """The tile height the launcher picks for in_h -> out_h rows (resample_tile_h; tests size their cases by it)."""
    if in_h <= out_h:
        return 32
    s = in_h / out_h
    return 16 if s <= 2 else 8 if s <= 4 else 4 if s <= 8 else 2


def filter_name(f) -> str:
    """"lanczos" / "bicubic" from a name or a PIL resampling constant."""
    if isinstance(f, str):
        if f.lower() in FILTERS:
            return f.lower()
    elif int(f) == int(Image.LANCZOS):
        return "lanczos"
    elif int(f) == int(Image.BICUBIC):
        return "bicubic"
    raise ValueError(f"unsupported resampling filter {f!r} (lanczos or bicubic)")


def ksize(n_in: int, n_out: int, filter: str = "lanczos") -> int:
    """Taps per output index of one axis (the size-only call of irx_resample_coeffs)."""
    k = C.c_int()
    L.call("irx_resample_coeffs", int(n_in), int(n_out), FILTERS[filter_name(filter)], None, None, 0, C.byref(k))
    return k.value


def coeffs(n_in: int, n_out: int, filter: str = "lanczos") -> Tuple[np.ndarray, np.ndarray]:
    """One axis' host tables: bounds int32 [n_out, 2] = (first source index, taps), weights int32 [n_out, ksize]."""
    f = FILTERS[filter_name(filter)]
    k = ksize(n_in, n_out, filter)
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, k), np.int32)
    L.call("irx_resample_coeffs", int(n_in), int(n_out), f, C.c_void_p(bounds.ctypes.data),
           C.c_void_p(kk.ctypes.data), kk.size, C.byref(C.c_int()))
    return bounds, kk


def supported(in_size: Tuple[int, int], out_size: Tuple[int, int], filter: str = "lanczos") -> bool:
    """Whether (W, H) -> (w, h) is inside the kernel's range on both axes."""
    return all(a == b or ksize(a, b, filter) <= MAX_KSIZE for a, b in zip(in_size, out_size))


def _tables(n_in: int, n_out: int, filter: str, device) -> tuple:
    """(bounds, weights, ksize) on `device`, cached per (in, out, filter, device)."""
    key = (n_in, n_out, filter, str(device))
    t = _TABLES.get(key)
    if t is None:
        bounds, kk = coeffs(n_in, n_out, filter)
        t = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), kk.shape[1])
        while len(_TABLES) >= _MAX_TABLES:      # a driver over many image sizes: drop the oldest pair
            _TABLES.pop(next(iter(_TABLES)))
        _TABLES[key] = t
    return t


def resize_u8(x: torch.Tensor, size: Tuple[int, int], filter: str = "lanczos",
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`Image.resize(size, filter)` on a uint8 CUDA tensor [H, W, C] or [B, H, W, C], C = 1 or 3; size = (w, h).
    `out`: a contiguous uint8 tensor of the result's shape to write into (e.g. a slice of a batch tensor).  An
    unchanged size gives a clone (or a copy into `out`).  Ratios beyond the kernel's range raise IrxError."""
    if x.dtype != torch.uint8 or not x.is_cuda or x.dim() not in (3, 4):
        raise ValueError("expected a uint8 CUDA tensor [H, W, C] or [B, H, W, C]")
    filter = filter_name(filter)
    x = x.contiguous()
    single = x.dim() == 3
    xb = x.unsqueeze(0) if single else x
    B, H, W, Cc = xb.shape
    if Cc not in (1, 3):
        raise ValueError("resize_u8: 1 or 3 channels")
    w, h = int(size[0]), int(size[1])
    if w < 1 or h < 1:
        raise ValueError("height and width must be > 0")
    shape = (h, w, Cc) if single else (B, h, w, Cc)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    elif (out.dtype != torch.uint8 or out.device != x.device or tuple(out.shape) != shape
          or not out.is_contiguous()):
        raise ValueError(f"out: expected a contiguous uint8 tensor of shape {shape} on {x.device}")
    if (h, w) == (H, W):
        out.copy_(x)
        return out
    xt = _tables(W, w, filter, x.device) if w != W else (None, None, 0)
    yt = _tables(H, h, filter, x.device) if h != H else (None, None, 0)
    L.call("irx_resample_u8", C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(xb.data_ptr()),
           B, H, W, Cc, L.ptr(xt[0]), L.ptr(xt[1]), xt[2], L.ptr(yt[0]), L.ptr(yt[1]), yt[2], h, w,
           C.c_void_p(out.data_ptr()))
    return out


def _fallback_reason(image: Image.Image, size, filter) -> Optional[str]:
    if image.mode not in ("RGB", "L"):
        return f"mode {image.mode!r}"
    try:
        f = filter_name(filter)
    except ValueError:
        return f"filter {filter!r}"
    if not supported(image.size, size, f):
        return f"ratio {image.size} -> {tuple(size)} beyond ksize {MAX_KSIZE}"
    return None


def upload(image: Image.Image, device) -> torch.Tensor:
    """An "RGB" / "L" image's bytes as a device tensor [H, W, C] (one host-to-device copy)."""
    a = np.array(image)
    if a.ndim == 2:
        a = a[..., None]
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def resize_pil(image: Image.Image, size: Tuple[int, int], filter="lanczos", device="cuda") -> Image.Image:
    """`image.resize(size, filter)` for "RGB" and "L" images: one upload, the kernel, one download; same mode, same
    bytes.  Any other mode, or a ratio outside the kernel's range, goes to Pillow (logged once at debug level)."""
    size = (int(size[0]), int(size[1]))
    if size == image.size:
        return image.copy()                    # as Image.resize does
    why = _fallback_reason(image, size, filter)
    if why is not None:
        kind = why.split(" ", 1)[0]            # one debug line per kind of fallback, not per image
        if kind not in _logged_fallback:
            _logged_fallback.add(kind)
            logger.debug(f"resize_pil: {why}: resized by Pillow on the host")
        return image.resize(size, _PIL_FILTERS[filter.lower()] if isinstance(filter, str) else filter)
    res = resize_u8(upload(image, device), size, filter).cpu().numpy()
    return Image.fromarray(res[..., 0] if image.mode == "L" else res, image.mode)
