"""PSNR, SSIM, dE76 and the INTER_LINEAR shape match of `metrics.py` on the GPU (csrc/metrics.hip, C ABI
`irx_metrics_pair_u8` / `irx_resize_linear_u8`): uint8 HWC device tensors in, per-image device scalars out, so the
outputs of `restore_batch` are scored where they lie and a directory of pairs is scored with one synchronisation.

`pair_stats` is the kernel's Python entry: the exact int64 squared error, skimage's SSIM and (on request) the mean
dE76 of every pair of a batch, two launches, no host synchronisation.  PSNR is formed on the host from the squared
error with `metrics.psnr`'s own expression (`psnr_from_sse`), which makes it bit-equal to the host value.  SSIM and
dE are fp64 sums in a fixed order: the same bits on every run, at every position of every batch size.

The host builds two kinds of tables with the numpy expressions `metrics.py` itself uses: the float32 sRGB
linearisation of the 256 byte values (`srgb_table`, `metrics.srgb_linear`) and the per-axis (i0, i1, w1) tables of
cv2's INTER_LINEAR (`axis_table`, `metrics.linear_axis`).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import metrics as M

TILE_W = 32          # the kernel's tile: TILE_W x TILE_H windows (7x7, so W - 6 windows per row) per block
TILE_H = 32          # (csrc/metrics.hip MT_TW / MT_TH)
WIN = 7

_TABLES: Dict[tuple, torch.Tensor] = {}
_MAX_TABLES = 256


def supported(shape) -> bool:
    """Whether images of this shape ([H, W], [H, W, C] or [B, H, W, C]) are inside the kernel's range."""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 2:
        shape = shape + (1,)
    if len(shape) == 4:
        if shape[0] < 1:
            return False
        shape = shape[1:]
    if len(shape) != 3:
        return False
    H, W, Cc = shape
    return H >= WIN and W >= WIN and Cc in (1, 3)


def srgb_table() -> np.ndarray:
    """float32 [256]: what `metrics.rgb2lab` makes of a channel value v, `srgb_linear(float32(v) / 255.0)`."""
    return M.srgb_linear(np.arange(256).astype(np.float32) / 255.0)


def axis_table(n_out: int, n_in: int) -> np.ndarray:
    """int32 [n_out, 3] = (i0, i1, w1) of one INTER_LINEAR axis (w0 = 2048 - w1)."""
    i0, i1, _, w1 = M.linear_axis(n_out, n_in)
    return np.stack([i0, i1, w1], axis=1).astype(np.int32)


def _cached(key: tuple, make, device) -> torch.Tensor:
    key = key + (str(device),)
    t = _TABLES.get(key)
    if t is None:
        t = torch.from_numpy(np.ascontiguousarray(make())).to(device)
        while len(_TABLES) >= _MAX_TABLES:
            _TABLES.pop(next(iter(_TABLES)))
        _TABLES[key] = t
    return t


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _batch4(x: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or not x.is_cuda or x.dim() not in (2, 3, 4):
        raise ValueError(f"{what}: expected a uint8 CUDA tensor [H, W], [H, W, C] or [B, H, W, C]")
    x = x.contiguous()
    if x.dim() == 2:
        return x[None, :, :, None]
    return x[None] if x.dim() == 3 else x


def pair_stats(pred: torch.Tensor, gt: torch.Tensor, delta_e: bool = False
               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """(sse int64 [B], ssim float64 [B], delta_e float64 [B] or None) of uint8 device tensors of one shape.
    Enqueues on the current stream and returns; nothing here waits for the device."""
    p, g = _batch4(pred, "pred"), _batch4(gt, "gt")
    if p.shape != g.shape:
        raise ValueError("Input images must have the same dimensions.")
    if g.device != p.device:
        raise ValueError("pred and gt on different devices")
    B, H, W, Cc = p.shape
    if not supported(p.shape):
        raise ValueError(f"pair_stats: shape {tuple(p.shape)} outside the kernel's range (H, W >= 7, C 1 or 3)")
    if delta_e and Cc != 3:
        raise ValueError("delta_e needs 3 channels")
    dev = p.device
    nws = int(L.call("irx_metrics_ws_bytes", B, H, W, Cc))
    if nws <= 0:
        raise ValueError(f"pair_stats: shape {tuple(p.shape)} too large for one launch")
    ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
    sse = torch.empty(B, dtype=torch.int64, device=dev)
    ssim = torch.empty(B, dtype=torch.float64, device=dev)
    de = torch.empty(B, dtype=torch.float64, device=dev) if delta_e else None
    lut = _cached(("srgb",), srgb_table, dev) if delta_e else None
    L.call("irx_metrics_pair_u8", _s(), _p(p), _p(g), B, H, W, Cc, _p(lut), _p(ws), _p(sse), _p(ssim), _p(de))
    return sse, ssim, de


def psnr_from_sse(sse, n: int) -> float:
    """`metrics.psnr` from the exact squared error over n values: the same expression on the same double."""
    err = np.float64(int(sse)) / n
    with np.errstate(divide="ignore"):
        return float(10 * np.log10((255.0 ** 2) / err))


def to_device(img, device="cuda") -> torch.Tensor:
    """A uint8 image (numpy [H, W] / [H, W, C] or a tensor) as a contiguous device tensor."""
    if isinstance(img, torch.Tensor):
        return img.to(device).contiguous()
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8:
        raise ValueError("expected a uint8 image")
    return torch.from_numpy(a).to(device)


def resize_linear_u8(x: torch.Tensor, width: int, height: int) -> torch.Tensor:
    """`metrics.resize_linear` on a uint8 device tensor [H, W], [H, W, C] or [B, H, W, C], byte for byte."""
    xb = _batch4(x, "resize_linear")
    B, H, W, Cc = xb.shape
    width, height = int(width), int(height)
    if Cc not in (1, 3) or width < 1 or height < 1:
        raise ValueError("resize_linear: 1 or 3 channels, positive size")
    if (H, W) == (height, width):
        return x.clone()
    xt = _cached(("lin", width, W), lambda: axis_table(width, W), xb.device)
    yt = _cached(("lin", height, H), lambda: axis_table(height, H), xb.device)
    out = torch.empty((B, height, width, Cc), dtype=torch.uint8, device=xb.device)
    L.call("irx_resize_linear_u8", _s(), _p(xb), B, H, W, Cc, _p(xt), _p(yt), height, width, _p(out))
    return out[0, :, :, 0] if x.dim() == 2 else out[0] if x.dim() == 3 else out


def resize_linear(img, width: int, height: int, device="cuda"):
    """`metrics.resize_linear(img, width, height)`: numpy in, numpy out; device tensor in, device tensor out."""
    if isinstance(img, torch.Tensor):
        return resize_linear_u8(img, width, height)
    return resize_linear_u8(to_device(img, device), width, height).cpu().numpy()


def _pair(pred, gt, device):
    p, g = to_device(pred, device), to_device(gt, device)
    if p.shape != g.shape:
        raise ValueError("Input images must have the same dimensions.")
    return p, g


def psnr(gt, pred, device="cuda") -> float:
    """`metrics.psnr(gt, pred)` of one pair (numpy or device tensors)."""
    p, g = _pair(pred, gt, device)
    return psnr_from_sse(pair_stats(p, g)[0][0].item(), g.numel())


def ssim(gt, pred, device="cuda") -> float:
    """`metrics.ssim(gt, pred)` of one pair (numpy or device tensors)."""
    p, g = _pair(pred, gt, device)
    return float(pair_stats(p, g)[1][0].item())


def delta_e(pred, gt, device="cuda") -> float:
    """`MetricsCalculator.calculate_delta_e(pred, gt)` of one RGB pair of one shape (numpy or device tensors)."""
    p, g = _pair(pred, gt, device)
    return float(pair_stats(p, g, delta_e=True)[2][0].item())
