"""Real-ESRGAN's compact network on the GPU (csrc/srvgg_model.cpp, csrc/srvgg.hip, C ABI `irx_srvgg_u8`): what
`RestorationPipeline._sr_realesrgan` of the reference gets from `model.enhance(img, outscale=4)`
(`src/inference.py:579-591`), on uint8 device tensors.

`RealESRGANCompact(weights)` is a `NativeModel` of kind `IRX_MODEL_SRVGG`: the weights (`srvgg_host.load_weights`) are
packed through the manifest and bound once, the input table (`srvgg_host.input_table`) is uploaded once, and the
workspace is kept per shape.  `dtype="fp16"` is the product (the reference's `half` on a GPU), `"fp32"` the parity
engine.  `enhance` enqueues on the current stream and returns a device tensor; nothing here waits for the device.
`srvgg_host.forward(..., dtype=torch.float64)` is the ground truth, with `half=True` the oracle of the fp16 engine
(DESIGN.md §21).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import srvgg_host as H
from .engine import NativeModel, dtype_code

SCALE = H.UPSCALE
_MAX_SHAPES = 64


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class RealESRGANCompact(NativeModel):
    def __init__(self, weights: Dict[str, torch.Tensor], device="cuda", dtype="fp16"):
        if dtype_code(dtype) not in (L.IRX_F16, L.IRX_F32):
            raise ValueError("RealESRGANCompact: dtype 'fp16' or 'fp32'")
        super().__init__(L.IRX_MODEL_SRVGG, None, dtype, device)
        self.load_state_dict(H.check_weights(weights))
        self.table = H.input_table().to(self.device)
        self._shape_ws: Dict[tuple, torch.Tensor] = {}

    def workspace_bytes(self, batch: int, h: int, w: int) -> int:
        return self._size("irx_srvgg_workspace_bytes", batch, h, w)

    def _workspace(self, B: int, h: int, w: int) -> torch.Tensor:
        need = max(self.workspace_bytes(B, h, w), 256)      # (it depends on the srvgg_fused option)
        ws = self._shape_ws.get((B, h, w))
        if ws is None or ws.numel() < need:
            while len(self._shape_ws) >= _MAX_SHAPES:
                self._shape_ws.pop(next(iter(self._shape_ws)))
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._shape_ws[(B, h, w)] = ws
        return ws

    def _batch(self, images) -> torch.Tensor:
        x = torch.from_numpy(np.ascontiguousarray(images)).to(self.device) if isinstance(images, np.ndarray) else images
        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or not x.is_cuda or x.dim() not in (3, 4) \
                or x.shape[-1] != 3 or min(x.shape) < 1:
            raise ValueError("images: expected uint8 RGB [H, W, 3] or [B, H, W, 3] (numpy, or a tensor on the device)")
        return x.contiguous()

    def _run(self, images, out: Optional[torch.Tensor], want_f: bool):
        x = self._batch(images)
        single = x.dim() == 3
        xb = x[None] if single else x
        B, h, w, _ = xb.shape
        shape = (SCALE * h, SCALE * w, 3) if single else (B, SCALE * h, SCALE * w, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif (out.dtype != torch.uint8 or out.device != x.device or tuple(out.shape) != shape
              or not out.is_contiguous()):
            raise ValueError(f"out: expected a contiguous uint8 tensor of shape {shape} on {x.device}")
        out_f = torch.empty(shape, dtype=torch.float32, device=self.device) if want_f else None
        ws = self._workspace(B, h, w)
        L.call("irx_srvgg_u8", self.h, self.stream(), _p(xb), B, h, w, _p(self.table), _p(out), _p(out_f), _p(ws),
               ws.numel())
        return out, out_f

    def enhance(self, images, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 RGB [H, W, 3] or [B, H, W, 3] -> the uint8 x4 result on the device, [4H, 4W, 3] or [B, 4H, 4W, 3].
        `out`: a contiguous uint8 tensor of that shape to write into (e.g. a slice of a batch tensor)."""
        return self._run(images, out, False)[0]

    def forward_float(self, images):
        """(uint8 result, fp32 result before the clamp), both NHWC on the device (tests)."""
        return self._run(images, None, True)


# ---- the kernels on their own (tests)
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def conv_layer(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, slope: torch.Tensor) -> torch.Tensor:
    """One body layer: x fp16 NHWC [B, H, W, 64], w fp16 [64, 3, 3, 64] (O, KH, KW, I), bias / slope fp32 [64]."""
    B, h, wd, _ = x.shape
    out = torch.empty_like(x)
    L.call("irx_op_srvgg_conv", _stream(), _p(x.contiguous()), B, h, wd, _p(w.contiguous()), _p(bias), _p(slope),
           _p(out))
    return out


def tail(x: torch.Tensor, img: torch.Tensor, table: torch.Tensor, w: torch.Tensor, bias: torch.Tensor):
    """The last conv + pixel shuffle + input add: x fp16 [B, H, W, 64], img uint8 [B, H, W, 3], w fp16 [48, 3, 3, 64],
    bias fp32 [48] -> (uint8, fp32) [B, 4H, 4W, 3]."""
    B, h, wd, _ = x.shape
    out = torch.empty((B, SCALE * h, SCALE * wd, 3), dtype=torch.uint8, device=x.device)
    out_f = torch.empty(out.shape, dtype=torch.float32, device=x.device)
    L.call("irx_op_srvgg_tail", _stream(), _p(x.contiguous()), _p(img.contiguous()), B, h, wd, _p(table),
           _p(w.contiguous()), _p(bias), _p(out), _p(out_f))
    return out, out_f


def prelu(x: torch.Tensor, slope: torch.Tensor) -> torch.Tensor:
    """Per-channel PReLU of an fp32 or fp16 device tensor [..., C] (slope fp32 [C])."""
    out = torch.empty_like(x)
    L.call("irx_op_srvgg_prelu", _stream(), dtype_code(x.dtype), _p(x.contiguous()), x.numel() // x.shape[-1],
           x.shape[-1], _p(slope), _p(out))
    return out
