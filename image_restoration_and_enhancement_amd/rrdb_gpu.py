"""Real-ESRGAN's RRDBNet on the GPU (csrc/rrdb_model.cpp, csrc/rrdb.hip, C ABI `irx_rrdb_u8`): what
`RestorationPipeline._sr_realesrgan` of the reference would get from `model.enhance(img, outscale=4)`
(`src/inference.py:579-591`) had its strict load of `RealESRGAN_x4plus.pth` (`:335-346`) succeeded, on uint8 device
tensors.

`RealESRGANx4plus(weights)` is a `NativeModel` of kind `IRX_MODEL_RRDB`: the weights (`rrdb_host.load_weights`) are
packed through the manifest and bound once, the input table (`srvgg_host.input_table`) is uploaded once, and the
workspace is kept per shape.  `dtype="fp16"` is the product (the reference's `half` on a GPU), `"fp32"` the parity
engine.  `enhance` enqueues on the current stream and returns a device tensor; nothing here waits for the device.
`rrdb_host.forward(..., dtype=torch.float64)` is the ground truth, with `half=True` the oracle of the fp16 engine
(DESIGN.md §24).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import rrdb_host as H
from .engine import NativeModel, dtype_code

SCALE = H.UPSCALE
_MAX_SHAPES = 64


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class RRDBConfig:
    """What `engine.model_config` reads for `IRX_MODEL_RRDB`."""

    def __init__(self, num_block: int = H.NUM_BLOCK, num_feat: int = H.NUM_FEAT, num_grow_ch: int = H.NUM_GROW):
        self.num_block, self.num_feat, self.num_grow_ch = int(num_block), int(num_feat), int(num_grow_ch)


class RealESRGANx4plus(NativeModel):
    def __init__(self, weights: Dict[str, torch.Tensor], device="cuda", dtype="fp16"):
        if dtype_code(dtype) not in (L.IRX_F16, L.IRX_F32):
            raise ValueError("RealESRGANx4plus: dtype 'fp16' or 'fp32'")
        weights = H.check_weights(weights)
        super().__init__(L.IRX_MODEL_RRDB, RRDBConfig(H.num_blocks(weights)), dtype, device)
        self.load_state_dict(weights)
        self.table = H.input_table().to(self.device)
        self._shape_ws: Dict[tuple, torch.Tensor] = {}

    def workspace_bytes(self, batch: int, h: int, w: int) -> int:
        return self._size("irx_rrdb_workspace_bytes", batch, h, w)

    def _workspace(self, B: int, h: int, w: int) -> torch.Tensor:
        need = max(self.workspace_bytes(B, h, w), 256)      # (it depends on the rrdb_fused option)
        ws = self._shape_ws.get((B, h, w))
        if ws is None or ws.numel() < need:
            while len(self._shape_ws) >= _MAX_SHAPES:
                self._shape_ws.pop(next(iter(self._shape_ws)))
            self._shape_ws.pop((B, h, w), None)
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
        L.call("irx_rrdb_u8", self.h, self.stream(), _p(xb), B, h, w, _p(self.table), _p(out), _p(out_f), _p(ws),
               ws.numel())
        return out, out_f

    def enhance(self, images, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 RGB [H, W, 3] or [B, H, W, 3] -> the uint8 x4 result on the device, [4H, 4W, 3] or [B, 4H, 4W, 3].
        `out`: a contiguous uint8 tensor of that shape to write into (e.g. a slice of a batch tensor)."""
        return self._run(images, out, False)[0]

    def forward_float(self, images):
        """(uint8 result, fp32 result before the clamp), both NHWC on the device (tests)."""
        return self._run(images, None, True)


# ---- the body kernel on its own (tests)
def body_conv(x: torch.Tensor, cin: int, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, lrelu: bool = False,
              res1: Optional[torch.Tensor] = None, res1_scaled: bool = True,
              res2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One conv of a dense block.  x: fp16 [B, H, W, ldx] (channels [0, cin) are read); w: fp16 [cout, 3, 3, cin]
    (O, KH, KW, I); bias fp32 [cout]; out / res1 / res2: fp16 views [B, H, W, cout] whose last dimension is a channel
    slice of a wider NHWC buffer (pixel stride `stride(2)`).  Writes `out` and returns it."""
    B, h, wd, ldx = x.shape
    cout = w.shape[0]

    def ld(t):
        assert t.shape == (B, h, wd, cout) and t.stride(3) == 1 and t.stride(1) == wd * t.stride(2) \
            and t.stride(0) == h * wd * t.stride(2)
        return t.stride(2)

    assert x.is_contiguous() and w.is_contiguous()
    L.call("irx_op_rrdb_conv", C.c_void_p(torch.cuda.current_stream().cuda_stream), _p(x), ldx, cin, B, h, wd, _p(w),
           _p(bias), cout, int(lrelu), _p(res1), 0 if res1 is None else ld(res1), int(res1_scaled), _p(res2),
           0 if res2 is None else ld(res2), _p(out), ld(out))
    return out
