"""LPIPS(alex) on the GPU (csrc/lpips_model.cpp, csrc/lpips.hip, C ABI `irx_lpips_u8`): what
`MetricsCalculator.calculate_lpips` of the reference computes (`src/metrics.py:97-111`), on uint8 device tensors.

`LpipsAlex(weights)` is a `NativeModel` of kind `IRX_MODEL_LPIPS`: the weights (`lpips_host.load_weights`) are packed
and bound once, the input table (`lpips_host.input_table`, the restatement's own float32 expression) is uploaded once,
and the workspace is kept per shape.  `score` enqueues on the current stream and returns device float64 tensors; nothing
here waits for the device.  `lpips_host.lpips_alex(..., dtype=torch.float64)` is the oracle.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from . import _lib as L
from . import lpips_host as H
from .engine import NativeModel

MIN_SIDE = H.MIN_SIDE
_MAX_SHAPES = 64


def supported(shape) -> bool:
    """Whether uint8 images of this shape ([H, W, 3] or [B, H, W, 3]) are inside the model's range."""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 4:
        if shape[0] < 1:
            return False
        shape = shape[1:]
    return len(shape) == 3 and shape[2] == 3 and min(shape[:2]) >= MIN_SIDE


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class LpipsAlex(NativeModel):
    def __init__(self, weights: Dict[str, torch.Tensor], device="cuda"):
        super().__init__(L.IRX_MODEL_LPIPS, None, L.IRX_F32, device)
        self.load_state_dict(H.check_weights(weights))
        self.table = H.input_table().to(self.device)
        self._shape_ws: Dict[tuple, torch.Tensor] = {}

    def workspace_bytes(self, batch: int, h: int, w: int) -> int:
        return self._size("irx_lpips_workspace_bytes", batch, h, w)

    def _workspace(self, B: int, h: int, w: int) -> torch.Tensor:
        ws = self._shape_ws.get((B, h, w))
        if ws is None:
            while len(self._shape_ws) >= _MAX_SHAPES:
                self._shape_ws.pop(next(iter(self._shape_ws)))
            ws = torch.empty(max(self.workspace_bytes(B, h, w), 256), dtype=torch.uint8, device=self.device)
            self._shape_ws[(B, h, w)] = ws
        return ws

    def score(self, pred: torch.Tensor, gt: torch.Tensor, layers: bool = False):
        """pred, gt: uint8 device tensors [H, W, 3] or [B, H, W, 3] of one shape -> device float64 [B] (and the five
        taps' terms [B, 5] with `layers`).  Enqueues and returns."""
        for x, what in ((pred, "pred"), (gt, "gt")):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or not x.is_cuda or x.dim() not in (3, 4):
                raise ValueError(f"{what}: expected a uint8 CUDA tensor [H, W, 3] or [B, H, W, 3]")
        if pred.shape != gt.shape:
            raise ValueError("Input images must have the same dimensions.")
        if not supported(pred.shape):
            raise ValueError(f"LPIPS(alex): shape {tuple(pred.shape)} outside the model's range "
                             f"(3 channels, H, W >= {MIN_SIDE})")
        p = pred.contiguous() if pred.dim() == 4 else pred.contiguous()[None]
        g = gt.contiguous() if gt.dim() == 4 else gt.contiguous()[None]
        B, h, w, _ = p.shape
        ws = self._workspace(B, h, w)
        total = torch.empty(B, dtype=torch.float64, device=self.device)
        lay = torch.empty((B, 5), dtype=torch.float64, device=self.device) if layers else None
        L.call("irx_lpips_u8", self.h, self.stream(), _p(p), _p(g), B, h, w, _p(self.table), _p(total), _p(lay),
               _p(ws), ws.numel())
        return (total, lay) if layers else total

    # ---- the two data-movement kernels on their own (tests)
    def input_tensor(self, pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
        """The trunk's input for uint8 [B, H, W, 3] pred and gt: float32 [2B, H, W, 4], pred first, channel 3 zero."""
        B, h, w, _ = pred.shape
        out = torch.empty((2 * B, h, w, 4), dtype=torch.float32, device=self.device)
        L.call("irx_op_lpips_input", self.stream(), _p(pred.contiguous()), _p(gt.contiguous()), B, h, w,
               _p(self.table), _p(out))
        return out


def relu_pool(x: torch.Tensor, win: int, stride: int) -> torch.Tensor:
    """ReLU, then a win x win / stride max pool without padding, of a float32 NHWC device tensor [N, H, W, C]."""
    N, h, w, c = x.shape
    out = torch.empty((N, (h - win) // stride + 1, (w - win) // stride + 1, c), dtype=torch.float32, device=x.device)
    L.call("irx_op_lpips_relu_pool", C.c_void_p(torch.cuda.current_stream().cuda_stream), _p(x.contiguous()), N, h, w,
           c, win, stride, _p(out))
    return out
