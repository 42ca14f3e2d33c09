"""FID features on the GPU (csrc/fid_model.cpp, csrc/fid.hip, C ABI `irx_fid_features`): what
`MetricsCalculator._get_inception_features` of the reference computes (`src/metrics.py:150-162`), on uint8 device
tensors.

`InceptionFeatures(weights)` is a `NativeModel` of kind `IRX_MODEL_FID`: the weights (`fid_host.load_weights`) are
packed and bound once, with every BatchNorm folded into a scale / shift pair on the host (`fid_host.fold_bn`); the
resize tap tables (`fid_host.aa_taps`) are uploaded once per source size; the workspace is kept per chunk size.
`features` and `FeatureQueue` enqueue on the current stream and return device tensors; nothing here waits for the
device.  `fid_host.inception_features(..., dtype=torch.float64)` is the oracle.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List

import torch

from . import _lib as L
from . import fid_host as H
from .engine import NativeModel

SIDE = H.SIDE
FEATURES = H.FEATURES
CHUNK = 32                # images per trunk call at the most
_MAX_TABLES = 64


def supported(shape) -> bool:
    """Whether a uint8 image of this shape is inside the input kernel's range: [H, W, 3], both sides positive."""
    shape = tuple(int(v) for v in shape)
    return len(shape) == 3 and shape[2] == 3 and min(shape[:2]) >= 1


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class InceptionFeatures(NativeModel):
    def __init__(self, weights: Dict[str, torch.Tensor], device="cuda"):
        if not H.ANTIALIAS:
            raise RuntimeError("the GPU input kernel implements the antialiased resize only (fid_host.ANTIALIAS)")
        super().__init__(L.IRX_MODEL_FID, None, L.IRX_F32, device)
        self.load_state_dict(H.fold_bn(H.check_weights(weights)))
        self._tables: Dict[int, tuple] = {}
        self._chunk_ws: Dict[int, torch.Tensor] = {}

    # ---- sizes and tables
    def workspace_bytes(self, batch: int, h: int = SIDE, w: int = SIDE) -> int:
        return self._size("irx_fid_workspace_bytes", batch, h, w)

    def _workspace(self, B: int) -> torch.Tensor:
        ws = self._chunk_ws.get(B)
        if ws is None:
            ws = torch.empty(max(self.workspace_bytes(B), 256), dtype=torch.uint8, device=self.device)
            self._chunk_ws[B] = ws
        return ws

    def _taps(self, n: int):
        """Device (start, count, weights, kmax) of one axis of length n."""
        t = self._tables.get(n)
        if t is None:
            while len(self._tables) >= _MAX_TABLES:
                self._tables.pop(next(iter(self._tables)))
            start, count, w, kmax = H.aa_taps(n, SIDE)
            t = (torch.from_numpy(start).to(self.device), torch.from_numpy(count).to(self.device),
                 torch.from_numpy(w).contiguous().to(self.device), kmax)
            self._tables[n] = t
        return t

    # ---- the pieces
    def input_into(self, img: torch.Tensor, slot: torch.Tensor) -> None:
        """uint8 device [H, W, 3] -> float32 [299, 299, 4] `slot` (a contiguous view): ToTensor, Resize, Normalize."""
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or not img.is_cuda or not supported(img.shape):
            raise ValueError("FID input: expected a uint8 CUDA tensor [H, W, 3]")
        if not isinstance(slot, torch.Tensor) or slot.dtype != torch.float32 or not slot.is_cuda \
                or tuple(slot.shape) != (SIDE, SIDE, 4) or not slot.is_contiguous() or slot.device != img.device:
            raise ValueError("FID input: the slot must be a contiguous float32 [299, 299, 4] tensor on the image's device")
        img = img.contiguous()
        h, w, _ = img.shape
        xs, xn, xw, kx = self._taps(w)
        ys, yn, yw, ky = self._taps(h)
        L.call("irx_op_fid_input", self.stream(), _p(img), h, w, _p(xs), _p(xn), _p(xw), kx, _p(ys), _p(yn), _p(yw),
               ky, _p(slot))

    def trunk(self, x: torch.Tensor) -> torch.Tensor:
        """float32 device NHWC4 [B, h, w, 4] (channel 3 zero, h, w >= 75) -> float32 [B, 2048].  The workspace is
        cached per chunk size for the metric's own 299 x 299 input and sized per call for any other."""
        B, h, w, c = x.shape
        if c != 4 or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("FID trunk: expected contiguous float32 [B, h, w, 4]")
        if (h, w) == (SIDE, SIDE):
            ws = self._workspace(B)
        else:
            ws = torch.empty(max(self.workspace_bytes(B, h, w), 256), dtype=torch.uint8, device=self.device)
        out = torch.empty((B, FEATURES), dtype=torch.float32, device=self.device)
        L.call("irx_fid_features", self.h, self.stream(), _p(x), B, h, w, _p(out), _p(ws), ws.numel())
        return out

    def features(self, images: List[torch.Tensor]) -> torch.Tensor:
        """uint8 device images [H, W, 3] of any sizes -> device float32 [N, 2048].  Enqueues and returns."""
        q = FeatureQueue(self)
        for im in images:
            q.add(im)
        return q.finish()


class FeatureQueue:
    """Images in, features out, without keeping the images: each image is resized into a slot of one
    [CHUNK, 299, 299, 4] buffer as it arrives, and the trunk runs whenever the buffer is full (and once more in
    `finish`).  An image's features do not depend on its slot or on the chunk size, so the result is the same as
    scoring every image alone."""

    def __init__(self, net: InceptionFeatures, chunk: int = CHUNK):
        self.net = net
        self.chunk = int(chunk)
        self.buf = torch.empty((self.chunk, SIDE, SIDE, 4), dtype=torch.float32, device=net.device)
        self.n = 0
        self.out: List[torch.Tensor] = []

    def add(self, img: torch.Tensor) -> None:
        self.net.input_into(img, self.buf[self.n])
        self.n += 1
        if self.n == self.chunk:
            self._flush()

    def _flush(self) -> None:
        if self.n:
            self.out.append(self.net.trunk(self.buf[:self.n]))
            self.n = 0
            # the trunk call above reads the buffer in stream order; the next chunk's input kernels come after it

    def __len__(self) -> int:
        return self.n + sum(int(t.shape[0]) for t in self.out)

    def finish(self) -> torch.Tensor:
        self._flush()
        if not self.out:
            return torch.empty((0, FEATURES), dtype=torch.float32, device=self.net.device)
        return self.out[0] if len(self.out) == 1 else torch.cat(self.out, 0)


# ---- the glue kernels on their own (tests)
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bn_relu(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, out: torch.Tensor = None, coff: int = 0):
    """max(x * scale + shift, 0) of float32 NHWC x [..., C] into channels [coff, coff + C) of `out` [..., ldo]
    (a new tensor of x's shape when `out` is None)."""
    x = x.contiguous()
    Cn = x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    L.call("irx_op_fid_bn_relu", _stream(), _p(x), x.numel() // Cn, Cn, _p(scale.contiguous()),
           _p(shift.contiguous()), _p(out), out.shape[-1], coff)
    return out


def avgpool3(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    N, h, w, c = x.shape
    out = torch.empty_like(x)
    L.call("irx_op_fid_avgpool3", _stream(), _p(x), N, h, w, c, _p(out))
    return out


def maxpool3s2(x: torch.Tensor, out: torch.Tensor = None, coff: int = 0) -> torch.Tensor:
    x = x.contiguous()
    N, h, w, c = x.shape
    if out is None:
        out = torch.empty((N, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c), dtype=torch.float32, device=x.device)
    L.call("irx_op_fid_maxpool3s2", _stream(), _p(x), N, h, w, c, _p(out), out.shape[-1], coff)
    return out


def gap(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    N, h, w, c = x.shape
    out = torch.empty((N, c), dtype=torch.float32, device=x.device)
    L.call("irx_op_fid_gap", _stream(), _p(x), N, h * w, c, _p(out))
    return out
