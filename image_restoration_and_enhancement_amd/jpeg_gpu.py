"""Baseline JPEG files from uint8 device batches: what `PIL.Image.save(path)` writes for a `.jpg` name
(scripts/generate_predictions.py:83-84), byte for byte, without moving the pixels to the host.

`encode` runs the kernels of csrc/jpeg_encode.hip (`irx_jpeg_encode`: libjpeg's integer chain up to the quantiser,
then a Huffman coder with one wavefront per 8x8 block, bit placement by prefix sums and byte stuffing) and copies
back one array of lengths and then the used bytes only; the 623 header bytes (`irx_jpeg_header`) and the EOI marker
are added on the host.  A CPU tensor goes through `jpeg_host.encode`, the numpy statement of the same coder.

Out of scope: grayscale (`L`) files, PNG, optimised or progressive JPEG, other subsamplings, decoding.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import List, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from . import degrade_host as DH
from . import jpeg_host as JH

# device memory one irx_jpeg_encode call may ask for (workspace + output at their worst-case bounds): larger
# batches are encoded in slices
MAX_CALL_BYTES = 2 << 30


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _qualities(quality, B: int) -> List[int]:
    qs = [int(quality)] * B if np.isscalar(quality) else [int(q) for q in quality]
    if len(qs) != B:
        raise ValueError("one quality, or one per image")
    return qs


def header(H: int, W: int, quality: int) -> bytes:
    """The bytes in front of the scan, from the library (`jpeg_host.header` is the same bytes in numpy)."""
    qt = np.ascontiguousarray(DH.jpeg_quant_tables(quality), dtype=np.int32)
    buf = (C.c_uint8 * 1024)()
    n = L.call("irx_jpeg_header", H, W, qt.ctypes.data_as(C.c_void_p), C.cast(buf, C.c_void_p), len(buf))
    return bytes(buf[:n])


def _encode_device(x: torch.Tensor, qs: Sequence[int], rgb: bool) -> List[bytes]:
    B, H, W, _ = x.shape
    qt = torch.from_numpy(np.stack([DH.jpeg_quant_tables(q) for q in qs])).to(x.device)
    bound = int(L.call("irx_jpeg_encode_bound", H, W))
    if bound <= 0:
        raise L.IrxError(f"irx_jpeg_encode: 8 <= H, W <= 65535 (got {H} x {W})")
    nws = int(L.call("irx_jpeg_encode_ws_bytes", B, H, W))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
    out = torch.empty((B, bound), dtype=torch.uint8, device=x.device)
    lens = torch.empty(B, dtype=torch.int32, device=x.device)
    L.call("irx_jpeg_encode", _s(), _p(x), B, H, W, _p(qt), int(rgb), _p(ws), _p(out), bound, _p(lens))
    n = lens.cpu().tolist()                                            # D2H 1: the lengths
    data = torch.cat([out[b, :n[b]] for b in range(B)]).cpu().numpy().tobytes()   # D2H 2: the used bytes
    files, at = [], 0
    heads = {}
    for b in range(B):
        if qs[b] not in heads:
            heads[qs[b]] = header(H, W, qs[b])
        files.append(heads[qs[b]] + data[at:at + n[b]] + b"\xff\xd9")
        at += n[b]
    return files


def encode(batch_u8: torch.Tensor, quality: Union[int, Sequence[int]] = 75, rgb: bool = True) -> List[bytes]:
    """uint8 [B][H][W][3] or [H][W][3] -> one baseline JPEG file per image (a list even for a single image), each
    equal to `Image.fromarray(img).save(f, "JPEG", quality=q)`.  `quality`: one int, or one per image.  rgb=False:
    the tensor is in B,G,R order (the file is the same)."""
    if batch_u8.dtype != torch.uint8 or batch_u8.dim() not in (3, 4) or batch_u8.shape[-1] != 3:
        raise ValueError("expected a uint8 tensor [B][H][W][3] or [H][W][3]")
    x = (batch_u8 if batch_u8.dim() == 4 else batch_u8[None]).contiguous()
    B, H, W, _ = x.shape
    qs = _qualities(quality, B)
    if B == 0:
        return []
    if not x.is_cuda:
        xs = x.numpy()
        return [JH.encode(xs[b], qs[b], rgb) for b in range(B)]
    per = int(L.call("irx_jpeg_encode_ws_bytes", 1, H, W)) + int(L.call("irx_jpeg_encode_bound", H, W))
    step = max(1, MAX_CALL_BYTES // max(per, 1))
    files: List[bytes] = []
    for b0 in range(0, B, step):
        files += _encode_device(x[b0:b0 + step], qs[b0:b0 + step], rgb)
    return files


def save(batch_u8: torch.Tensor, paths: Sequence[Union[str, Path]], quality: Union[int, Sequence[int]] = 75) -> None:
    """Write image b (R,G,B order) to paths[b] as `Image.save(path, quality=quality)` would for a .jpg name."""
    files = encode(batch_u8, quality)
    if len(files) != len(paths):
        raise ValueError("one path per image")
    for f, p in zip(files, paths):
        Path(p).write_bytes(f)
