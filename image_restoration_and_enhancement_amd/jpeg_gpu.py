"""Baseline JPEG files from uint8 device batches: what `PIL.Image.save(path)` writes for a `.jpg` name
(scripts/generate_predictions.py:83-84), byte for byte, without moving the pixels to the host.

`encode` runs the kernels of csrc/jpeg_encode.hip (`irx_jpeg_encode`: libjpeg's integer chain up to the quantiser,
then a Huffman coder with one wavefront per 8x8 block, bit placement by prefix sums and byte stuffing) and copies
back one array of lengths and then the used bytes only; the 623 header bytes (`irx_jpeg_header`) and the EOI marker
are added on the host.  A CPU tensor goes through `jpeg_host.encode`, the numpy statement of the same coder.

`decode` is the other direction, `PIL.Image.open(path).convert("RGB")` (the reference's src/metrics.py:40-46 and
scripts/generate_predictions.py:68) with the pixels born on the device: the host walks the markers
(`irx_jpeg_parse`), the entropy-coded bytes of the whole batch go up in one copy, `irx_jpeg_decode`
(csrc/jpeg_decode.hip: a self-synchronising Huffman decoder, then the pixel half of the JPEG round trip) writes the
images, and one array of statuses comes back.  A file outside the contract (anything but baseline 8-bit 4:2:0 or
grayscale, one scan, no restart markers) or with a non-zero status is decoded by PIL instead and uploaded, so
the call returns what PIL returns or raises what PIL raises; `last_fallbacks` names those files.

Out of scope of the encoder: grayscale (`L`) files, PNG, optimised or progressive JPEG, other subsamplings.
"""
from __future__ import annotations

import ctypes as C
import io
import os
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


# ------------------------------------------------------------------------------------------------ decoding
# indices (into the `files` of the last `decode` call) that PIL decoded: refused by the parser, or a non-zero status
last_fallbacks: List[int] = []
# the statuses behind them: the parser's negative status, or the decoder's positive one
last_fallback_status: List[int] = []


def parse(data: bytes):
    """`irx_jpeg_parse` on a file -> (status, JpegInfo): status 0, or a negative refusal (include/irx.h)."""
    info = L.JpegInfo()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")
    st = L.load().irx_jpeg_parse(C.cast(buf, C.c_void_p), len(data), C.byref(info))
    return int(st), info


def _read(f) -> bytes:
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    return Path(os.fspath(f)).read_bytes()


def _pil_pixels(data: bytes, mode: str) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert(mode))


def _shape(info, mode: str):
    return (info.H, info.W, 3) if mode == "RGB" else (info.H, info.W)


def decode_device(datas: Sequence[bytes], infos, mode: str, device, subseq_bits: int = 0, want_coef: bool = False):
    """`irx_jpeg_decode` on parsed files: -> (images, status list, rounds list[, coefficient tensors]).  One H2D copy
    of the scans, one D2H copy of status and rounds."""
    B = len(datas)
    arr = (L.JpegInfo * B)(*infos)
    lens = [int(i.scan_len) for i in infos]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    host = np.empty(int(offs[-1]), np.uint8)
    for b, (d, i) in enumerate(zip(datas, infos)):
        host[offs[b]:offs[b + 1]] = np.frombuffer(d, np.uint8, lens[b], int(i.scan_off))
    scans = torch.from_numpy(host).to(device)                                  # H2D: the entropy-coded bytes
    nws = int(L.call("irx_jpeg_decode_ws_bytes", C.cast(arr, C.c_void_p), B, subseq_bits))
    if nws <= 0:
        raise L.IrxError("irx_jpeg_decode: refused arguments")
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    ch = 3 if mode == "RGB" else 1
    sizes = [i.H * i.W * ch for i in infos]
    ooff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = torch.empty(int(ooff[-1]), dtype=torch.uint8, device=device)
    sr = torch.empty((2, B), dtype=torch.int32, device=device)
    coef, coff = None, None
    if want_coef:
        nb = [_nblocks(i) * 64 for i in infos]
        coff = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
        coef = torch.empty(int(coff[-1]), dtype=torch.int16, device=device)
    with torch.cuda.device(scans.device):
        L.call("irx_jpeg_decode", _s(), _p(scans), offs.ctypes.data_as(C.c_void_p), C.cast(arr, C.c_void_p), B,
               subseq_bits, int(mode == "RGB"), _p(ws), _p(out), ooff.ctypes.data_as(C.c_void_p), _p(sr[0]), _p(sr[1]),
               _p(coef) if want_coef else None, coff.ctypes.data_as(C.c_void_p) if want_coef else None)
    srh = sr.cpu().tolist()                                                    # D2H: status and rounds
    imgs = [out[ooff[b]:ooff[b + 1]].view(_shape(infos[b], mode)) for b in range(B)]
    if want_coef:
        return imgs, srh[0], srh[1], [coef[coff[b]:coff[b + 1]].view(-1, 64) for b in range(B)]
    return imgs, srh[0], srh[1]


def _nblocks(info) -> int:
    if info.ncomp == 3:
        return 6 * (-(-info.H // 16)) * (-(-info.W // 16))
    return (-(-info.H // 8)) * (-(-info.W // 8))


def decode(files: Sequence[Union[bytes, str, Path]], mode: str = "RGB", device="cuda",
           subseq_bits: int = 0) -> List[torch.Tensor]:
    """JPEG files (bytes or paths) -> uint8 tensors on `device`, in input order: [H][W][3] for mode "RGB", [H][W] for
    mode "L"; each equal to `np.asarray(PIL.Image.open(f).convert(mode))`.  Files the device decoder does not take
    (see the head of this module; for mode "L" also every colour file) go through PIL; what PIL raises is raised.
    On a CPU device the pixels come from `jpeg_host.decode` / PIL."""
    global last_fallbacks, last_fallback_status
    if mode not in ("RGB", "L"):
        raise ValueError("mode 'RGB' or 'L'")
    device = torch.device(device)
    datas = [_read(f) for f in files]
    res: List[torch.Tensor] = [None] * len(datas)
    fallbacks, statuses = {}, {}
    if device.type != "cuda":
        for b, d in enumerate(datas):
            try:
                info = JH.parse(d)
                if mode == "L" and info["ncomp"] != 1:
                    raise JH.Refused(JH.E_COMPONENTS, "mode L of a colour file")
                res[b] = torch.from_numpy(JH.pixels(JH.decode_coefficients(d, info), info, mode))
            except JH.Refused as e:
                fallbacks[b] = e.status
                res[b] = torch.from_numpy(_pil_pixels(d, mode))
        last_fallbacks, last_fallback_status = sorted(fallbacks), [fallbacks[b] for b in sorted(fallbacks)]
        return res
    good, infos = [], []
    for b, d in enumerate(datas):
        st, info = parse(d)
        if st == 0 and mode == "L" and info.ncomp != 1:
            st = JH.E_COMPONENTS
        if st == 0:
            good.append(b)
            infos.append(info)
        else:
            fallbacks[b] = st
    if good:
        imgs, status, _ = decode_device([datas[b] for b in good], infos, mode, device, subseq_bits)
        for j, b in enumerate(good):
            if status[j]:
                fallbacks[b] = status[j]
            else:
                res[b] = imgs[j]
    for b in sorted(fallbacks):
        res[b] = torch.from_numpy(_pil_pixels(datas[b], mode)).to(device)
    last_fallbacks, last_fallback_status = sorted(fallbacks), [fallbacks[b] for b in sorted(fallbacks)]
    return res


def open(path: Union[str, Path, bytes], mode: str = "RGB", device="cuda") -> torch.Tensor:
    """`decode` of a single file."""
    return decode([path], mode, device)[0]
