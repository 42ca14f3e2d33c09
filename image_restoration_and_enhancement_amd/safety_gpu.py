"""The Stable Diffusion safety checker on the GPU (csrc/safety_model.cpp, csrc/safety.hip, C ABI `irx_safety_*`): what
`run_safety_checker` does at the end of the reference's img2img calls (`src/inference.py:486, :566, :664`), on the
decoded uint8 batch while it is still on the device.

`SafetyChecker(weights_dir, dtype, device)` is a `NativeModel` of kind `IRX_MODEL_SAFETY`: `safety_host.load` reads and
checks the directory, the two embedding tables are normalised once on the host (fp64 -> fp32), everything is packed
through the manifest and bound once.  `check(images_u8)` resizes and crops with the Pillow-exact resample kernel — the
coefficient tables of the uncropped resize, sliced to the crop window, so the bytes are `CLIPImageProcessor`'s — and
runs the tower and the head; `apply` then zeroes the flagged images in place.  Everything is enqueued on the current
stream: the flags stay on the device, nothing here waits for it.  The tower runs in the engine dtype, as the reference
runs it in its pipeline dtype; the head is fp32.  `safety_host` is the oracle.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import resample
from . import safety_host as H
from .configs import SafetyConfig
from .engine import NativeModel, dtype_code

MAX_BATCH = 64            # SafetyChecker::kMaxBatch (csrc/models.h): larger batches run in chunks
MAX_EDGE_RATIO = 32       # longest input edge / crop side the sliced tables are handed to the kernel for
_MAX_SHAPES = 64


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sliced_tables(h: int, w: int, cfg: SafetyConfig):
    """Host tables of the resize + centre crop of an h x w image as one `irx_resample_u8` call: ((xbounds, xcoeffs),
    (ybounds, ycoeffs)) for the S output columns / rows of the crop window, each None where that axis is not resized.
    Cropping the output of Pillow's two-pass resize is slicing its tables: output pixel (y, x) of the crop is pixel
    (top + y, left + x) of the resize, whose horizontal taps depend on left + x alone and whose vertical taps on
    top + y alone; the horizontal temporary is rounded to uint8 per source row either way."""
    nh, nw, top, left = H.crop_window(h, w, cfg)
    S = cfg.crop_size
    xt = yt = None
    if nw != w:
        b, k = resample.coeffs(w, nw, "bicubic")
        xt = (np.ascontiguousarray(b[left:left + S]), np.ascontiguousarray(k[left:left + S]))
    if nh != h:
        b, k = resample.coeffs(h, nh, "bicubic")
        yt = (np.ascontiguousarray(b[top:top + S]), np.ascontiguousarray(k[top:top + S]))
    return xt, yt, (nh, nw, top, left)


class SafetyChecker(NativeModel):
    def __init__(self, weights_dir=None, dtype="fp16", device="cuda", cfg: Optional[SafetyConfig] = None,
                 weights: Optional[Dict[str, torch.Tensor]] = None, preprocessor_dir=None):
        """`weights_dir`: a `safety_checker/` directory (its `feature_extractor/` next to it, or `preprocessor_dir`).
        Tests pass `cfg` and `weights` (a checked state dict) instead."""
        if weights is None:
            cfg, weights = H.load(weights_dir, preprocessor_dir)
        else:
            weights = H.check_weights(weights, cfg)
        super().__init__(L.IRX_MODEL_SAFETY, cfg, dtype, device)
        sd = dict(weights)
        for k in ("special_care_embeds", "concept_embeds"):
            sd[k] = H.unit_rows(sd[k])
        self.load_state_dict(sd)
        self.source = str(weights_dir) if weights_dir is not None else "state dict"
        self.table = H.input_table(cfg).contiguous().to(self.device)
        self.rows = cfg.n_special + cfg.n_concepts
        self._prep: Dict[Tuple[int, int], tuple] = {}
        self._shape_ws: Dict[int, torch.Tensor] = {}

    # ---------------------------------------------------------------- preprocessing
    def _tables(self, h: int, w: int):
        t = self._prep.get((h, w))
        if t is None:
            S = self.cfg.crop_size
            nh, nw, top, left = H.crop_window(h, w, self.cfg)
            if max(h, w) > MAX_EDGE_RATIO * S or not resample.supported((w, h), (nw, nh), "bicubic"):
                t = ("host", None, None)
            else:
                xt, yt, _ = sliced_tables(h, w, self.cfg)
                dev = lambda a: None if a is None else tuple(torch.from_numpy(x).to(self.device) for x in a)
                t = ("crop" if xt is None and yt is None else "kernel", dev(xt), dev(yt), (top, left))
            while len(self._prep) >= _MAX_SHAPES:
                self._prep.pop(next(iter(self._prep)))
            self._prep[(h, w)] = t
        return t

    def preprocess_u8(self, images_u8: torch.Tensor) -> torch.Tensor:
        """uint8 [B, H, W, 3] on the device -> the resized, cropped uint8 [B, S, S, 3] (`CLIPImageProcessor`'s bytes)."""
        B, h, w, _ = images_u8.shape
        S = self.cfg.crop_size
        t = self._tables(h, w)
        if t[0] == "host":      # a ratio past the kernel's range: Pillow on the host, as resample.resize_pil does
            a = images_u8.cpu().numpy()
            return torch.from_numpy(np.stack([H.preprocess_u8(x, self.cfg) for x in a])).to(self.device)
        _, xt, yt, (top, left) = t
        if t[0] == "crop":      # nothing to resize: the crop window alone
            return images_u8[:, top:top + S, left:left + S].contiguous()
        out = torch.empty((B, S, S, 3), dtype=torch.uint8, device=self.device)
        # an axis that is not resized can still be cropped: the kernel copies rows / columns [0, S) of it, so the
        # window is cut first
        src = images_u8
        if xt is None:
            src = src[:, :, left:left + S]
        if yt is None:
            src = src[:, top:top + S]
        src = src.contiguous()
        L.call("irx_resample_u8", _stream(), _p(src), B, src.shape[1], src.shape[2], 3,
               _p(xt[0]) if xt else None, _p(xt[1]) if xt else None, xt[1].shape[1] if xt else 0,
               _p(yt[0]) if yt else None, _p(yt[1]) if yt else None, yt[1].shape[1] if yt else 0, S, S, _p(out))
        return out

    # ---------------------------------------------------------------- the model
    def _workspace(self, B: int) -> torch.Tensor:
        ws = self._shape_ws.get(B)
        if ws is None:
            ws = torch.empty(max(self._size("irx_safety_workspace_bytes", B), 256), dtype=torch.uint8,
                             device=self.device)
            self._shape_ws[B] = ws
        return ws

    def _images(self, images_u8) -> torch.Tensor:
        x = torch.from_numpy(np.ascontiguousarray(images_u8)).to(self.device) if isinstance(images_u8, np.ndarray) \
            else images_u8
        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or not x.is_cuda or x.dim() != 4 \
                or x.shape[-1] != 3 or min(x.shape) < 1:
            raise ValueError("images: expected uint8 RGB [B, H, W, 3] (numpy, or a tensor on the device)")
        return x

    def check_crops(self, crops: torch.Tensor):
        """uint8 [B, S, S, 3] (already resized and cropped) -> (scores fp32 [B, rows], flags int32 [B]), device."""
        B = crops.shape[0]
        scores = torch.empty((B, self.rows), dtype=torch.float32, device=self.device)
        flags = torch.empty((B,), dtype=torch.int32, device=self.device)
        crops = crops.contiguous()
        for i in range(0, B, MAX_BATCH):
            n = min(MAX_BATCH, B - i)
            ws = self._workspace(n)
            L.call("irx_safety_check_u8", self.h, _stream(), _p(crops[i:]), n, _p(self.table), _p(scores[i:]),
                   _p(flags[i:]), _p(ws), ws.numel())
        return scores, flags

    def embeds_crops(self, crops: torch.Tensor) -> torch.Tensor:
        """The fp32 image embeddings [B, projection_dim] the head reads (tests)."""
        B = crops.shape[0]
        out = torch.empty((B, self.cfg.projection_dim), dtype=torch.float32, device=self.device)
        crops = crops.contiguous()
        for i in range(0, B, MAX_BATCH):
            n = min(MAX_BATCH, B - i)
            ws = self._workspace(n)
            L.call("irx_safety_embed_u8", self.h, _stream(), _p(crops[i:]), n, _p(self.table), _p(out[i:]), _p(ws),
                   ws.numel())
        return out

    def check(self, images_u8):
        """uint8 RGB [B, H, W, 3] -> (scores fp32 [B, n_special + n_concepts], the unrounded cosines with the
        special-care rows first; flags int32 [B]), both on the device."""
        return self.check_crops(self.preprocess_u8(self._images(images_u8)))

    def apply(self, images_u8: torch.Tensor, f01: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`check`, then every flagged image of `images_u8` (and of its fp32 [0, 1] copy `f01`) zeroed in place: the
        black image `run_safety_checker` returns.  The flags (int32 [B], device) are returned, not read."""
        x = self._images(images_u8)
        if not x.is_contiguous() or (f01 is not None and (not f01.is_contiguous() or f01.dtype != torch.float32
                                                          or tuple(f01.shape) != tuple(x.shape))):
            raise ValueError("apply: contiguous uint8 images and a contiguous float32 copy of the same shape")
        _, flags = self.check(x)
        B, h, w, _ = x.shape
        for i in range(0, B, 65535):
            n = min(65535, B - i)
            L.call("irx_safety_blank_u8", _stream(), _p(x[i:]), None if f01 is None else _p(f01[i:]), n, h, w,
                   _p(flags[i:]))
        return flags


# ---- the kernels on their own (tests)
def patches(crops: torch.Tensor, table: torch.Tensor, patch: int, kpad: int, dtype, out: torch.Tensor) -> torch.Tensor:
    B, S = crops.shape[0], crops.shape[1]
    L.call("irx_op_safety_patches", _stream(), dtype_code(dtype), _p(crops), B, S, patch, kpad, _p(table), _p(out))
    return out


def tokens(patch_out: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    B, P, D = patch_out.shape
    L.call("irx_op_safety_tokens", _stream(), dtype_code(patch_out.dtype), _p(patch_out), _p(cls), _p(pos), B, P, D,
           _p(out))
    return out


def head(embeds, special, concepts, thr_special, thr_concepts, scores, flags):
    B, n = embeds.shape
    L.call("irx_op_safety_head", _stream(), _p(embeds), B, n, _p(special), special.shape[0], _p(concepts),
           concepts.shape[0], _p(thr_special), _p(thr_concepts), _p(scores), _p(flags))
    return scores, flags


def blank(images_u8: torch.Tensor, f01: Optional[torch.Tensor], flags: torch.Tensor, B: int, h: int, w: int) -> None:
    L.call("irx_safety_blank_u8", _stream(), _p(images_u8), _p(f01), B, h, w, _p(flags))
