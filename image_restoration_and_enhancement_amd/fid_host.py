"""FID on the host — a plain-torch restatement of what the reference's `MetricsCalculator` computes
(`src/metrics.py:70-80`, `:150-223`): torchvision's `inception_v3(transform_input=False)` in eval mode with
`fc = Identity`, fed through `ToTensor`, `Resize((299, 299))` on the tensor and `Normalize`, and the Fréchet distance
of the two feature sets.

No torchvision: the trunk is written out here and the weights come from the `inception_v3_google-*.pth` state dict
the user already has (`AuxLogits.*`, `fc.*` and `num_batches_tracked` are ignored).

* input:   uint8 RGB HWC -> `float32(v) / 255`, CHW (`ToTensor`)
* resize:  `F.interpolate(size=(299, 299), mode="bilinear", align_corners=False, antialias=ANTIALIAS)` — what
           `transforms.Resize` does to a tensor.  torchvision >= 0.17 antialiases by default, 0.16 (the oldest release
           the reference's requirements.txt admits) did not; `ANTIALIAS` below is the one place that decides, and it
           follows the current behaviour.  The GPU input kernel implements antialias=True only (`aa_taps`).
* normalise: `(x - mean) / std` with the ImageNet constants as float32 tensors
* trunk:   every unit is conv (no bias) -> BatchNorm(eps=1e-3, running statistics) -> ReLU; `UNITS` lists them in
           forward order; `inception_features` is the graph
* FID:     `frechet_distance` — mean in float32, `np.cov` in float64, `scipy.linalg.sqrtm` — line for line

`inception_features(..., dtype=torch.float64)` is the ground truth of the tests; `dtype=torch.float32` serves
`MetricsCalculator(device="cpu")`.  The GPU path (`fid_gpu`, csrc/fid_model.cpp, csrc/fid.hip) reads `UNITS`' shapes
through the native manifest, `fold_bn` for its scale / shift vectors and `aa_taps` for the resize tables.

This restatement is not pinned against torchvision: neither the package nor the checkpoint is available offline, so
parity with it rests on reading its source (parity unpinned, like `lpips_host`).
"""
from __future__ import annotations

import math
from functools import lru_cache
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

ANTIALIAS = True          # transforms.Resize on a tensor, torchvision >= 0.17 (see the module docstring)
SIDE = 299
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BN_EPS = 1e-3
FEATURES = 2048
MIN_SIDE = 75             # below it Mixed_7a's pool has no window left


def _units() -> List[Tuple[str, int, int, int, int, int, int, int]]:
    """(name, Cin, Cout, kh, kw, stride, pad_h, pad_w) of every BasicConv2d of the trunk, in forward order."""
    u = [("Conv2d_1a_3x3", 3, 32, 3, 3, 2, 0, 0), ("Conv2d_2a_3x3", 32, 32, 3, 3, 1, 0, 0),
         ("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1), ("Conv2d_3b_1x1", 64, 80, 1, 1, 1, 0, 0),
         ("Conv2d_4a_3x3", 80, 192, 3, 3, 1, 0, 0)]
    for n, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        u += [(n + ".branch1x1", cin, 64, 1, 1, 1, 0, 0), (n + ".branch5x5_1", cin, 48, 1, 1, 1, 0, 0),
              (n + ".branch5x5_2", 48, 64, 5, 5, 1, 2, 2), (n + ".branch3x3dbl_1", cin, 64, 1, 1, 1, 0, 0),
              (n + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), (n + ".branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1),
              (n + ".branch_pool", cin, pf, 1, 1, 1, 0, 0)]
    u += [("Mixed_6a.branch3x3", 288, 384, 3, 3, 2, 0, 0), ("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1, 1, 0, 0),
          ("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), ("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3, 2, 0, 0)]
    for n, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        u += [(n + ".branch1x1", 768, 192, 1, 1, 1, 0, 0), (n + ".branch7x7_1", 768, c7, 1, 1, 1, 0, 0),
              (n + ".branch7x7_2", c7, c7, 1, 7, 1, 0, 3), (n + ".branch7x7_3", c7, 192, 7, 1, 1, 3, 0),
              (n + ".branch7x7dbl_1", 768, c7, 1, 1, 1, 0, 0), (n + ".branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0),
              (n + ".branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3), (n + ".branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0),
              (n + ".branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3), (n + ".branch_pool", 768, 192, 1, 1, 1, 0, 0)]
    u += [("Mixed_7a.branch3x3_1", 768, 192, 1, 1, 1, 0, 0), ("Mixed_7a.branch3x3_2", 192, 320, 3, 3, 2, 0, 0),
          ("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1, 1, 0, 0), ("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3),
          ("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0), ("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3, 2, 0, 0)]
    for n, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        u += [(n + ".branch1x1", cin, 320, 1, 1, 1, 0, 0), (n + ".branch3x3_1", cin, 384, 1, 1, 1, 0, 0),
              (n + ".branch3x3_2a", 384, 384, 1, 3, 1, 0, 1), (n + ".branch3x3_2b", 384, 384, 3, 1, 1, 1, 0),
              (n + ".branch3x3dbl_1", cin, 448, 1, 1, 1, 0, 0), (n + ".branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1),
              (n + ".branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1), (n + ".branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0),
              (n + ".branch_pool", cin, 192, 1, 1, 1, 0, 0)]
    return u


UNITS = tuple(_units())
_BY_NAME = {u[0]: u for u in UNITS}
_BN_KEYS = ("weight", "bias", "running_mean", "running_var")


# ------------------------------------------------------------------------------------------------ weights
def weight_specs():
    """(key, shape) of every tensor the metric reads."""
    out = []
    for name, ci, co, kh, kw, _, _, _ in UNITS:
        out.append((name + ".conv.weight", (co, ci, kh, kw)))
        out += [(f"{name}.bn.{k}", (co,)) for k in _BN_KEYS]
    return out


def check_weights(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The float32 tensors of `weight_specs()` out of `sd` (`AuxLogits.*`, `fc.*`, `num_batches_tracked` and any other
    key ignored); a missing key or a wrong shape is a ValueError naming the key."""
    out = {}
    for key, shape in weight_specs():
        t = sd.get(key)
        if t is None:
            raise ValueError(f"FID weights: key {key} missing")
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if tuple(t.shape) != shape:
            raise ValueError(f"FID weights: {key} has shape {tuple(t.shape)}, expected {shape}")
        out[key] = t.detach().to(torch.float32).contiguous()
    return out


def load_weights(path) -> Dict[str, torch.Tensor]:
    """torchvision's InceptionV3 state dict from a `.pth` / `.safetensors` file, or from the first
    `inception_v3*.pth` of a directory."""
    p = Path(path)
    if p.is_dir():
        found = sorted(p.glob("inception_v3*.pth")) + sorted(p.glob("inception_v3*.safetensors"))
        if not found:
            raise FileNotFoundError(f"FID weights: {p} holds no inception_v3*.pth")
        p = found[0]
    elif not p.is_file():
        raise FileNotFoundError(f"FID weights: {p} does not exist")
    if p.suffix == ".safetensors":
        from safetensors.torch import load_file
        sd = dict(load_file(str(p)))
    else:
        sd = torch.load(str(p), map_location="cpu", weights_only=True)
        if not isinstance(sd, dict):
            raise ValueError(f"FID weights: {p} does not hold a state_dict")
    return check_weights(sd)


def fold_bn(weights: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """`weights` plus, per unit, `<unit>.bn.scale` = gamma / sqrt(var + eps) and `<unit>.bn.shift` = beta - mean *
    scale, formed in float64 and stored as float32: the two vectors csrc/fid.hip's BN + ReLU kernel applies.  The conv
    weights are left alone, so a conv's output is what this file's conv produces."""
    out = dict(weights)
    for name, *_ in UNITS:
        g, b, m, v = (weights[f"{name}.bn.{k}"].double() for k in _BN_KEYS)
        scale = g / torch.sqrt(v + BN_EPS)
        out[name + ".bn.scale"] = scale.float()
        out[name + ".bn.shift"] = (b - m * scale).float()
    return out


# ------------------------------------------------------------------------------------------------ preprocessing
def _batch_u8(img, what: str = "image") -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img.detach().cpu()
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError(f"{what}: expected uint8 RGB [H, W, 3] or [B, H, W, 3]")
    return t[None] if t.dim() == 3 else t


def preprocess(img_u8, dtype=torch.float32) -> torch.Tensor:
    """uint8 [H, W, 3] or [B, H, W, 3] -> the trunk's input [B, 3, 299, 299]: ToTensor, Resize((299, 299)) on the
    tensor, Normalize (`src/metrics.py:74-80`)."""
    x = _batch_u8(img_u8).to(dtype) / 255.0
    x = F.interpolate(x.permute(0, 3, 1, 2), size=(SIDE, SIDE), mode="bilinear", align_corners=False,
                      antialias=ANTIALIAS)
    mean = torch.tensor(MEAN, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    return (x - mean) / std


@lru_cache(maxsize=256)
def aa_taps(in_size: int, out_size: int = SIDE):
    """The taps of ATen's `_upsample_bilinear2d_aa` along one axis, computed in float32 as ATen does for a float32
    tensor: (start int32 [out], count int32 [out], weights float32 [out, kmax], kmax).  scale = in / out, support =
    max(scale, 1), centre = scale * (i + 0.5); taps [int(centre - support + 0.5), int(centre + support + 0.5)) clipped
    to the axis, triangle weights `1 - |(j + start - centre + 0.5) / max(scale, 1)|` (0 outside), divided by their
    sum.  Output i = sum_j src[start_i + j] * weights[i, j] in tap order."""
    f = np.float32
    scale = f(in_size) / f(out_size)
    support = scale if scale >= 1 else f(1.0)
    inv = f(1.0) / scale if scale >= 1 else f(1.0)
    kmax = int(math.ceil(float(support))) * 2 + 1
    start = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    w = np.zeros((out_size, kmax), np.float32)
    for i in range(out_size):
        centre = scale * f(i + 0.5)
        lo = max(int(centre - support + f(0.5)), 0)
        n = min(int(centre + support + f(0.5)), in_size) - lo
        j = np.arange(n, dtype=np.float32)
        t = np.abs((j + f(lo) - centre + f(0.5)) * inv)
        ww = np.where(t < 1, f(1.0) - t, f(0.0)).astype(np.float32)
        total = f(0.0)
        for v in ww:                       # ATen adds the weights one by one
            total = f(total + v)
        if total != 0:
            ww = (ww / total).astype(np.float32)
        start[i], count[i] = lo, n
        w[i, :n] = ww
    return start, count, w, kmax


# ------------------------------------------------------------------------------------------------ the trunk
def _unit(x: torch.Tensor, w: Dict[str, torch.Tensor], name: str) -> torch.Tensor:
    _, _, _, _, _, stride, ph, pw = _BY_NAME[name]
    dt = x.dtype
    x = F.conv2d(x, w[name + ".conv.weight"].to(dt), None, stride=stride, padding=(ph, pw))
    x = F.batch_norm(x, w[name + ".bn.running_mean"].to(dt), w[name + ".bn.running_var"].to(dt),
                     w[name + ".bn.weight"].to(dt), w[name + ".bn.bias"].to(dt), False, 0.0, BN_EPS)
    return F.relu(x)


def _seq(x, w, prefix, names):
    for n in names:
        x = _unit(x, w, prefix + n)
    return x


def _block_a(x, w, p):
    return torch.cat([_unit(x, w, p + ".branch1x1"),
                      _seq(x, w, p, (".branch5x5_1", ".branch5x5_2")),
                      _seq(x, w, p, (".branch3x3dbl_1", ".branch3x3dbl_2", ".branch3x3dbl_3")),
                      _unit(F.avg_pool2d(x, 3, 1, 1), w, p + ".branch_pool")], 1)


def _block_b(x, w, p):
    return torch.cat([_unit(x, w, p + ".branch3x3"),
                      _seq(x, w, p, (".branch3x3dbl_1", ".branch3x3dbl_2", ".branch3x3dbl_3")),
                      F.max_pool2d(x, 3, 2)], 1)


def _block_c(x, w, p):
    return torch.cat([_unit(x, w, p + ".branch1x1"),
                      _seq(x, w, p, (".branch7x7_1", ".branch7x7_2", ".branch7x7_3")),
                      _seq(x, w, p, tuple(f".branch7x7dbl_{i}" for i in range(1, 6))),
                      _unit(F.avg_pool2d(x, 3, 1, 1), w, p + ".branch_pool")], 1)


def _block_d(x, w, p):
    return torch.cat([_seq(x, w, p, (".branch3x3_1", ".branch3x3_2")),
                      _seq(x, w, p, tuple(f".branch7x7x3_{i}" for i in range(1, 5))),
                      F.max_pool2d(x, 3, 2)], 1)


def _block_e(x, w, p):
    a = _unit(x, w, p + ".branch3x3_1")
    b = _seq(x, w, p, (".branch3x3dbl_1", ".branch3x3dbl_2"))
    return torch.cat([_unit(x, w, p + ".branch1x1"),
                      _unit(a, w, p + ".branch3x3_2a"), _unit(a, w, p + ".branch3x3_2b"),
                      _unit(b, w, p + ".branch3x3dbl_3a"), _unit(b, w, p + ".branch3x3dbl_3b"),
                      _unit(F.avg_pool2d(x, 3, 1, 1), w, p + ".branch_pool")], 1)


def trunk(x: torch.Tensor, weights: Dict[str, torch.Tensor], shapes: list | None = None) -> torch.Tensor:
    """x [B, 3, H, W] (H, W >= 75) -> the last mixed block's output [B, 2048, h, w]; `shapes`, if given, receives
    (stage name, shape) after every stage."""
    def note(name, t):
        if shapes is not None:
            shapes.append((name, tuple(t.shape)))
        return t

    if min(x.shape[2], x.shape[3]) < MIN_SIDE:
        raise ValueError(f"InceptionV3 needs images of at least {MIN_SIDE} x {MIN_SIDE} pixels")
    with torch.no_grad():
        for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            x = note(n, _unit(x, weights, n))
        x = note("maxpool1", F.max_pool2d(x, 3, 2))
        for n in ("Conv2d_3b_1x1", "Conv2d_4a_3x3"):
            x = note(n, _unit(x, weights, n))
        x = note("maxpool2", F.max_pool2d(x, 3, 2))
        for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = note(n, _block_a(x, weights, n))
        x = note("Mixed_6a", _block_b(x, weights, "Mixed_6a"))
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = note(n, _block_c(x, weights, n))
        x = note("Mixed_7a", _block_d(x, weights, "Mixed_7a"))
        for n in ("Mixed_7b", "Mixed_7c"):
            x = note(n, _block_e(x, weights, n))
    return x


def inception_features(x: torch.Tensor, weights: Dict[str, torch.Tensor], dtype=torch.float32) -> torch.Tensor:
    """The pooled features [B, 2048] of a preprocessed batch x [B, 3, H, W] (adaptive average pool to 1 x 1, dropout
    and fc = Identity)."""
    return trunk(x.to(dtype), weights).mean(dim=(2, 3))


def features_u8(images, weights: Dict[str, torch.Tensor], dtype=torch.float32) -> torch.Tensor:
    """[N, 2048] for a list of uint8 RGB images of any sizes, one image at a time as the reference runs them."""
    return torch.cat([inception_features(preprocess(im, dtype), weights, dtype) for im in images], 0)


# ------------------------------------------------------------------------------------------------ the distance
def _sqrtm_trace_eig(prod: np.ndarray) -> float:
    """trace(sqrtm(prod).real) from the eigenvalues of prod (float64): the trace of a matrix function is the sum of
    the function over the spectrum; the real part of the principal root of each eigenvalue."""
    ev = np.linalg.eigvals(np.asarray(prod, dtype=np.float64)).astype(np.complex128)
    return float(np.sqrt(ev).real.sum())


def frechet_distance(feats_pred, feats_gt, use_scipy: bool | None = None) -> float:
    """`src/metrics.py:199-223` on two [N, D] float32 feature arrays: mean in float32, `np.cov(rowvar=False)` in
    float64, `ssdiff + trace(s1 + s2 - 2 sqrtm(s1 s2).real)`.  scipy's `sqrtm` when scipy imports (`use_scipy` None),
    else the trace of the root from the eigenvalues of s1 s2."""
    f1 = np.asarray(feats_pred, dtype=np.float32)
    f2 = np.asarray(feats_gt, dtype=np.float32)
    mu1, sigma1 = f1.mean(axis=0), np.cov(f1, rowvar=False)
    mu2, sigma2 = f2.mean(axis=0), np.cov(f2, rowvar=False)
    ssdiff = np.sum((mu1 - mu2) ** 2.0)
    sqrtm = None
    if use_scipy is None or use_scipy:
        try:
            from scipy.linalg import sqrtm
        except ImportError:
            if use_scipy:
                raise
    if sqrtm is not None:
        covmean = sqrtm(sigma1.dot(sigma2))
        if np.iscomplexobj(covmean):
            covmean = covmean.real
        return float(ssdiff + np.trace(sigma1 + sigma2 - 2.0 * covmean))
    return float(ssdiff + np.trace(sigma1) + np.trace(sigma2) - 2.0 * _sqrtm_trace_eig(sigma1.dot(sigma2)))
