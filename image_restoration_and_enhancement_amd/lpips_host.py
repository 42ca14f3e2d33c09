"""LPIPS (AlexNet) on the host — a plain-torch restatement of `lpips.LPIPS(net='alex')` v0.1 in eval mode with
`spatial=False`, fed the way the reference feeds it (`src/metrics.py:49-55`, `:97-111`).

No torchvision, no `lpips` package: the network is written out here and the weights come from two plain
`state_dict` files the user already has (torchvision's AlexNet checkpoint and the lpips package's `alex.pth`).

* input:    uint8 RGB HWC -> `float32(v) / 255.0`, `* 2.0 - 1.0`, NCHW (`src/metrics.py:49-55`)
* scaling:  `(x - shift) / scale`, shift = [-.030, -.088, -.188], scale = [.458, .448, .450]
* trunk:    torchvision AlexNet `features`, tapped after each of the five ReLUs
* head:     per tap `f / (sqrt(sum_c f^2) + 1e-10)` for both images, squared difference, 1x1 conv without bias
            (`lin{k}.model.1.weight`), spatial mean; the score is the sum over the five taps

`lpips_alex(..., dtype=torch.float64)` is the ground truth of the tests; `dtype=torch.float32` serves
`MetricsCalculator(device="cpu")` and is the oracle's own rounding level.  The GPU path (`lpips_gpu`, csrc/lpips.hip)
builds its input table with `input_table()`, the float32 expression of this file.

This restatement is not pinned against the real `lpips` package: neither the package nor the two weight files are
available offline, so parity with it rests on reading its source (parity unpinned, like the INTER_LINEAR resize of
`metrics.py`).
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (state_dict prefix, Cout, Cin, kernel, stride, padding) of the five convs; a 3 / stride-2 max pool follows the
# ReLU of the first two
CONVS = (("features.0", 64, 3, 11, 4, 2), ("features.3", 192, 64, 5, 1, 2), ("features.6", 384, 192, 3, 1, 1),
         ("features.8", 256, 384, 3, 1, 1), ("features.10", 256, 256, 3, 1, 1))
CHANNELS = tuple(c[1] for c in CONVS)
LIN_KEYS = tuple(f"lin{k}.model.1.weight" for k in range(5))
MIN_SIDE = 31      # below it the second pool has no window left (torch raises there)
EPS = 1e-10


def weight_specs():
    """(key, shape) of every tensor the metric reads."""
    out = []
    for name, co, ci, k, _, _ in CONVS:
        out += [(name + ".weight", (co, ci, k, k)), (name + ".bias", (co,))]
    out += [(key, (1, c, 1, 1)) for key, c in zip(LIN_KEYS, CHANNELS)]
    return out


def check_weights(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The float32 tensors of `weight_specs()` out of `sd` (other keys ignored); a missing key or a wrong shape is a
    ValueError naming the key."""
    out = {}
    for key, shape in weight_specs():
        t = sd.get(key)
        if t is None:
            raise ValueError(f"LPIPS weights: key {key} missing")
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if tuple(t.shape) != shape:
            raise ValueError(f"LPIPS weights: {key} has shape {tuple(t.shape)}, expected {shape}")
        out[key] = t.detach().to(torch.float32).contiguous()
    return out


def _read(f: Path) -> Dict[str, torch.Tensor]:
    if f.suffix == ".safetensors":
        from safetensors.torch import load_file
        return dict(load_file(str(f)))
    sd = torch.load(str(f), map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"LPIPS weights: {f} does not hold a state_dict")
    return sd


def load_weights(path) -> Dict[str, torch.Tensor]:
    """A directory with `alexnet*.pth` (keys `features.{0,3,6,8,10}.{weight,bias}`) and `alex.pth` (keys
    `lin{0..4}.model.1.weight`), or one `.pth` / `.safetensors` file with both key sets."""
    p = Path(path)
    if p.is_dir():
        trunk = sorted(p.glob("alexnet*.pth"))
        lin = p / "alex.pth"
        if not trunk or not lin.exists():
            raise FileNotFoundError(f"LPIPS weights: {p} needs an alexnet*.pth and an alex.pth")
        sd = dict(_read(trunk[0]))
        sd.update(_read(lin))
    elif p.is_file():
        sd = _read(p)
    else:
        raise FileNotFoundError(f"LPIPS weights: {p} does not exist")
    return check_weights(sd)


def feature_sizes(H: int, W: int):
    """(h, w) of the five taps for an H x W image."""
    def conv(n, k, s, p):
        return (n + 2 * p - k) // s + 1

    def pool(n):
        return (n - 3) // 2 + 1

    h0, w0 = conv(H, 11, 4, 2), conv(W, 11, 4, 2)
    h1, w1 = pool(h0), pool(w0)
    h2, w2 = pool(h1), pool(w1)
    return ((h0, w0), (h1, w1), (h2, w2), (h2, w2), (h2, w2))


def input_table() -> torch.Tensor:
    """float32 [256, 3]: the trunk's input for byte value v in channel c, `(float32(v) / 255 * 2 - 1 - shift) / scale`
    as `scaled_input` forms it in float32."""
    v = torch.arange(256, dtype=torch.float32)[:, None].expand(256, 3)
    x = (v / 255.0) * 2.0 - 1.0
    return ((x - torch.tensor(SHIFT, dtype=torch.float32)) / torch.tensor(SCALE, dtype=torch.float32)).contiguous()


def _batch_u8(img, what: str) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img.detach().cpu()
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError(f"{what}: expected uint8 RGB [H, W, 3] or [B, H, W, 3]")
    return t[None] if t.dim() == 3 else t


def scaled_input(img_u8, dtype=torch.float32) -> torch.Tensor:
    """uint8 [B, H, W, 3] -> the trunk's input [B, 3, H, W] (image_to_tensor, then the scaling layer)."""
    t = _batch_u8(img_u8, "image")
    x = t.to(dtype) / 255.0
    x = x.permute(0, 3, 1, 2) * 2.0 - 1.0
    shift = torch.tensor(SHIFT, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    return (x - shift) / scale


def features(x: torch.Tensor, weights: Dict[str, torch.Tensor]):
    """The five ReLU outputs of the AlexNet trunk for x [B, 3, H, W]."""
    taps = []
    for i, (name, _, _, _, stride, pad) in enumerate(CONVS):
        if i in (1, 2):
            x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = F.relu(F.conv2d(x, weights[name + ".weight"].to(x.dtype), weights[name + ".bias"].to(x.dtype),
                            stride=stride, padding=pad))
        taps.append(x)
    return taps


def _normalize(f: torch.Tensor) -> torch.Tensor:
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + EPS)


def lpips_alex(pred_u8, gt_u8, weights: Dict[str, torch.Tensor], dtype=torch.float32
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(total [B], per_layer [B, 5]) of uint8 RGB images [H, W, 3] or [B, H, W, 3] of one shape."""
    p, g = _batch_u8(pred_u8, "pred"), _batch_u8(gt_u8, "gt")
    if p.shape != g.shape:
        raise ValueError("Input images must have the same dimensions.")
    if min(p.shape[1], p.shape[2]) < MIN_SIDE:
        raise ValueError(f"LPIPS(alex) needs images of at least {MIN_SIDE} x {MIN_SIDE} pixels, got "
                         f"{p.shape[1]} x {p.shape[2]}")
    with torch.no_grad():
        fp = features(scaled_input(p, dtype), weights)
        fg = features(scaled_input(g, dtype), weights)
        layers = []
        for k in range(5):
            d = (_normalize(fp[k]) - _normalize(fg[k])) ** 2
            layers.append(F.conv2d(d, weights[LIN_KEYS[k]].to(dtype)).mean(dim=(2, 3))[:, 0])
        per_layer = torch.stack(layers, dim=1)
        total = layers[0]
        for k in range(1, 5):
            total = total + layers[k]
    return total, per_layer
