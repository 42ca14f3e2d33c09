"""Real-ESRGAN's compact network on the host — a plain-torch restatement of
`SRVGGNetCompact(3, 3, num_feat=64, num_conv=32, upscale=4, act_type='prelu')`, the net the reference constructs
(`src/inference.py:335-336`), and of `RealESRGANer.enhance` as `_sr_realesrgan` calls it (`:579-591`) for an 8-bit RGB
image at `outscale == 4`.

No `realesrgan`, `basicsr` or `cv2`: the network is written out here from the package's published source
(`realesrgan/archs/srvgg_arch.py`, `realesrgan/utils.py`) and the weights come from a file the user already has.  The
files whose keys fit this net are `realesr-general-x4v3.pth` and `realesr-general-wdn-x4v3.pth`; the reference itself
names `RealESRGAN_x4plus.pth`, an RRDBNet checkpoint, which `check_weights` refuses with the mismatching keys.

* body:     conv 3->64, PReLU, 32 x (conv 64->64, PReLU), conv 64->48, all 3x3 / pad 1 (`body.{0..66}`)
* tail:     `pixel_shuffle(4)`, then `out += interpolate(x, scale_factor=4, mode='nearest')`
* enhance:  `float32(u8) / 255`, the net (the RGB<->BGR swaps of `_sr_realesrgan` and `enhance` cancel), no `pre_pad`,
            no `mod_pad` at scale 4, `tile=0`; `.float().clamp_(0, 1)`, `* 255.0`, `np.round`, uint8

`forward(..., half=True)` is the model under `.half()` as `RealESRGANer(half=True)` runs it on a GPU: weights, biases,
slopes and the input rounded to fp16, the arithmetic in `dtype`, and the value rounded to fp16 once after each
conv + bias, once after each PReLU and once after the final add.  With `dtype=torch.float64` it is the oracle of the
fp16 engine (`srvgg_gpu`, csrc/srvgg.hip); `forward(float64)` is the ground truth of the tests.

This restatement is not pinned against the real package (parity unpinned, like `lpips_host`): neither the package nor
its weight files are available offline.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

NUM_FEAT, NUM_CONV, UPSCALE, NUM_OUT = 64, 32, 4, 3
N_CONVS = NUM_CONV + 2                          # body.0, body.2, ..., body.66
CONV_IDS = tuple(range(0, 2 * N_CONVS, 2))
PRELU_IDS = tuple(range(1, 2 * N_CONVS - 1, 2))
WEIGHTS_ENV = "IRX_REALESRGAN_WEIGHTS"


def conv_shape(i: int):
    """(Cout, Cin) of conv i of 34."""
    return (NUM_OUT * UPSCALE * UPSCALE if i == N_CONVS - 1 else NUM_FEAT, 3 if i == 0 else NUM_FEAT)


def weight_specs():
    """(key, shape) of every tensor the net reads."""
    out = []
    for i, k in enumerate(CONV_IDS):
        co, ci = conv_shape(i)
        out += [(f"body.{k}.weight", (co, ci, 3, 3)), (f"body.{k}.bias", (co,))]
        if i < N_CONVS - 1:
            out.append((f"body.{k + 1}.weight", (NUM_FEAT,)))
    return out


def _short(keys, n=8):
    keys = sorted(keys)
    return ", ".join(keys[:n]) + (f", ... ({len(keys)} in all)" if len(keys) > n else "")


def check_weights(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The float32 tensors of `weight_specs()` out of `sd`, which may be nested under `params_ema` (preferred, as
    `RealESRGANer` does) or `params`.  Any other key set (an RRDBNet checkpoint, say) is a ValueError that lists the
    missing and the unexpected keys; a wrong shape names the key."""
    if not isinstance(sd, dict):
        raise ValueError("Real-ESRGAN weights: not a state_dict")
    for nest in ("params_ema", "params"):
        if isinstance(sd.get(nest), dict):
            sd = sd[nest]
            break
    specs = weight_specs()
    want = {k for k, _ in specs}
    missing, extra = want - set(sd), set(sd) - want
    if missing or extra:
        raise ValueError("Real-ESRGAN weights: the keys do not fit SRVGGNetCompact(num_feat=64, num_conv=32, "
                         f"upscale=4); missing: [{_short(missing)}]; unexpected: [{_short(extra)}]")
    out = {}
    for key, shape in specs:
        t = sd[key]
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if tuple(t.shape) != shape:
            raise ValueError(f"Real-ESRGAN weights: {key} has shape {tuple(t.shape)}, expected {shape}")
        out[key] = t.detach().to(torch.float32).contiguous()
    return out


def _read(f: Path):
    if f.suffix == ".safetensors":
        from safetensors.torch import load_file
        return dict(load_file(str(f)))
    return torch.load(str(f), map_location="cpu", weights_only=True)


def load_weights(path) -> Dict[str, torch.Tensor]:
    """One `.pth` / `.safetensors` file, or a directory that holds exactly one."""
    p = Path(path)
    if p.is_dir():
        files = sorted(list(p.glob("*.pth")) + list(p.glob("*.safetensors")))
        if len(files) != 1:
            raise FileNotFoundError(f"Real-ESRGAN weights: {p} must hold one *.pth / *.safetensors file, found "
                                    f"{len(files)}")
        p = files[0]
    elif not p.is_file():
        raise FileNotFoundError(f"Real-ESRGAN weights: {p} does not exist")
    return check_weights(_read(p))


def input_table() -> torch.Tensor:
    """float32 [256]: `float32(v) / 255` as numpy divides it (a true fp32 division)."""
    return torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0))


def _batch_u8(img) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img.detach().cpu()
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError("image: expected uint8 RGB [H, W, 3] or [B, H, W, 3]")
    return t[None] if t.dim() == 3 else t


def _r16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(t.dtype)


def prelu(x: torch.Tensor, slope: torch.Tensor) -> torch.Tensor:
    return torch.where(x > 0, x, slope.view(1, -1, 1, 1) * x)


def forward(x: torch.Tensor, weights: Dict[str, torch.Tensor], dtype=torch.float32, half: bool = False) -> torch.Tensor:
    """x [B, 3, H, W] in [0, 1] -> [B, 3, 4H, 4W] (not clamped), computed in `dtype`."""
    q = _r16 if half else (lambda t: t)
    with torch.no_grad():
        x = q(x.to(torch.float32)).to(dtype) if half else x.to(dtype)
        out = x
        for i, k in enumerate(CONV_IDS):
            w = q(weights[f"body.{k}.weight"]).to(dtype)
            b = q(weights[f"body.{k}.bias"]).to(dtype)
            out = q(F.conv2d(out, w, b, padding=1))
            if i < N_CONVS - 1:
                out = q(prelu(out, q(weights[f"body.{k + 1}.weight"]).to(dtype)))
        out = F.pixel_shuffle(out, UPSCALE)
        return q(out + F.interpolate(x, scale_factor=UPSCALE, mode="nearest"))


def to_u8(out: torch.Tensor) -> torch.Tensor:
    """[B, 3, 4H, 4W] -> uint8 [B, 4H, 4W, 3]: `.float().clamp_(0, 1)`, `* 255.0` in fp32, round half to even."""
    y = out.to(torch.float32).clamp_(0, 1).permute(0, 2, 3, 1)
    return torch.from_numpy(np.round(y.numpy() * np.float32(255.0)).astype(np.uint8))


def net_input(img_u8) -> torch.Tensor:
    """uint8 [B, H, W, 3] -> float32 [B, 3, H, W], `u8.astype(float32) / 255`."""
    t = _batch_u8(img_u8)
    return torch.from_numpy(t.numpy().astype(np.float32) / np.float32(255.0)).permute(0, 3, 1, 2).contiguous()


def enhance(img_u8, weights: Dict[str, torch.Tensor], dtype=torch.float32, half: bool = False):
    """`RealESRGANer.enhance(img, outscale=4)[0]` for uint8 RGB [H, W, 3] (numpy in, numpy out) or [B, H, W, 3]
    (a uint8 tensor out)."""
    single = (img_u8.ndim if isinstance(img_u8, np.ndarray) else img_u8.dim()) == 3
    out = to_u8(forward(net_input(img_u8), weights, dtype, half))
    return out[0].numpy() if single and isinstance(img_u8, np.ndarray) else (out[0] if single else out)
