"""Real-ESRGAN's RRDBNet on the host — a plain-torch restatement of
`RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=23, num_grow_ch=32, scale=4)`, the network
`RealESRGAN_x4plus.pth` belongs to.  That file is the one the reference names (`src/inference.py:326-350`); the
reference constructs `SRVGGNetCompact` around it, so its own strict load fails and it lands on LANCZOS.  Here the file
runs when `config["sr"]["realesrgan_arch"]` is `"rrdbnet"` or `"auto"`.

No `realesrgan`, `basicsr` or `cv2`: the network is written out from its definition (basicsr's `rrdbnet_arch.py`) and
the weights come from a file the user already has.  All convs are 3x3, pad 1, with bias; LeakyReLU slope 0.2.

* `feat = conv_first(x)`
* 23 x RRDB: `out = rdb3(rdb2(rdb1(x))) * 0.2 + x`; an RDB is `x1 = lrelu(conv1(x))`, `x2 = lrelu(conv2(cat(x, x1)))`,
  `x3 = lrelu(conv3(cat(x, x1, x2)))`, `x4 = lrelu(conv4(cat(x, x1, x2, x3)))`, `x5 = conv5(cat(x, x1, x2, x3, x4))`,
  result `x5 * 0.2 + x`
* `feat = feat + conv_body(body(feat))`
* `feat = lrelu(conv_up1(nearest x2(feat)))`, `feat = lrelu(conv_up2(nearest x2(feat)))`
* `out = conv_last(lrelu(conv_hr(feat)))`
* around it `RealESRGANer.enhance` for 8-bit RGB at x4, `tile=0`, `pre_pad=0`: `srvgg_host.net_input` / `to_u8`
  (scale 4 needs no mod-pad)

`forward(..., half=True)` emulates PyTorch's eager fp16 rounding points in `dtype` arithmetic: weights, biases and the
input rounded to fp16; conv + bias rounded once; LeakyReLU `v > 0 ? v : round16(0.2f * v)` with the slope the fp32
scalar 0.2f (not an fp16 value, unlike the PReLU slopes of `srvgg_host`); each `t * 0.2 + x` is
`round16(round16(0.2f * t) + x)`.  With `dtype=torch.float64` it is the oracle of the fp16 engine (`rrdb_gpu`,
csrc/rrdb.hip); `forward(float64)` is the ground truth of the tests.

This restatement is not pinned against the real package (parity unpinned, like `srvgg_host`): neither the package nor
its weight files are available offline.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from .srvgg_host import _batch_u8, _r16, _read, _short, input_table, net_input, to_u8  # noqa: F401

NUM_FEAT, NUM_GROW, NUM_BLOCK, UPSCALE, NUM_OUT = 64, 32, 23, 4, 3
SLOPE32 = float(np.float32(0.2))               # the fp32 scalar the fp16 kernels multiply by
OUTER = ("conv_first", "conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last")


def conv_names(num_block: int = NUM_BLOCK):
    """(name, Cout, Cin) of every conv, in forward order."""
    out = [("conv_first", NUM_FEAT, 3)]
    for i in range(num_block):
        for j in (1, 2, 3):
            for k in range(5):
                out.append((f"body.{i}.rdb{j}.conv{k + 1}", NUM_FEAT if k == 4 else NUM_GROW, NUM_FEAT + k * NUM_GROW))
    out += [("conv_body", NUM_FEAT, NUM_FEAT), ("conv_up1", NUM_FEAT, NUM_FEAT), ("conv_up2", NUM_FEAT, NUM_FEAT),
            ("conv_hr", NUM_FEAT, NUM_FEAT), ("conv_last", NUM_OUT, NUM_FEAT)]
    return out


def weight_specs(num_block: int = NUM_BLOCK):
    """(key, shape) of every tensor the net reads."""
    out = []
    for n, co, ci in conv_names(num_block):
        out += [(f"{n}.weight", (co, ci, 3, 3)), (f"{n}.bias", (co,))]
    return out


def _unnest(sd):
    if not isinstance(sd, dict):
        raise ValueError("Real-ESRGAN weights: not a state_dict")
    for nest in ("params_ema", "params"):
        if isinstance(sd.get(nest), dict):
            return sd[nest]
    return sd


def looks_like_rrdb(sd) -> bool:
    """True if the key set is an RRDBNet's (`conv_first.weight` and a dense block), whatever the block count."""
    try:
        sd = _unnest(sd)
    except ValueError:
        return False
    return "conv_first.weight" in sd and "body.0.rdb1.conv1.weight" in sd


def count_blocks(sd) -> int:
    """Number of `body.{i}` RRDBs in the (unnested) key set."""
    ids = {int(k.split(".")[1]) for k in sd if k.startswith("body.") and k.split(".")[1].isdigit()}
    return max(ids) + 1 if ids else 0


def check_weights(sd: Dict[str, torch.Tensor], num_block: int | None = None) -> Dict[str, torch.Tensor]:
    """The float32 tensors of `weight_specs(num_block)` out of `sd`, which may be nested under `params_ema` (preferred,
    as `RealESRGANer` does) or `params`.  `num_block=None` takes the block count from the keys (23 in the published
    file).  Any other key set is a ValueError that lists the missing and the unexpected keys; a wrong shape names the
    key."""
    sd = _unnest(sd)
    nb = num_block if num_block is not None else max(count_blocks(sd), 1)
    specs = weight_specs(nb)
    want = {k for k, _ in specs}
    missing, extra = want - set(sd), set(sd) - want
    if missing or extra:
        raise ValueError(f"Real-ESRGAN weights: the keys do not fit RRDBNet(num_feat=64, num_block={nb}, "
                         f"num_grow_ch=32, scale=4); missing: [{_short(missing)}]; unexpected: [{_short(extra)}]")
    out = {}
    for key, shape in specs:
        t = sd[key]
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if tuple(t.shape) != shape:
            raise ValueError(f"Real-ESRGAN weights: {key} has shape {tuple(t.shape)}, expected {shape}")
        out[key] = t.detach().to(torch.float32).contiguous()
    return out


def num_blocks(weights: Dict[str, torch.Tensor]) -> int:
    return count_blocks(weights)


def read_file(path):
    """The raw state_dict of one `.pth` / `.safetensors` file, or of the one such file in a directory."""
    p = Path(path)
    if p.is_dir():
        files = sorted(list(p.glob("*.pth")) + list(p.glob("*.safetensors")))
        if len(files) != 1:
            raise FileNotFoundError(f"Real-ESRGAN weights: {p} must hold one *.pth / *.safetensors file, found "
                                    f"{len(files)}")
        p = files[0]
    elif not p.is_file():
        raise FileNotFoundError(f"Real-ESRGAN weights: {p} does not exist")
    return _read(p)


def load_weights(path, num_block: int | None = None) -> Dict[str, torch.Tensor]:
    """One `.pth` / `.safetensors` file, or a directory that holds exactly one."""
    return check_weights(read_file(path), num_block)


def forward(x: torch.Tensor, weights: Dict[str, torch.Tensor], dtype=torch.float32, half: bool = False) -> torch.Tensor:
    """x [B, 3, H, W] in [0, 1] -> [B, 3, 4H, 4W] (not clamped), computed in `dtype`."""
    q = _r16 if half else (lambda t: t)
    # the scalar 0.2: PyTorch multiplies an fp16 tensor by the fp32 value; fp32 / fp64 tensors by the double
    slope = SLOPE32 if half else 0.2
    nb = num_blocks(weights)

    def conv(t, name):
        w = q(weights[f"{name}.weight"]).to(dtype)
        b = q(weights[f"{name}.bias"]).to(dtype)
        return q(F.conv2d(t, w, b, padding=1))

    def scaled(t):          # round16(0.2f * t): the product is an fp32 value first
        return q((t * slope).to(torch.float32).to(dtype)) if half else t * slope

    def lrelu(t):
        return torch.where(t > 0, t, scaled(t))

    def scaled_add(t, res):
        return q(scaled(t) + res)

    def rdb(t, name):
        cat = t
        for k in range(1, 5):
            cat = torch.cat((cat, lrelu(conv(cat, f"{name}.conv{k}"))), 1)
        return scaled_add(conv(cat, f"{name}.conv5"), t)

    with torch.no_grad():
        x = q(x.to(torch.float32)).to(dtype) if half else x.to(dtype)
        feat = conv(x, "conv_first")
        body = feat
        for i in range(nb):
            t = body
            for j in (1, 2, 3):
                t = rdb(t, f"body.{i}.rdb{j}")
            body = scaled_add(t, body)
        feat = q(feat + conv(body, "conv_body"))
        feat = lrelu(conv(F.interpolate(feat, scale_factor=2, mode="nearest"), "conv_up1"))
        feat = lrelu(conv(F.interpolate(feat, scale_factor=2, mode="nearest"), "conv_up2"))
        return conv(lrelu(conv(feat, "conv_hr")), "conv_last")


def enhance(img_u8, weights: Dict[str, torch.Tensor], dtype=torch.float32, half: bool = False):
    """`RealESRGANer.enhance(img, outscale=4)[0]` for uint8 RGB [H, W, 3] (numpy in, numpy out) or [B, H, W, 3]
    (a uint8 tensor out)."""
    single = (img_u8.ndim if isinstance(img_u8, np.ndarray) else img_u8.dim()) == 3
    out = to_u8(forward(net_input(img_u8), weights, dtype, half))
    return out[0].numpy() if single and isinstance(img_u8, np.ndarray) else (out[0] if single else out)
