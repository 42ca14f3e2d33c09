"""The Stable Diffusion safety checker on the host — a plain-torch fp32 restatement of what diffusers 0.35.2 runs at
the end of `StableDiffusionImg2ImgPipeline.__call__` (`run_safety_checker`; the reference's calls at
`src/inference.py:486, :566, :664`, switched off for inpainting at `:444-451, :746-752`):

* `preprocess`     `CLIPImageProcessor` as `feature_extractor/preprocessor_config.json` sets it up: Pillow BICUBIC resize
                   of the shortest edge to S (`(S, int(S * long / short))`), centre crop S x S (`(h - S) // 2`), rescale
                   and normalise in the processor's own operation order (`input_table`);
* `vision_pooled`  `CLIPVisionModel`: bias-free patch conv, class + position embeddings, `pre_layrnorm`, pre-LN encoder
                   layers (quick-GELU), `post_layernorm` of token 0;
* `image_embeds`   `visual_projection(pooled)`;
* `cosines`        `normalize(image_embeds) @ normalize(embeds).T`, `F.normalize` dividing by `max(|x|, 1e-12)`;
* `decide`         `StableDiffusionSafetyChecker.forward`'s loop, literally, on numpy float32.

No `diffusers`: the decision loop and the module layout are written out from its published source; the tower and the
processor are pinned against `transformers` where that package imports (tests/test_safety_host.py).  This module is the
oracle of the native checker (`safety_gpu`, csrc/safety_model.cpp, csrc/safety.hip).  No CPU product path uses it: the
diffusion engine does not run on a CPU, and the reference does not filter its classical fallbacks either.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from . import weights as W
from .configs import SafetyConfig

WEIGHTS_ENV = "IRX_SAFETY_CHECKER"
WEIGHT_FILES = ("model.safetensors", "model.fp16.safetensors", "pytorch_model.bin")
NSFW_WARNING = ("Potential NSFW content was detected in one or more images. A black image will be returned instead. "
                "Try again with a different prompt and/or seed.")
_IGNORED = ("position_ids",)          # buffers some checkpoints carry; not parameters
_PREFIX = "vision_model.vision_model."


# ------------------------------------------------------------------------------------------- weights
def _short(keys, n=8):
    keys = sorted(keys)
    return ", ".join(keys[:n]) + (f", ... ({len(keys)} in all)" if len(keys) > n else "")


def check_weights(sd: Dict[str, torch.Tensor], cfg: SafetyConfig) -> Dict[str, torch.Tensor]:
    """The float32 tensors the checker reads out of `sd` (`position_ids` buffers dropped).  The rows of the two
    embedding tables are taken from `sd` and written into `cfg` (`n_special`, `n_concepts`).  A key set that does not
    fit is a ValueError listing the missing and the unexpected keys; a wrong shape names the key."""
    if not isinstance(sd, dict):
        raise ValueError("safety checker weights: not a state_dict")
    sd = {k: v for k, v in sd.items() if not k.endswith(_IGNORED)}
    for key, attr in (("special_care_embeds", "n_special"), ("concept_embeds", "n_concepts")):
        t = sd.get(key)
        if t is not None and getattr(t, "ndim", 0) == 2:
            setattr(cfg, attr, int(t.shape[0]))
    specs = W.param_specs("safety", cfg)
    want = {k for k, _ in specs}
    missing, extra = want - set(sd), set(sd) - want
    if missing or extra:
        raise ValueError("safety checker weights: the keys do not fit StableDiffusionSafetyChecker "
                         f"({cfg.num_hidden_layers} layers); missing: [{_short(missing)}]; unexpected: [{_short(extra)}]")
    out = {}
    for key, shape in specs:
        t = sd[key]
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"safety checker weights: {key} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        out[key] = t.detach().to(torch.float32).contiguous()
    return out


def weight_file(checker_dir) -> Optional[Path]:
    """The weight file `from_pretrained` would read from `safety_checker/`, or None."""
    for name in WEIGHT_FILES:
        f = Path(checker_dir) / name
        if f.is_file():
            return f
    return None


def load(checker_dir, preprocessor_dir=None) -> Tuple[SafetyConfig, Dict[str, torch.Tensor]]:
    """(config, checked float32 weights) of a `safety_checker/` directory: `config.json`, one of `model.safetensors`,
    `model.fp16.safetensors`, `pytorch_model.bin`, and the `feature_extractor/preprocessor_config.json` next to it (or
    under `preprocessor_dir`) when there is one."""
    p = Path(checker_dir)
    if not (p / "config.json").is_file():
        raise FileNotFoundError(f"safety checker: {p / 'config.json'} does not exist")
    f = weight_file(p)
    if f is None:
        raise FileNotFoundError(f"safety checker: none of {', '.join(WEIGHT_FILES)} under {p}")
    cfg = SafetyConfig.from_dir(p, preprocessor_dir)
    if f.suffix == ".safetensors":
        from safetensors.torch import load_file
        sd = dict(load_file(str(f)))
    else:
        sd = torch.load(str(f), map_location="cpu", weights_only=True)
    return cfg, check_weights(sd, cfg)


def listed_in_model_index(model_dir) -> bool:
    """Whether `<model_dir>/model_index.json` names a safety checker (`"safety_checker": [library, class]`, both not
    null).  The fine-tuned `best/` directories carry `[null, null]`; no file, no checker."""
    f = Path(model_dir) / "model_index.json"
    if not f.is_file():
        return False
    v = json.loads(f.read_text()).get("safety_checker")
    return isinstance(v, (list, tuple)) and len(v) == 2 and v[0] is not None and v[1] is not None


def unit_rows(t: torch.Tensor) -> torch.Tensor:
    """F.normalize(t) computed in fp64 and rounded to fp32 once (what the native head is given)."""
    d = t.detach().double()
    return (d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)).float()


# ------------------------------------------------------------------------------------------- preprocessing
def input_table(cfg: SafetyConfig) -> torch.Tensor:
    """float32 [256, 3]: the processor's value for byte v in channel c, in its operation order (transformers
    `rescale`, then `normalize`): float32(float64(v) * rescale_factor), then (r - float32(mean)) / float32(std) in
    float32."""
    r = (np.arange(256, dtype=np.uint8).astype(np.float64) * cfg.rescale_factor).astype(np.float32)
    mean = np.array(cfg.image_mean, dtype=np.float32)
    std = np.array(cfg.image_std, dtype=np.float32)
    return torch.from_numpy((r[:, None] - mean[None, :]) / std[None, :])


def resized_size(h: int, w: int, size: int) -> Tuple[int, int]:
    """(h, w) after the shortest edge goes to `size`: transformers get_resize_output_image_size,
    default_to_square=False."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def crop_window(h: int, w: int, cfg: SafetyConfig) -> Tuple[int, int, int, int]:
    """(resized h, resized w, top, left) of the centre crop of an h x w image."""
    nh, nw = resized_size(h, w, cfg.resize_size)
    return nh, nw, (nh - cfg.crop_size) // 2, (nw - cfg.crop_size) // 2


def preprocess_u8(img_u8: np.ndarray, cfg: SafetyConfig) -> np.ndarray:
    """uint8 RGB [H, W, 3] -> the resized and cropped uint8 [S, S, 3] (Pillow does the resize)."""
    h, w = img_u8.shape[:2]
    nh, nw, top, left = crop_window(h, w, cfg)
    im = Image.fromarray(img_u8)
    if (nh, nw) != (h, w):
        im = im.resize((nw, nh), Image.BICUBIC)
    S = cfg.crop_size
    return np.ascontiguousarray(np.array(im)[top:top + S, left:left + S])


def preprocess(images_u8, cfg: SafetyConfig) -> torch.Tensor:
    """uint8 RGB [B, H, W, 3] (or one [H, W, 3]) -> pixel_values float32 [B, 3, S, S]."""
    a = images_u8.cpu().numpy() if isinstance(images_u8, torch.Tensor) else np.asarray(images_u8)
    a = a[None] if a.ndim == 3 else a
    tab = input_table(cfg).numpy()
    ch = np.arange(3)
    out = [tab[preprocess_u8(x, cfg), ch] for x in a]
    return torch.from_numpy(np.stack(out)).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------- the tower
def _layer(x: torch.Tensor, wd: Dict[str, torch.Tensor], b: str, cfg: SafetyConfig) -> torch.Tensor:
    B, L, D = x.shape
    H = cfg.num_attention_heads
    d = D // H
    h = F.layer_norm(x, (D,), wd[b + "layer_norm1.weight"], wd[b + "layer_norm1.bias"], cfg.layer_norm_eps)
    s = b + "self_attn."
    q, k, v = (F.linear(h, wd[s + n + ".weight"], wd[s + n + ".bias"]).view(B, L, H, d).transpose(1, 2)
               for n in ("q_proj", "k_proj", "v_proj"))
    a = torch.softmax((q * d ** -0.5) @ k.transpose(-1, -2), dim=-1) @ v
    a = a.transpose(1, 2).reshape(B, L, D)
    x = x + F.linear(a, wd[s + "out_proj.weight"], wd[s + "out_proj.bias"])
    h = F.layer_norm(x, (D,), wd[b + "layer_norm2.weight"], wd[b + "layer_norm2.bias"], cfg.layer_norm_eps)
    h = F.linear(h, wd[b + "mlp.fc1.weight"], wd[b + "mlp.fc1.bias"])
    h = h * torch.sigmoid(1.702 * h) if cfg.hidden_act == "quick_gelu" else F.gelu(h)
    return x + F.linear(h, wd[b + "mlp.fc2.weight"], wd[b + "mlp.fc2.bias"])


def vision_pooled(pixel_values: torch.Tensor, wd: Dict[str, torch.Tensor], cfg: SafetyConfig,
                  dtype=torch.float32) -> torch.Tensor:
    """pixel_values [B, 3, S, S] -> `CLIPVisionModel(...).pooler_output` [B, hidden], computed in `dtype`."""
    with torch.no_grad():
        wd = {k: v.to(dtype) for k, v in wd.items()}
        p = _PREFIX
        x = F.conv2d(pixel_values.to(dtype), wd[p + "embeddings.patch_embedding.weight"], stride=cfg.patch_size)
        x = x.flatten(2).transpose(1, 2)                                   # [B, P, D]
        cls = wd[p + "embeddings.class_embedding"].expand(x.shape[0], 1, -1)
        x = torch.cat([cls, x], dim=1) + wd[p + "embeddings.position_embedding.weight"]
        D = x.shape[-1]
        x = F.layer_norm(x, (D,), wd[p + "pre_layrnorm.weight"], wd[p + "pre_layrnorm.bias"], cfg.layer_norm_eps)
        for i in range(cfg.num_hidden_layers):
            x = _layer(x, wd, f"{p}encoder.layers.{i}.", cfg)
        return F.layer_norm(x[:, 0], (D,), wd[p + "post_layernorm.weight"], wd[p + "post_layernorm.bias"],
                            cfg.layer_norm_eps)


def image_embeds(pixel_values: torch.Tensor, wd: Dict[str, torch.Tensor], cfg: SafetyConfig,
                 dtype=torch.float32) -> torch.Tensor:
    """`visual_projection(pooled)` [B, projection_dim]."""
    with torch.no_grad():
        return F.linear(vision_pooled(pixel_values, wd, cfg, dtype), wd["visual_projection.weight"].to(dtype))


def cosines(emb: torch.Tensor, wd: Dict[str, torch.Tensor], dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """(special [B, n_special], concept [B, n_concepts]) cosine_distance of diffusers' safety_checker.py."""
    with torch.no_grad():
        e = F.normalize(emb.to(dtype))
        return (e @ F.normalize(wd["special_care_embeds"].to(dtype)).t(),
                e @ F.normalize(wd["concept_embeds"].to(dtype)).t())


def decide(cos_special, cos_concept, thr_special, thr_concept) -> np.ndarray:
    """has_nsfw_concept per image: StableDiffusionSafetyChecker.forward's loop on numpy float32 (the cosines are
    `.cpu().float().numpy()` there; Python scalars do not widen a float32)."""
    cs, cc = np.asarray(cos_special, dtype=np.float32), np.asarray(cos_concept, dtype=np.float32)
    ts, tc = np.asarray(thr_special, dtype=np.float32), np.asarray(thr_concept, dtype=np.float32)
    flags = np.zeros(cc.shape[0], dtype=bool)
    for i in range(cc.shape[0]):
        adjustment = np.float32(0.0)          # (float32 whatever the numpy version's scalar promotion)
        for k in range(cs.shape[1]):
            if round(cs[i][k] - ts[k] + adjustment, 3) > 0:
                adjustment = np.float32(0.01)
        for k in range(cc.shape[1]):
            if round(cc[i][k] - tc[k] + adjustment, 3) > 0:
                flags[i] = True
    return flags


def check(images_u8, wd: Dict[str, torch.Tensor], cfg: SafetyConfig):
    """(scores float32 [B, n_special + n_concepts], flags bool [B]) of uint8 RGB images, all in fp32."""
    cs, cc = cosines(image_embeds(preprocess(images_u8, cfg), wd, cfg), wd)
    flags = decide(cs.numpy(), cc.numpy(), wd["special_care_embeds_weights"].numpy(),
                   wd["concept_embeds_weights"].numpy())
    return torch.cat([cs, cc], dim=1), flags
