"""Model / scheduler configuration for the SD-1.5 restoration engine.

The reference never defines these shapes itself: they come from the diffusers
component configs saved next to each task's weights
(`outputs/models/{task}/best/{unet,vae,text_encoder,scheduler}/*.json`, e.g.
`outputs/models/denoising/best/unet/config.json:5-67`,
`outputs/models/denoising/best/vae/config.json:5-37`,
`outputs/models/denoising/best/text_encoder/config.json:10-23`,
`outputs/models/denoising/best/scheduler/scheduler_config.json:2-13`).
The defaults below restate those files; `*.from_dir()` reads the same JSON
layout from a local model directory so a real `best/` directory drives the
engine unchanged.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field, asdict
from pathlib import Path
from typing import List, Optional


@dataclass
class UNetConfig:
    in_channels: int = 4               # 9 for the inpainting UNet (inpainting/best/unet/config.json:37)
    out_channels: int = 4
    block_out_channels: List[int] = field(default_factory=lambda: [320, 640, 1280, 1280])
    layers_per_block: int = 2
    attention_heads: int = 8           # config "attention_head_dim": 8 is the head COUNT in SD-1.5
    cross_attention_dim: int = 768
    norm_num_groups: int = 32
    norm_eps: float = 1e-5
    sample_size: int = 64
    flip_sin_to_cos: bool = True
    freq_shift: int = 0
    # CrossAttnDownBlock2D x3 + DownBlock2D; UpBlock2D + CrossAttnUpBlock2D x3
    down_attn: List[bool] = field(default_factory=lambda: [True, True, True, False])
    up_attn: List[bool] = field(default_factory=lambda: [False, True, True, True])

    @classmethod
    def from_dict(cls, d: dict) -> "UNetConfig":
        c = cls()
        c.in_channels = int(d.get("in_channels", c.in_channels))
        c.out_channels = int(d.get("out_channels", c.out_channels))
        c.block_out_channels = list(d.get("block_out_channels", c.block_out_channels))
        c.layers_per_block = int(d.get("layers_per_block", c.layers_per_block))
        heads = d.get("num_attention_heads") or d.get("attention_head_dim", c.attention_heads)
        if isinstance(heads, (list, tuple)):
            heads = heads[0]
        c.attention_heads = int(heads)
        c.cross_attention_dim = int(d.get("cross_attention_dim", c.cross_attention_dim))
        c.norm_num_groups = int(d.get("norm_num_groups", c.norm_num_groups))
        c.norm_eps = float(d.get("norm_eps", c.norm_eps))
        c.sample_size = int(d.get("sample_size", c.sample_size))
        c.flip_sin_to_cos = bool(d.get("flip_sin_to_cos", c.flip_sin_to_cos))
        c.freq_shift = int(d.get("freq_shift", c.freq_shift))
        if "down_block_types" in d:
            c.down_attn = [t.startswith("CrossAttn") for t in d["down_block_types"]]
        if "up_block_types" in d:
            c.up_attn = [t.startswith("CrossAttn") for t in d["up_block_types"]]
        if d.get("use_linear_projection", False):
            raise ValueError("use_linear_projection=True UNets are not SD-1.5; unsupported")
        return c


@dataclass
class VAEConfig:
    in_channels: int = 3
    out_channels: int = 3
    latent_channels: int = 4
    block_out_channels: List[int] = field(default_factory=lambda: [128, 256, 512, 512])
    layers_per_block: int = 2
    norm_num_groups: int = 32
    norm_eps: float = 1e-6
    scaling_factor: float = 0.18215
    sample_size: int = 512

    @classmethod
    def from_dict(cls, d: dict) -> "VAEConfig":
        c = cls()
        for k in ("in_channels", "out_channels", "latent_channels", "layers_per_block",
                  "norm_num_groups", "sample_size"):
            if k in d:
                setattr(c, k, int(d[k]))
        if "block_out_channels" in d:
            c.block_out_channels = list(d["block_out_channels"])
        if "scaling_factor" in d:
            c.scaling_factor = float(d["scaling_factor"])
        return c


@dataclass
class CLIPConfig:
    vocab_size: int = 49408
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    max_position_embeddings: int = 77
    layer_norm_eps: float = 1e-5
    hidden_act: str = "quick_gelu"

    @classmethod
    def from_dict(cls, d: dict) -> "CLIPConfig":
        c = cls()
        for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers",
                  "num_attention_heads", "max_position_embeddings"):
            if k in d:
                setattr(c, k, int(d[k]))
        if "layer_norm_eps" in d:
            c.layer_norm_eps = float(d["layer_norm_eps"])
        if "hidden_act" in d:
            c.hidden_act = str(d["hidden_act"])
        if c.hidden_act not in ("quick_gelu", "gelu"):
            raise ValueError(f"unsupported CLIP activation {c.hidden_act}")
        return c


@dataclass
class SafetyConfig:
    """diffusers' StableDiffusionSafetyChecker: `safety_checker/config.json` (its `vision_config` is the CLIP ViT-L/14
    tower; the defaults restate the file of `sd-legacy/stable-diffusion-v1-5`) and `feature_extractor/
    preprocessor_config.json` (CLIPImageProcessor).  Only what those two files set in the SD-1.5 snapshot is supported:
    anything else is a ValueError, never a silent approximation."""
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    patch_size: int = 14
    image_size: int = 224
    layer_norm_eps: float = 1e-5
    hidden_act: str = "quick_gelu"
    projection_dim: int = 768
    n_special: int = 3                 # rows of special_care_embeds
    n_concepts: int = 17               # rows of concept_embeds
    # CLIPImageProcessor
    resize_size: int = 224             # the shortest edge after the resize (Pillow BICUBIC)
    crop_size: int = 224               # the centre crop, square
    rescale_factor: float = 1 / 255
    image_mean: List[float] = field(default_factory=lambda: [0.48145466, 0.4578275, 0.40821073])
    image_std: List[float] = field(default_factory=lambda: [0.26862954, 0.26130258, 0.27577711])

    @classmethod
    def from_dict(cls, d: dict) -> "SafetyConfig":
        c = cls()
        v = d.get("vision_config") or d.get("vision_config_dict") or {}
        for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "patch_size",
                  "image_size"):
            if k in v:
                setattr(c, k, int(v[k]))
        if "layer_norm_eps" in v:
            c.layer_norm_eps = float(v["layer_norm_eps"])
        if "hidden_act" in v:
            c.hidden_act = str(v["hidden_act"])
        if "projection_dim" in d:
            c.projection_dim = int(d["projection_dim"])
        elif "projection_dim" in v:
            c.projection_dim = int(v["projection_dim"])
        if c.hidden_act not in ("quick_gelu", "gelu"):
            raise ValueError(f"unsupported CLIP activation {c.hidden_act}")
        if c.image_size % c.patch_size or c.hidden_size % c.num_attention_heads:
            raise ValueError("safety checker: image_size must be a multiple of patch_size and hidden_size of the heads")
        c.resize_size = c.crop_size = c.image_size
        return c

    def from_preprocessor(self, d: dict) -> "SafetyConfig":
        """The same config with `preprocessor_config.json` read into it: both the old form (`"size": 224,
        "crop_size": 224`) and the new one (`{"shortest_edge": 224}`, `{"height": 224, "width": 224}`)."""
        for k in ("do_resize", "do_center_crop", "do_normalize", "do_rescale"):
            if not d.get(k, True):
                raise ValueError(f"safety checker preprocessor: {k} = false is unsupported")
        if int(d.get("resample", 3)) != 3:
            raise ValueError(f"safety checker preprocessor: resample {d.get('resample')} is unsupported (3, BICUBIC)")
        size = d.get("size", self.resize_size)
        if isinstance(size, dict):
            if set(size) != {"shortest_edge"}:
                raise ValueError(f"safety checker preprocessor: size {size} is unsupported (shortest_edge)")
            size = size["shortest_edge"]
        crop = d.get("crop_size", self.crop_size)
        if isinstance(crop, dict):
            if set(crop) != {"height", "width"} or crop["height"] != crop["width"]:
                raise ValueError(f"safety checker preprocessor: crop_size {crop} is unsupported (a square)")
            crop = crop["height"]
        if int(crop) != self.image_size:
            raise ValueError(f"safety checker preprocessor: crop_size {crop} is not the tower's image_size "
                             f"{self.image_size}")
        if int(size) < int(crop):
            raise ValueError(f"safety checker preprocessor: size {size} below crop_size {crop} (the crop would pad)")
        self.resize_size, self.crop_size = int(size), int(crop)
        if "rescale_factor" in d:
            self.rescale_factor = float(d["rescale_factor"])
        for k in ("image_mean", "image_std"):
            if k in d:
                val = [float(x) for x in d[k]]
                if len(val) != 3:
                    raise ValueError(f"safety checker preprocessor: {k} must have three entries")
                setattr(self, k, val)
        return self

    @classmethod
    def from_dir(cls, checker_dir: str | Path, preprocessor_dir: str | Path | None = None) -> "SafetyConfig":
        """`<checker_dir>/config.json`, and `preprocessor_config.json` from `preprocessor_dir` (default: the
        `feature_extractor/` directory next to `checker_dir`) when that file exists."""
        p = Path(checker_dir)
        c = cls.from_dict(json.loads((p / "config.json").read_text()))
        f = (Path(preprocessor_dir) if preprocessor_dir else p.parent / "feature_extractor") / "preprocessor_config.json"
        return c.from_preprocessor(json.loads(f.read_text())) if f.exists() else c


@dataclass
class SchedulerConfig:
    kind: str = "pndm"                 # "pndm" (denoise/sr/colorize) | "ddim" (inpaint)
    num_train_timesteps: int = 1000
    beta_start: float = 0.00085
    beta_end: float = 0.012
    beta_schedule: str = "scaled_linear"
    steps_offset: int = 1
    set_alpha_to_one: bool = False
    skip_prk_steps: bool = True
    timestep_spacing: str = "leading"
    prediction_type: str = "epsilon"

    @classmethod
    def from_dict(cls, d: dict) -> "SchedulerConfig":
        c = cls()
        name = d.get("_class_name", "PNDMScheduler")
        if name == "PNDMScheduler":
            c.kind = "pndm"
        elif name == "DDIMScheduler":
            c.kind = "ddim"
        else:
            raise ValueError(f"unsupported scheduler {name}")
        for k in ("num_train_timesteps", "steps_offset"):
            if k in d:
                setattr(c, k, int(d[k]))
        for k in ("beta_start", "beta_end"):
            if k in d:
                setattr(c, k, float(d[k]))
        for k in ("beta_schedule", "timestep_spacing", "prediction_type"):
            if k in d:
                setattr(c, k, str(d[k]))
        for k in ("set_alpha_to_one", "skip_prk_steps"):
            if k in d:
                setattr(c, k, bool(d[k]))
        if c.beta_schedule != "scaled_linear" or c.timestep_spacing != "leading":
            raise ValueError("only scaled_linear / leading schedules (the saved SD-1.5 configs) are supported")
        if c.prediction_type != "epsilon":
            raise ValueError("only epsilon prediction is supported")
        if c.kind == "pndm" and not c.skip_prk_steps:
            raise ValueError("PNDM with PRK warm-up steps is not used by the reference configs")
        if d.get("thresholding", False) or d.get("clip_sample", False):
            raise ValueError("DDIM thresholding/clip_sample are off in the reference configs")
        return c


@dataclass
class PipelineConfig:
    """Everything one task's `best/` directory describes."""
    unet: UNetConfig
    vae: VAEConfig
    clip: CLIPConfig
    scheduler: SchedulerConfig
    model_dir: Optional[str] = None

    @classmethod
    def default(cls, task: str) -> "PipelineConfig":
        unet = UNetConfig(in_channels=9 if task == "inpaint" else 4)
        sched = SchedulerConfig(kind="ddim" if task == "inpaint" else "pndm")
        return cls(unet=unet, vae=VAEConfig(), clip=CLIPConfig(), scheduler=sched)

    @classmethod
    def from_dir(cls, model_dir: str | Path, task: str) -> "PipelineConfig":
        p = Path(model_dir)
        base = cls.default(task)

        def rd(*parts):
            f = p.joinpath(*parts)
            return json.loads(f.read_text()) if f.exists() else None

        d = rd("unet", "config.json")
        unet = UNetConfig.from_dict(d) if d else base.unet
        d = rd("vae", "config.json")
        vae = VAEConfig.from_dict(d) if d else base.vae
        d = rd("text_encoder", "config.json")
        clip = CLIPConfig.from_dict(d) if d else base.clip
        d = rd("scheduler", "scheduler_config.json")
        sched = SchedulerConfig.from_dict(d) if d else base.scheduler
        return cls(unet=unet, vae=vae, clip=clip, scheduler=sched, model_dir=str(p))

    def to_dict(self) -> dict:
        return {"unet": asdict(self.unet), "vae": asdict(self.vae), "clip": asdict(self.clip),
                "scheduler": asdict(self.scheduler), "model_dir": self.model_dir}
