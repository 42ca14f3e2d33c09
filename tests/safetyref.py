"""Shared inputs of the safety-checker tests: the tower configurations, seeded weights under the checkpoint's names,
uint8 images, the literal diffusers decision loop, and the directed / random decision rows.

No weights are committed.  `weights(name)` draws every tensor of `weights.param_specs("safety", cfg)` from the project's
seeded initialiser; the real checkpoint (`safety_checker/model.safetensors` of sd-legacy/stable-diffusion-v1-5) is a
download."""
import functools

import numpy as np
import torch

from image_restoration_and_enhancement_amd import safety_host as H
from image_restoration_and_enhancement_amd import weights as W
from image_restoration_and_enhancement_amd.configs import SafetyConfig

N_SPECIAL, N_CONCEPTS = 3, 17

# name: the geometry, what it exercises
CONFIGS = {
    # 5 tokens, 2 heads of d = 64: the small case
    "A": dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, patch_size=14,
              image_size=28, projection_dim=32),
    # 65 tokens: one key past a 64-key attention tile
    "B": dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, patch_size=14,
              image_size=112, projection_dim=32),
    # the real width, one layer: K = 588 padding, the real tile plans, the Lk = 257 tail
    "C": dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=1, num_attention_heads=16, patch_size=14,
              image_size=224, projection_dim=768),
}
# (H, W) of the preprocessing cases: landscape, portrait, the crop size itself, an upscale, a square downscale
SIZES = ((333, 500), (457, 300), (224, 224), (80, 120), (512, 512))


# The class token reaches the image only through attention, and with the initialiser's gains one or two layers leave
# token 0 dominated by the class and position embeddings every image shares (cosines of 0.8-0.9 between a black and a
# white image; the real checkpoint has 24 layers to do better).  The seeded weights scale every attention output
# projection by this, which puts those cosines below 0: the flags of the model tests then have a wide margin.
ATTN_GAIN = 4.0
# solid colours whose embeddings lie far apart under weights(): rows 1 and 2 have cosines below 0.1 with row 0 in all
# three configurations (asserted on the host by the model test before the GPU is asked)
SOLID = ((0, 0, 0), (255, 255, 255), (255, 255, 0))


def solid_images(side: int) -> np.ndarray:
    """uint8 [3, side, side, 3]: black, white, yellow."""
    return np.stack([np.broadcast_to(np.array(c, np.uint8), (side, side, 3)).copy() for c in SOLID])


def config(name: str) -> SafetyConfig:
    c = SafetyConfig(**CONFIGS[name], n_special=N_SPECIAL, n_concepts=N_CONCEPTS)
    c.resize_size = c.crop_size = c.image_size
    return c


@functools.lru_cache(maxsize=4)
def weights(name: str, seed: int = 0):
    """The checked float32 state dict of configuration `name` (shared by the tests: do not modify it)."""
    cfg = config(name)
    sd = W.random_state_dict("safety", cfg, seed)
    for k in sd:
        if k.endswith("self_attn.out_proj.weight"):
            sd[k] = sd[k] * ATTN_GAIN
    return H.check_weights(sd, cfg)


def images(shape, seed: int = 0) -> np.ndarray:
    """uint8 [B, H, W, 3]: a smooth gradient plus uniform noise (a resize of pure noise would be nearly flat)."""
    B, h, w = shape
    rng = np.random.default_rng(2000 + seed + 7 * B + 3 * h + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for b in range(B):
        ph = rng.uniform(0, 6.28, 3)
        base = np.stack([128 + 100 * np.sin(xx / (9 + 4 * c) + yy / (13 - 3 * c) + ph[c]) for c in range(3)], axis=-1)
        out.append(np.clip(base + rng.uniform(-40, 40, base.shape), 0, 255).astype(np.uint8))
    return np.stack(out)


# ------------------------------------------------------------------------------------------- the decision
def diffusers_loop(special_cos_dist, cos_dist, special_care_embeds_weights, concept_embeds_weights):
    """StableDiffusionSafetyChecker.forward (diffusers 0.35.2) from the cosine distances on, written out as there:
    the numpy float32 arrays of `.cpu().float().numpy()`, Python float adjustments, `round(x, 3)`."""
    result = []
    batch_size = cos_dist.shape[0]
    for i in range(batch_size):
        result_img = {"special_scores": {}, "special_care": [], "concept_scores": {}, "bad_concepts": []}
        adjustment = 0.0
        for concept_idx in range(len(special_cos_dist[0])):
            concept_cos = special_cos_dist[i][concept_idx]
            concept_threshold = special_care_embeds_weights[concept_idx].item()
            result_img["special_scores"][concept_idx] = round(concept_cos - concept_threshold + adjustment, 3)
            if result_img["special_scores"][concept_idx] > 0:
                result_img["special_care"].append({concept_idx, result_img["special_scores"][concept_idx]})
                adjustment = 0.01
        for concept_idx in range(len(cos_dist[0])):
            concept_cos = cos_dist[i][concept_idx]
            concept_threshold = concept_embeds_weights[concept_idx].item()
            result_img["concept_scores"][concept_idx] = round(concept_cos - concept_threshold + adjustment, 3)
            if result_img["concept_scores"][concept_idx] > 0:
                result_img["bad_concepts"].append(concept_idx)
        result.append(result_img)
    return np.array([len(res["bad_concepts"]) > 0 for res in result])


def margins(cs, cc, ts, tc):
    """Every float32 `cos - thr + adj` the loop rounds, per row (the adjustment as the loop applies it)."""
    cs, cc, ts, tc = (np.asarray(a, dtype=np.float32) for a in (cs, cc, ts, tc))
    out = []
    for i in range(cc.shape[0]):
        adj, row = np.float32(0.0), []
        for k in range(cs.shape[1]):
            x = cs[i][k] - ts[k] + adj
            row.append(x)
            if round(x, 3) > 0:
                adj = np.float32(0.01)
        row += [cc[i][k] - tc[k] + adj for k in range(cc.shape[1])]
        out.append(row)
    return np.array(out, dtype=np.float32)


def random_rows(n: int, seed: int, edge: float = 1e-3):
    """(cos_special [n, 3], cos_concept [n, 17], thr_special [3], thr_concept [17]) float32, cosines around their
    thresholds so that about half the rows are flagged, redrawn until every rounded quantity is at least `edge` away
    from the rounding edge 0.0005."""
    rng = np.random.default_rng(seed)
    ts = rng.uniform(0.1, 0.3, N_SPECIAL).astype(np.float32)
    tc = rng.uniform(0.1, 0.3, N_CONCEPTS).astype(np.float32)
    cs = np.empty((n, N_SPECIAL), np.float32)
    cc = np.empty((n, N_CONCEPTS), np.float32)
    for i in range(n):
        while True:
            s = (ts + rng.uniform(-0.06, 0.02, N_SPECIAL)).astype(np.float32)
            c = (tc + rng.uniform(-0.06, 0.003, N_CONCEPTS)).astype(np.float32)
            if np.all(np.abs(margins(s[None], c[None], ts, tc) - 0.0005) >= edge):
                break
        cs[i], cc[i] = s, c
    return cs, cc, ts, tc


# directed rows with exact cosines: the image embedding and every concept embedding are one-hot, so a cosine is exactly
# 1 (same axis) or 0, and thr = 1 - x puts `cos - thr` at x (1 - (1 - x) is exact for these x in float32, up to the
# rounding of 1 - x itself).  The image is the unit vector of axis 0; concept row 0 lies on that axis, and so does
# special row 0 where the case has a special-care hit; every other row lies on an axis of its own.
#   name: (special x or None, concept x, flagged)
DIRECTED = {
    "special_flips_concept": (0.05, -0.005, True),    # the 0.01 adjustment lifts -0.005 to +0.005
    "no_special_no_flag": (None, -0.005, False),      # the same concept without the special-care hit
    "below_half": (None, 2.0 ** -11, False),          # 0.000488...: v = 0.488 < 0.5 rounds to 0
    "above_half": (None, 0.000511, True),             # v = 0.511 rounds to 1
}


def directed_case(name: str, n: int):
    """(embeds [1, n], special [3, n], concepts [17, n], thr_special [3], thr_concept [17]) float32 for DIRECTED[name]:
    unit one-hot rows; rows that play no part sit on axes the image has no component on, with threshold 0.5."""
    sx, cx, _ = DIRECTED[name]
    special = np.zeros((N_SPECIAL, n), np.float32)
    concepts = np.zeros((N_CONCEPTS, n), np.float32)
    for k in range(N_SPECIAL):
        special[k, 2 + k] = 1.0
    for k in range(N_CONCEPTS):
        concepts[k, 2 + N_SPECIAL + k] = 1.0
    ts = np.full(N_SPECIAL, 0.5, np.float32)
    tc = np.full(N_CONCEPTS, 0.5, np.float32)
    emb = np.zeros((1, n), np.float32)
    # the image lies on ONE axis (norm exactly 1): axis 0, which special row 0 (if it takes part) and concept row 0 share
    emb[0, 0] = 1.0
    concepts[0] = 0
    concepts[0, 0] = 1.0
    tc[0] = np.float32(1.0) - np.float32(cx)
    if sx is not None:
        special[0] = 0
        special[0, 0] = 1.0
        ts[0] = np.float32(1.0) - np.float32(sx)
    return emb, special, concepts, ts, tc


def host_cosines(emb, special, concepts, dtype=torch.float64):
    """The cosines of `safety_host.cosines` for raw arrays, in `dtype`."""
    wd = {"special_care_embeds": torch.from_numpy(special), "concept_embeds": torch.from_numpy(concepts)}
    cs, cc = H.cosines(torch.from_numpy(emb), wd, dtype)
    return cs.numpy(), cc.numpy()


# ------------------------------------------------------------------------------------------- transformers
def to_transformers_keys(wd, model_keys):
    """The tower's tensors of a checkpoint-named state dict under the keys of `CLIPVisionModel.state_dict()` of the
    installed transformers, matched by suffix (the checkpoint says `vision_model.vision_model.embeddings...`, this
    transformers `embeddings...` or `vision_model.embeddings...`)."""
    prefix = "vision_model.vision_model."
    tower = {k[len(prefix):]: v for k, v in wd.items() if k.startswith(prefix)}
    out = {}
    for mk in model_keys:
        if mk.endswith("position_ids"):
            continue
        hit = [k for k in tower if mk == k or mk.endswith("." + k)]
        assert len(hit) == 1, (mk, hit)
        out[mk] = tower[hit[0]]
    return out
