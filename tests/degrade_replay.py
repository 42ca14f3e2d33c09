"""Shared by test_degrade_artifacts_host.py and test_degrade_artifacts_gpu.py (not a test module): the reference
generator's draws (scripts/make_synthetic_pairs.py:38-81, :162-190) replayed by hand from the seeded `random` /
`np.random` streams, and the outputs those parameters give under the host references."""
import random

import numpy as np

from image_restoration_and_enhancement_amd import degrade as D
from image_restoration_and_enhancement_amd import degrade_host as DH
from oracle import degrade_ref as R


def replay_degrade_sr(use_jpeg, use_motion_blur):
    """degrade_sr (:67-81) -> {"motion": (kernel size, angle) | None, "k": Gaussian size | None, "q": quality | None}."""
    p = {"motion": None, "k": None, "q": None}
    if use_motion_blur and random.random() < 0.3:
        ks = random.randint(5, 12)
        p["motion"] = (ks, random.uniform(0, 360))
    else:
        p["k"] = random.choice([3, 5, 7])
    if use_jpeg:
        p["q"] = random.randint(40, 85)
    return p


def replay_make_pairs(B, H, W, denoise_with_artifacts, sr_with_jpeg, sr_with_motion_blur, easy_ratio=0.7):
    """process_split's loop body (:162-190), image by image -> a list of per-image parameter dicts."""
    per = []
    for _ in range(B):
        p = {"dn_q": None, "dn_motion": None}
        p["sigma"] = random.uniform(3, 15) if denoise_with_artifacts else random.uniform(5, 8)
        p["z"] = np.random.randn(H, W, 3)
        if denoise_with_artifacts:
            if random.random() < 0.3:
                p["dn_q"] = random.randint(40, 85)
            if random.random() < 0.2:
                ks = random.randint(3, 8)
                p["dn_motion"] = (ks, random.uniform(0, 360))
        p["sr"] = replay_degrade_sr(sr_with_jpeg, sr_with_motion_blur)
        p["easy"] = random.random() < easy_ratio
        p["strokes"] = D.draw_free_form_strokes(H, W, (3, 7), (5, 20)) if p["easy"] else \
            D.draw_free_form_strokes(H, W, (8, 15), (20, 40))
        per.append(p)
    return per


def expected_sr(img, p, scale, rgb=False):
    """One image through degrade_sr's pixel work under the replayed parameters `p`."""
    if p["motion"] is not None:
        blur = DH.motion_blur_ref(img, DH.motion_kernel_taps(*p["motion"])[0])
    else:
        blur = R.gaussian_blur_u8(img, p["k"])
    lr = R.resize_cubic_down_u8(blur, scale)
    if p["q"] is not None:
        lr = DH.jpeg_roundtrip_ref(lr, p["q"], rgb)
    return lr


def expected_pairs(imgs, per, scale, rgb=False, mode="simple"):
    """The make_pairs outputs for uint8 [B][H][W][3] `imgs` under the replayed parameters (grayscale `mode`
    "simple" is integer-exact on the GPU; "lab" is fp32 there and within one level of the float64 oracle)."""
    H, W = imgs.shape[1:3]
    out = {"denoise": [], "sr": [], "colorize": [], "inpaint": [], "inpaint_mask": []}
    for img, p in zip(imgs, per):
        noisy = R.add_gaussian_noise(img, p["sigma"], p["z"])
        if p["dn_q"] is not None:
            noisy = DH.jpeg_roundtrip_ref(noisy, p["dn_q"], rgb)
        if p["dn_motion"] is not None:
            noisy = DH.motion_blur_ref(noisy, DH.motion_kernel_taps(*p["dn_motion"])[0])
        out["denoise"].append(noisy)
        out["sr"].append(expected_sr(img, p["sr"], scale, rgb))
        out["colorize"].append(R.gray_lab_u8(img, rgb) if mode == "lab" else R.gray_simple_u8(img, rgb))
        mask = R.stroke_mask(H, W, p["strokes"])
        masked = img.copy()
        masked[mask == 255] = 0
        out["inpaint"].append(masked)
        out["inpaint_mask"].append(mask)
    return {k: np.stack(v) for k, v in out.items()}
