"""Inputs shared by tests/test_jpeg_host.py and tests/test_jpeg_gpu.py: the sizes, qualities and seeded images the
baseline encoder is pinned on.  Odd block counts (24x40, 17x33, 8x8, 40x24, 33x47, 50x70) need libjpeg's dummy-block
rule; 16x16, 64x96, 9x9 and the constant image do not."""
import io

import numpy as np

# (name, H, W, quality, kind)
CASES = [("n8", 8, 8, 50, "noise"), ("n16", 16, 16, 75, "noise"), ("n17x33", 17, 33, 90, "noise"),
         ("n24x40", 24, 40, 75, "noise"), ("n40x24", 40, 24, 10, "noise"), ("n33x47", 33, 47, 100, "noise"),
         ("n9", 9, 9, 1, "noise"), ("r64x96", 64, 96, 75, "ramp"), ("r50x70", 50, 70, 95, "ramp"),
         ("c32", 32, 32, 75, "const")]
IDS = [c[0] for c in CASES]

# seeds of the noise cases (default H * 1000 + W); 33x47 at quality 100: the first seed with a 10-bit AC value
SEEDS = {"n33x47": 73}

# the constant 32x32 image (every sample 200) at quality 75: luma DC 72 (category 7) once, then DC differences of
# zero and EOBs: 11110 1001000 1010, 15 x (00 1010), then (00 00) x 2 per MCU, (00 1010) x 4 in between: 138 bits,
# padded with six 1-bits.  It follows from Annex K alone, so the check needs no Pillow.
CONST_VALUE = 200
CONST_SCAN = bytes.fromhex("f48a28a2800a28a2800a28a2800a28a2803f")


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def ramp(H, W, seed):
    """A smooth ramp plus mild noise: mostly small coefficients and long zero runs."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (2.0 * xx + 1.5 * yy)[..., None] + np.array([0, 40, 90])
    return np.clip(base % 256 * 0.9 + rng.normal(0, 4, (H, W, 3)), 0, 255).astype(np.uint8)


def case_image(case):
    name, H, W, _, kind = case
    return image(H, W, kind, SEEDS.get(name))


def image(H, W, kind, seed=None):
    seed = H * 1000 + W if seed is None else seed
    if kind == "noise":
        return noise(H, W, seed)
    if kind == "ramp":
        return ramp(H, W, seed)
    return np.full((H, W, 3), CONST_VALUE, np.uint8)


def pillow_bytes(img, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def have_turbo():
    try:
        from PIL import features
    except ImportError:
        return False
    return bool(features.check_feature("libjpeg_turbo"))
