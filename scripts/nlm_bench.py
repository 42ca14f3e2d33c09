"""Throughput of the GPU fast-NLM invoker (csrc/nlmeans.hip) on the reference's classical denoise setting:
fastNlMeansDenoisingColored(h = hColor = 20, template 7, search 21) on synthetic noisy 512x512 Lab batches
resident in HBM (L group + ab group = two launches per batch).  Prints one JSON line; `--cpu` adds the
product numpy form (classical.nl_means_u8, 1 core) on one image as the CPU reference point."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import classical as CL
from image_restoration_and_enhancement_amd import nlmeans as N

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--cpu", action="store_true")
ap.add_argument("--strip2", type=int, default=0, help="irx option nlm2_strip (0: library default)")
a = ap.parse_args()

if a.strip2:
    L.call("irx_set_option", b"nlm2_strip", a.strip2)
rng = np.random.default_rng(0)
y, x = np.mgrid[0:a.size, 0:a.size]
clean = np.stack([(x + y) / 4, 128 + 40 * np.sin(x / 25.0), 128 + 40 * np.cos(y / 30.0)], -1)
noisy = np.clip(np.rint(clean[None] + rng.normal(0, 8, (a.batch, *clean.shape))), 0, 255).astype(np.uint8)
lab = torch.from_numpy(noisy).cuda()
out = torch.empty_like(lab)
for _ in range(2):
    N.denoise_group(lab, out, 20.0, 0, 1)
    N.denoise_group(lab, out, 20.0, 1, 2)
torch.cuda.synchronize()
L.profile_begin()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(a.iters):
    N.denoise_group(lab, out, 20.0, 0, 1)
    N.denoise_group(lab, out, 20.0, 1, 2)
e1.record()
torch.cuda.synchronize()
prof = L.profile_end()
ms = e0.elapsed_time(e1) / a.iters
pix = a.batch * a.size * a.size
res = {"metric": "fastNlMeansDenoisingColored 7/21, images/s", "value": round(a.batch / (ms / 1e3), 2),
       "unit": "images/s", "ms_per_batch": round(ms, 3), "batch": a.batch, "size": a.size,
       "mpix_per_s": round(pix / (ms / 1e3) / 1e6, 1),
       # distance taps evaluated by the direct form: 441 offsets x 49 taps x 3 channels per pixel
       "direct_taps_per_s_T": round(pix * 441 * 49 * 3 / (ms / 1e3) / 1e12, 3),
       "hbm_bytes_per_batch": 2 * pix * 3 * 2,
       "kernels": [(n, c, round(t / max(c, 1) * 1e3, 1)) for n, c, t, _ in prof]}
rgb = lab
for name, fn in (("bilateral_9_75_75", lambda: N.bilateral_filter(rgb, 9, 75, 75)),
                 ("median_5", lambda: N.median_blur(rgb, 5))):
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    res[name + "_ms_per_batch"] = round(e0.elapsed_time(e1) / a.iters, 3)
# the whole classical denoise chain at strength 0.9 on the batch (device-resident): LBGR->Lab, NLM L + ab,
# Lab->LBGR, bilateral(9, 75, 75), median(5) -- what RestorationPipeline._denoise_opencv runs per image
def chain():
    d = N.fast_nl_means_denoising_colored(rgb, 20.0, 20.0)
    return N.median_blur(N.bilateral_filter(d, 9, 75, 75), 5)


chain()
torch.cuda.synchronize()
e0.record()
for _ in range(a.iters):
    chain()
e1.record()
torch.cuda.synchronize()
cms = e0.elapsed_time(e1) / a.iters
res["denoise_chain_ms_per_batch"] = round(cms, 3)
res["denoise_chain_images_per_s"] = round(a.batch / (cms / 1e3), 1)
if a.cpu:
    t = time.time()
    img = noisy[0]
    CL.nl_means_u8(img[..., :1], 20.0)
    CL.nl_means_u8(img[..., 1:], 20.0)
    res["cpu_baseline"] = {"value": round(1 / (time.time() - t), 4), "unit": "images/s", "cores": 1,
                           "kind": "port", "sample": f"1 image {a.size}^2, classical.nl_means_u8 (numpy)"}
    from PIL import Image
    t = time.time()
    CL.denoise_opencv(Image.fromarray(noisy[0]), 0.9)
    res["cpu_denoise_chain_images_per_s"] = round(1 / (time.time() - t), 4)
print(json.dumps(res))
