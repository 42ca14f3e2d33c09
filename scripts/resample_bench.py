"""Timing of the GPU PIL resize (csrc/resample.hip) against Pillow on the host, per shape:
  * the kernel's device time (the library profiler's HIP event pair around each of `--iters` launches on
    device-resident data; `launch_loop_us` is one event pair around the whole loop) beside its byte-count floor:
    (source bytes + destination bytes) / 8.0 TB/s, the HBM3E peak — every source byte read once, every
    destination byte written once;
  * the wall time of the PIL-in / PIL-out GPU form `resample.resize_pil` (upload, kernel, download; it ends in a
    device-to-host copy, so the host clock covers the device work), median of `--reps` calls;
  * Pillow's wall time for the same `Image.resize` call on the host, median of `--reps` calls.
The first four shapes are the kernel's reference shapes; the last three are the drop-in's call sites that return a
PIL image (_sr_lanczos on a demo image, _cap_area, normalize_mask), which decide their wiring.
Prints one JSON line per shape and a final summary line.  Needs a GPU: there is no CPU timing fallback."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import resample as RS

HBM_PEAK = 8.0e12      # bytes/s

# name, mode, (W, H) -> (w, h)
SHAPES = [("x4_512_to_2048", "RGB", (512, 512), (2048, 2048)),
          ("demo_640x457_to_512", "RGB", (640, 457), (512, 512)),
          ("one_axis_640x457_to_640x456", "RGB", (640, 457), (640, 456)),
          ("mask_640x457_to_512", "L", (640, 457), (512, 512)),
          ("site_sr_lanczos_x4_160x114", "RGB", (160, 114), (640, 456)),
          ("site_cap_area_1100x1000", "RGB", (1100, 1000), (1024, 930)),
          ("site_normalize_mask_500x333_to_640x457", "L", (500, 333), (640, 457))]

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5000, help="kernel launches per device timing (a window of >= 0.1 s)")
ap.add_argument("--reps", type=int, default=50, help="calls per wall-clock median")
ap.add_argument("--filter", default="lanczos", choices=["lanczos", "bicubic"])
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("resample_bench: no GPU (device times are not estimated on the host)")
pil_filter = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC}[a.filter]


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts)


rng = np.random.default_rng(0)
rows = []
for name, mode, (W, H), (w, h) in SHAPES:
    C = 3 if mode == "RGB" else 1
    arr = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    img = Image.fromarray(arr if C == 3 else arr[..., 0], mode)
    x = torch.from_numpy(arr).cuda()
    out = torch.empty((h, w, C), dtype=torch.uint8, device="cuda")
    for _ in range(5):                                   # warm: code object, tables
        RS.resize_u8(x, (w, h), a.filter, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    L.profile_begin()                                    # a HIP event pair around every launch
    e0.record()
    for _ in range(a.iters):
        RS.resize_u8(x, (w, h), a.filter, out=out)
    e1.record()
    torch.cuda.synchronize()
    prof = [p for p in L.profile_end() if "resample_kernel" in p[0]]
    assert len(prof) == 1 and prof[0][1] == a.iters, prof
    kernel_us = prof[0][2] / a.iters * 1e3
    loop_us = e0.elapsed_time(e1) / a.iters * 1e3        # launch to launch, the host's enqueue rate included
    same = bool(np.array_equal(out.cpu().numpy(), np.asarray(img.resize((w, h), pil_filter)).reshape(h, w, C)))
    nbytes = (H * W + h * w) * C
    for _ in range(3):
        RS.resize_pil(img, (w, h), pil_filter, "cuda")
    gpu_med, gpu_min = wall_ms(lambda: RS.resize_pil(img, (w, h), pil_filter, "cuda"), a.reps)
    pil_med, pil_min = wall_ms(lambda: img.resize((w, h), pil_filter), a.reps)
    row = {"shape": name, "mode": mode, "in": [W, H], "out": [w, h], "filter": a.filter,
           "equals_pillow": same,
           "kernel_us": round(kernel_us, 2), "launch_loop_us": round(loop_us, 2), "bytes": nbytes,
           "floor_us": round(nbytes / HBM_PEAK * 1e6, 3),
           "kernel_GBps": round(nbytes / (kernel_us * 1e-6) / 1e9, 1),
           "pil_to_pil_gpu_ms_median": round(gpu_med, 3), "pil_to_pil_gpu_ms_min": round(gpu_min, 3),
           "pillow_host_ms_median": round(pil_med, 3), "pillow_host_ms_min": round(pil_min, 3),
           "gpu_form_faster": bool(gpu_med < pil_med)}
    rows.append(row)
    print(json.dumps(row), flush=True)
print(json.dumps({"metric": "PIL resize, GPU form vs Pillow on the host", "iters": a.iters, "reps": a.reps,
                  "device": torch.cuda.get_device_name(0), "pillow": Image.__version__,
                  "all_equal_pillow": all(r["equals_pillow"] for r in rows),
                  "gpu_form_faster": {r["shape"]: r["gpu_form_faster"] for r in rows}}))
