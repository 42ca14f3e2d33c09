"""Timing of the GPU JPEG encoder against today's save path, per batch shape and input kind:
  (a) `jpeg_gpu.encode` on a device-resident uint8 batch: the kernels, one D2H of the lengths, one of the used bytes,
      header and EOI on the host;
  (b) today's path: D2H of the pixels, then `Image.fromarray(...).save(BytesIO, "JPEG", quality=q)` per image on one
      host thread.
Both end on the host (a D2H copy or host work after a synchronise), so the host clock covers the device work; path
(a) is also bracketed by a HIP event pair.  The two paths alternate, `--repeats` times each after one warm call.
Inputs: seeded ramp + noise images (a typical file size) and pure noise (the worst-case stream).  Reports ms per image
and the bytes moved to the host for both paths; one JSON line per row.  `--kernels-only` runs path (a) alone a few
times, for a kernel trace taken from outside (`rocprofv3 --kernel-trace --stats -- python scripts/jpeg_bench.py
--kernels-only`).  profiles/jpeg_bench.txt holds the rows of one run followed by that trace's kernel statistics.
Needs a GPU: there is no CPU timing fallback."""
import argparse
import io
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_restoration_and_enhancement_amd import jpeg_gpu as JG

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--quality", type=int, default=75)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
ap.add_argument("--kernels-only", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("jpeg_bench: no GPU (device times are not estimated on the host)")


def make(kind, B, S, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:S, 0:S]
    out = []
    for b in range(B):
        base = (0.37 * xx + 0.21 * yy + 40 * np.sin(xx / (17.0 + b)) * np.cos(yy / 23.0))[..., None] + np.array([0, 35, 80])
        out.append(np.clip(base % 256 * 0.85 + rng.normal(0, 5, (S, S, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


def path_gpu(x):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    files = JG.encode(x, a.quality)
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    return files, wall, e0.elapsed_time(e1)


def path_pil(x):
    torch.cuda.synchronize()
    t = time.perf_counter()
    arr = x.cpu().numpy()
    t_copy = (time.perf_counter() - t) * 1e3
    files = []
    for im in arr:
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, "JPEG", quality=a.quality)
        files.append(buf.getvalue())
    return files, (time.perf_counter() - t) * 1e3, t_copy


for S in a.sizes:
    for kind in ("ramp_noise", "noise"):
        B = a.batch
        x = torch.from_numpy(make(kind, B, S, seed=S)).cuda()
        if a.kernels_only:
            for _ in range(3):
                JG.encode(x, a.quality)
            torch.cuda.synchronize()
            continue
        fa, _, _ = path_gpu(x)                       # warm: code objects, allocator
        fb, _, _ = path_pil(x)
        rows = {"gpu": [], "gpu_events": [], "pil": [], "pil_copy": []}
        for _ in range(a.repeats):
            fa, w, ev = path_gpu(x)
            rows["gpu"].append(w)
            rows["gpu_events"].append(ev)
            fb, w, c = path_pil(x)
            rows["pil"].append(w)
            rows["pil_copy"].append(c)
        nfile = sum(len(f) for f in fa)
        print(json.dumps({
            "size": S, "batch": B, "input": kind, "quality": a.quality, "files_equal_pillow": fa == fb,
            "file_bytes_per_image": nfile // B,
            "gpu_ms_per_image": [round(v / B, 3) for v in rows["gpu"]],
            "gpu_event_ms_per_image": [round(v / B, 3) for v in rows["gpu_events"]],
            "pil_ms_per_image": [round(v / B, 3) for v in rows["pil"]],
            "pil_pixel_copy_ms_per_image": [round(v / B, 3) for v in rows["pil_copy"]],
            "gpu_bytes_to_host": nfile - B * (623 + 2) + 4 * B, "pil_bytes_to_host": B * S * S * 3,
            "gpu_faster": bool(min(rows["gpu"]) < min(rows["pil"]))}), flush=True)
if not a.kernels_only:
    print(json.dumps({"metric": "JPEG files from a device batch: jpeg_gpu.encode vs D2H + Pillow save",
                      "device": torch.cuda.get_device_name(0), "pillow": Image.__version__, "repeats": a.repeats}))
