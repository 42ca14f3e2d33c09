"""Timing of the GPU JPEG decoder against today's load path, per shape and quality (batch 8 of Pillow-written files):
  (a) `jpeg_gpu.decode` from the file bytes in host memory: the marker walk, one H2D of the entropy-coded bytes, the
      kernels of csrc/jpeg_decode.hip, one D2H of the statuses;
  (b) today's path (`metrics.load_image` + `to_device`): `Image.open(...).convert("RGB")` per file on one host thread,
      then one H2D of the pixels.
Both end with the pixels on the device and a synchronise, so the host clock covers the device work.  The two paths
alternate, `--repeats` times each after one warm call; every ratio is printed with the spread of its repeats.  Also
reported: `rounds` of the entry-state kernel per image, the device time of the op alone (HIP events around
`irx_jpeg_decode`), and the per-pair time of `evaluate_task(device="cuda")` with decode="gpu" against "pil" on a
directory of 512 x 512 pairs.  `--kernels-only` runs the op alone a few times, for a kernel trace taken from outside
(`rocprofv3 --kernel-trace --stats -- python scripts/jpeg_decode_bench.py --kernels-only`).  profiles/
jpeg_decode_bench.txt holds the rows of one run followed by that trace's kernel statistics.
Needs a GPU: there is no CPU timing fallback."""
import argparse
import contextlib
import io
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_restoration_and_enhancement_amd import jpeg_gpu as JG
from image_restoration_and_enhancement_amd import metrics as M

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--qualities", type=int, nargs="+", default=[75, 95])
ap.add_argument("--shapes", type=str, nargs="+", default=["457x640", "512x512", "2048x2048"])   # H x W; the demo shape first
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--kernels-only", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("jpeg_decode_bench: no GPU (device times are not estimated on the host)")


def image(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (0.37 * xx + 0.21 * yy + 40 * np.sin(xx / (17.0 + seed % 7)) * np.cos(yy / 23.0))[..., None] + np.array([0, 35, 80])
    return np.clip(base % 256 * 0.85 + rng.normal(0, 5, (H, W, 3)), 0, 255).astype(np.uint8)


def jpeg(img, q):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=q)
    return buf.getvalue()


def path_gpu(files):
    t = time.perf_counter()
    out = JG.decode(files, device="cuda")
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def path_pil(files):
    t = time.perf_counter()
    arr = [np.array(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
    t_dec = (time.perf_counter() - t) * 1e3
    out = torch.from_numpy(np.stack(arr)).cuda()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3, t_dec


def op_alone(files):
    """Device time of irx_jpeg_decode (HIP events), and rounds."""
    infos = [JG.parse(f)[1] for f in files]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _, status, rounds = JG.decode_device(files, infos, "RGB", torch.device("cuda"))
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), status, rounds      # includes the H2D of the scans and the D2H of the statuses


def spread(v):
    return f"{min(v):.2f}..{max(v):.2f}"


for shape in a.shapes:
    H, W = (int(v) for v in shape.split("x"))
    for q in a.qualities:
        files = [jpeg(image(H, W, 100 + b), q) for b in range(a.batch)]
        if a.kernels_only:
            for _ in range(3):
                op_alone(files)
            continue
        ga, _ = path_gpu(files)                       # warm: code objects, allocator, pinned staging
        pb, _, _ = path_pil(files)
        equal = all(torch.equal(x, y) for x, y in zip(ga, pb))
        rows = {"gpu": [], "pil": [], "pil_decode": [], "op": []}
        for _ in range(a.repeats):
            _, w = path_gpu(files)
            rows["gpu"].append(w / a.batch)
            _, w, d = path_pil(files)
            rows["pil"].append(w / a.batch)
            rows["pil_decode"].append(d / a.batch)
            ev, status, rounds = op_alone(files)
            rows["op"].append(ev / a.batch)
        ratios = [p / g for p, g in zip(rows["pil"], rows["gpu"])]
        print(json.dumps({
            "shape": shape, "batch": a.batch, "quality": q, "pixels_equal_pillow": equal,
            "fallbacks": len(JG.last_fallbacks), "file_bytes_per_image": sum(len(f) for f in files) // a.batch,
            "gpu_ms_per_image": [round(v, 3) for v in rows["gpu"]],
            "gpu_op_event_ms_per_image": [round(v, 3) for v in rows["op"]],
            "pil_ms_per_image": [round(v, 3) for v in rows["pil"]],
            "pil_decode_only_ms_per_image": [round(v, 3) for v in rows["pil_decode"]],
            "pil_over_gpu": [round(r, 2) for r in ratios], "pil_over_gpu_spread": spread(ratios),
            "rounds": rounds, "status": status, "gpu_faster": bool(min(ratios) > 1.0)}), flush=True)

if not a.kernels_only:
    with tempfile.TemporaryDirectory() as td:
        pd, gd = Path(td) / "pred", Path(td) / "gt"
        pd.mkdir()
        gd.mkdir()
        for i in range(a.pairs):
            gt = image(512, 512, 300 + i)
            pred = np.clip(gt.astype(np.int16) + np.random.default_rng(i).integers(-9, 10, gt.shape), 0, 255).astype(np.uint8)
            Image.fromarray(gt).save(gd / f"im{i}.jpg", quality=95)
            Image.fromarray(pred).save(pd / f"im{i}.jpg", quality=75)
        res, times = {}, {"pil": [], "gpu": []}
        for rep in range(a.repeats + 1):              # the first round warms both paths
            for mode in ("pil", "gpu"):
                torch.cuda.synchronize()
                t = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    res[mode] = M.evaluate_task(pd, gd, use_lpips=False, use_fid=False, device="cuda", decode=mode)
                torch.cuda.synchronize()
                if rep:
                    times[mode].append((time.perf_counter() - t) * 1e3 / a.pairs)
        ratios = [p / g for p, g in zip(times["pil"], times["gpu"])]
        print(json.dumps({"evaluate_task": "512x512 pairs, PSNR + SSIM", "pairs": a.pairs,
                          "same_result": res["pil"] == res["gpu"],
                          "pil_ms_per_pair": [round(v, 3) for v in times["pil"]],
                          "gpu_ms_per_pair": [round(v, 3) for v in times["gpu"]],
                          "pil_over_gpu": [round(r, 2) for r in ratios], "pil_over_gpu_spread": spread(ratios)}))
    print(json.dumps({"metric": "JPEG files to device pixels: jpeg_gpu.decode vs Pillow open + H2D",
                      "device": torch.cuda.get_device_name(0), "pillow": Image.__version__, "repeats": a.repeats}))
