"""Timing of the GPU metrics (csrc/metrics.hip, metrics_gpu.pair_stats) against the numpy code of metrics.py, at
512x512x3 and batches of 1, 8 and 64, once for PSNR + SSIM and once with dE76 added:
  * device-resident input: time per pair of `pair_stats` (both launches), one HIP event pair around `--iters`
    calls after warm-up, and the achieved bytes/s against the 2 B H W C input bytes (every byte of both images
    read once; the outputs are a few words);
  * from numpy arrays: wall time per pair of upload + `pair_stats` + one download of the results (the host clock
    ends after a device-to-host copy, so it covers the device work), median of `--reps` calls;
  * the host: wall time per pair of `metrics.psnr` + `metrics.ssim` (and `calculate_delta_e`), median of
    `--host-reps` pairs.
The results of the timed GPU runs are compared with the host's on the first pair of every batch.  Prints one JSON
line per (batch, dE) and a final summary line with the sanity condition: from host arrays at batch 8 the GPU path is
not slower than the host path.  Needs a GPU: there is no CPU timing fallback."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_restoration_and_enhancement_amd import metrics as M
from image_restoration_and_enhancement_amd import metrics_gpu as G

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200, help="pair_stats calls per device timing")
ap.add_argument("--reps", type=int, default=10, help="calls per end-to-end wall-clock median")
ap.add_argument("--host-reps", type=int, default=3, help="pairs per host wall-clock median")
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("metrics_bench: no GPU (device times are not estimated on the host)")

H = W = a.size
C = 3
rng = np.random.default_rng(0)
calc = M.MetricsCalculator(use_lpips=False, use_fid=False)


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def host_pair(pred, gt, de):
    out = (M.psnr(gt, pred), M.ssim(gt, pred))
    return out + (calc.calculate_delta_e(pred, gt),) if de else out


def gpu_from_numpy(pred, gt, de):
    sse, ssim, dE = G.pair_stats(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), delta_e=de)
    parts = [sse.to(torch.float64), ssim] + ([dE] if de else [])
    return torch.stack(parts).cpu().numpy()              # one download, the call's only synchronisation


gt1 = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
pred1 = np.clip(gt1.astype(int) + rng.integers(-20, 21, gt1.shape), 0, 255).astype(np.uint8)
host_ms = {de: wall_ms(lambda: host_pair(pred1, gt1, de), a.host_reps) for de in (False, True)}
want = host_pair(pred1, gt1, True)

rows = []
for B in a.batches:
    gt = np.repeat(gt1[None], B, axis=0)
    pred = gt.copy()
    pred[0] = pred1
    for b in range(1, B):                                # different pairs behind the first
        pred[b] = np.roll(pred1, b, axis=1)
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    for de in (False, True):
        for _ in range(5):                               # warm: code object, workspace allocations, the table
            G.pair_stats(dp, dg, delta_e=de)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            res = G.pair_stats(dp, dg, delta_e=de)
        e1.record()
        torch.cuda.synchronize()
        dev_us = e0.elapsed_time(e1) / a.iters * 1e3     # per call of B pairs
        got = gpu_from_numpy(pred, gt, de)
        ok = (M.psnr(gt1, pred1) == G.psnr_from_sse(int(got[0][0]), gt1.size) and abs(got[1][0] - want[1]) < 1e-9
              and (not de or abs(got[2][0] - want[2]) < 1e-9))
        e2e_ms = wall_ms(lambda: gpu_from_numpy(pred, gt, de), a.reps)
        nbytes = 2 * B * H * W * C
        row = {"batch": B, "size": [H, W, C], "delta_e": de, "matches_host": bool(ok),
               "device_us_per_call": round(dev_us, 2), "device_us_per_pair": round(dev_us / B, 3),
               "input_bytes": nbytes, "device_GBps": round(nbytes / (dev_us * 1e-6) / 1e9, 1),
               "from_numpy_ms_per_pair": round(e2e_ms / B, 4), "host_ms_per_pair": round(host_ms[de], 2),
               "from_numpy_speedup": round(host_ms[de] / (e2e_ms / B), 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)

b8 = [r for r in rows if r["batch"] == 8]
print(json.dumps({"metric": "PSNR + SSIM (+ dE76) per pair, GPU vs numpy on the host", "iters": a.iters, "reps": a.reps,
                  "device": torch.cuda.get_device_name(0),
                  "all_match_host": all(r["matches_host"] for r in rows),
                  "batch8_gpu_from_numpy_not_slower_than_host":
                      all(r["from_numpy_ms_per_pair"] <= r["host_ms_per_pair"] for r in b8) if b8 else None}))
