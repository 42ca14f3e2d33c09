"""Timing of LPIPS(alex) on the GPU (lpips_gpu.LpipsAlex, csrc/lpips.hip + the fp32 conv trunk) against the host
restatement (`lpips_host.lpips_alex`, fp32 torch on 16 threads), seeded weights, 512x512x3 and 256x256x3, batch 1
and 8:
  * device time per pair: one HIP event pair around `--iters` `score` calls on resident tensors, after warm-up;
  * wall time per pair from numpy arrays: upload + `score` + one download (the host clock ends after a
    device-to-host copy, so it covers the device work), median of `--reps` calls;
  * the host: wall time per pair of `lpips_host.lpips_alex` in fp32, median of `--host-reps` pairs.
The GPU score of the first pair is compared with the host's.  Prints one JSON line per (size, batch) and a summary
line.  `--trace N` instead runs N `score` calls at 512x512, batch 1, and exits: the workload for a
`rocprofv3 --kernel-trace --stats` run of its own (the per-kernel split).  Needs a GPU: there is no CPU timing
fallback.  No speed-up is promised; the lines say what was measured."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_restoration_and_enhancement_amd import lpips_gpu as G
from image_restoration_and_enhancement_amd import lpips_host as H
from tests import lpipsref as R

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200, help="score calls per device timing")
ap.add_argument("--reps", type=int, default=10, help="calls per end-to-end wall-clock median")
ap.add_argument("--host-reps", type=int, default=5, help="pairs per host wall-clock median")
ap.add_argument("--sizes", type=int, nargs="+", default=[512, 256])
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
ap.add_argument("--trace", type=int, default=0, help="run this many score calls at 512x512 and exit (profiler runs)")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("lpips_bench: no GPU (device times are not estimated on the host)")

torch.set_num_threads(16)
w = H.check_weights(R.seeded_weights(0))
net = G.LpipsAlex(w, "cuda")
rng = np.random.default_rng(0)


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def from_numpy(pred, gt):
    return net.score(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()).cpu().numpy()


if a.trace:
    gt = R.image_like(rng, 1, 512, 512)
    dp, dg = torch.from_numpy(R.near(rng, gt)).cuda(), torch.from_numpy(gt).cuda()
    for _ in range(a.trace):
        net.score(dp, dg)
    torch.cuda.synchronize()
    sys.exit(0)

rows = []
for size in a.sizes:
    gt1 = R.image_like(rng, 1, size, size)
    pred1 = R.near(rng, gt1)
    H.lpips_alex(pred1, gt1, w)                          # warm the host path too
    host_ms = wall_ms(lambda: H.lpips_alex(pred1, gt1, w), a.host_reps)
    want = float(H.lpips_alex(pred1, gt1, w, dtype=torch.float64)[0][0])
    for B in a.batches:
        gt = np.concatenate([gt1] + [np.roll(gt1, b, axis=2) for b in range(1, B)])
        pred = np.concatenate([pred1] + [np.roll(pred1, 2 * b, axis=2) for b in range(1, B)])
        dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
        for _ in range(5):                               # warm: code objects, the workspace of this shape
            net.score(dp, dg)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            net.score(dp, dg)
        e1.record()
        torch.cuda.synchronize()
        dev_us = e0.elapsed_time(e1) / a.iters * 1e3     # per call of B pairs
        got = from_numpy(pred, gt)
        e2e_ms = wall_ms(lambda: from_numpy(pred, gt), a.reps)
        row = {"size": [size, size, 3], "batch": B, "score": round(want, 6), "abs_err_vs_fp64": abs(float(got[0]) - want),
               "device_us_per_call": round(dev_us, 1), "device_us_per_pair": round(dev_us / B, 1),
               "from_numpy_ms_per_pair": round(e2e_ms / B, 4), "host_fp32_ms_per_pair": round(host_ms, 2),
               "host_threads": torch.get_num_threads()}
        rows.append(row)
        print(json.dumps(row), flush=True)
print(json.dumps({"metric": "LPIPS(alex) per pair, GPU vs fp32 torch on the host", "iters": a.iters, "reps": a.reps,
                  "host_reps": a.host_reps, "device": torch.cuda.get_device_name(0),
                  "all_within_5e-5_of_fp64": all(r["abs_err_vs_fp64"] <= 5e-5 for r in rows)}))
