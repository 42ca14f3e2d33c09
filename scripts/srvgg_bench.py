"""Timing of Real-ESRGAN's compact network on the GPU (srvgg_gpu.RealESRGANCompact, csrc/srvgg.hip), seeded weights,
input 128x128, 256x256 and 512x512, batch 1 and 8:
  * device time per `irx_srvgg_u8` call of the fp16 engine with `srvgg_fused=1` (the fused head / body / tail kernels)
    and with `srvgg_fused=0` (the same model on the general conv kernels + the PReLU kernel): one HIP event pair around
    `iters` calls on resident tensors, after warm-up, the two variants alternating over `--rounds` rounds in one
    process; the median and the min .. max spread over the rounds;
  * the body kernel on its own (`irx_op_srvgg_conv`, one 64 -> 64 layer): time per layer, achieved TF/s (2 * 576 * 64
    FLOP per pixel) and the floor over that time, the floor being the larger of 256 B per pixel over the HBM rate and
    the FLOPs over the fp16 MFMA peak (MI355X: 8 TB/s, 2.5 PFLOP/s).
The uint8 result of the first call of each variant is checked against the fp64 restatement at 128x128 (every pixel
within one level).  Prints one JSON line per (size, batch) and a summary line.  `--trace N` instead runs N fused calls
at 512x512, batch 1, and exits: the workload for a `rocprofv3 --kernel-trace --stats` run of its own.  Needs a GPU:
there is no CPU timing fallback.  No speed-up is promised; the lines say what was measured."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import srvgg_gpu as G
from image_restoration_and_enhancement_amd import srvgg_host as H
from tests import srvggref as R

HBM_BYTES_PER_S, F16_FLOPS = 8.0e12, 2.5e15

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7, help="alternating rounds per variant")
ap.add_argument("--window-ms", type=float, default=150.0, help="device time aimed at per timed window")
ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
ap.add_argument("--trace", type=int, default=0, help="run this many fused calls at 512x512 and exit (profiler runs)")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("srvgg_bench: no GPU (device times are not estimated on the host)")

w = H.check_weights(R.seeded_weights(0))
net = G.RealESRGANCompact(w, "cuda", "fp16")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def iters_for(fn, window_ms):
    for _ in range(3):                                 # warm: code objects, the workspace of this shape
        fn()
    torch.cuda.synchronize()
    return max(3, int(window_ms * 1e3 / max(timed(fn, 3), 1.0)))


def stats(v):
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}


if a.trace:
    x = torch.from_numpy(R.images((1, 512, 512))).cuda()
    for _ in range(a.trace):
        net.enhance(x)
    torch.cuda.synchronize()
    sys.exit(0)

small = R.images((1, 128, 128))
want = H.to_u8(H.forward(H.net_input(small), w, torch.float64))
checks = {}
for fused in (1, 0):
    with L.option(srvgg_fused=fused):
        got = net.enhance(small).cpu()
    checks[fused] = int((got.int() - want.int()).abs().max())

rows = []
for size in a.sizes:
    for B in a.batches:
        x = torch.from_numpy(R.images((B, size, size))).cuda()
        out = torch.empty((B, 4 * size, 4 * size, 3), dtype=torch.uint8, device="cuda")
        runs = {1: [], 0: []}
        its = {}
        for fused in (1, 0):
            with L.option(srvgg_fused=fused):
                its[fused] = iters_for(lambda: net.enhance(x, out=out), a.window_ms)
        for _ in range(a.rounds):
            for fused in (1, 0):
                with L.option(srvgg_fused=fused):
                    runs[fused].append(timed(lambda: net.enhance(x, out=out), its[fused]))
        # one body layer on its own
        act = torch.randn((B, size, size, 64), device="cuda").half()
        wl = w["body.2.weight"].permute(0, 2, 3, 1).contiguous().half().cuda()
        bl, sl = w["body.2.bias"].cuda(), w["body.3.weight"].cuda()
        layer = lambda: G.conv_layer(act, wl, bl, sl)      # noqa: E731
        li = iters_for(layer, a.window_ms / 4)
        lt = [timed(layer, li) for _ in range(a.rounds)]
        npix = B * size * size
        flops = 2.0 * 576 * 64 * npix
        floor_us = max(256.0 * npix / HBM_BYTES_PER_S, flops / F16_FLOPS) * 1e6
        lm = statistics.median(lt)
        f1, f0 = stats(runs[1]), stats(runs[0])
        row = {"input": [size, size, 3], "batch": B, "fused": f1, "unfused": f0,
               "unfused_over_fused": round(f0["median_us"] / f1["median_us"], 3),
               "ranges_disjoint": f1["max_us"] < f0["min_us"] or f0["max_us"] < f1["min_us"],
               "fused_us_per_image": round(f1["median_us"] / B, 1),
               "body_layer": dict(stats(lt), tflops=round(flops / lm / 1e6, 1), floor_us=round(floor_us, 2),
                                  floor_over_time=round(floor_us / lm, 3)),
               "iters": its}
        rows.append(row)
        print(json.dumps(row), flush=True)
print(json.dumps({"metric": "irx_srvgg_u8 device time per call, fp16 engine, fused vs unfused", "rounds": a.rounds,
                  "window_ms": a.window_ms, "device": torch.cuda.get_device_name(0),
                  "max_level_diff_vs_fp64_at_128": {"fused": checks[1], "unfused": checks[0]}}))
