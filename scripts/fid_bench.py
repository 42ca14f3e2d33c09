"""Timing of the FID feature path on the GPU (fid_gpu.InceptionFeatures: csrc/fid.hip + the fp32 conv trunk) against
the host restatement (`fid_host`, fp32 torch on 16 threads), seeded weights:
  * device time per image of the trunk at 299 x 299, batch 1, 8 and 32: a HIP event pair around `--iters` `trunk`
    calls on a resident batch, after warm-up, the median of `--windows` such windows (with the fastest and slowest
    window next to it), and the fp32 TFLOP/s that is (the convolutions' FLOPs are counted from the restatement's
    own conv calls);
  * device time of the input kernel for a 640 x 457 source (windows of 10 x `--iters` calls, the same median);
  * wall time per image from numpy arrays of 640 x 457: upload + input kernel + trunk in chunks of 32 + one
    download of the features (the host clock ends after a device-to-host copy), median of `--reps` runs of 32 images;
  * the host: wall time per image of `fid_host.features_u8` in fp32, median of `--host-reps` images.
Prints one JSON line per measurement and a summary line.  `--trace N` instead runs N trunk calls at batch 8 plus N
input kernels and exits: the workload for a profiler run of its own (the per-kernel split),
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o fid -- python scripts/fid_bench.py --trace 10
The table at the end of profiles/fid_bench.txt is that run's <dir>/fid_kernel_stats.csv (calls, total, average, share,
kernel name without its namespace), appended to this script's JSON lines by hand; this script does not write it.
Needs a GPU: there is no CPU timing fallback.  No speed-up is promised; the lines say what was measured."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_restoration_and_enhancement_amd import fid_gpu as G
from image_restoration_and_enhancement_amd import fid_host as H
from tests import fidref as R

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20, help="trunk calls per timed window")
ap.add_argument("--windows", type=int, default=5, help="timed windows per device-time median")
ap.add_argument("--reps", type=int, default=5, help="runs per end-to-end wall-clock median")
ap.add_argument("--host-reps", type=int, default=5, help="images per host wall-clock median")
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
ap.add_argument("--trace", type=int, default=0, help="run this many trunk calls at batch 8 and exit (profiler runs)")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("fid_bench: no GPU (device times are not estimated on the host)")

torch.set_num_threads(16)
w = H.check_weights(R.seeded_weights())
net = G.InceptionFeatures(w, "cuda")
rng = np.random.default_rng(0)
SRC = (457, 640)


def conv_flops() -> float:
    """2 * MACs of the trunk's convolutions for one 299 x 299 image, counted at the restatement's conv calls."""
    total = [0.0]
    orig = H.F.conv2d

    def counting(x, wt, b=None, **k):
        y = orig(x, wt, b, **k)
        total[0] += 2.0 * y.numel() * wt[0].numel()
        return y

    H.F.conv2d = counting
    try:
        H.trunk(torch.zeros((1, 3, H.SIDE, H.SIDE)), w)
    finally:
        H.F.conv2d = orig
    return total[0]


def device_us(fn, iters):
    """(median, min, max) microseconds per call over `--windows` event-pair windows of `iters` calls each."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


img = R.image_like(rng, 1, *SRC)[0]
dimg = torch.from_numpy(img).cuda()
slot = torch.empty((G.SIDE, G.SIDE, 4), dtype=torch.float32, device="cuda")

if a.trace:
    xb = R.nhwc4(R.trunk_case((8, 299, 299))).cuda()
    for _ in range(a.trace):
        net.input_into(dimg, slot)
        net.trunk(xb)
    torch.cuda.synchronize()
    sys.exit(0)

flops = conv_flops()
rows = []
for B in a.batches:
    xb = R.nhwc4(R.trunk_case((B, 299, 299))).cuda()
    us, lo, hi = device_us(lambda: net.trunk(xb), a.iters)
    row = {"what": "trunk 299x299", "batch": B, "device_us_per_call": round(us, 1),
           "window_min_max_us": [round(lo, 1), round(hi, 1)],
           "device_us_per_image": round(us / B, 1), "conv_gflop_per_image": round(flops / 1e9, 3),
           "fp32_tflops": round(flops * B / us / 1e6, 2), "workspace_mib": round(net.workspace_bytes(B) / 2 ** 20, 1)}
    rows.append(row)
    print(json.dumps(row), flush=True)

us_in, lo, hi = device_us(lambda: net.input_into(dimg, slot), 10 * a.iters)
print(json.dumps({"what": "input kernel", "source": [SRC[0], SRC[1], 3], "device_us_per_image": round(us_in, 1),
                  "window_min_max_us": [round(lo, 1), round(hi, 1)]}), flush=True)

imgs = [np.roll(img, 3 * i, axis=1) for i in range(32)]


def from_numpy():
    return net.features([torch.from_numpy(i).cuda() for i in imgs]).cpu().numpy()


got = from_numpy()
e2e = wall_ms(from_numpy, a.reps)
H.features_u8([img], w)
host = wall_ms(lambda: H.features_u8([img], w), a.host_reps)
want = H.features_u8([img], w, torch.float64)
err = float((torch.from_numpy(got[:1]).double() - want).abs().max())
print(json.dumps({"what": "from numpy, 32 images", "source": [SRC[0], SRC[1], 3],
                  "from_numpy_ms_per_image": round(e2e / 32, 3), "host_fp32_ms_per_image": round(host, 1),
                  "host_threads": torch.get_num_threads(), "abs_err_vs_fp64": err}), flush=True)
print(json.dumps({"metric": "FID features per image, GPU vs fp32 torch on the host", "iters": a.iters, "reps": a.reps,
                  "windows": a.windows, "host_reps": a.host_reps, "device": torch.cuda.get_device_name(0)}))
