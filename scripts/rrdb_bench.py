"""Timing of Real-ESRGAN's RRDBNet on the GPU (rrdb_gpu.RealESRGANx4plus, csrc/rrdb.hip), seeded weights of the
published geometry (23 blocks), input 128x128 and 512x512 (output 512x512 and 2048x2048), batch 1 and 8:
  * device time per `irx_rrdb_u8` call of the fp16 engine with `rrdb_fused=1` (the slab conv kernel) and with
    `rrdb_fused=0` (the same graph on the general conv kernels + gather / epilogue kernels): one HIP event pair around
    `iters` calls on resident tensors, after warm-up, the two variants alternating over `--rounds` repeats in one
    process; every repeat is printed.  The general conv kernels count elements in an int, so the unfused graph refuses
    batch 8 at 512x512; it is then timed as two calls of batch 4 inside the same event pair (`unfused_split: 2`);
  * the five convs of one dense block on their own (`irx_op_rrdb_conv` on a 192-channel buffer, 64/96/128/160 -> 32 and
    192 -> 64 with both residuals): time per conv, the block's achieved TF/s (2 * 9 * Cin * Cout FLOP per pixel) and its
    share of the fp16 MFMA peak (MI355X: 2.5 PFLOP/s); and each conv again with `rrdb_resident=0` (weight slabs streamed
    per tile) and `=2` (the panel kept in LDS wherever it fits; the 192 -> 64 conv streams either way).  The default
    keeps the panel from 16 tiles per block.
The uint8 result of the first call of each variant is checked against the fp64 restatement at 32x32 (every pixel within
one level).  Prints one JSON line per (size, batch) and a summary line.  Needs a GPU: there is no CPU timing fallback.
No speed-up is promised; the lines say what was measured."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import rrdb_gpu as G
from image_restoration_and_enhancement_amd import rrdb_host as H
from tests import rrdbref as R

F16_FLOPS = 2.5e15
INT_MAX = 2 ** 31 - 1

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2, help="alternating repeats per variant")
ap.add_argument("--window-ms", type=float, default=400.0, help="device time aimed at per timed window")
ap.add_argument("--sizes", type=int, nargs="+", default=[128, 512])
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
ap.add_argument("--blocks", type=int, default=H.NUM_BLOCK)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("rrdb_bench: no GPU (device times are not estimated on the host)")

w = H.check_weights(R.seeded_weights(a.blocks))
net = G.RealESRGANx4plus(w, "cuda", "fp16")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def iters_for(fn, window_ms):
    for _ in range(2):                                 # warm: code objects, the workspace of this shape
        fn()
    torch.cuda.synchronize()
    return max(2, int(window_ms * 1e3 / max(timed(fn, 2), 1.0)))


small = R.images((1, 32, 32))
want = H.to_u8(H.forward(H.net_input(small), w, torch.float64))
checks = {}
for fused in (1, 0):
    with L.option(rrdb_fused=fused):
        got = net.enhance(small).cpu()
    checks[fused] = int((got.int() - want.int()).abs().max())

body_flops_px = sum(2.0 * 9 * ci * co for n, co, ci in H.conv_names(a.blocks) if ".rdb" in n)
rows = []
for size in a.sizes:
    for B in a.batches:
        x = torch.from_numpy(R.images((B, size, size))).cuda()
        out = torch.empty((B, 4 * size, 4 * size, 3), dtype=torch.uint8, device="cuda")
        split = 1
        while B * 16 * size * size * 64 // split > INT_MAX:
            split *= 2

        def run(fused, x=x, out=out, split=split, B=B):
            n = 1 if fused else split
            for k in range(n):
                lo, hi = k * B // n, (k + 1) * B // n
                net.enhance(x[lo:hi], out=out[lo:hi])

        runs = {1: [], 0: []}
        its = {}
        for fused in (1, 0):
            with L.option(rrdb_fused=fused):
                its[fused] = iters_for(lambda: run(fused), a.window_ms)
        for _ in range(a.rounds):
            for fused in (1, 0):
                with L.option(rrdb_fused=fused):
                    runs[fused].append(round(timed(lambda: run(fused), its[fused]), 1))
        # one dense block, conv by conv, on a 192-channel buffer (rdb3: its conv5 carries both residuals)
        buf = (torch.randn((B, size, size, 192), device="cuda") * 0.5).half()
        nxt = (torch.randn((B, size, size, 192), device="cuda") * 0.5).half()
        convs = []
        for k in range(5):
            name = f"body.0.rdb3.conv{k + 1}"
            convs.append((64 + 32 * k, w[name + ".weight"].permute(0, 2, 3, 1).contiguous().half().cuda(),
                          w[name + ".bias"].cuda()))
        per, streamed, resident = [], [], []
        for k, (cin, wk, bk) in enumerate(convs):
            if k < 4:
                def fn(cin=cin, wk=wk, bk=bk):
                    G.body_conv(buf, cin, wk, bk, buf[..., cin:cin + 32], lrelu=True)
            else:
                def fn(cin=cin, wk=wk, bk=bk):
                    G.body_conv(buf, cin, wk, bk, nxt[..., :64], res1=buf[..., :64], res2=nxt[..., :64])
            it = iters_for(fn, a.window_ms / 8)
            per.append(statistics.median(timed(fn, it) for _ in range(3)))
            with L.option(rrdb_resident=0):            # the same conv streaming its weight slabs per tile (A/B)
                streamed.append(statistics.median(timed(fn, it) for _ in range(3)))
            with L.option(rrdb_resident=2):            # ... and with the panel kept in LDS wherever it fits
                resident.append(statistics.median(timed(fn, it) for _ in range(3)))
        npix = B * size * size
        rdb_flops = sum(2.0 * 9 * (64 + 32 * k) * (64 if k == 4 else 32) for k in range(5)) * npix
        rdb_us = sum(per)
        f1, f0 = statistics.median(runs[1]), statistics.median(runs[0])
        row = {"input": [size, size, 3], "batch": B, "blocks": a.blocks, "fused_us": runs[1], "unfused_us": runs[0],
               "unfused_split": split, "unfused_over_fused": round(f0 / f1, 3),
               "ranges_disjoint": max(runs[1]) < min(runs[0]) or max(runs[0]) < min(runs[1]),
               "fused_ms_per_image": round(f1 / B / 1e3, 3),
               "model_body_tflops_lower_bound": round(body_flops_px * npix / f1 / 1e6, 1),
               "dense_block": {"conv_us": [round(t, 1) for t in per],
                               "conv_us_streamed_weights": [round(t, 1) for t in streamed],
                               "conv_us_resident_weights": [round(t, 1) for t in resident], "us": round(rdb_us, 1),
                               "tflops": round(rdb_flops / rdb_us / 1e6, 1),
                               "share_of_f16_peak": round(rdb_flops / rdb_us / 1e6 / (F16_FLOPS / 1e12), 3)},
               "iters": its}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, out, buf, nxt
        net._shape_ws.clear()
        torch.cuda.empty_cache()
print(json.dumps({"metric": "irx_rrdb_u8 device time per call, fp16 engine, fused vs unfused", "rounds": a.rounds,
                  "window_ms": a.window_ms, "device": torch.cuda.get_device_name(0),
                  "max_level_diff_vs_fp64_at_32": {"fused": checks[1], "unfused": checks[0]}}))
