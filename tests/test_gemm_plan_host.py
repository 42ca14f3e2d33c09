"""CPU regression test of the GEMM planning code (csrc/gemm_plan.cpp): the answers the models size their arenas from.

No GPU: the planning functions are pure host code.  Everything goes through existing C entry points — the shape-only
query irx_op_gemm_workspace_bytes, the `out == NULL` query forms of irx_op_gn_proj / irx_op_gn_conv3 and the models'
workspace dry runs (every conv and linear of the UNet / VAE / CLIP asks the planner which path it takes, which partial
buffers it gets and how many split-K bytes it needs; the arena size is the sum of those answers).  The expected values
in tests/golden/gemm_plan_ws.json were recorded before gemm_plan.cpp existed, from the ten separate query functions it
replaced: any drift of a tile / split / path decision for these shapes moves a number here.

Re-record (only when a policy change is intended): python tests/test_gemm_plan_host.py --record
"""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd.configs import CLIPConfig, UNetConfig, VAEConfig
from image_restoration_and_enhancement_amd.engine import CLIPText, UNet, VAE

GOLDEN = Path(__file__).resolve().parent / "golden" / "gemm_plan_ws.json"
SHAPES = [(16, 64, 64), (2, 64, 64), (6, 96, 96), (3, 62, 41), (32, 32, 32)]
DTYPES = ["bf16", "fp16", "fp32"]
OPTIONS = [{}, {"gn_parts": 0}, {"halo_strip": 0}, {"ln_parts": 0}, {"gemm_sk": 0}, {"gn_parts": 0, "halo_strip": 0},
           {"gn_fuse": 1}]
DT = {"bf16": L.IRX_BF16, "fp16": L.IRX_F16, "fp32": L.IRX_F32}


def _opt_key(opts):
    return ",".join(f"{k}={v}" for k, v in sorted(opts.items())) or "default"


def _models():
    return {dt: (UNet(UNetConfig(), dt, "cpu"), VAE(VAEConfig(), dt, "cpu"), CLIPText(CLIPConfig(), dt, "cpu"))
            for dt in DTYPES}


def _gn_proj(dt, n, hw, k, nout):
    folded, splits = C.c_int(), C.c_int()
    L.call("irx_op_gn_proj", None, dt, None, n, hw, k, 32, 1e-5, None, None, None, None, nout, None, None,
           C.byref(folded), C.byref(splits))
    return [folded.value, splits.value]


def _gn_conv3(dt, c0, c1, n, h, w, cout):
    fused = C.c_int()
    L.call("irx_op_gn_conv3", None, dt, None, None, c0, c1, n, h, w, 32, 1e-5, None, None, 1, None, None, cout, None, 0,
           None, None, None, C.byref(fused))
    return fused.value


def collect(models, opts):
    """Every planner answer of the grid under `opts`, as {key: value}."""
    out = {}
    with L.option(**opts):
        for dt in DTYPES:
            unet, vae, clip = models[dt]
            for B, h, w in SHAPES:
                k = f"{dt} {B}x{h}x{w}"
                out[f"unet {k}"] = unet.workspace_bytes(B, h, w)
                if B % 2 == 0:
                    out[f"unet cfg_share {k}"] = unet.workspace_bytes(B, h, w, True)
                out[f"vae_decode {k}"] = vae._size("irx_vae_decode_workspace_bytes", B, h, w)
                out[f"vae_encode {k}"] = vae._size("irx_vae_encode_workspace_bytes", B, 8 * h, 8 * w)
                out[f"clip {k}"] = clip._size("irx_clip_workspace_bytes", B, 77)
            if dt == "fp32":
                continue
            d = DT[dt]
            for M in (2, 154, 256, 257, 512, 4096, 65536) if not opts else ():   # (the shape-only query: defaults only)
                for N in (320, 1280, 2560, 10240):
                    for K in (320, 1280, 3072, 11520):
                        for act, f32, imgs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 16 if M % 16 == 0 else 2)):
                            out[f"gemm_ws {dt} {M} {N} {K} {act} {f32} {imgs}"] = L.call(
                                "irx_op_gemm_workspace_bytes", d, M, N, K, act, f32, imgs)
            for n in (2, 3, 16):
                for hw, ch in ((4096, 320), (1024, 640), (256, 1280), (64, 1280), (62 * 41, 320)):
                    out[f"gn_proj {dt} {n} {hw} {ch}"] = _gn_proj(d, n, hw, ch, ch)
                for h, w, c0, c1, cout in ((64, 64, 320, 0, 320), (32, 32, 640, 320, 640), (16, 16, 1280, 1280, 1280),
                                           (8, 8, 1280, 0, 1280), (62, 41, 320, 0, 320), (128, 128, 256, 0, 256)):
                    out[f"gn_conv3 {dt} {n} {h}x{w} {c0}+{c1}->{cout}"] = _gn_conv3(d, c0, c1, n, h, w, cout)
    return out


@pytest.fixture(scope="module")
def models():
    return _models()


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("opts", OPTIONS, ids=_opt_key)
def test_planner_answers_match_golden(models, golden, opts):
    want = golden[_opt_key(opts)]
    got = collect(models, opts)
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, f"{len(diff)} planner answers moved, e.g. {list(diff.items())[:5]}"


def test_golden_responds_to_options(golden):
    """The fixture is a fingerprint, not a constant: the figures quoted when the grid was chosen, and the options that
    change which partial buffers exist move some answer (ln_parts / gemm_sk change paths, not the arena's peak)."""
    d = golden["default"]
    assert d["unet bf16 16x64x64"] == 550481920
    assert d["unet cfg_share bf16 16x64x64"] == 570142720
    assert golden["gn_parts=0,halo_strip=0"]["unet bf16 16x64x64"] == 504606720
    for key in ("gn_parts=0", "halo_strip=0", "gn_fuse=1"):
        assert any(v != d[k] for k, v in golden[key].items()), key


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gemm_plan_host.py --record")
    m = _models()
    GOLDEN.write_text(json.dumps({_opt_key(o): collect(m, o) for o in OPTIONS}, indent=0, sort_keys=True) + "\n")
    print(f"wrote {GOLDEN} ({GOLDEN.stat().st_size} bytes)")
