"""Real-ESRGAN's compact network on the GPU (csrc/srvgg_model.cpp, csrc/srvgg.hip, srvgg_gpu.py) against the fp64
restatement `srvgg_host.forward(..., dtype=torch.float64)`, with seeded weights of the real shapes (tests/srvggref.py).

Body layer and tail (derived, not measured): fp16 x fp16 is exact in fp32, so the accumulation's only error is the fp32
summation, at most 576 * 2^-24 * sum|a||w|; the epilogue applied to a given fp16 value is deterministic.  An output is
accepted if it is the epilogue of some fp16 value v with |v - pre| <= ulp16(pre) / 2 + 576 * 2^-24 * sum|a||w|, where
pre is the exact conv + the fp16 bias — v is round16(pre) or one of its two fp16 neighbours, except where the sum
cancels to |pre| < 2e-4: there an fp32 summation error of 1e-7 is two fp16 steps and v lies further out.

fp32 engine: the condition is 1e-3 (INTEGRATION, "GPU compute dtype"); the asserted bound is 8x the worst |GPU - fp64|
measured on an MI355X (profiles/srvgg_parity.txt) and lies below it.  fp16 engine: rms within 1.05x and max within 1.5x
of the fp64-arithmetic emulation's own error (`forward(float64, half=True)`), both against fp64.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import srvgg_host as H
from tests import srvggref as R

pytestmark = pytest.mark.gpu

COND_F32 = 1e-3
# 8x the worst |GPU - fp64| of out_f over the shapes of tests/srvggref.py (profiles/srvgg_parity.txt: 9.003e-07; the
# fp32 restatement itself on the CPU: 4.66e-07)
BOUND_F32 = 8 * 9.003e-07
assert BOUND_F32 <= COND_F32
RMS_RATIO, MAX_RATIO, SHARE_RATIO = 1.05, 1.5, 1.5


@pytest.fixture(scope="module")
def weights():
    return H.check_weights(R.seeded_weights(0))


@pytest.fixture(scope="module")
def nets(weights, device):
    from image_restoration_and_enhancement_amd import srvgg_gpu
    return {dt: srvgg_gpu.RealESRGANCompact(weights, device, dt) for dt in ("fp16", "fp32")}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def cases(weights):
    """Per shape: the uint8 input, fp64 out [B, 4H, 4W, 3], its uint8, and the fp16 emulation's out — computed once."""
    out = {}
    for shape in R.SHAPES:
        img = R.images(shape)
        x = H.net_input(img)
        f64 = H.forward(x, weights, torch.float64)
        emu = H.forward(x, weights, torch.float64, half=True)
        out[shape] = dict(img=img, f64=_nhwc(f64), u8=H.to_u8(f64), emu=_nhwc(emu), emu_u8=H.to_u8(emu))
    return out


# ------------------------------------------------------------------------------------------- body layer
def _ulp16(v: torch.Tensor) -> torch.Tensor:
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -24))).clamp_min(-14.0)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10.0)


def _around(v16: torch.Tensor, steps: int):
    """v16 and the `steps` fp16 values on either side of it."""
    a = v16.numpy()
    inf = np.float16(np.inf)
    out, up, down = [v16], a, a
    for _ in range(steps):
        up, down = np.nextafter(up, inf), np.nextafter(down, -inf)
        out += [torch.from_numpy(up), torch.from_numpy(down)]
    return out


def _accept(got: torch.Tensor, pre: torch.Tensor, slack: torch.Tensor, epilogue, preimage):
    """got fp16 == epilogue(v) bit for bit for some fp16 v with |v - pre| <= ulp16(pre) / 2 + slack.  The candidates
    are round16(pre) with its two neighbours and, where pre is so small that the bound spans several fp16 steps, the
    fp16 values around `preimage(got)`, an fp16 value the epilogue maps to got if any does."""
    bound = 0.5 * _ulp16(pre) + slack
    ok = torch.zeros(got.shape, dtype=torch.bool)
    for v in _around(pre.to(torch.float16), 1) + _around(preimage(got), 8):
        near = (v.double() - pre).abs() <= bound
        ok |= near & (epilogue(v).view(torch.int16) == got.view(torch.int16))
    return ok


def _layer_inputs(weights, shape, k=2):
    g = torch.Generator().manual_seed(7 + sum(shape))
    a = (torch.randn(shape + (64,), generator=g) * 0.5).to(torch.float16)
    w = weights[f"body.{k}.weight"].to(torch.float16)
    return a, w, weights[f"body.{k}.bias"], weights.get(f"body.{k + 1}.weight")


def _exact_conv(a16, w16, b16):
    """(exact conv + fp16 bias, 576 * 2^-24 * sum|a||w|) in fp64, NHWC."""
    x = a16.double().permute(0, 3, 1, 2)
    pre = F.conv2d(x, w16.double(), b16.to(torch.float16).double(), padding=1)
    s = F.conv2d(x.abs(), w16.double().abs(), padding=1)
    return _nhwc(pre), _nhwc(s) * (576 * 2.0 ** -24)


@pytest.fixture(scope="module")
def layer_results(weights, device):
    """Per shape: inputs, the kernel's output with the auto grid and with two persistent blocks."""
    from image_restoration_and_enhancement_amd import srvgg_gpu as G
    out = {}
    for shape in R.SHAPES:
        a, w, b, s = _layer_inputs(weights, shape)
        args = (a.to(device), w.permute(0, 2, 3, 1).contiguous().to(device), b.to(device), s.to(device))
        auto = G.conv_layer(*args).cpu()
        with L.option(srvgg_blocks=2):
            two = G.conv_layer(*args).cpu()
        out[shape] = (a, w, b, s, auto, two, args)
    return out


@pytest.mark.parametrize("shape", R.SHAPES)
def test_body_layer(layer_results, shape):
    a, w, b, s, auto, two, _ = layer_results[shape]
    pre, slack = _exact_conv(a, w, b)
    s16 = s.to(torch.float16).double()

    def epilogue(v):
        return torch.where(v > 0, v, (s16 * v.double()).to(torch.float16))

    def preimage(got):      # got > 0 is v itself, else v = got / slope up to the rounding
        return torch.where(got > 0, got, (got.double() / s16).to(torch.float16))

    ok = _accept(auto, pre, slack, epilogue, preimage)
    want = epilogue(pre.to(torch.float16))
    print(f"srvgg body {shape}: {int((~ok).sum())} refused of {ok.numel()}, "
          f"{int((want.view(torch.int16) != auto.view(torch.int16)).sum())} differ from the oracle's own rounding")
    assert bool(ok.all())
    # every block walks many tiles, or one tile each: the same bits
    assert torch.equal(auto.view(torch.int16), two.view(torch.int16))


def test_body_layer_batch_position(layer_results):
    from image_restoration_and_enhancement_amd import srvgg_gpu as G
    *_, auto, _, args = layer_results[(3, 17, 130)]
    one = G.conv_layer(args[0][1:2].contiguous(), *args[1:]).cpu()
    assert torch.equal(one.view(torch.int16), auto[1:2].view(torch.int16))


# ------------------------------------------------------------------------------------------- tail
@pytest.mark.parametrize("shape", R.SHAPES)
def test_tail(weights, device, shape):
    from image_restoration_and_enhancement_amd import srvgg_gpu as G
    a, w, b, _ = _layer_inputs(weights, shape, k=66)
    a = (a.float() * 3.0).to(torch.float16)       # conv rms 0.4: part of the output leaves [0, 1]
    img = torch.from_numpy(R.images(shape, seed=3))
    table = H.input_table()
    u8, out_f = G.tail(a.to(device), img.to(device), table.to(device), w.permute(0, 2, 3, 1).contiguous().to(device),
                       b.to(device))
    u8, out_f = u8.cpu(), out_f.cpu()
    pre, slack = _exact_conv(a, w, b)                                   # [B, H, W, 48]
    shuffle = lambda t: _nhwc(F.pixel_shuffle(t.permute(0, 3, 1, 2), 4))  # noqa: E731
    x16 = table[img.long()].to(torch.float16)                           # [B, H, W, 3]
    xin = _nhwc(F.interpolate(x16.double().permute(0, 3, 1, 2), scale_factor=4, mode="nearest"))
    got = out_f.to(torch.float16)
    assert torch.equal(got.float(), out_f)                              # out_f holds fp16 values
    ok = _accept(got, shuffle(pre), shuffle(slack), lambda v: (v.double() + xin).to(torch.float16),
                 lambda o: (o.double() - xin).to(torch.float16))
    print(f"srvgg tail {shape}: {int((~ok).sum())} refused of {ok.numel()}")
    assert bool(ok.all())
    want_u8 = np.round(np.clip(out_f.numpy(), 0, 1) * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(u8.numpy(), want_u8)
    assert 0 < int((out_f < 0).sum()) + int((out_f > 1).sum()) < out_f.numel()   # the clamp is exercised


def test_tail_pixel_shuffle_map(device):
    from image_restoration_and_enhancement_amd import srvgg_gpu as G
    B, h, wd = 2, 9, 35
    g = torch.Generator().manual_seed(11)
    x = torch.rand((B, h, wd, 64), generator=g).to(torch.float16)
    w = torch.zeros((48, 3, 3, 64), dtype=torch.float16)
    for ch in range(48):
        w[ch, 1, 1, ch] = 1.0
    img = torch.zeros((B, h, wd, 3), dtype=torch.uint8)
    _, out_f = G.tail(x.to(device), img.to(device), H.input_table().to(device), w.to(device),
                      torch.zeros(48, device=device))
    want = _nhwc(F.pixel_shuffle(x[..., :48].float().permute(0, 3, 1, 2), 4))
    assert torch.equal(out_f.cpu(), want)


# ------------------------------------------------------------------------------------------- PReLU kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_prelu_kernel_bit_equal(device, dtype):
    from image_restoration_and_enhancement_amd import srvgg_gpu as G
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3, 7, 13, 64), generator=g).to(dtype)
    s = 0.15 + 0.1 * torch.rand(64, generator=g)
    got = G.prelu(x.to(device), s.to(device)).cpu()
    if dtype == torch.float32:
        want = torch.where(x > 0, x, s * x)
    else:
        want = torch.where(x > 0, x, (s.to(dtype).double() * x.double()).to(dtype))
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------- whole model
def _frac_dist(pre_round):
    return (pre_round - torch.floor(pre_round) - 0.5).abs()


@pytest.mark.parametrize("shape", R.SHAPES)
def test_fp32_engine(nets, cases, shape, device):
    c = cases[shape]
    u8, out_f = nets["fp32"].forward_float(torch.from_numpy(c["img"]).to(device))
    u8, out_f = u8.cpu(), out_f.cpu().double()
    err = float((out_f - c["f64"]).abs().max())
    diff = (u8.int() - c["u8"].int()).abs()
    print(f"srvgg fp32 {shape}: max|GPU - fp64| {err:.3e}, uint8 pixels differing {int((diff > 0).sum())}")
    assert err <= BOUND_F32
    assert int(diff.max()) <= 1
    pre_round = c["f64"].clamp(0, 1) * 255.0
    assert bool((_frac_dist(pre_round)[diff > 0] <= 255 * BOUND_F32).all())


def _errors(x, ref):
    d = (x.double() - ref).abs()
    return float(d.pow(2).mean().sqrt()), float(d.max())


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_fp16_engine(nets, cases, shape, fused, device):
    c = cases[shape]
    x = torch.from_numpy(c["img"]).to(device)
    with L.option(srvgg_fused=fused):
        u8, out_f = nets["fp16"].forward_float(x)
        u8b, out_fb = nets["fp16"].forward_float(x)
    assert torch.equal(u8, u8b) and torch.equal(out_f.view(torch.int32), out_fb.view(torch.int32))   # determinism
    u8, out_f = u8.cpu(), out_f.cpu()
    rms, mx = _errors(out_f, c["f64"])
    erms, emx = _errors(c["emu"], c["f64"])
    diff = (u8.int() - c["u8"].int()).abs()
    share = float((diff > 0).float().mean())
    eshare = float((c["emu_u8"] != c["u8"]).float().mean())
    print(f"srvgg fp16 {shape} fused={fused}: rms {rms:.4e} / emulation {erms:.4e} = {rms / erms:.4f}, "
          f"max {mx:.4e} / {emx:.4e} = {mx / emx:.4f}, uint8 share {share:.4f} / {eshare:.4f}")
    assert int((c["emu_u8"].int() - c["u8"].int()).abs().max()) <= 1
    assert rms <= RMS_RATIO * erms
    assert mx <= MAX_RATIO * emx
    assert int(diff.max()) <= 1
    assert share <= SHARE_RATIO * eshare


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
def test_batch_position(nets, cases, dt, device):
    x = torch.from_numpy(cases[(3, 17, 130)]["img"]).to(device)
    u8, out_f = nets[dt].forward_float(x)
    u1, f1 = nets[dt].forward_float(x[1:2])
    assert torch.equal(u1, u8[1:2]) and torch.equal(f1.view(torch.int32), out_f[1:2].view(torch.int32))
    single = nets[dt].enhance(x[1])
    assert single.shape == (68, 520, 3) and torch.equal(single, u8[1])
    batch = torch.zeros_like(u8)
    nets[dt].enhance(x[2], out=batch[2])
    assert torch.equal(batch[2], u8[2]) and not batch[:2].any()


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(nets, weights, device):
    from image_restoration_and_enhancement_amd import srvgg_gpu
    from image_restoration_and_enhancement_amd.configs import PipelineConfig
    from image_restoration_and_enhancement_amd.engine import NativeModel
    lib = L.load()
    net = nets["fp16"]
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=device)
    out = torch.full((1, 32, 32, 3), 7, dtype=torch.uint8, device=device)
    out_f = torch.full((1, 32, 32, 3), -7.0, dtype=torch.float32, device=device)
    ws = torch.zeros(net.workspace_bytes(1, 8, 8), dtype=torch.uint8, device=device)
    unet = NativeModel(L.IRX_MODEL_UNET, PipelineConfig.default("denoise").unet, "bf16", "cpu")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    ok = dict(m=net.h, img=p(img), H=8, lut=p(net.table), out=p(out), ws=p(ws), cap=ws.numel())
    for what, change in [("null input", dict(img=None)), ("a UNet handle", dict(m=unet.h)), ("H = 0", dict(H=0)),
                         ("null output", dict(out=None)), ("short workspace", dict(cap=ws.numel() - 256))]:
        a = dict(ok, **change)
        rc = lib.irx_srvgg_u8(a["m"], net.stream(), a["img"], 1, a["H"], 8, a["lut"], a["out"], p(out_f), a["ws"],
                              a["cap"])
        assert rc != 0, what
        assert lib.irx_last_error(), what
    torch.cuda.synchronize()
    assert bool((out.cpu() == 7).all()) and bool((out_f.cpu() == -7.0).all()) and not ws.cpu().any()
    with pytest.raises(L.IrxError, match="bf16"):
        NativeModel(L.IRX_MODEL_SRVGG, None, "bf16", "cpu")
    with pytest.raises(ValueError):
        srvgg_gpu.RealESRGANCompact(weights, device, "bf16")
    with pytest.raises(ValueError):
        net.enhance(img[..., :2])


# ------------------------------------------------------------------------------------------- wiring
@pytest.fixture(scope="module")
def weight_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("srvgg") / "realesr-seeded.pth"
    torch.save({"params_ema": R.seeded_weights(0)}, str(path))
    return str(path)


def _pipeline(weight_file):
    from image_restoration_and_enhancement_amd.inference import RestorationPipeline
    return RestorationPipeline(device="cuda", config={"sr": {
        "fine_tuned_dir": "missing", "pretrained_id": "unused", "default_backend": "realesrgan",
        "realesrgan_weights": weight_file}})


def test_pipeline_wiring(nets, weight_file, device):
    from image_restoration_and_enhancement_amd import resample
    pipe = _pipeline(weight_file)
    img = Image.fromarray(R.images((1, 21, 37), seed=5)[0])
    want = nets["fp16"].enhance(np.array(img)).cpu().numpy()
    got = pipe.super_resolve(img)
    assert got.size == (148, 84) and np.array_equal(np.array(got), want)
    half = pipe.super_resolve(img, scale=2)
    assert half.size == (74, 42)
    assert np.array_equal(np.array(half), np.array(resample.resize_pil(Image.fromarray(want), (74, 42), Image.LANCZOS,
                                                                       "cuda")))
    assert np.array_equal(np.array(pipe.process(img, ["sr"])["final"]), want)


def test_restore_batch(weight_file, device):
    pipe = _pipeline(weight_file)
    ims = [Image.fromarray(R.images((1, 12, 20), seed=s)[0]) for s in (1, 2)]
    ims.insert(1, Image.fromarray(R.images((1, 9, 33), seed=3)[0]))
    res = pipe.restore_batch("sr", ims)
    for im, r in zip(ims, res):
        assert r.size == (im.size[0] * 4, im.size[1] * 4)
        assert np.array_equal(np.array(r), np.array(pipe.super_resolve(im)))
