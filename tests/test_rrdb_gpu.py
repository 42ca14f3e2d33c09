"""Real-ESRGAN's RRDBNet on the GPU (csrc/rrdb_model.cpp, csrc/rrdb.hip, rrdb_gpu.py) against the fp64 restatement
`rrdb_host.forward(..., dtype=torch.float64)`, with seeded weights of the real shapes (tests/rrdbref.py).

Body conv (derived, not measured, as in tests/test_srvgg_gpu.py): fp16 x fp16 is exact in fp32, so the accumulation's
only error is the fp32 summation, at most 9 Cin * 2^-24 * sum|a||w|; the epilogue applied to a given fp16 value is
deterministic.  An output is accepted if it is the epilogue of some fp16 value v with |v - pre| <= ulp16(pre) / 2 +
9 Cin * 2^-24 * sum|a||w|, where pre is the exact conv + the fp16 bias: v is round16(pre) or an fp16 neighbour, except
where the sum cancels to a small |pre| and the bound spans more fp16 steps (the candidates then also come from the
output's own preimage).

fp32 engine: the condition is 1e-3 (INTEGRATION, "GPU compute dtype"); the asserted bound is 8 x the error of
`rrdb_host.forward(float32)` itself against fp64, computed here, and must lie below the condition.  fp16 engine: rms
within 1.05 x and max within 1.5 x of the fp64-arithmetic emulation's own error (`forward(float64, half=True)`), both
against fp64 and taken over all outputs of all shapes together (1.2e5 samples).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import rrdb_host as H
from tests import rrdbref as R

pytestmark = pytest.mark.gpu

COND_F32 = 1e-3
RMS_RATIO, MAX_RATIO = 1.05, 1.5
SLOPE = np.float32(0.2)


@pytest.fixture(scope="module")
def weights():
    return H.check_weights(R.seeded_weights())


@pytest.fixture(scope="module")
def nets(weights, device):
    from image_restoration_and_enhancement_amd import rrdb_gpu
    return {dt: rrdb_gpu.RealESRGANx4plus(weights, device, dt) for dt in ("fp16", "fp32")}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _case(weights, shape):
    img = R.images(shape)
    x = H.net_input(img)
    f64 = H.forward(x, weights, torch.float64)
    emu = H.forward(x, weights, torch.float64, half=True)
    f32 = H.forward(x, weights, torch.float32)
    return dict(img=img, f64=_nhwc(f64), u8=H.to_u8(f64), emu=_nhwc(emu), emu_u8=H.to_u8(emu),
                f32_err=float((f32.double() - f64).abs().max()))


@pytest.fixture(scope="module")
def cases(weights):
    """Per shape: the uint8 input, fp64 out [B, 4H, 4W, 3], its uint8, the fp16 emulation's out, and the error of the
    fp32 restatement — computed once."""
    return {shape: _case(weights, shape) for shape in R.SHAPES}


# ------------------------------------------------------------------------------------------- body conv
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


def _accept(got, pre, slack, epilogue, preimage=None):
    """got fp16 == epilogue(v) bit for bit for some fp16 v with |v - pre| <= ulp16(pre) / 2 + slack."""
    bound = 0.5 * _ulp16(pre) + slack
    cands = _around(pre.to(torch.float16), 3)
    if preimage is not None:
        cands += _around(preimage(got), 8)
    ok = torch.zeros(got.shape, dtype=torch.bool)
    for v in cands:
        near = (v.double() - pre).abs() <= bound
        ok |= near & (epilogue(v).view(torch.int16) == got.view(torch.int16))
    return ok


def _scaled(v16):
    """round16(0.2f * v): the product is an fp32 value first."""
    return (v16.float() * SLOPE).to(torch.float16)


def _lrelu(v16):
    return torch.where(v16 > 0, v16, _scaled(v16))


def _add16(a16, b16):
    return (a16.float() + b16.float()).to(torch.float16)       # two fp16 values: the fp32 sum is exact or rounds once


# (Cin, Cout, mode): the four growing convs of a dense block and conv5 without / with one / with both residuals
CONVS = ((64, 32, "lrelu"), (96, 32, "lrelu"), (128, 32, "lrelu"), (160, 32, "lrelu"), (192, 64, "plain"),
         (192, 64, "res1"), (192, 64, "res2"))
GUARD, POISON = 4096, 777.0


def _guarded(shape, device):
    """An fp16 tensor of `shape` filled with POISON inside a flat allocation with GUARD poisoned elements on each
    side; returns (flat, view)."""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float16, device=device)
    return flat, flat[GUARD:GUARD + n].view(shape)


def _conv_case(weights, shape, cin, cout, device):
    from image_restoration_and_enhancement_amd import rrdb_gpu as G
    g = torch.Generator().manual_seed(11 + cin + sum(shape))
    B, h, wd = shape
    a = (torch.randn(shape + (cin,), generator=g) * 0.5).to(torch.float16)
    name = "body.1.rdb2.conv%d" % (cin // 32 - 1)
    w, b = weights[name + ".weight"].to(torch.float16), weights[name + ".bias"]
    assert w.shape == (cout, cin, 3, 3)
    r1 = (torch.randn(shape + (64,), generator=g) * 0.5).to(torch.float16)     # conv5: x, channels 0..63 of the source
    r2 = (torch.randn(shape + (64,), generator=g) * 0.5).to(torch.float16)     # the RRDB's input, in the destination
    xflat, x = _guarded(shape + (192,), device)
    x[..., :cin] = a.to(device)
    if cout == 64:
        x[..., :64] = r1.to(device)
        a = torch.cat((r1, a[..., 64:]), -1)
    return dict(G=G, a=a, w=w, b=b, r1=r1, r2=r2, xflat=xflat, x=x,
                wd=w.permute(0, 2, 3, 1).contiguous().to(device), bd=b.to(device))


def _exact_conv(a16, w16, b, cin):
    """(exact conv + fp16 bias, 9 Cin * 2^-24 * sum|a||w|) in fp64, NHWC."""
    x = a16.double().permute(0, 3, 1, 2)
    pre = F.conv2d(x, w16.double(), b.to(torch.float16).double(), padding=1)
    s = F.conv2d(x.abs(), w16.double().abs(), padding=1)
    return _nhwc(pre), _nhwc(s) * (9 * cin * 2.0 ** -24)


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("cin,cout,mode", CONVS)
def test_body_conv(weights, device, shape, cin, cout, mode):
    c = _conv_case(weights, shape, cin, cout, device)
    G, x, r1, r2 = c["G"], c["x"], c["r1"], c["r2"]
    before = c["xflat"].clone()
    if cout == 32:                                   # conv k writes its slice of the buffer it reads
        dflat, dest, off = c["xflat"], x, cin
    else:                                            # conv5 writes channels 0..63 of the next block's buffer
        dflat, dest = _guarded(shape + (192,), device)
        off = 0
        if mode == "res2":
            dest[..., :64] = r2.to(device)           # ... over the RRDB's input, which it reads first
    dbefore = dflat.clone()
    out = dest[..., off:off + cout]
    # one block per CU, one block walking every tile, three blocks; the weight panel kept in LDS from 16 tiles per
    # block (the default: never at these sizes), wherever it fits (Cin <= 160), and never
    for blocks in (0, 1, 3):
        if blocks:
            dflat.copy_(dbefore)
        with L.option(rrdb_blocks=blocks, rrdb_resident={0: 1, 1: 2, 3: 0}[blocks]):
            G.body_conv(x, cin, c["wd"], c["bd"], out, lrelu=mode == "lrelu",
                        res1=x[..., :64] if mode in ("res1", "res2") else None,
                        res2=out if mode == "res2" else None)
        if blocks:
            assert torch.equal(dflat.view(torch.int16), after.view(torch.int16)), f"rrdb_blocks={blocks}"
        else:
            after = dflat.clone()
    got = out.cpu()
    # the written slice is exactly the slice: nothing else in either allocation changed
    keep = torch.ones(dest.shape, dtype=torch.bool)
    keep[..., off:off + cout] = False
    dv, bv = after[GUARD:-GUARD].view(dest.shape).cpu(), dbefore[GUARD:-GUARD].view(dest.shape).cpu()
    assert torch.equal(dv[keep].view(torch.int16), bv[keep].view(torch.int16))
    assert bool((after[:GUARD] == POISON).all()) and bool((after[-GUARD:] == POISON).all())
    if cout == 64:
        assert torch.equal(c["xflat"].view(torch.int16), before.view(torch.int16))
    assert not bool((got == POISON).any())

    pre, slack = _exact_conv(c["a"], c["w"], c["b"], cin)
    epi = {"lrelu": _lrelu, "plain": lambda v: v, "res1": lambda v: _add16(_scaled(v), r1),
           "res2": lambda v: _add16(_scaled(_add16(_scaled(v), r1)), r2)}[mode]
    pim = {"lrelu": lambda o: torch.where(o > 0, o, (o.double() / 0.2).to(torch.float16)), "plain": lambda o: o,
           "res1": None, "res2": None}[mode]
    ok = _accept(got, pre, slack, epi, pim)
    want = epi(pre.to(torch.float16))
    print(f"rrdb conv {cin}->{cout} {mode} {shape}: {int((~ok).sum())} refused of {ok.numel()}, "
          f"{int((want.view(torch.int16) != got.view(torch.int16)).sum())} differ from the oracle's own rounding")
    assert bool(ok.all())
    if mode in ("res1", "res2"):
        # the test can tell a lost residual: the expectations differ on most elements, and the output is refused
        less = _scaled if mode == "res1" else (lambda v: _scaled(_add16(_scaled(v), r1)))    # the last `+ x` left out
        assert float((less(pre.to(torch.float16)) != want).float().mean()) > 0.5
        assert not bool(_accept(got, pre, slack, less).all())


def test_body_conv_batch_position(weights, device):
    shape = (2, 13, 37)
    c = _conv_case(weights, shape, 192, 64, device)
    G, x = c["G"], c["x"]
    both = torch.zeros(shape + (64,), dtype=torch.float16, device=device)
    G.body_conv(x, 192, c["wd"], c["bd"], both, res1=x[..., :64])
    x1 = x[1:2].contiguous()
    one = torch.zeros((1,) + shape[1:] + (64,), dtype=torch.float16, device=device)
    G.body_conv(x1, 192, c["wd"], c["bd"], one, res1=x1[..., :64])
    assert torch.equal(one.view(torch.int16), both[1:2].view(torch.int16))


# ------------------------------------------------------------------------------------------- whole model
def _frac_dist(pre_round):
    return (pre_round - torch.floor(pre_round) - 0.5).abs()


@pytest.mark.parametrize("shape", R.SHAPES)
def test_fp32_engine(nets, cases, shape, device):
    c = cases[shape]
    bound = 8 * c["f32_err"]
    assert 0 < bound <= COND_F32
    u8, out_f = nets["fp32"].forward_float(torch.from_numpy(c["img"]).to(device))
    u8, out_f = u8.cpu(), out_f.cpu().double()
    err = float((out_f - c["f64"]).abs().max())
    diff = (u8.int() - c["u8"].int()).abs()
    print(f"rrdb fp32 {shape}: max|GPU - fp64| {err:.3e}, host fp32 {c['f32_err']:.3e}, bound {bound:.3e}, "
          f"uint8 pixels differing {int((diff > 0).sum())}")
    assert err <= bound
    assert int(diff.max()) <= 1
    pre_round = c["f64"].clamp(0, 1) * 255.0
    assert bool((_frac_dist(pre_round)[diff > 0] <= 255 * bound).all())


def _pooled(outs, refs):
    d = torch.cat([(o.double() - r).abs().flatten() for o, r in zip(outs, refs)])
    return float(d.pow(2).mean().sqrt()), float(d.max()), d.numel()


def _check_fp16(net, cs, fused, device, label):
    outs = []
    for c in cs:
        x = torch.from_numpy(c["img"]).to(device)
        with L.option(rrdb_fused=fused):
            u8, out_f = net.forward_float(x)
            u8b, out_fb = net.forward_float(x)
        assert torch.equal(u8, u8b) and torch.equal(out_f.view(torch.int32), out_fb.view(torch.int32))   # determinism
        u8, out_f = u8.cpu(), out_f.cpu()
        assert torch.equal(out_f.to(torch.float16).float(), out_f)                 # out_f holds fp16 values
        assert int((u8.int() - c["emu_u8"].int()).abs().max()) <= 1
        assert np.array_equal(u8.numpy(), np.round(np.clip(out_f.numpy(), 0, 1) * np.float32(255.0)).astype(np.uint8))
        outs.append(out_f)
    rms, mx, n = _pooled(outs, [c["f64"] for c in cs])
    erms, emx, _ = _pooled([c["emu"] for c in cs], [c["f64"] for c in cs])
    print(f"rrdb fp16 {label} fused={fused}: {n} samples, rms {rms:.4e} / emulation {erms:.4e} = {rms / erms:.4f}, "
          f"max {mx:.4e} / {emx:.4e} = {mx / emx:.4f}")
    return rms, mx, erms, emx, n


@pytest.mark.parametrize("fused", [1, 0])
def test_fp16_engine(nets, cases, fused, device):
    rms, mx, erms, emx, n = _check_fp16(nets["fp16"], [cases[s] for s in R.SHAPES], fused, device, "2 blocks")
    assert n >= 100000
    assert rms <= RMS_RATIO * erms
    assert mx <= MAX_RATIO * emx


def test_fp16_engine_full_depth(device):
    """The published geometry, 23 blocks, once: one exact tile."""
    from image_restoration_and_enhancement_amd import rrdb_gpu
    weights = H.check_weights(R.seeded_weights(H.NUM_BLOCK))
    net = rrdb_gpu.RealESRGANx4plus(weights, device, "fp16")
    rms, mx, erms, emx, _ = _check_fp16(net, [_case(weights, R.FULL_SHAPE)], 1, device, "23 blocks")
    assert rms <= RMS_RATIO * erms
    assert mx <= MAX_RATIO * emx


@pytest.mark.parametrize("dt,fused", [("fp16", 1), ("fp16", 0), ("fp32", 1)])
def test_batch_position_and_blocks(nets, cases, dt, fused, device):
    x = torch.from_numpy(cases[(2, 13, 37)]["img"]).to(device)
    with L.option(rrdb_fused=fused):
        u8, out_f = nets[dt].forward_float(x)
        u1, f1 = nets[dt].forward_float(x[1:2])
        assert torch.equal(u1, u8[1:2]) and torch.equal(f1.view(torch.int32), out_f[1:2].view(torch.int32))
        for blocks in (1, 3):
            with L.option(rrdb_blocks=blocks):
                ub, fb = nets[dt].forward_float(x)
            assert torch.equal(ub, u8) and torch.equal(fb.view(torch.int32), out_f.view(torch.int32))
        with L.option(rrdb_resident=2):                 # every panel that fits stays in LDS: the same K order
            ub, fb = nets[dt].forward_float(x)
        assert torch.equal(ub, u8) and torch.equal(fb.view(torch.int32), out_f.view(torch.int32))
        single = nets[dt].enhance(x[1])
        assert single.shape == (52, 148, 3) and torch.equal(single, u8[1])
        batch = torch.zeros_like(u8)
        nets[dt].enhance(x[0], out=batch[0])
        assert torch.equal(batch[0], u8[0]) and not batch[1:].any()


def test_workspace_depends_on_the_graph(nets):
    fused = nets["fp16"].workspace_bytes(1, 19, 70)
    with L.option(rrdb_fused=0):
        unfused = nets["fp16"].workspace_bytes(1, 19, 70)
    # the peak is the two 64-channel fp16 tensors at 4H x 4W around conv_hr; the conv2d graph adds its fp32 sums
    assert fused >= 2 * 16 * 19 * 70 * 64 * 2
    assert unfused > fused


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(nets, weights, device):
    from image_restoration_and_enhancement_amd import rrdb_gpu
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
    ok = dict(m=net.h, img=p(img), H=8, W=8, lut=p(net.table), out=p(out), ws=p(ws), cap=ws.numel())
    for what, change in [("null input", dict(img=None)), ("a UNet handle", dict(m=unet.h)), ("H = 0", dict(H=0)),
                         ("W = 0", dict(W=0)), ("null output", dict(out=None)), ("null table", dict(lut=None)),
                         ("null workspace", dict(ws=None)), ("short workspace", dict(cap=ws.numel() - 256))]:
        a = dict(ok, **change)
        rc = lib.irx_rrdb_u8(a["m"], net.stream(), a["img"], 1, a["H"], a["W"], a["lut"], a["out"], p(out_f), a["ws"],
                             a["cap"])
        assert rc != 0, what
        assert lib.irx_last_error(), what
    # the body kernel's own refusals: a ragged Cin, a Cout it is not built for, an output slice inside the channels read
    x = torch.zeros((1, 8, 8, 192), dtype=torch.float16, device=device)
    w = torch.zeros((32, 3, 3, 64), dtype=torch.float16, device=device)
    b = torch.zeros(64, device=device)
    s = net.stream()
    for what, (cin, cout, off) in [("Cin 48", (48, 32, 64)), ("Cout 16", (64, 16, 64)), ("overlap", (64, 32, 32))]:
        rc = lib.irx_op_rrdb_conv(s, p(x), 192, cin, 1, 8, 8, p(w), p(b), cout, 1, None, 0, 0, None, 0,
                                  C.c_void_p(x.data_ptr() + 2 * off), 192)
        assert rc != 0 and lib.irx_last_error(), what
    torch.cuda.synchronize()
    assert bool((out.cpu() == 7).all()) and bool((out_f.cpu() == -7.0).all()) and not ws.cpu().any()
    assert not x.cpu().any()
    with pytest.raises(L.IrxError, match="bf16"):
        NativeModel(L.IRX_MODEL_RRDB, rrdb_gpu.RRDBConfig(), "bf16", "cpu")
    with pytest.raises(ValueError):
        rrdb_gpu.RealESRGANx4plus(weights, device, "bf16")
    with pytest.raises(ValueError):
        net.enhance(img[..., :2])


# ------------------------------------------------------------------------------------------- wiring
@pytest.fixture(scope="module")
def weight_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("rrdb") / "RealESRGAN_x4plus.pth"
    torch.save({"params_ema": R.seeded_weights()}, str(path))
    return str(path)


def _pipeline(weight_file, arch="rrdbnet"):
    from image_restoration_and_enhancement_amd.inference import RestorationPipeline
    return RestorationPipeline(device="cuda", config={"sr": {
        "fine_tuned_dir": "missing", "pretrained_id": "unused", "default_backend": "realesrgan",
        "realesrgan_weights": weight_file, "realesrgan_arch": arch}})


def test_pipeline_wiring(nets, weight_file, device):
    from image_restoration_and_enhancement_amd import resample, rrdb_gpu
    pipe = _pipeline(weight_file)
    img = Image.fromarray(R.images((1, 11, 37), seed=5)[0])
    want = nets["fp16"].enhance(np.array(img)).cpu().numpy()
    got = pipe.super_resolve(img)
    assert isinstance(pipe.models["sr"].net, rrdb_gpu.RealESRGANx4plus) and pipe.models["sr"].arch == "rrdbnet"
    assert got.size == (148, 44) and np.array_equal(np.array(got), want)
    half = pipe.super_resolve(img, scale=2)
    assert half.size == (74, 22)
    assert np.array_equal(np.array(half), np.array(resample.resize_pil(Image.fromarray(want), (74, 22), Image.LANCZOS,
                                                                       "cuda")))
    assert np.array_equal(np.array(pipe.process(img, ["sr"])["final"]), want)
    assert np.array_equal(np.array(_pipeline(weight_file, "auto").super_resolve(img)), want)


def test_restore_batch(weight_file, device):
    pipe = _pipeline(weight_file)
    ims = [Image.fromarray(R.images((1, 6, 20), seed=s)[0]) for s in (1, 2)]
    ims.insert(1, Image.fromarray(R.images((1, 9, 33), seed=3)[0]))
    res = pipe.restore_batch("sr", ims)
    for im, r in zip(ims, res):
        assert r.size == (im.size[0] * 4, im.size[1] * 4)
        assert np.array_equal(np.array(r), np.array(pipe.super_resolve(im)))
