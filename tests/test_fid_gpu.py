"""FID on the GPU (csrc/fid_model.cpp, csrc/fid.hip, fid_gpu.py) against the fp64 restatement of `fid_host`, with
seeded weights of the real shapes (tests/fidref.py).

Bounds are 8x the worst |GPU - fp64| measured on an MI355X for that quantity (scripts/fid_parity.py ->
profiles/fid_parity.txt, the same cases), on the condition that the measured figure is at most 4x the fp32 host
restatement's own error on the same inputs — both are fp32 evaluations of one graph in different summation orders.
The set-level tests compare device="cuda" with device="cpu" within 8x the GPU figure alone, as §19's LPIPS tests do.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import fid_host as H
from image_restoration_and_enhancement_amd import metrics as M
from tests import fidref as R

pytestmark = pytest.mark.gpu

# profiles/fid_parity.txt: worst |gpu - f64| and the fp32 restatement's |f32 - f64| on the same inputs
MEASURED_INPUT, HOST_INPUT = 2.007e-05, 2.007e-05        # input kernel, per element (values in [-2.2, 2.7])
MEASURED_TRUNK, HOST_TRUNK = 1.714e-05, 7.854e-06        # irx_fid_features, per feature (features up to 60)
MEASURED_PATH, HOST_PATH = 1.994e-05, 1.496e-05          # uint8 image -> features, per feature
MEASURED_FID, HOST_FID = 6.748e-05, 1.160e-04            # 12-pair FID (76.79)
BOUND_INPUT, BOUND_TRUNK, BOUND_PATH = 8 * MEASURED_INPUT, 8 * MEASURED_TRUNK, 8 * MEASURED_PATH
BOUND_FID = 8 * MEASURED_FID                             # (the measured |gpu - cpu| itself is 4.850e-05)
assert MEASURED_INPUT <= 4 * HOST_INPUT and MEASURED_TRUNK <= 4 * HOST_TRUNK and MEASURED_PATH <= 4 * HOST_PATH
assert MEASURED_FID <= 4 * HOST_FID


@pytest.fixture(scope="module")
def weights():
    return H.check_weights(R.seeded_weights())


@pytest.fixture(scope="module")
def net(weights, device):
    from image_restoration_and_enhancement_amd import fid_gpu
    return fid_gpu.InceptionFeatures(weights, device)


@pytest.fixture(scope="module")
def pair_cpu(weights):
    """The 12 pairs and their FID on device="cpu" — computed once."""
    pairs = R.pair_set()
    calc = M.MetricsCalculator(use_lpips=False, device="cpu", fid_weights=weights)
    return pairs, calc.calculate_fid([p for p, _ in pairs], [g for _, g in pairs])


# ------------------------------------------------------------------------------------------- ops
def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


OP_SHAPES = ((2, 35, 35, 288), (1, 3, 3, 768), (2, 8, 8, 2048), (1, 17, 13, 192))


@pytest.mark.parametrize("shape", OP_SHAPES)
def test_bn_relu_bit_equal(shape, device):
    """`torch.clamp_min(x * a + b, 0)` in float32: one multiply, one add (no FMA), the max."""
    from image_restoration_and_enhancement_amd import fid_gpu
    c = shape[3]
    x, a, b = _rand(shape, 1), _rand((c,), 2) + 1.0, _rand((c,), 3)
    want = torch.clamp_min(x * a + b, 0)
    got = fid_gpu.bn_relu(x.to(device), a.to(device), b.to(device)).cpu()
    assert torch.equal(got, want)
    # into channels [384, 384 + c) of a 768-wide (or just wide enough) concat row; the rest is untouched
    ldo = max(768, 384 + c)
    out = torch.full(shape[:3] + (ldo,), -7.0, device=device)
    fid_gpu.bn_relu(x.to(device), a.to(device), b.to(device), out, 384)
    out = out.cpu()
    assert torch.equal(out[..., 384:384 + c], want)
    assert bool((out[..., :384] == -7.0).all()) and bool((out[..., 384 + c:] == -7.0).all())


@pytest.mark.parametrize("shape", OP_SHAPES)
def test_avgpool_bit_equal(shape, device):
    """`F.avg_pool2d(x, 3, 1, 1)` (count_include_pad): the taps inside the image added row by row from 0, then / 9."""
    from image_restoration_and_enhancement_amd import fid_gpu
    x = _rand(shape, 4)
    want = F.avg_pool2d(x.permute(0, 3, 1, 2).contiguous(), 3, 1, 1).permute(0, 2, 3, 1)
    assert torch.equal(fid_gpu.avgpool3(x.to(device)).cpu(), want)


@pytest.mark.parametrize("shape", OP_SHAPES)
def test_maxpool_bit_equal(shape, device):
    """`F.max_pool2d(x, 3, 2)`, alone and into a concat slice."""
    from image_restoration_and_enhancement_amd import fid_gpu
    x = _rand(shape, 5)
    c = shape[3]
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
    assert torch.equal(fid_gpu.maxpool3s2(x.to(device)).cpu(), want)
    ldo = max(768, 384 + c)
    out = torch.full(tuple(want.shape[:3]) + (ldo,), -7.0, device=device)
    fid_gpu.maxpool3s2(x.to(device), out, 384)
    out = out.cpu()
    assert torch.equal(out[..., 384:384 + c], want)
    assert bool((out[..., :384] == -7.0).all()) and bool((out[..., 384 + c:] == -7.0).all())


@pytest.mark.parametrize("shape", OP_SHAPES)
def test_gap_bit_equal(shape, device):
    """The pixels added one by one in row-major order in float32, then one division by H * W."""
    from image_restoration_and_enhancement_amd import fid_gpu
    x = _rand(shape, 6)
    flat = x.reshape(shape[0], -1, shape[3])
    s = flat[:, 0].clone()
    for k in range(1, flat.shape[1]):
        s = s + flat[:, k]
    assert torch.equal(fid_gpu.gap(x.to(device)).cpu(), s / float(flat.shape[1]))


@pytest.mark.parametrize("size", R.SIZES)
def test_input_kernel_against_fp64(net, size, device):
    img = R.input_image(size)
    want = H.preprocess(img, torch.float64)[0].permute(1, 2, 0)
    slot = torch.full((299, 299, 4), -7.0, dtype=torch.float32, device=device)
    net.input_into(torch.from_numpy(img).to(device), slot)
    got = slot.cpu()
    assert not got[..., 3].any()
    e = float((got[..., :3].double() - want).abs().max())
    print(f"fid input {size}: err {e:.3e}")
    assert e <= BOUND_INPUT


# ------------------------------------------------------------------------------------------- trunk
@pytest.mark.parametrize("shape", R.TRUNK_SHAPES)
def test_trunk_against_fp64(net, weights, shape, device):
    x = R.trunk_case(shape)
    want = H.inception_features(x, weights, torch.float64)
    got = net.trunk(R.nhwc4(x).to(device)).cpu()
    assert got.shape == (shape[0], 2048) and got.dtype == torch.float32
    e = float((got.double() - want).abs().max())
    print(f"fid trunk {shape}: features up to {float(want.max()):.3f}, err {e:.3e}")
    assert e <= BOUND_TRUNK


def test_batch_position_and_size(net, device):
    """Each image of a batch of 3 at 299 x 299, scored alone, has the same bits."""
    xb = R.nhwc4(R.trunk_case((3, 299, 299))).to(device)
    fb = net.trunk(xb)
    for i in range(3):
        f1 = net.trunk(xb[i:i + 1].contiguous())
        assert torch.equal(f1.view(torch.int32), fb[i:i + 1].view(torch.int32)), i
    assert torch.equal(net.trunk(xb).view(torch.int32), fb.view(torch.int32))


def test_whole_path_and_queue(net, weights, device):
    """uint8 images of mixed sizes -> features, against fp64; the queue in chunks of 2 gives the same bits."""
    from image_restoration_and_enhancement_amd import fid_gpu
    imgs = [R.input_image(s) for s in R.SIZES[:3]]
    dev = [torch.from_numpy(i).to(device) for i in imgs]
    got = net.features(dev)
    want = H.features_u8(imgs, weights, torch.float64)
    e = float((got.cpu().double() - want).abs().max())
    print(f"fid whole path: err {e:.3e}")
    assert e <= BOUND_PATH
    q = fid_gpu.FeatureQueue(net, chunk=2)
    for d in dev:
        q.add(d)
    assert len(q) == 3
    assert torch.equal(q.finish().view(torch.int32), got.view(torch.int32))


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(net, device):
    lib = L.load()
    x = torch.zeros((1, 75, 75, 4), dtype=torch.float32, device=device)
    out = torch.full((1, 2048), -7.0, dtype=torch.float32, device=device)
    ws = torch.zeros(net.workspace_bytes(1, 75, 75), dtype=torch.uint8, device=device)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    ok = dict(x=p(x), H=75, out=p(out), ws=p(ws), cap=ws.numel())
    for what, change in [("H = 74", dict(H=74)), ("null x", dict(x=None)), ("null out", dict(out=None)),
                         ("short workspace", dict(cap=ws.numel() - 256))]:
        a = dict(ok, **change)
        rc = lib.irx_fid_features(net.h, net.stream(), a["x"], 1, a["H"], 75, a["out"], a["ws"], a["cap"])
        assert rc != 0 and lib.irx_last_error(), what
    torch.cuda.synchronize()
    assert bool((out.cpu() == -7.0).all()) and not ws.cpu().any()
    with pytest.raises(ValueError):
        net.input_into(torch.zeros((8, 8), dtype=torch.uint8, device=device), x[0])
    # a slot the kernel could not write as [299, 299, 4] float32 is refused before the call
    img = torch.zeros((16, 16, 3), dtype=torch.uint8, device=device)
    for slot in (x[0], torch.zeros((299, 299, 4)), torch.zeros((299, 299, 4), dtype=torch.float64, device=device),
                 torch.zeros((299, 299, 8), device=device)[..., :4]):
        with pytest.raises(ValueError):
            net.input_into(img, slot)


# ------------------------------------------------------------------------------------------- set level
def test_calculate_fid_gpu_against_cpu(weights, pair_cpu, device):
    pairs, want = pair_cpu
    dev = M.MetricsCalculator(use_lpips=False, device="cuda", fid_weights=weights)
    assert dev.use_fid and dev._gpu_module() is not None
    preds = [torch.from_numpy(p).to(device) if i % 3 == 0 else p for i, (p, _) in enumerate(pairs)]
    v = dev.calculate_fid(preds, [g for _, g in pairs])
    print(f"fid set: cpu {want:.9f} gpu {v:.9f} diff {abs(v - want):.3e}")
    assert isinstance(v, float) and abs(v - want) <= BOUND_FID
    assert dev.calculate_fid(preds[:5], [g for _, g in pairs]) is None


def test_evaluate_task_on_gpu(tmp_path, weights, pair_cpu, device, monkeypatch):
    monkeypatch.delenv(M.FID_WEIGHTS_ENV, raising=False)
    monkeypatch.delenv(M.LPIPS_WEIGHTS_ENV, raising=False)
    pairs, want = pair_cpu
    (tmp_path / "pred").mkdir()
    (tmp_path / "gt").mkdir()
    for i, (pred, gt) in enumerate(pairs):
        Image.fromarray(gt).save(tmp_path / "gt" / f"{i:02d}.png")
        Image.fromarray(pred).save(tmp_path / "pred" / f"{i:02d}.png")
    gpu = M.evaluate_task(tmp_path / "pred", tmp_path / "gt", "colorize", device="cuda", fid_weights=weights)
    assert set(gpu["metrics"]) == {"psnr", "ssim", "fid"}
    st = gpu["metrics"]["fid"]
    print(f"fid task: cpu {want:.9f} gpu {st['mean']:.9f} diff {abs(st['mean'] - want):.3e}")
    assert abs(st["mean"] - want) <= BOUND_FID and st["min"] == st["max"] == st["mean"]
    plain = M.evaluate_task(tmp_path / "pred", tmp_path / "gt", "colorize", device="cuda")
    assert set(plain["metrics"]) == {"psnr", "ssim"}
    assert plain["metrics"]["psnr"] == gpu["metrics"]["psnr"] and plain["metrics"]["ssim"] == gpu["metrics"]["ssim"]
