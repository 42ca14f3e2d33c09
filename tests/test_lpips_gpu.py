"""LPIPS(alex) on the GPU (csrc/lpips_model.cpp, csrc/lpips.hip, lpips_gpu.py) against the fp64 restatement
`lpips_host.lpips_alex(..., dtype=torch.float64)`, with seeded weights of the real shapes (tests/lpipsref.py).

Conditions (derived, not measured): the total within 5e-5 absolute — `print_results` and evaluate_model.py print four
decimals, so the table is the same — and each tap within 1e-5, a fifth of that.  The asserted bounds are 8x the worst
error measured on an MI355X for that quantity (profiles/lpips_parity.txt) and lie below the conditions.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import lpips_host as H
from image_restoration_and_enhancement_amd import metrics as M
from tests import lpipsref as R

pytestmark = pytest.mark.gpu

COND_TOTAL, COND_TAP = 5e-5, 1e-5
# 8x the worst |GPU - fp64| over the shapes of tests/lpipsref.py, unrelated and +-25 pairs (profiles/lpips_parity.txt:
# total 7.853e-08, tap 3.629e-08; the fp32 restatement itself: 1.410e-07 and 8.484e-08)
BOUND_TOTAL, BOUND_TAP = 8 * 7.853e-08, 8 * 3.629e-08
assert BOUND_TOTAL <= COND_TOTAL and BOUND_TAP <= COND_TAP
ONE_BYTE_REL = 1e-2       # condition: orders below the O(1) error of the expanded square, ~30x the fp32 restatement's own


@pytest.fixture(scope="module")
def weights():
    return H.check_weights(R.seeded_weights(0))


@pytest.fixture(scope="module")
def net(weights, device):
    from image_restoration_and_enhancement_amd import lpips_gpu
    return lpips_gpu.LpipsAlex(weights, device)


@pytest.fixture(scope="module")
def cases(weights):
    """Per shape: gt, an unrelated pred, a +-25 pred, and the fp64 (total, layers) of both pairs — computed once."""
    out = {}
    for shape in R.SHAPES:
        rng = np.random.default_rng(100 + sum(shape))
        gt = R.image_like(rng, *shape)
        preds = {"unrelated": R.image_like(rng, *shape), "near": R.near(rng, gt)}
        out[shape] = (gt, preds, {k: H.lpips_alex(p, gt, weights, dtype=torch.float64) for k, p in preds.items()})
    return out


def _score(net, pred, gt, layers=True):
    dev = net.device
    return net.score(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), layers=layers)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_parity_with_fp64(net, cases, shape):
    gt, preds, want = cases[shape]
    for kind, pred in preds.items():
        total, layers = _score(net, pred, gt)
        assert total.dtype == torch.float64 and total.shape == (shape[0],) and layers.shape == (shape[0], 5)
        t64, l64 = want[kind]
        et = float((total.cpu() - t64).abs().max())
        el = float((layers.cpu() - l64).abs().max())
        print(f"lpips parity {shape} {kind}: score {t64.tolist()} total err {et:.3e} tap err {el:.3e}")
        assert et <= BOUND_TOTAL and el <= BOUND_TAP, (kind, et, el)
        assert torch.equal(layers.sum(1), total) or float((layers.sum(1) - total).abs().max()) < 1e-15


@pytest.mark.parametrize("shape", R.SHAPES)
def test_one_byte_pairs(net, weights, shape):
    """pred = gt with one byte changed by 1: strictly positive, and within 1e-2 relative of fp64 — the form that
    takes the difference before the square does not cancel."""
    rng = np.random.default_rng(200 + sum(shape))
    gt = rng.integers(0, 256, (6,) + shape[1:] + (3,), dtype=np.uint8)
    pred = R.one_byte(rng, gt)
    total = _score(net, pred, gt, layers=False).cpu()
    t64, _ = H.lpips_alex(pred, gt, weights, dtype=torch.float64)
    rel = ((total - t64).abs() / t64).tolist()
    print(f"lpips one-byte {shape}: fp64 {t64.tolist()} rel err {rel}")
    assert float(t64.min()) > 0
    assert float(total.min()) > 0
    assert max(rel) <= ONE_BYTE_REL, rel


def test_identical_images_are_exactly_zero(net, cases):
    for shape in R.SHAPES:
        gt = cases[shape][0]
        total, layers = _score(net, gt.copy(), gt)
        assert total.cpu().tolist() == [0.0] * shape[0], shape
        assert not layers.cpu().any(), shape


def test_determinism(net, cases):
    for shape in ((2, 97, 130), (1, 31, 31)):
        gt, preds, _ = cases[shape]
        a = _score(net, preds["unrelated"], gt)
        b = _score(net, preds["unrelated"], gt)
        assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
        assert torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))


def test_batch_position_and_size(net, cases):
    """Image 1 of the batch of 3, scored alone: within the parity bound of fp64, and the bits it has in the batch."""
    gt, preds, want = cases[(3, 64, 64)]
    both, both_l = _score(net, preds["near"], gt)
    one, one_l = _score(net, preds["near"][1:2], gt[1:2])
    t64, l64 = want["near"]
    assert abs(float(one[0]) - float(t64[1])) <= BOUND_TOTAL
    assert float((one_l[0].cpu() - l64[1]).abs().max()) <= BOUND_TAP
    # the same bits: a conv output's K order and a tap's head tiling do not depend on the batch
    assert torch.equal(one.view(torch.int64), both[1:2].view(torch.int64))
    assert torch.equal(one_l.view(torch.int64), both_l[1:2].view(torch.int64))


# ------------------------------------------------------------------------------------------- component kernels
def test_input_kernel_bit_equal(net, device):
    rng = np.random.default_rng(5)
    both = torch.from_numpy(rng.integers(0, 256, (2, 2, 31, 33, 3), dtype=np.uint8)).to(device)
    pred, gt = both[0], both[1]                     # gt starts 2 * 31 * 33 * 3 bytes in: not a multiple of 4
    for p, g in ((pred, gt), (pred[:1], gt[1:])):    # ... and B = 1: 1023 pixels, a partial last group
        x = net.input_tensor(p, g).cpu()
        B = p.shape[0]
        assert x.shape == (2 * B, 31, 33, 4) and not x[..., 3].any()
        want = torch.cat([H.scaled_input(p.cpu()), H.scaled_input(g.cpu())]).permute(0, 2, 3, 1)
        assert torch.equal(x[..., :3], want)


@pytest.mark.parametrize("c", [64, 192])
@pytest.mark.parametrize("hw", [(15, 15), (8, 11)])
def test_relu_pool_kernel_bit_equal(c, hw, device):
    from image_restoration_and_enhancement_amd import lpips_gpu
    g = torch.Generator().manual_seed(c + hw[0])
    x = torch.randn((3, hw[0], hw[1], c), generator=g)
    xd = x.to(device)
    nchw = x.permute(0, 3, 1, 2)
    pooled = lpips_gpu.relu_pool(xd, 3, 2).cpu()
    assert torch.equal(pooled, F.max_pool2d(F.relu(nchw), kernel_size=3, stride=2).permute(0, 2, 3, 1))
    assert torch.equal(lpips_gpu.relu_pool(xd, 1, 1).cpu(), F.relu(x))


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(net, device):
    from image_restoration_and_enhancement_amd.configs import PipelineConfig
    from image_restoration_and_enhancement_amd.engine import NativeModel
    lib = L.load()
    img = torch.zeros((1, 31, 31, 3), dtype=torch.uint8, device=device)
    total = torch.full((1,), -7.0, dtype=torch.float64, device=device)
    layers = torch.full((1, 5), -7.0, dtype=torch.float64, device=device)
    ws = torch.zeros(net.workspace_bytes(1, 31, 31), dtype=torch.uint8, device=device)
    unet = NativeModel(L.IRX_MODEL_UNET, PipelineConfig.default("denoise").unet, "bf16", "cpu")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    ok = dict(m=net.h, pred=p(img), gt=p(img), H=31, lut=p(net.table), total=p(total), ws=p(ws), cap=ws.numel())
    for what, change in [("H = 30", dict(H=30)), ("null pred", dict(pred=None)), ("null total", dict(total=None)),
                         ("a UNet handle", dict(m=unet.h)), ("short workspace", dict(cap=ws.numel() - 256))]:
        a = dict(ok, **change)
        rc = lib.irx_lpips_u8(a["m"], net.stream(), a["pred"], a["gt"], 1, a["H"], 31, a["lut"], a["total"],
                              p(layers), a["ws"], a["cap"])
        assert rc != 0, what
        assert lib.irx_last_error(), what
    torch.cuda.synchronize()
    assert total.cpu().tolist() == [-7.0] and bool((layers.cpu() == -7.0).all()) and not ws.cpu().any()
    with pytest.raises(ValueError):
        net.score(img[:, :30], img[:, :30])
    with pytest.raises(ValueError):
        net.score(img, img[:, :, :, :2])


# ------------------------------------------------------------------------------------------- wiring
def test_calculator_wiring(weights, device):
    rng = np.random.default_rng(6)
    gt = R.image_like(rng, 1, 40, 52)[0]
    pred = R.near(rng, gt)
    small = R.image_like(rng, 1, 33, 35)[0]
    host = M.MetricsCalculator(use_fid=False, device="cpu", lpips_weights=weights)
    dev = M.MetricsCalculator(use_fid=False, device="cuda", lpips_weights=weights)
    assert dev.use_lpips and dev._gpu_module() is not None
    want = float(H.lpips_alex(pred, gt, weights, dtype=torch.float64)[0][0])
    for a, b in ((pred, gt), (torch.from_numpy(pred).to(device), torch.from_numpy(gt).to(device))):
        v = dev.calculate_lpips(a, b)
        assert isinstance(v, float) and abs(v - want) <= BOUND_TOTAL
        out = dev.calculate_all(a, b)
        assert set(out) == {"psnr", "ssim", "lpips"} and out["lpips"] == v
        assert out["psnr"] == host.calculate_psnr(pred, gt)
    # a pred of another size is resized on the GPU, byte for byte the host's INTER_LINEAR
    want = float(H.lpips_alex(M.resize_linear(small, 52, 40), gt, weights, dtype=torch.float64)[0][0])
    assert abs(dev.calculate_lpips(small, gt) - want) <= BOUND_TOTAL
    assert abs(dev.calculate_lpips(torch.from_numpy(small).to(device), gt) - want) <= BOUND_TOTAL
    # a pair below 31 px is the host code's to refuse
    tiny = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
    with pytest.raises(ValueError):
        dev.calculate_lpips(tiny, tiny)


def test_evaluate_task_on_gpu(tmp_path, weights, device, monkeypatch):
    monkeypatch.delenv(M.LPIPS_WEIGHTS_ENV, raising=False)
    rng = np.random.default_rng(7)
    (tmp_path / "pred").mkdir()
    (tmp_path / "gt").mkdir()
    for name in ("a", "b", "c"):
        gt = R.image_like(rng, 1, 40, 52)[0]
        Image.fromarray(gt).save(tmp_path / "gt" / f"{name}.png")
        Image.fromarray(R.near(rng, gt)).save(tmp_path / "pred" / f"{name}.png")
    cpu = M.evaluate_task(tmp_path / "pred", tmp_path / "gt", "denoise", device="cpu", lpips_weights=weights)
    gpu = M.evaluate_task(tmp_path / "pred", tmp_path / "gt", "denoise", device="cuda", lpips_weights=weights)
    assert set(gpu["metrics"]) == set(cpu["metrics"]) == {"psnr", "ssim", "lpips"}
    for k in ("mean", "min", "max", "median"):
        assert abs(gpu["metrics"]["lpips"][k] - cpu["metrics"]["lpips"][k]) <= BOUND_TOTAL, k
        assert gpu["metrics"]["psnr"][k] == cpu["metrics"]["psnr"][k], k
    plain = M.evaluate_task(tmp_path / "pred", tmp_path / "gt", "denoise", device="cuda")
    assert set(plain["metrics"]) == {"psnr", "ssim"}
    assert plain["metrics"]["psnr"] == gpu["metrics"]["psnr"] and plain["metrics"]["ssim"] == gpu["metrics"]["ssim"]
