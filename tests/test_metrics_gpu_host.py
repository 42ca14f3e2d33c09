"""GPU metrics (csrc/metrics.hip, metrics_gpu.py), host checks: the C ABI's refusals and workspace query, the tables
the host builds for the kernels (float32 sRGB linearisation, INTER_LINEAR axes) against `metrics.py`, the host PSNR
expression, `supported()` and the calculator's fall-back to the numpy code.  No GPU calls."""
import ctypes as C

import numpy as np
import pytest

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import build as B
from image_restoration_and_enhancement_amd import metrics as M
from image_restoration_and_enhancement_amd import metrics_gpu as G


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def _pair(rng, shape, amp=20):
    gt = rng.integers(0, 256, shape, dtype=np.uint8)
    pred = np.clip(gt.astype(int) + rng.integers(-amp, amp + 1, shape), 0, 255).astype(np.uint8)
    return pred, gt


def test_ws_bytes_query(lib):
    assert L.call("irx_metrics_ws_bytes", 1, 7, 7, 3) > 0
    assert L.call("irx_metrics_ws_bytes", 1, 7, 7, 1) > 0
    # one 24-byte partial per tile of TILE_W x TILE_H windows and image
    tiles = -(-(333 - 6) // G.TILE_W) * -(-(200 - 6) // G.TILE_H)
    assert L.call("irx_metrics_ws_bytes", 3, 200, 333, 3) == 3 * tiles * 24
    for args in ((0, 7, 7, 3), (-1, 7, 7, 3), (1, 6, 7, 3), (1, 7, 6, 3), (1, 7, 7, 2), (1, 7, 7, 4), (1, 7, 7, 0)):
        assert L.call("irx_metrics_ws_bytes", *args) == 0, args


def test_pair_refusals_are_statuses_without_a_device(lib):
    """Every argument is checked before anything touches a device: a status and irx_last_error, no launch."""
    buf = (C.c_uint8 * 4096)()                  # host memory: never dereferenced by a refused call
    p = C.cast(buf, C.c_void_p)
    ok = dict(pred=p, gt=p, batch=1, H=16, W=16, C=3, lut=p, ws=p, sse=p, ssim=p, de=None)
    cases = [("null pred", dict(pred=None), b"null"), ("null gt", dict(gt=None), b"null"),
             ("null sse", dict(sse=None), b"null"), ("null ssim", dict(ssim=None), b"null"),
             ("batch 0", dict(batch=0), b"batch"), ("batch -2", dict(batch=-2), b"batch"),
             ("C = 2", dict(C=2), b"channels"), ("C = 4", dict(C=4), b"channels"),
             ("H = 6", dict(H=6), b"H, W >= 7"), ("W = 6", dict(W=6), b"H, W >= 7"),
             ("dE with C = 1", dict(C=1, de=p), b"3 channels"), ("dE without table", dict(de=p, lut=None), b"table"),
             ("null workspace", dict(ws=None), b"workspace")]
    for what, change, text in cases:
        a = dict(ok, **change)
        rc = lib.irx_metrics_pair_u8(None, a["pred"], a["gt"], a["batch"], a["H"], a["W"], a["C"], a["lut"], a["ws"],
                                     a["sse"], a["ssim"], a["de"])
        assert rc != 0, what
        assert text in lib.irx_last_error(), (what, lib.irx_last_error())
    assert not any(buf)


def test_resize_refusals_are_statuses_without_a_device(lib):
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 32)
    for what, args in [("null src", (None, 1, 8, 8, 3, p, p, 4, 4, q)), ("null table", (p, 1, 8, 8, 3, None, p, 4, 4, q)),
                       ("src == dst", (p, 1, 8, 8, 3, p, p, 4, 4, p)), ("batch 0", (p, 0, 8, 8, 3, p, p, 4, 4, q)),
                       ("C = 2", (p, 1, 8, 8, 2, p, p, 4, 4, q)), ("h = 0", (p, 1, 8, 8, 3, p, p, 0, 4, q))]:
        assert lib.irx_resize_linear_u8(None, *args) != 0, what
        assert lib.irx_last_error(), what


def test_srgb_table_reproduces_rgb2lab():
    """Lab from the 256-entry float32 table equals `rgb2lab` of the float32 image, difference 0.0: every byte value
    in every channel, the other two channels sweeping the range at other rates."""
    lut = G.srgb_table()
    assert lut.dtype == np.float32 and lut.shape == (256,)
    v = np.arange(256)
    img = np.stack([np.stack([v, (v * 7 + 3) % 256, (v * 13 + 101) % 256], axis=-1),
                    np.stack([(v * 5 + 17) % 256, v, 255 - v], axis=-1),
                    np.stack([255 - v, (v * 11 + 64) % 256, v], axis=-1)]).astype(np.uint8)     # [3, 256, 3]
    want = M.rgb2lab(img.astype(np.float32) / 255.0)
    got = M.lab_from_linear(lut[img])
    assert got.dtype == np.float64 and np.array_equal(got, want)
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, (64, 48, 3), dtype=np.uint8)
    assert np.array_equal(M.lab_from_linear(lut[big]), M.rgb2lab(big.astype(np.float32) / 255.0))


def _resize_by_tables(img, width, height):
    """The kernel's arithmetic in numpy from the (i0, i1, w1) tables."""
    xt, yt = G.axis_table(width, img.shape[1]).astype(np.int64), G.axis_table(height, img.shape[0]).astype(np.int64)
    a = img.astype(np.int64).reshape(img.shape[0], img.shape[1], -1)
    rows = a[:, xt[:, 0]] * (2048 - xt[:, 2])[None, :, None] + a[:, xt[:, 1]] * xt[:, 2][None, :, None]
    out = rows[yt[:, 0]] * (2048 - yt[:, 2])[:, None, None] + rows[yt[:, 1]] * yt[:, 2][:, None, None]
    assert out.max() + (1 << 21) < 2 ** 31      # the kernel's int32 accumulator
    out = np.clip((out + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    return out[..., 0] if img.ndim == 2 else out


RESIZE_CASES = [((20, 30, 3), 15, 10), ((17, 23, 3), 40, 9), ((9, 11), 22, 18), ((64, 48, 3), 63, 47),
                ((1, 9, 3), 4, 4), ((5, 1, 3), 3, 7), ((12, 10, 3), 10, 12)]      # (image shape, width, height)


@pytest.mark.parametrize("shape,width,height", RESIZE_CASES)
def test_axis_tables_reproduce_resize_linear(shape, width, height):
    rng = np.random.default_rng(sum(shape) + width)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    t = G.axis_table(width, shape[1])
    assert t.dtype == np.int32 and t.shape == (width, 3)
    assert t[:, :2].min() >= 0 and t[:, :2].max() <= shape[1] - 1 and t[:, 2].min() >= 0 and t[:, 2].max() <= 2048
    assert np.array_equal(_resize_by_tables(img, width, height), M.resize_linear(img, width, height))


def test_psnr_from_sse_is_the_host_psnr():
    rng = np.random.default_rng(11)
    for shape, amp in (((7, 7, 3), 20), ((40, 48, 3), 3), ((31, 37), 60), ((200, 333, 3), 255)):
        pred, gt = _pair(rng, shape, amp)
        sse = int(((gt.astype(np.int64) - pred.astype(np.int64)) ** 2).sum())
        assert G.psnr_from_sse(sse, gt.size) == M.psnr(gt, pred)
        assert G.psnr_from_sse(np.int64(sse), gt.size) == M.psnr(gt, pred)
    a = np.full((8, 8, 3), 7, np.uint8)
    assert G.psnr_from_sse(0, a.size) == M.psnr(a, a) == float("inf")
    z, o = np.zeros((9, 9, 3), np.uint8), np.full((9, 9, 3), 255, np.uint8)
    assert G.psnr_from_sse(255 * 255 * z.size, z.size) == M.psnr(z, o) == 0.0


def test_supported_edges():
    assert G.supported((7, 7)) and G.supported((7, 7, 1)) and G.supported((7, 7, 3)) and G.supported((2, 7, 7, 3))
    assert G.supported((512, 512, 3)) and G.supported((7, 4000, 1))
    for shape in ((6, 7, 3), (7, 6, 3), (6, 7), (7, 7, 2), (7, 7, 4), (7, 7, 0), (0, 7, 7, 3), (7,), (1, 1, 7, 7, 3)):
        assert not G.supported(shape), shape


def test_tile_constants_fit_the_kernel_source():
    src = (B.CSRC / "metrics.hip").read_text()
    assert f"MT_TW = {G.TILE_W}, MT_TH = {G.TILE_H};" in src


def test_calculator_without_gpu_gives_host_results(monkeypatch):
    """`device="cuda"` with no usable GPU is the host code, silently (as is the default device)."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    rng = np.random.default_rng(3)
    pred, gt = _pair(rng, (24, 31, 3))
    small = rng.integers(0, 256, (12, 15, 3), dtype=np.uint8)
    host, dev = M.MetricsCalculator(use_lpips=False, use_fid=False), M.MetricsCalculator(False, False, device="cuda")
    assert dev._gpu_module() is None and host._gpu_module() is None
    assert dev.calculate_all(pred, gt) == host.calculate_all(pred, gt)
    assert dev.calculate_all(small, gt) == host.calculate_all(small, gt)
    assert dev.calculate_delta_e(pred, gt) == host.calculate_delta_e(pred, gt)
    assert dev.calculate_psnr(pred, gt) == M.psnr(gt, pred) and dev.calculate_ssim(pred, gt) == M.ssim(gt, pred)
    # tensors are accepted on the host path too
    assert host.calculate_all(torch.from_numpy(pred), torch.from_numpy(gt)) == host.calculate_all(pred, gt)


def test_evaluate_task_without_gpu_is_the_host_run(tmp_path, monkeypatch, capsys):
    import torch
    from PIL import Image
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    rng = np.random.default_rng(4)
    (tmp_path / "pred").mkdir()
    (tmp_path / "gt").mkdir()
    for name in ("a", "b"):
        pred, gt = _pair(rng, (16, 20, 3))
        Image.fromarray(gt).save(tmp_path / "gt" / f"{name}.png")
        Image.fromarray(pred).save(tmp_path / "pred" / f"{name}.png")
    a = M.evaluate_task(tmp_path / "pred", tmp_path / "gt", "denoise", device="cpu")
    b = M.evaluate_task(tmp_path / "pred", tmp_path / "gt", "denoise", device="cuda")
    assert a == b and a["num_samples"] == 2 and set(a["metrics"]) == {"psnr", "ssim"}
