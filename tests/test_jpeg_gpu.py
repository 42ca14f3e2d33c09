"""GPU tests of the baseline JPEG encoder (csrc/jpeg_encode.hip, jpeg_gpu.py): the files equal the numpy coder
`jpeg_host.encode` and, where Pillow has libjpeg-turbo, Pillow's own bytes; the op runs on a garbage workspace and
into a guarded output (tests/guard.py), writes exactly lens[b] bytes per image and refuses bad arguments."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import degrade as D
from image_restoration_and_enhancement_amd import degrade_host as DH
from image_restoration_and_enhancement_amd import jpeg_gpu as JG
from image_restoration_and_enhancement_amd import jpeg_host as JH
from tests import guard as G
from tests import jpeg_cases as K

pytestmark = pytest.mark.gpu

SLACK = 37        # out_stride - bound: sentinel bytes between the images' buffers


def _p(t):
    return C.c_void_p(t.data_ptr())


def _scans(device, imgs, quals, rgb=True):
    """irx_jpeg_encode on a 0xFF workspace into a guarded uint8 output, once 0x00- and once 0xFF-filled: the scans
    (bytes [0, lens[b]) of each image's buffer), after the guard's and the fill's checks."""
    B, H, W, _ = imgs.shape
    x = torch.from_numpy(imgs).to(device)
    qt = torch.from_numpy(np.stack([DH.jpeg_quant_tables(q) for q in quals])).to(device)
    bound = L.call("irx_jpeg_encode_bound", H, W)
    assert bound == 2 * 6 * (-(-H // 16)) * (-(-W // 16)) * 208 + 2
    nws = L.call("irx_jpeg_encode_ws_bytes", B, H, W)
    assert nws > 0
    rows = -(-bound // 256)                     # an image's buffer as rows of 256 bytes (keeps the guard's bands small)
    stride = rows * 256 + SLACK
    runs = []
    for fill in (0x00, 0xFF):
        o = G.Out(device, torch.uint8, rows, 256, batch=B, stride=stride, fill=fill)
        ws = G.ws(nws, device)
        lens = torch.full((B,), -1, dtype=torch.int32, device=device)
        L.call("irx_jpeg_encode", D._s(), _p(x), B, H, W, _p(qt), int(rgb), _p(ws), C.c_void_p(o.ptr()), stride,
               _p(lens))
        torch.cuda.synchronize()
        buf = o.check("irx_jpeg_encode").contiguous().cpu().numpy().reshape(B, rows * 256)
        n = lens.cpu().numpy()
        assert (n > 0).all() and (n <= bound).all()
        for b in range(B):
            assert (buf[b, n[b]:] == fill).all(), f"image {b}: bytes past lens[b] = {n[b]} were written (fill {fill:#x})"
        runs.append([buf[b, :n[b]].tobytes() for b in range(B)])
    assert runs[0] == runs[1], "the scan depends on what the output held before the call"
    return runs[1]


def _check(device, imgs, quals):
    imgs = np.ascontiguousarray(imgs)
    scans = _scans(device, imgs, quals)
    files = JG.encode(torch.from_numpy(imgs).to(device), list(quals))
    for b, q in enumerate(quals):
        ref = JH.encode(imgs[b], q)
        H, W = imgs[b].shape[:2]
        assert JG.header(H, W, q) == JH.header(H, W, q)
        got = JH.header(H, W, q) + scans[b] + b"\xff\xd9"
        assert len(got) == len(ref), (b, q, len(got), len(ref))
        assert got == ref, (b, q)
        assert files[b] == ref, (b, q)
        if K.have_turbo():
            assert got == K.pillow_bytes(imgs[b], q), (b, q)


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_files_equal_reference(device, case):
    _check(device, K.case_image(case)[None], [case[3]])


def test_batch_of_three_qualities(device):
    """Per-image tables, lengths and offsets in one call."""
    imgs = np.stack([K.noise(24, 40, s) for s in (1, 2, 3)])
    _check(device, imgs, [10, 75, 100])


def test_many_workgroups_and_segments(device):
    """224x224 noise at quality 95: 196 MCUs = 25 coder workgroups, and a scan of about 58 KB that crosses many
    2048-byte stuffing segments."""
    _check(device, K.noise(224, 224, 7)[None], [95])


def test_scans_longer_than_one_pass(device):
    """A 17 x 32805 strip at quality 100: 2 x 2051 MCUs = 513 coder workgroups and about 570 stuffing segments, both
    more than one 256-lane pass of the per-image scans; two tiles of MCU rows with a dummy block row; 10-bit AC
    values and DC categories up to 10."""
    img = K.noise(17, 32805, 7)
    info = JH.scan(JH.quantised_coefficients(img, 100))[1]
    assert info["bits"] > 256 * 2048 * 8 and info["max_ac_bits"] == 10 and info["max_dc_cat"] >= 10
    _check(device, img[None], [100])


def test_bgr_and_cpu_inputs(device):
    img = K.noise(24, 40, 5)
    ref = JH.encode(img, 80)
    bgr = torch.from_numpy(np.ascontiguousarray(img[..., ::-1])).to(device)
    assert JG.encode(bgr, 80, rgb=False) == [ref]
    assert JG.encode(torch.from_numpy(img), 80) == [ref]                  # a CPU tensor: the numpy coder
    assert JG.encode(torch.from_numpy(img).to(device)[None].expand(2, -1, -1, -1), [80, 80]) == [ref, ref]


def test_save_writes_the_files(device, tmp_path):
    imgs = np.stack([K.noise(16, 24, s) for s in (1, 2)])
    paths = [tmp_path / "a.jpg", tmp_path / "b.jpg"]
    JG.save(torch.from_numpy(imgs).to(device), paths, quality=60)
    for p, im in zip(paths, imgs):
        assert p.read_bytes() == JH.encode(im, 60)


def test_roundtrip_pixels_unchanged(device):
    """irx_degrade_jpeg shares its forward half with the encoder (csrc/jpeg_fdct.h): same pixels as before."""
    imgs = np.stack([K.noise(17, 33, s) for s in (1, 2)])
    got = D.jpeg_roundtrip(torch.from_numpy(imgs).to(device), [30, 90], rgb=True).cpu().numpy()
    for b, q in enumerate((30, 90)):
        assert np.array_equal(got[b], DH.jpeg_roundtrip_ref(imgs[b], q, rgb=True))


def test_restore_batch_jpeg_output(device):
    """Each file of output="jpeg" equals saving the "pil" result of the same call; input order is kept across size
    groups."""
    from image_restoration_and_enhancement_amd import inference as INF
    from tests import models_common as MC
    p = INF.RestorationPipeline(device="cuda", config={"engine": {"dtype": "bf16"}, "denoise": {
        "fine_tuned_dir": "unused", "pretrained_id": "unused", "weights": "random"}})
    imgs = [MC.pil(MC.smooth_image(32, 48, seed=3)), MC.pil(MC.smooth_image(48, 32, seed=4)),
            MC.pil(MC.smooth_image(32, 48, seed=5))]
    pil = p.restore_batch("denoise", imgs, strength=0.3)
    files = p.restore_batch("denoise", imgs, strength=0.3, output="jpeg", jpeg_quality=85)
    assert len(files) == 3 and all(isinstance(f, bytes) for f in files)
    for im, f in zip(pil, files):
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=85)
        if K.have_turbo():
            assert f == buf.getvalue()
        assert f == JH.encode(np.asarray(im), 85)
    with pytest.raises(ValueError):
        p.restore_batch("denoise", imgs, output="png")


def test_refusals(device):
    lib = L.load()
    x = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=device)
    qt = torch.from_numpy(DH.jpeg_quant_tables(50)[None]).to(device)
    bound = L.call("irx_jpeg_encode_bound", 16, 16)
    og = G.Out(device, torch.uint8, -(-bound // 256), 256, fill=0xFF)       # no call below may write it
    ws = G.ws(L.call("irx_jpeg_encode_ws_bytes", 1, 16, 16), device)
    lens = torch.full((1,), -7, dtype=torch.int32, device=device)
    out = C.c_void_p(og.ptr())
    assert lib.irx_jpeg_encode(None, _p(x), 1, 4, 16, _p(qt), 1, _p(ws), out, bound, _p(lens)) != 0
    assert b"8 <= H, W" in lib.irx_last_error()
    assert lib.irx_jpeg_encode(None, _p(x), 1, 16, 16, _p(qt), 1, _p(ws), out, bound - 1, _p(lens)) != 0
    assert b"out_stride" in lib.irx_last_error()
    assert lib.irx_jpeg_encode(None, _p(x), 1, 16, 16, _p(qt), 1, _p(ws), out, bound, None) != 0
    assert b"bad arguments" in lib.irx_last_error()
    assert lib.irx_jpeg_encode(None, _p(x), 0, 16, 16, _p(qt), 1, None, out, bound, _p(lens)) == 0      # batch 0
    assert L.call("irx_jpeg_encode_bound", 4, 16) == 0 and L.call("irx_jpeg_encode_ws_bytes", 1, 16, 70000) == 0
    torch.cuda.synchronize()
    assert bool((og.check("refused encode calls") == 0xFF).all()) and bool((ws == 0xFF).all())
    assert int(lens.cpu()[0]) == -7
    qh = np.ascontiguousarray(DH.jpeg_quant_tables(50))
    buf = (C.c_uint8 * 700)()
    assert lib.irx_jpeg_header(16, 16, qh.ctypes.data_as(C.c_void_p), C.cast(buf, C.c_void_p), 100) < 0
    assert b"need 623" in lib.irx_last_error()
    assert lib.irx_jpeg_header(16, 70000, qh.ctypes.data_as(C.c_void_p), C.cast(buf, C.c_void_p), 700) < 0
    with pytest.raises(L.IrxError):
        JG.encode(torch.zeros((4, 16, 3), dtype=torch.uint8, device=device))
