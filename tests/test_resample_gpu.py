"""PIL resize on the GPU (csrc/resample.hip, resample.resize_u8): every output byte of every case equals Pillow's
`Image.resize`; no pixel is excluded and there is no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import resample as RS
from tests.resample_ref import SIZES, pil_resize

pytestmark = pytest.mark.gpu

FILTS = ["lanczos", "bicubic"]


def content(kind: str, size, channels: int, seed: int = 0) -> np.ndarray:
    w, h = size
    if kind == "random":
        return np.random.default_rng(seed + 1000 * w + h).integers(0, 256, (h, w, channels), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((h, w, channels), np.uint8)
    if kind == "full":
        return np.full((h, w, channels), 255, np.uint8)
    assert kind == "checker"      # 0 / 255 cells: the negative lobes overshoot, both clamps fire in both passes
    yy, xx = np.mgrid[0:h, 0:w]
    a = (((yy // 3 + xx // 2) % 2) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(a[..., None], channels, axis=2))


def gpu_resize(a: np.ndarray, size, filt: str, device) -> np.ndarray:
    return RS.resize_u8(torch.from_numpy(a).to(device), size, filt).cpu().numpy()


def check(a: np.ndarray, size, filt: str, device):
    got = gpu_resize(a, size, filt, device)
    ref = pil_resize(a, size, filt)
    assert got.shape == ref.shape
    bad = got != ref
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("filt", FILTS)
@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("src,dst", SIZES)
def test_sizes_random(device, src, dst, channels, filt):
    check(content("random", src, channels), dst, filt, device)


@pytest.mark.parametrize("filt", FILTS)
@pytest.mark.parametrize("kind", ["zeros", "full", "checker"])
@pytest.mark.parametrize("src,dst,channels", [((37, 23), (148, 92), 3), ((64, 48), (17, 9), 3),
                                              ((125, 83), (120, 80), 3), ((125, 83), (120, 80), 1),
                                              ((100, 60), (100, 56), 3), ((100, 60), (91, 60), 3)])
def test_contents(device, src, dst, channels, kind, filt):
    check(content(kind, src, channels), dst, filt, device)


# tile height -> source rows per output row that select it (resample.tile_height mirrors the launcher)
TILE_SCALES = {32: 0.5, 16: 1.5, 8: 3.0, 4: 6.0, 2: 12.0}


@pytest.mark.parametrize("dw", [-1, 0, 1])
@pytest.mark.parametrize("dh", [-1, 0, 1])
@pytest.mark.parametrize("th", sorted(TILE_SCALES))
def test_tile_edges(device, th, dh, dw):
    """Output sizes of tile - 1, tile and tile + 1 in each dimension, for every tile height the launcher uses."""
    h, w = th + dh, RS.TILE_W + dw
    H = max(1, int(round(h * TILE_SCALES[th])))
    assert RS.tile_height(H, h) == th
    for W in (97, 41):                   # width down and up
        check(content("random", (W, H), 3, seed=th), (w, h), "lanczos", device)
    check(content("checker", (97, H), 1), (w, h), "bicubic", device)


@pytest.mark.parametrize("src,dst", [((13, 23), (1, 40)), ((37, 11), (50, 1)), ((9, 7), (1, 1)), ((1, 1), (5, 4)),
                                     ((1, 9), (1, 4)), ((640, 3), (640, 5))])
def test_one_pixel_outputs(device, src, dst):
    """Output width 1 and output height 1 (sources within the 1/16 range), a one-pixel source, one-column images."""
    for channels in (3, 1):
        check(content("random", src, channels), dst, "lanczos", device)


@pytest.mark.parametrize("W", [8, 9, 10, 11])
def test_row_alignment(device, W):
    """3-byte pixels: source row lengths of 0, 3, 2 and 1 bytes mod 4, so rows start at every byte phase (the
    unaligned head and tail of the row transfers), on the source and on the destination side."""
    assert (W * 3) % 4 == {8: 0, 9: 3, 10: 2, 11: 1}[W]
    a = content("random", (W, 13), 3, seed=W)
    for dst in ((W + 5, 17), (W, 20), (W + 7, 13), (W - 3, 6)):
        for filt in FILTS:
            check(a, dst, filt, device)
    wide = content("random", (4 * W + 1, 7), 3, seed=W)
    check(wide, (W, 7), "lanczos", device)


def test_batch_equals_single_calls(device):
    xs = [content("random", (37, 23), 3, seed=s) for s in (1, 2, 3)]          # 2553 bytes per image: odd
    xb = torch.from_numpy(np.stack(xs)).to(device)
    for dst in ((148, 92), (17, 9)):
        got = RS.resize_u8(xb, dst, "lanczos").cpu().numpy()
        for i, a in enumerate(xs):
            single = gpu_resize(a, dst, "lanczos", device)
            assert np.array_equal(got[i], single)
            assert np.array_equal(single, pil_resize(a, dst, "lanczos"))


def test_destination_slice_of_batch_tensor(device):
    """`out` = one image of a larger batch tensor: the neighbouring images keep their sentinel bytes."""
    a = content("random", (37, 23), 3, seed=9)
    for (w, h) in ((51, 31), (13, 7)):                                     # odd image byte counts
        big = torch.full((3, h, w, 3), 0xA5, dtype=torch.uint8, device=device)
        r = RS.resize_u8(torch.from_numpy(a).to(device), (w, h), "lanczos", out=big[1])
        assert r.data_ptr() == big[1].data_ptr()
        host = big.cpu().numpy()
        assert (host[0] == 0xA5).all() and (host[2] == 0xA5).all()
        assert np.array_equal(host[1], pil_resize(a, (w, h), "lanczos"))


def test_many_tiles(device):
    check(content("random", (128, 128), 3), (512, 512), "lanczos", device)


def test_window_streamed_in_chunks(device):
    """1/8 on both axes: the source window of a tile is larger than the staging area and streams through it."""
    check(content("random", (800, 400), 3), (100, 50), "lanczos", device)


@pytest.mark.parametrize("channels", [3, 1])
def test_just_inside_range(device, channels):
    assert RS.ksize(320, 20) == RS.ksize(16, 1) == RS.MAX_KSIZE
    check(content("random", (320, 16), channels), (20, 1), "lanczos", device)
    check(content("checker", (320, 48), channels), (20, 3), "lanczos", device)


def test_just_outside_range_is_refused(device):
    a = torch.from_numpy(content("random", (340, 17), 3)).to(device)
    assert RS.ksize(340, 20) > RS.MAX_KSIZE and not RS.supported((340, 17), (20, 1))
    dst = torch.full((1, 20, 3), 0x5A, dtype=torch.uint8, device=device)
    xb, xc, xk = RS._tables(340, 20, "lanczos", device)
    yb, yc, yk = RS._tables(17, 1, "lanczos", device)
    h = L.load()
    rc = h.irx_resample_u8(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(a.data_ptr()), 1, 17, 340,
                           3, C.c_void_p(xb.data_ptr()), C.c_void_p(xc.data_ptr()), xk, C.c_void_p(yb.data_ptr()),
                           C.c_void_p(yc.data_ptr()), yk, 1, 20, C.c_void_p(dst.data_ptr()))
    assert rc != 0
    msg = h.irx_last_error().decode()
    assert "ksize 103" in msg and "97" in msg, msg
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0x5A).all()
    with pytest.raises(L.IrxError):
        RS.resize_u8(a, (20, 1), "lanczos")
    # the PIL form hands such a ratio to Pillow
    im = Image.fromarray(a.cpu().numpy())
    assert np.array_equal(np.asarray(RS.resize_pil(im, (20, 1), "lanczos", device)),
                          np.asarray(im.resize((20, 1), Image.LANCZOS)))


def test_c_abi_copy_and_argument_checks(device):
    """irx_resample_u8 itself: no tables and the same size is a copy; an axis without tables must keep its size;
    2-channel images and src == dst are refused.  Refused calls leave the destination alone."""
    a = content("random", (21, 10), 3)
    x = torch.from_numpy(np.stack([a, a[::-1].copy()])).to(device)
    dst = torch.full_like(x, 0x5A)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, dp = C.c_void_p(x.data_ptr()), C.c_void_p(dst.data_ptr())
    L.call("irx_resample_u8", st, xp, 2, 10, 21, 3, None, None, 0, None, None, 0, 10, 21, dp)
    assert torch.equal(dst, x)
    dst.fill_(0x5A)
    h = L.load()
    yb, yc, yk = RS._tables(10, 7, "lanczos", device)
    ybp, ycp = C.c_void_p(yb.data_ptr()), C.c_void_p(yc.data_ptr())
    for args, text in (((xp, 2, 10, 21, 3, None, None, 0, ybp, ycp, yk, 7, 20, dp), b"keep its size"),
                       ((xp, 2, 10, 21, 3, None, None, 0, None, None, 0, 7, 21, dp), b"keep its size"),
                       ((xp, 3, 10, 21, 2, None, None, 0, ybp, ycp, yk, 7, 21, dp), b"channels"),
                       ((xp, 2, 10, 21, 3, None, None, 0, ybp, None, yk, 7, 21, dp), b"both tables"),
                       ((xp, 2, 10, 21, 3, None, None, 0, ybp, ycp, yk, 7, 21, xp), b"bad arguments")):
        assert h.irx_resample_u8(st, *args) != 0, text
        assert text in h.irx_last_error(), (text, h.irx_last_error())
    torch.cuda.synchronize()
    assert (dst == 0x5A).all() and torch.equal(x[0].cpu(), torch.from_numpy(a))


def test_unchanged_size_is_a_copy(device):
    a = content("random", (21, 10), 3)
    x = torch.from_numpy(a).to(device)
    y = RS.resize_u8(x, (21, 10))
    assert y.data_ptr() != x.data_ptr() and np.array_equal(y.cpu().numpy(), a)
    out = torch.zeros_like(x)
    assert RS.resize_u8(x, (21, 10), out=out) is out and np.array_equal(out.cpu().numpy(), a)


def test_resize_pil_modes(device):
    rgb = Image.fromarray(content("random", (45, 30), 3))
    for im in (rgb, rgb.convert("L")):
        for size, f in (((90, 61), Image.LANCZOS), ((20, 30), Image.BICUBIC), ((45, 30), "lanczos")):
            got = RS.resize_pil(im, size, f, device)
            ref = im.resize(size, f if not isinstance(f, str) else Image.LANCZOS)
            assert got.mode == ref.mode and got.size == ref.size
            assert np.array_equal(np.asarray(got), np.asarray(ref))
