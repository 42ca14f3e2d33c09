"""Host side of the baseline JPEG encoder (numpy only): the file `PIL.Image.save(f, "JPEG", quality=q)` writes for
an RGB image, byte for byte (Pillow + libjpeg-turbo; pinned by tests/test_jpeg_host.py).  It serves CPU tensors in
`jpeg_gpu.encode` and is the oracle the kernels of csrc/jpeg_encode.hip are held to.

The file is baseline sequential, 4:2:0, the Annex K Huffman tables (not optimised), no restart markers:

* `header(H, W, quality)`  — the 623 bytes in front of the scan: SOI, APP0 (JFIF 1.1, density 1x1), two DQT (zigzag
  order), SOF0, four DHT (DC0, AC0, DC1, AC1) and SOS.  They depend on H, W and the quality alone.
* `quantised_coefficients` — the int16 coefficients in zigzag order, [MCU][6][64] (MCUs in raster order, blocks
  Y00 Y01 Y10 Y11 Cb Cr), from `degrade_host`'s colour conversion, down-sampling, DCT and quantiser, plus the one
  rule the pixel round trip never needed: libjpeg pads the image to whole 8x8 *blocks* only, and a Y block of the
  last MCU column / row beyond ceil(W/8) x ceil(H/8) is a dummy: AC zero, DC that of the previous block of the same
  MCU (jccoefct.c compress_data), so its DC difference codes as zero.
* `scan(coef)`             — the entropy-coded segment: DC differences per component, AC run lengths with ZRL and
  EOB, 1-bit padding of the last byte, a 0x00 after every 0xFF.  Vectorised the way the kernels work: every
  coefficient forms its own bit string (at most 3 ZRL codes + a code + the value bits = 59 bits), a prefix sum of
  the lengths places it.
* `encode(img, quality)`   — header + scan + EOI.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from . import degrade_host as DH

# ITU-T T.81 Annex K.3-K.6: code counts per length 1..16 and the symbols in code order
DC_LUMA_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC_CHROMA_BITS = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
DC_VALS = tuple(range(12))
AC_LUMA_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d)
AC_LUMA_VALS = tuple(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA_BITS = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)
AC_CHROMA_VALS = tuple(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))

# natural (row-major) index of the k-th zigzag coefficient
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                   38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

HEADER_BYTES = 623
# per-block bound of the scan: 11-bit longest DC code + 11 value bits, 63 x (16-bit code + 10 value bits)
BLOCK_MAX_BITS = 22 + 63 * 26


def _derive(bits, vals) -> Tuple[np.ndarray, np.ndarray]:
    """Annex C: canonical codes.  -> (code[256], length[256]) indexed by symbol (length 0: no code)."""
    code, size = np.zeros(256, np.uint64), np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], size[vals[k]] = c, ln
            c, k = c + 1, k + 1
        c <<= 1
    assert k == len(vals)
    return code, size


_DC = [_derive(DC_LUMA_BITS, DC_VALS), _derive(DC_CHROMA_BITS, DC_VALS)]
_AC = [_derive(AC_LUMA_BITS, AC_LUMA_VALS), _derive(AC_CHROMA_BITS, AC_CHROMA_VALS)]
_DC_CODE, _DC_SIZE = np.stack([t[0] for t in _DC]), np.stack([t[1] for t in _DC])
_AC_CODE, _AC_SIZE = np.stack([t[0] for t in _AC]), np.stack([t[1] for t in _AC])
_NBITS = np.array([int(i).bit_length() for i in range(1 << 12)], np.int64)


def _dht(tc_th: int, bits, vals) -> bytes:
    return b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc_th]) + bytes(bits) + bytes(vals)


def header(H: int, W: int, quality: int) -> bytes:
    """The bytes of the file in front of the scan (SOI .. SOS)."""
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("H and W must fit 16 bits")
    qt = DH.jpeg_quant_tables(quality)
    out = b"\xff\xd8" + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    for i in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in qt[i][ZIGZAG])
    out += (b"\xff\xc0\x00\x11\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big")
            + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01")
    out += _dht(0x00, DC_LUMA_BITS, DC_VALS) + _dht(0x10, AC_LUMA_BITS, AC_LUMA_VALS)
    out += _dht(0x01, DC_CHROMA_BITS, DC_VALS) + _dht(0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return out


def quantised_coefficients(img: np.ndarray, quality: int, rgb: bool = True) -> np.ndarray:
    """uint8 [H][W][3] -> int16 [MCUs][6][64]: the quantised coefficients of the 4:2:0 file in zigzag order, MCUs in
    raster order, blocks Y00 Y01 Y10 Y11 Cb Cr, dummy blocks as libjpeg makes them."""
    DH._check_side(img)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("expected [H][W][3]")
    H, W = img.shape[:2]
    qt = DH.jpeg_quant_tables(quality)
    Y, Cb, Cr = DH._to_ycbcr(img, rgb)
    mh, mw = -(-H // 16), -(-W // 16)
    yq = DH._quantise_plane(DH._pad_edge(Y, 16 * mh, 16 * mw), qt[0]).reshape(2 * mh, 2 * mw, 64)
    out = np.zeros((mh, mw, 6, 64), np.int64)
    for k in range(4):
        out[:, :, k] = yq[k >> 1::2, k & 1::2]
    # dummy blocks: beyond the image padded to whole blocks; never block 0 of an MCU
    bh, bw = -(-H // 8), -(-W // 8)
    for k in range(1, 4):
        dummy = ((2 * np.arange(mh) + (k >> 1) >= bh)[:, None] | (2 * np.arange(mw) + (k & 1) >= bw)[None, :])
        blk = out[:, :, k]
        blk[dummy] = 0
        blk[dummy, 0] = out[:, :, k - 1, 0][dummy]
    for k, p in ((4, Cb), (5, Cr)):
        out[:, :, k] = DH._quantise_plane(DH._downsample_h2v2(p), qt[1]).reshape(mh, mw, 64)
    return out.reshape(mh * mw, 6, 64)[:, :, ZIGZAG].astype(np.int16)


def scan(coef: np.ndarray) -> Tuple[bytes, Dict[str, int]]:
    """int16 [MCUs][6][64] (zigzag) -> the entropy-coded segment (stuffed, padded) and figures of its symbol stream:
    zrl (ZRL symbols), max_ac_bits, max_dc_cat, stuffed (0x00 bytes inserted), pad_bits (1-bits appended)."""
    c = np.asarray(coef, np.int64).reshape(-1, 6, 64)
    n = c.shape[0]
    tbl = np.array([0, 0, 0, 0, 1, 1])
    # DC: difference to the previous block of the same component in scan order
    dc = c[:, :, 0]
    pred = np.zeros_like(dc)
    ys = dc[:, :4].reshape(-1)
    pred[:, :4] = np.concatenate([[0], ys[:-1]]).reshape(n, 4)
    pred[1:, 4:] = dc[:-1, 4:]
    d = dc - pred
    cat = _NBITS[np.abs(d)]
    t2 = np.broadcast_to(tbl, (n, 6))
    dbits = np.where(d < 0, d - 1, d) & ((1 << cat) - 1)
    s = np.zeros((n, 6, 65), np.uint64)          # slot 0: DC, 1..63: AC, 64: EOB of a block whose last AC is non-zero
    ln = np.zeros((n, 6, 65), np.int64)          # (an EOB after coefficient k < 63 sits in slot k + 1, which is zero)
    s[:, :, 0] = (_DC_CODE[t2, cat] << cat.astype(np.uint64)) | dbits.astype(np.uint64)
    ln[:, :, 0] = _DC_SIZE[t2, cat] + cat
    # AC: zero run of every non-zero coefficient = distance to the previous non-zero one
    ac = c[:, :, 1:]
    nz = ac != 0
    k = np.arange(1, 64)
    last = np.maximum.accumulate(np.where(nz, k, 0), axis=-1)                   # last non-zero index up to k
    prev = np.concatenate([np.zeros((n, 6, 1), np.int64), last[:, :, :-1]], -1)  # ... before k
    run = k - prev - 1
    nb = _NBITS[np.abs(ac)]
    t3 = np.broadcast_to(tbl[None, :, None], ac.shape)
    sym = ((run & 15) << 4) | nb
    code, size = _AC_CODE[t3, sym], _AC_SIZE[t3, sym]
    vbits = (np.where(ac < 0, ac - 1, ac) & ((1 << nb) - 1)).astype(np.uint64)
    zc, zs = _AC_CODE[t3, 0xF0], _AC_SIZE[t3, 0xF0]
    nzrl = run >> 4
    sa, la = np.zeros(ac.shape, np.uint64), np.zeros(ac.shape, np.int64)
    for i in range(3):
        m = nzrl > i
        sa = np.where(m, (sa << zs.astype(np.uint64)) | zc, sa)
        la = la + np.where(m, zs, 0)
    sa = (((sa << size.astype(np.uint64)) | code) << nb.astype(np.uint64)) | vbits
    la = la + size + nb
    s[:, :, 1:64] = np.where(nz, sa, 0)
    ln[:, :, 1:64] = np.where(nz, la, 0)
    assert not nz.any() or int(size[nz].min()) > 0
    # EOB in the slot after the last non-zero coefficient, unless that is coefficient 63
    lastnz = last[:, :, -1]
    has = lastnz < 63
    bi, ci = np.nonzero(has)
    s[bi, ci, lastnz[has] + 1] = _AC_CODE[tbl[ci], 0]
    ln[bi, ci, lastnz[has] + 1] = _AC_SIZE[tbl[ci], 0]
    assert int(ln.reshape(n * 6, -1).sum(-1).max()) <= BLOCK_MAX_BITS
    # placement: exclusive prefix sum of the lengths; a string of <= 59 bits touches at most two 64-bit words
    s, ln = s.reshape(-1), ln.reshape(-1)
    keep = ln > 0
    s, ln = s[keep], ln[keep]
    end = np.cumsum(ln)
    pos = end - ln
    total = int(end[-1])
    words = np.zeros(total // 64 + 2, np.uint64)
    w, o = pos >> 6, pos & 63
    room = 64 - o                                                         # bits left in the first word
    fits = ln <= room
    first = np.where(fits, s << (room - ln).clip(0).astype(np.uint64), s >> (ln - room).clip(0).astype(np.uint64))
    np.bitwise_or.at(words, w, first)
    sp = ~fits
    np.bitwise_or.at(words, w[sp] + 1, s[sp] << (64 - (ln[sp] - room[sp])).astype(np.uint64))
    nbytes = (total + 7) // 8
    raw = words.astype(">u8").view(np.uint8)[:nbytes].copy()
    pad = (8 - total % 8) % 8
    if pad:
        raw[-1] |= (1 << pad) - 1
    ff = np.nonzero(raw == 0xFF)[0]
    out = np.insert(raw, ff + 1, 0)
    info = {"zrl": int(np.where(nz, nzrl, 0).sum()), "max_ac_bits": int(nb.max()), "max_dc_cat": int(cat.max()),
            "stuffed": int(ff.size), "pad_bits": pad, "bits": total}
    return out.tobytes(), info


def encode(img: np.ndarray, quality: int = 75, rgb: bool = True) -> bytes:
    """uint8 [H][W][3] -> the bytes of `Image.fromarray(img).save(f, "JPEG", quality=quality)` (img in R,G,B order;
    rgb=False: the same file for an image handed over in B,G,R order)."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    return header(H, W, quality) + scan(quantised_coefficients(img, quality, rgb))[0] + b"\xff\xd9"
