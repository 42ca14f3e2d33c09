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

The other direction (`parse`, `decode_coefficients`, `decode`, further down) reads such files, and the grayscale and
optimised-table kinds next to them, back into the pixels `PIL.Image.open(f).convert("RGB")` returns; it serves CPU
devices in `jpeg_gpu.decode` and is the oracle of csrc/jpeg_decode.hip (pinned by tests/test_jpeg_decode_host.py).
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


# ------------------------------------------------------------------------------------------------ decoding
# The other direction: what `PIL.Image.open(f).convert("RGB")` (src/metrics.py:40-46, scripts/generate_predictions.py:68)
# returns for the files this project, Pillow and cv2 write by default: baseline SOF0, 8 bit, 4:2:0 with sampling
# (2,2)(1,1)(1,1) or one component, one scan, no restart markers, JFIF.  `parse` refuses everything else with a
# status of its own (the same numbers as csrc/jpeg_parse.cpp); `decode_coefficients` is a plain sequential Huffman
# decoder (slow and correct, the oracle of csrc/jpeg_decode.hip); `decode` runs the coefficients through
# `degrade_host`'s inverse functions.

# refusal statuses (include/irx.h IRX_JPEG_*)
E_TRUNCATED, E_NOT_JPEG, E_SOF, E_PRECISION, E_DQT16, E_SAMPLING, E_MULTISCAN, E_DRI = -1, -2, -3, -4, -5, -6, -7, -8
E_ADOBE, E_RGB_IDS, E_COMPONENTS, E_SIZE, E_TABLES, E_SCAN_CUT, E_MALFORMED = -9, -10, -11, -12, -13, -14, -15

DEFAULT_SUBSEQ_BITS = 1024
PASS_LANES = 256              # subsequences per pass of the entry-state kernel


class Refused(ValueError):
    """A file outside the decoder's contract; `.status` is the parser's negative status."""

    def __init__(self, status: int, msg: str):
        super().__init__(f"jpeg parse: {msg} (status {status})")
        self.status = status


def parse(data: bytes) -> dict:
    """The markers of a file -> dict(H, W, ncomp, qt int32 [2][64] natural order, dc / ac: two (bits, vals) pairs or
    None, qsel / dcsel / acsel per component, scan_off, scan_len: the entropy-coded bytes up to the first FF xx with
    xx != 00).  Raises `Refused` for everything outside the contract."""
    data = bytes(data)
    n = len(data)
    if n == 0:
        raise Refused(E_NOT_JPEG, "empty file")
    if n < 2:
        raise Refused(E_TRUNCATED, "truncated file")
    if data[0] != 0xFF or data[1] != 0xD8:
        raise Refused(E_NOT_JPEG, "no SOI marker")
    qt = np.zeros((2, 64), np.int32)
    have_q = [False, False]
    dc, ac = [None, None], [None, None]
    sof = None
    p = 2
    while True:
        if p + 4 > n:
            raise Refused(E_TRUNCATED, "file ends in the header")
        if data[p] != 0xFF:
            raise Refused(E_MALFORMED, "marker expected")
        m = data[p + 1]
        if m == 0xFF:                                   # fill byte
            p += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            raise Refused(E_MALFORMED, "stand-alone marker in the header")
        if m == 0xD9:
            raise Refused(E_MALFORMED, "EOI before a scan")
        ln = (data[p + 2] << 8) | data[p + 3]
        if ln < 2:
            raise Refused(E_MALFORMED, "segment length below 2")
        if p + 2 + ln > n:
            raise Refused(E_TRUNCATED, "file ends in a segment")
        seg = data[p + 4:p + 2 + ln]
        p += 2 + ln
        if m == 0xC0:
            if sof is not None:
                raise Refused(E_MALFORMED, "two frame headers")
            if len(seg) < 6:
                raise Refused(E_MALFORMED, "short SOF0")
            if seg[0] != 8:
                raise Refused(E_PRECISION, "sample precision other than 8 bits")
            H, W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nc == 4:
                raise Refused(E_COMPONENTS, "four components (CMYK / YCCK)")
            if nc not in (1, 3):
                raise Refused(E_COMPONENTS, "1 or 3 components")
            if len(seg) != 6 + 3 * nc:
                raise Refused(E_MALFORMED, "SOF0 length")
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i], seg[8 + 3 * i]) for i in range(nc)]
            if nc == 3:
                if [c[0] for c in comps] == [ord("R"), ord("G"), ord("B")]:
                    raise Refused(E_RGB_IDS, "component ids R, G, B")
                if [c[1] for c in comps] != [0x22, 0x11, 0x11]:
                    raise Refused(E_SAMPLING, "sampling other than 4:2:0")
            if any(c[2] > 1 for c in comps):
                raise Refused(E_TABLES, "quantisation table selector above 1")
            if H < DH.MIN_SIDE or W < DH.MIN_SIDE:
                raise Refused(E_SIZE, f"H and W must be at least {DH.MIN_SIDE}")
            sof = (H, W, nc, comps)
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Refused(E_SOF, "progressive, extended, lossless or arithmetic coding")
        elif m == 0xCC:
            raise Refused(E_SOF, "arithmetic coding conditioning")
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq != 0:
                    raise Refused(E_DQT16, "16-bit quantisation table")
                if tq > 1:
                    raise Refused(E_TABLES, "quantisation table id above 1")
                if q + 65 > len(seg):
                    raise Refused(E_MALFORMED, "short DQT")
                vals = np.frombuffer(seg[q + 1:q + 65], np.uint8).astype(np.int32)
                if (vals == 0).any():
                    raise Refused(E_MALFORMED, "zero quantisation value")
                qt[tq][ZIGZAG] = vals
                have_q[tq] = True
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise Refused(E_MALFORMED, "short DHT")
                tc, th = seg[q] >> 4, seg[q] & 15
                if tc > 1 or th > 1:
                    raise Refused(E_TABLES, "Huffman table class or id above 1")
                bits = tuple(seg[q + 1:q + 17])
                cnt = sum(bits)
                if cnt > 256 or q + 17 + cnt > len(seg):
                    raise Refused(E_MALFORMED, "short DHT")
                vals = tuple(seg[q + 17:q + 17 + cnt])
                code = 0
                for l in range(16):                     # the codes must fit their lengths, all-ones excluded
                    code += bits[l]
                    if code > (1 << (l + 1)) - 1:
                        raise Refused(E_MALFORMED, "over-subscribed Huffman table")
                    code <<= 1
                if tc == 0 and (cnt > 16 or any(v > 11 for v in vals)):
                    raise Refused(E_TABLES, "DC category above 11")
                if tc == 1 and any((v & 15) > 10 for v in vals):
                    raise Refused(E_TABLES, "AC size above 10")
                (dc if tc == 0 else ac)[th] = (bits, vals)
                q += 17 + cnt
        elif m == 0xDD:
            if len(seg) != 2:
                raise Refused(E_MALFORMED, "DRI length")
            if seg[0] or seg[1]:
                raise Refused(E_DRI, "restart interval")
        elif m == 0xEE:
            if seg[:5] == b"Adobe":
                raise Refused(E_ADOBE, "Adobe APP14 marker")
        elif m == 0xDA:
            if sof is None:
                raise Refused(E_MALFORMED, "SOS before SOF0")
            H, W, nc, comps = sof
            if len(seg) < 1 or seg[0] != nc:
                raise Refused(E_MULTISCAN, "a scan that does not hold every component")
            if len(seg) != 4 + 2 * nc:
                raise Refused(E_MALFORMED, "SOS length")
            dcsel, acsel = [], []
            for i in range(nc):
                if seg[1 + 2 * i] != comps[i][0]:
                    raise Refused(E_MALFORMED, "scan components out of frame order")
                d, a = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if d > 1 or a > 1 or dc[d] is None or ac[a] is None:
                    raise Refused(E_TABLES, "scan names a Huffman table the file does not define")
                dcsel.append(d)
                acsel.append(a)
            if seg[1 + 2 * nc] != 0 or seg[2 + 2 * nc] != 63 or seg[3 + 2 * nc] != 0:
                raise Refused(E_SOF, "spectral selection or successive approximation")
            qsel = [c[2] for c in comps]
            if not all(have_q[t] for t in qsel):
                raise Refused(E_TABLES, "frame names a quantisation table the file does not define")
            break
        # everything else (APPn, COM, DNL, ...) is skipped
    e = p
    while True:
        e = data.find(b"\xff", e)
        if e < 0 or e + 1 >= n:
            raise Refused(E_SCAN_CUT, "file ends in the scan")
        if data[e + 1] != 0:
            break
        e += 2
    if e == p:
        raise Refused(E_MALFORMED, "empty scan")
    if 0xD0 <= data[e + 1] <= 0xD7:
        raise Refused(E_DRI, "restart marker in the scan")
    if data[e + 1] != 0xD9:
        raise Refused(E_MULTISCAN, "the scan is not followed by EOI")
    return dict(H=H, W=W, ncomp=nc, qt=qt, dc=dc, ac=ac, qsel=qsel, dcsel=dcsel, acsel=acsel, scan_off=p,
                scan_len=e - p)


def _lookup(bits, vals):
    """16-bit window -> (length << 8) | symbol, 0 for an unassigned code (lists, for the Python loop)."""
    t = np.zeros(1 << 16, np.int32)
    code, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            lo = code << (16 - ln)
            t[lo:lo + (1 << (16 - ln))] = (ln << 8) | vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return t.tolist()


class _Stream:
    """The unstuffed scan of a parsed file as a bit stream (bits past the end read as 1) and its decode step."""

    def __init__(self, data: bytes, info: dict):
        raw = np.frombuffer(bytes(data[info["scan_off"]:info["scan_off"] + info["scan_len"]]), np.uint8)
        drop = np.nonzero((raw[1:] == 0) & (raw[:-1] == 0xFF))[0] + 1
        raw = np.delete(raw, drop)
        self.nbits = 8 * raw.size
        self.b = raw.tolist() + [0xFF] * 8
        nc = info["ncomp"]
        comp = [0, 0, 0, 0, 1, 2] if nc == 3 else [0]
        self.bpm = len(comp)
        self.comp = comp
        luts = {}
        for kind, sel in (("dc", info["dcsel"]), ("ac", info["acsel"])):
            for t in set(sel):
                luts[(kind, t)] = _lookup(*info[kind][t])
        self.dc = [luts[("dc", info["dcsel"][c])] for c in comp]
        self.ac = [luts[("ac", info["acsel"][c])] for c in comp]
        mh, mw = (-(-info["H"] // 16), -(-info["W"] // 16)) if nc == 3 else (-(-info["H"] // 8), -(-info["W"] // 8))
        self.nblocks = mh * mw * self.bpm

    def peek(self, p, n):
        """n <= 16 bits at bit p."""
        i = p >> 3
        b = self.b
        return (((b[i] << 16) | (b[i + 1] << 8) | b[i + 2]) >> (24 - (p & 7) - n)) & ((1 << n) - 1)

    def step(self, p, k, z):
        """One symbol at (bit p, block k of the MCU, zigzag position z; z == 0: a DC symbol is due).
        -> (p, k, z, begun, store, err): the state after it, whether it began a block, (zigzag position, value) to
        store or None, and whether the path is invalid here (an unassigned code, or a run past position 63).  An
        unassigned code consumes one bit and leaves (k, z) alone, so every step consumes at least one bit."""
        e = (self.dc if z == 0 else self.ac)[k][self.peek(p, 16)]
        if e == 0:
            return p + 1, k, z, 0, None, True
        ln, sym = e >> 8, e & 255
        p += ln
        err, store, begun = False, None, 0
        if z == 0:
            v = self.peek(p, sym) if sym else 0
            if sym and v < (1 << (sym - 1)):
                v -= (1 << sym) - 1
            p += sym
            store, z, begun = (0, v), 1, 1
        else:
            r, s = sym >> 4, sym & 15
            if s == 0:
                z = z + 16 if r == 15 else 64
                err = r == 15 and z > 63
            else:
                z += r
                v = self.peek(p, s)
                if v < (1 << (s - 1)):
                    v -= (1 << s) - 1
                p += s
                if z > 63:
                    err = True
                else:
                    store = (z, v)
                z += 1
        if z >= 64:
            k, z = (k + 1) % self.bpm, 0
        return p, k, z, begun, store, err


def decode_coefficients(data: bytes, info: dict | None = None) -> np.ndarray:
    """The quantised coefficients of a file in zigzag order, int16 [MCUs][6][64] (4:2:0; blocks Y00 Y01 Y10 Y11 Cb
    Cr, as `quantised_coefficients`) or [blocks][1][64] (one component, blocks in raster order).  Raises `Refused`
    (E_MALFORMED) where the stream is invalid or does not hold exactly the blocks of the frame."""
    info = parse(data) if info is None else info
    st = _Stream(data, info)
    out = np.zeros((st.nblocks, 64), np.int64)
    p = k = z = 0
    blk = -1
    while blk + 1 < st.nblocks or z != 0:
        if p >= st.nbits:
            raise Refused(E_MALFORMED, "the scan ends before the last block")
        p, k, z, begun, store, err = st.step(p, k, z)
        if err:
            raise Refused(E_MALFORMED, "invalid Huffman stream")
        blk += begun
        if store is not None:
            out[blk, store[0]] = store[1]
    if st.nbits - p >= 8 or p > st.nbits:
        raise Refused(E_MALFORMED, "bytes left over after the last block")
    out = out.reshape(-1, st.bpm, 64)
    for c in range(info["ncomp"]):
        sel = [i for i in range(st.bpm) if st.comp[i] == c]
        d = out[:, sel, 0]
        out[:, sel, 0] = np.cumsum(d.reshape(-1)).reshape(d.shape)
    return out.astype(np.int16)


def sync_rounds(data: bytes, subseq_bits: int = DEFAULT_SUBSEQ_BITS, lanes: int = PASS_LANES) -> int:
    """The rounds csrc/jpeg_decode.hip's entry-state kernel needs on this file, modelled on the sequential decoder:
    the stream is cut into subsequences of `subseq_bits`, walked in passes of `lanes`; round 0 decodes every
    subsequence from (0, 0, 0) (the first of a pass from the carried state), round r from its predecessor's exit
    state of round r - 1, until no exit state changes.  Returns the largest number of rounds of any pass,
    counting the final round that changes nothing."""
    info = parse(data)
    st = _Stream(data, info)
    S = int(subseq_bits)
    nsub = -(-st.nbits // S)

    def run(i, state):
        p, k, z = state[0] + i * S, state[1], state[2]
        end = min((i + 1) * S, st.nbits)
        while p < end:
            p, k, z = st.step(p, k, z)[:3]
        return (p - end, k, z)

    carry, worst = (0, 0, 0), 0
    for base in range(0, nsub, lanes):
        n = min(lanes, nsub - base)
        entry = [carry] + [(0, 0, 0)] * (n - 1)
        exits = [run(base + i, entry[i]) for i in range(n)]
        rounds = 1
        while True:
            new_entry = [carry] + exits[:-1]
            changed = False
            for i in range(n):
                if new_entry[i] != entry[i]:
                    e = run(base + i, new_entry[i])
                    changed |= e != exits[i]
                    exits[i] = e
            entry = new_entry
            rounds += 1
            if not changed:
                break
        carry = exits[-1]
        worst = max(worst, rounds)
    return worst


# decoder statuses (positive; bits of irx_jpeg_decode's status[b])
S_STREAM, S_BLOCKS, S_RANGE = 1, 2, 4
IDCT_SAFE_SUM = 32767


def range_limit_masked(v: np.ndarray) -> np.ndarray:
    """The output stage of libjpeg's C IDCT, `range_limit[v & RANGE_MASK]` on the level-shifted table (jdmaster.c
    prepare_range_limit_table): a clamp of v + 128 to 0..255 for -512 <= v < 512 and the table's wrap outside.  NOT
    what `decode` does: Pillow's libjpeg-turbo runs the SIMD IDCT, which saturates (tests/test_jpeg_decode_host.py
    holds both against Pillow on the crafted file)."""
    u = v & 1023
    return np.where(u < 128, u + 128, np.where(u < 512, 255, np.where(u < 896, 0, u - 896)))


def range_limit(v: np.ndarray) -> np.ndarray:
    """The output stage `decode` uses: a plain clamp of v + 128, as csrc/jpeg_idct.h."""
    return np.clip(v + 128, 0, 255)


def _check_range(t: np.ndarray) -> None:
    """The inputs of a 1-D pass (last axis) must sum to at most 32767 in magnitude: below that libjpeg's C code,
    libjpeg-turbo's SIMD code (16-bit lanes) and the kernel (32-bit) agree; above it the file is PIL's (S_RANGE)."""
    if t.size and int(np.abs(t).sum(-1).max()) > IDCT_SAFE_SUM:
        raise Refused(S_RANGE, "coefficients outside the range in which libjpeg's C and SIMD IDCTs agree")


def _idct_blocks(c: np.ndarray, q: np.ndarray) -> np.ndarray:
    """int64 [..., 64] zigzag coefficients, q int [64] natural -> samples 0..255 [..., 8, 8]."""
    nat = np.zeros(c.shape, np.int64)
    nat[..., ZIGZAG] = c
    nat = (nat * q.astype(np.int64)).reshape(c.shape[:-1] + (8, 8))
    _check_range(nat.swapaxes(-1, -2))
    t = DH._idct_pass(nat.swapaxes(-1, -2), DH._CONST_BITS - DH._PASS1_BITS).swapaxes(-1, -2)     # columns
    if t.size and int(np.abs(t).max()) > IDCT_SAFE_SUM:
        raise Refused(S_RANGE, "coefficients outside the range in which libjpeg's C and SIMD IDCTs agree")
    _check_range(t)
    t = DH._idct_pass(t, DH._CONST_BITS + DH._PASS1_BITS + 3)                                     # rows
    return range_limit(t)


def pixels(coef: np.ndarray, info: dict, mode: str = "RGB") -> np.ndarray:
    """Decoded coefficients -> uint8 [H][W][3] (mode "RGB") or [H][W] (mode "L", one-component files only)."""
    H, W, nc = info["H"], info["W"], info["ncomp"]
    if mode not in ("RGB", "L") or (mode == "L" and nc != 1):
        raise ValueError("mode 'RGB', or 'L' for a one-component file")
    c = coef.astype(np.int64)
    qt = info["qt"]
    if nc == 1:
        bh, bw = -(-H // 8), -(-W // 8)
        y = _idct_blocks(c[:, 0], qt[info["qsel"][0]]).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3)
        y = y.reshape(8 * bh, 8 * bw)[:H, :W].astype(np.uint8)
        return y if mode == "L" else np.repeat(y[..., None], 3, -1)
    mh, mw = -(-H // 16), -(-W // 16)
    yb = _idct_blocks(c[:, :4], qt[info["qsel"][0]]).reshape(mh, mw, 2, 2, 8, 8)                  # [my][mx][by][bx][r][c]
    Y = yb.transpose(0, 2, 4, 1, 3, 5).reshape(16 * mh, 16 * mw)[:H, :W]
    CH, CW = (H + 1) // 2, (W + 1) // 2
    ch = []
    for i in (1, 2):
        pl = _idct_blocks(c[:, 3 + i], qt[info["qsel"][i]]).reshape(mh, mw, 8, 8).transpose(0, 2, 1, 3)
        ch.append(DH._upsample_h2v2_fancy(pl.reshape(8 * mh, 8 * mw)[:CH, :CW], H, W) - 128)
    cb, cr = ch
    Ro = Y + ((DH._fix(1.402) * cr + 32768) >> 16)
    Bo = Y + ((DH._fix(1.772) * cb + 32768) >> 16)
    Go = Y + ((-DH._fix(.34414) * cb + 32768 - DH._fix(.71414) * cr) >> 16)
    return np.clip(np.stack([Ro, Go, Bo], -1), 0, 255).astype(np.uint8)


def decode(data: bytes, mode: str = "RGB") -> np.ndarray:
    """A file -> the pixels `np.asarray(PIL.Image.open(f).convert(mode))` holds (mode "L": one-component files)."""
    info = parse(data)
    return pixels(decode_coefficients(data, info), info, mode)
