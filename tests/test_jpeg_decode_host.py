"""CPU tests of the baseline JPEG decoder's host side (jpeg_host.parse / decode_coefficients / decode, the oracle of
csrc/jpeg_decode.hip; csrc/jpeg_parse.cpp through irx_jpeg_parse where the library is built): the pixels equal
`PIL.Image.open(f).convert(mode)` exactly, the coefficients equal the encoder's, files outside the contract are
refused with a status of their own, and `jpeg_gpu.decode` on a CPU device returns or raises what PIL does."""
import io

import numpy as np
import pytest

from image_restoration_and_enhancement_amd import jpeg_host as JH
from tests import jpeg_cases as K
from tests import jpeg_decode_cases as DC

turbo = pytest.mark.skipif(not K.have_turbo(), reason="Pillow without libjpeg-turbo: other IDCT / up-sampling rounding")


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_pinned_coefficients(case):
    """The decoder inverts the encoder: the ten pinned files give back `quantised_coefficients` of their source
    (8x8, 17x33, 24x40, 40x24, 33x47, 50x70 have dummy blocks in the stream)."""
    img = K.case_image(case)
    data = JH.encode(img, case[3])
    assert np.array_equal(JH.decode_coefficients(data), JH.quantised_coefficients(img, case[3]))
    assert JH.decode(data).shape == img.shape


@turbo
@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_pinned_pixels_equal_pillow(case):
    data = DC.pinned(case[0])
    assert np.array_equal(JH.decode_coefficients(data), JH.quantised_coefficients(K.case_image(case), case[3]))
    assert np.array_equal(JH.decode(data), DC.pil_pixels(data))


def test_known_answer_without_pillow():
    data = DC.const_file()
    coef = JH.decode_coefficients(data)
    assert coef.shape == (4, 6, 64) and (coef[:, :4, 0] == 72).all() and (coef[:, :, 1:] == 0).all()
    assert (coef[:, 4:, 0] == 0).all()
    px = JH.decode(data)
    assert px.shape == (32, 32, 3) and (px == K.CONST_VALUE).all()


@turbo
@pytest.mark.parametrize("name", ["optimize", "qtables1"])
def test_other_tables_equal_pillow(name):
    """optimize=True: DHT tables that are not Annex K; all-ones quantisation tables: large coefficients."""
    data = DC.other(name)
    info = JH.parse(data)
    if name == "optimize":
        assert info["ac"][0][0] != JH.AC_LUMA_BITS
    else:
        assert (info["qt"] == 1).all() and int(np.abs(JH.decode_coefficients(data)).max()) > 100
    assert np.array_equal(JH.decode(data), DC.pil_pixels(data))


@turbo
@pytest.mark.parametrize("name", DC.GRAYS + DC.DEMO_MASKS)
def test_grayscale_equals_pillow(name):
    """33x47 and 8x8 `L` files from Pillow, and the two demo masks (333x500, 457x640; another encoder's files)."""
    if name in DC.DEMO_MASKS and not DC.demo_present([name]):
        pytest.skip("demo mask not present")
    data = DC.demo(name) if name in DC.DEMO_MASKS else DC.other(name)
    assert JH.parse(data)["ncomp"] == 1
    assert np.array_equal(JH.decode(data, "L"), DC.pil_pixels(data, "L"))
    assert np.array_equal(JH.decode(data, "RGB"), DC.pil_pixels(data, "RGB"))


@turbo
@pytest.mark.parametrize("name", DC.DEMO_COLOUR)
def test_demo_colour_files_equal_pillow(name):
    """The six real 4:2:0 files of the format contract (under a second of sequential Python each)."""
    if not DC.demo_present([name]):
        pytest.skip("demo file not present")
    data = DC.demo(name)
    assert JH.parse(data)["ncomp"] == 3
    assert np.array_equal(JH.decode(data), DC.pil_pixels(data))


def test_mode_l_of_a_colour_file_is_refused():
    with pytest.raises(ValueError):
        JH.decode(DC.const_file(), "L")


@turbo
def test_crafted_file_decides_the_output_stage(monkeypatch):
    """A single 1023-valued AC coefficient swings the IDCT to about +-1100, outside the 10-bit window of libjpeg's
    range-limit table.  Pillow (libjpeg-turbo, SIMD islow IDCT) gives the clamp; the masked table of the C code gives
    other pixels, so the decoder clamps (csrc/jpeg_idct.h)."""
    data = DC.crafted_file()
    ref = DC.pil_pixels(data)
    assert np.array_equal(JH.decode_coefficients(data), DC.crafted_coefficients())
    got = JH.decode(data)
    assert np.array_equal(got, ref)
    assert got[:8, :8].min() == 0 and got[:8, :8].max() == 255
    monkeypatch.setattr(JH, "range_limit", JH.range_limit_masked)
    assert not np.array_equal(JH.decode(data), ref), "the file does not tell a clamp from the masked table"


def test_block_of_largest_coefficients_is_left_to_pil():
    """A block whose 63 AC coefficients are all +-1023: the sums of the IDCT pass the 16-bit lanes of libjpeg-turbo's
    SIMD code, whose saturating and wrapping there is no property of libjpeg's arithmetic (measured on this file:
    Pillow differs from both the clamp and the masked table of the C code in 102 resp. 120 samples of the block).
    The decoder does not guess: it reports S_RANGE, and `jpeg_gpu.decode` hands the file to PIL."""
    import torch
    from image_restoration_and_enhancement_amd import jpeg_gpu as JG
    coef = np.zeros((4, 6, 64), np.int16)
    coef[0, 0, 1:] = np.where(np.arange(63) % 2 == 0, 1023, -1023)
    data = JH.header(32, 32, 75) + JH.scan(coef)[0] + b"\xff\xd9"
    assert np.array_equal(JH.decode_coefficients(data), coef)
    with pytest.raises(JH.Refused) as e:
        JH.decode(data)
    assert e.value.status == JH.S_RANGE
    got = JG.decode([data], device="cpu")[0]
    assert JG.last_fallbacks == [0] and JG.last_fallback_status == [JH.S_RANGE]
    assert torch.equal(got, torch.from_numpy(DC.pil_pixels(data)))


def test_refusals_have_their_own_status():
    files = DC.refused_files()
    seen = {}
    for name, (data, status) in files.items():
        with pytest.raises(JH.Refused) as e:
            JH.parse(data)
        assert e.value.status == status, (name, e.value.status, str(e.value))
        seen[name] = e.value.status
    # one status per kind of refusal (the two samplings are one kind)
    kinds = {n: s for n, s in seen.items() if n != "subsampling1"}
    assert len(set(kinds.values())) == len(kinds)


def test_markers_outside_the_contract():
    """Hand-made headers: 12-bit precision, 16-bit DQT, Adobe APP14, R G B ids, CMYK, a second scan, a small image;
    APPn and COM are skipped."""
    statuses = set()
    for name, (data, status) in DC.handmade_refused().items():
        with pytest.raises(JH.Refused) as e:
            JH.parse(data)
        assert e.value.status == status, (name, str(e.value))
        statuses.add(status)
    assert len(statuses) == 7
    data = DC.with_app_and_com()
    info = JH.parse(data)
    assert (info["H"], info["W"], info["ncomp"]) == (32, 32, 3) and info["scan_len"] == len(K.CONST_SCAN)
    assert (JH.decode(data) == K.CONST_VALUE).all()


def test_native_parser_agrees():
    """irx_jpeg_parse (csrc/jpeg_parse.cpp) against jpeg_host.parse: every status, Pillow-written and hand-made, and
    every field of every file the tests decode (the demo files included).  Needs the built library, no GPU."""
    from image_restoration_and_enhancement_amd import _lib as L
    from image_restoration_and_enhancement_amd import jpeg_gpu as JG
    refused = dict(DC.refused_files())
    refused.update(DC.handmade_refused())
    for name, (data, status) in refused.items():
        st, _ = JG.parse(data)
        assert st == status, name
        assert L.load().irx_last_error().startswith(b"irx_jpeg_parse: ")
    for name, data in DC.all_decodable().items():
        st, info = JG.parse(data)
        ref = JH.parse(data)
        assert st == 0, name
        assert (info.H, info.W, info.ncomp, info.scan_off, info.scan_len) == \
            (ref["H"], ref["W"], ref["ncomp"], ref["scan_off"], ref["scan_len"]), name
        for c in range(info.ncomp):
            assert (info.qsel[c], info.dcsel[c], info.acsel[c]) == (ref["qsel"][c], ref["dcsel"][c], ref["acsel"][c])
            assert list(info.qt[info.qsel[c]]) == ref["qt"][ref["qsel"][c]].tolist()
            for kind, sel, bits, vals, count in (("dc", info.dcsel[c], info.dc_bits, info.dc_vals, info.dc_count),
                                                 ("ac", info.acsel[c], info.ac_bits, info.ac_vals, info.ac_count)):
                assert tuple(bits[sel]) == tuple(ref[kind][sel][0]), (name, kind)
                assert tuple(vals[sel])[:count[sel]] == tuple(ref[kind][sel][1]), (name, kind)


def test_cpu_device_returns_what_pil_returns():
    """`jpeg_gpu.decode` on a CPU device: decodable files through jpeg_host, refused ones through PIL; a file PIL
    cannot read raises PIL's error."""
    import torch
    from PIL import Image
    from image_restoration_and_enhancement_amd import jpeg_gpu as JG
    refused = DC.refused_files()
    files = [DC.pinned("n17x33"), refused["progressive"][0], DC.other("gray33x47"), refused["subsampling0"][0]]
    got = JG.decode(files, device="cpu")
    assert JG.last_fallbacks == [1, 3] and JG.last_fallback_status == [JH.E_SOF, JH.E_SAMPLING]
    if K.have_turbo():
        for f, t in zip(files, got):
            assert t.dtype == torch.uint8 and np.array_equal(t.numpy(), DC.pil_pixels(f))
    g = JG.decode([DC.other("gray8")], mode="L", device="cpu")[0]
    assert tuple(g.shape) == (8, 8)
    if K.have_turbo():
        assert np.array_equal(g.numpy(), DC.pil_pixels(DC.other("gray8"), "L"))
    # mode L of a colour file: PIL's convert
    JG.decode([DC.pinned("n16")], mode="L", device="cpu")
    assert JG.last_fallbacks == [0]
    for bad in (refused["empty"][0], refused["cut_header"][0]):
        with pytest.raises(Exception) as e:
            JG.decode([bad], device="cpu")
        with pytest.raises(type(e.value)):
            Image.open(io.BytesIO(bad)).convert("RGB")
    # a scan cut mid-stream: PIL either decodes what is there or raises; the call does the same
    cut = refused["cut_scan"][0]
    try:
        ref = DC.pil_pixels(cut)
    except Exception as e:
        with pytest.raises(type(e)):
            JG.decode([cut], device="cpu")
    else:
        assert np.array_equal(JG.decode([cut], device="cpu")[0].numpy(), ref)


def test_round_model_needs_more_than_one_round():
    """The inputs of the GPU tests' subseq_bits cases: on both files a lane started at (0, 0, 0) is wrong for its
    subsequence, so the entry-state kernel needs at least two rounds, and at 32 bits more than one 256-lane pass."""
    for name in ("n33x47", "r50x70"):
        data = DC.pinned(name)
        nbits = JH._Stream(data, JH.parse(data)).nbits
        assert nbits > 32 * JH.PASS_LANES
        for s in (32, 64, JH.DEFAULT_SUBSEQ_BITS):
            assert JH.sync_rounds(data, s) >= 2, (name, s)


def test_decode_refuses_an_info_the_parser_would_not_fill():
    """irx_jpeg_decode_ws_bytes (host only) is 0 for what irx_jpeg_decode refuses: a Huffman table whose code counts
    do not add up to its symbols or are over-subscribed, a missing table, a bad selector, a bad subseq_bits."""
    import ctypes as C
    from image_restoration_and_enhancement_amd import _lib as L
    from image_restoration_and_enhancement_amd import jpeg_gpu as JG
    st, good = JG.parse(DC.const_file())
    assert st == 0

    def ws(info, s=0):
        arr = (L.JpegInfo * 1)(info)
        return L.call("irx_jpeg_decode_ws_bytes", C.cast(arr, C.c_void_p), 1, s)

    assert ws(good) > 0 and ws(good, 32) > 0 and ws(good, 48) == 0 and ws(good, 16) == 0
    bad = L.JpegInfo.from_buffer_copy(bytes(good))
    bad.ac_bits[0][0] = 3                      # three codes of length 1
    assert ws(bad) == 0
    bad = L.JpegInfo.from_buffer_copy(bytes(good))
    bad.ac_bits[1][15] += 1                    # one code more than symbols
    assert ws(bad) == 0
    bad = L.JpegInfo.from_buffer_copy(bytes(good))
    bad.dc_count[0] = 0                        # the luma DC table is gone
    assert ws(bad) == 0
    bad = L.JpegInfo.from_buffer_copy(bytes(good))
    bad.acsel[2] = 2
    assert ws(bad) == 0
    bad = L.JpegInfo.from_buffer_copy(bytes(good))
    bad.scan_len = 0
    assert ws(bad) == 0
