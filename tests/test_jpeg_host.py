"""include/szg/jpeg.h on the CPU: szg_jpeg_open + szg_jpeg_reconstruct_host against the recorded outputs of the reference's
decoder (tests/golden/jpeg) and against the numpy model; the parser against an independent encoder (tests/jpeg_writer.py),
coefficient by coefficient; every refusal of rule 1 with its text. Everything is equality."""
import ctypes as C
import struct

import numpy as np
import pytest

from syzygy_amd import abi, assets, lib
from tests import jpeg_fixtures as jf
from tests import jpeg_model as jm
from tests import jpeg_writer as jw


def test_the_fixture_set_is_complete():
    names = jf.names()
    for size in ("1x1", "2x3", "7x5", "8x8", "9x17", "17x9", "33x31", "130x70"):
        for layout in ("444", "422", "420", "grey"):
            for mode in ("base", "prog", "rst"):
                assert sum(n.startswith(f"{layout}_{size}_{mode}_q") for n in names) == 2, (size, layout, mode)
    assert sum(n.startswith("h1v2_") for n in names) == 5 and sum(n.startswith("h4v1_") for n in names) == 3
    assert sum(n.startswith("h1v4_") for n in names) == 2
    assert "rgbids_17x9_base_q85" in names and "adobe0_17x9_base_q85" in names
    assert jf.refused_names() == ["refused_cmyk_17x9"]


@pytest.mark.parametrize("name", jf.names())
def test_fixture_equals_the_reference_and_the_model(name):
    want = jf.expected(name)
    with jf.Jpeg(jf.data(name)) as j:
        assert j.status == abi.SZG_OK, j.error
        f = j.frame
        assert (f.height, f.width) == want.shape[:2]
        assert f.progressive == (1 if "_prog_" in name else 0)
        got = j.reconstruct_host().reshape(f.height, f.width, 4)
        assert (got == want).all()
        assert (jm.reconstruct(j.model_frame()) == want).all()
    assert (assets.decode_jpeg_rgba(jf.data(name)) == want).all()


def test_frame_geometry_and_colour():
    with jf.Jpeg(jf.data("420_33x31_base_q92")) as j:
        f = j.frame
        assert (f.width, f.height, f.plane_count, f.color, f.h_max, f.v_max) == (33, 31, 3, abi.SZG_JPEG_YCBCR, 2, 2)
        assert [(p.h, p.v, p.width, p.height, p.blocks_w, p.blocks_h) for p in f.planes] == \
            [(2, 2, 33, 31, 6, 4), (1, 1, 17, 16, 3, 2), (1, 1, 17, 16, 3, 2)]
        assert lib().szg_jpeg_scratch_bytes(C.byref(f)) == (6 * 4 + 3 * 2 * 2) * 64
    for name, color in (("grey_9x17_base_q92", abi.SZG_JPEG_GREY), ("rgbids_17x9_base_q85", abi.SZG_JPEG_RGB),
                        ("adobe0_17x9_base_q85", abi.SZG_JPEG_RGB), ("h4v1_33x16_base_q85", abi.SZG_JPEG_YCBCR)):
        with jf.Jpeg(jf.data(name)) as j:
            assert j.frame.color == color, name


def test_padded_pitch_is_left_alone_and_masks_apply():
    name = "422_17x9_prog_q92"
    want = jf.expected(name)
    with jf.Jpeg(jf.data(name)) as j:
        pitch = 17 * 4 + 12
        got = j.reconstruct_host(pitch=pitch, fill=0xEE)
        assert (got[:, :68].reshape(9, 17, 4) == want).all() and (got[:, 68:] == 0xEE).all()
        # the loader's ORM overrides as masks: R := 255, and G := B := 0
        red = j.reconstruct_host(0xFFFFFFFF, 0x000000FF).reshape(9, 17, 4)
        assert (red[..., 0] == 255).all() and (red[..., 1:] == want[..., 1:]).all()
        occ = j.reconstruct_host(0xFF0000FF, 0).reshape(9, 17, 4)
        assert (occ[..., 1:3] == 0).all() and (occ[..., 0] == want[..., 0]).all() and (occ[..., 3] == 255).all()
        assert (occ == jm.reconstruct(j.model_frame(), 0xFF0000FF, 0)).all()
        # a frame whose geometry does not follow from its extent is refused, and so is a short pitch
        bad = abi.JpegFrame.from_buffer_copy(j.frame)
        bad.planes[1].blocks_w += 1
        out = np.zeros((9, 68), np.uint8)
        assert lib().szg_jpeg_reconstruct_host(C.byref(bad), 0xFFFFFFFF, 0, out.ctypes.data_as(C.c_void_p), 68) == abi.SZG_ERR_INVALID_ARGUMENT
        assert b"blocks_w" in lib().szg_last_error()
        assert lib().szg_jpeg_reconstruct_host(C.byref(j.frame), 0xFFFFFFFF, 0, out.ctypes.data_as(C.c_void_p), 64) == abi.SZG_ERR_INVALID_ARGUMENT
        assert not out.any()


# ---------------------------------------------------------------------------------------------------------------
# rule 1: refusals
# ---------------------------------------------------------------------------------------------------------------
def _sof(data):
    at = 2
    while data[at + 1] not in (0xC0, 0xC1, 0xC2):
        at += 2 + struct.unpack(">H", data[at + 2:at + 4])[0]
    return at


def _refused(data, text):
    j = jf.Jpeg(bytes(data))
    assert j.status == abi.SZG_ERR_PARSE and not j.handle, (j.status, text)
    assert text in j.error, j.error
    with pytest.raises(assets.AssetError, match="szg_jpeg_open"):
        assets.decode_jpeg_rgba(bytes(data))


def test_every_refusal_of_rule_1_has_its_text():
    base = bytearray(jf.data("444_8x8_base_q92"))
    sof = _sof(base)
    twelve = bytearray(base)
    twelve[sof + 4] = 12
    _refused(twelve, "only 8-bit precision")
    for marker, text in ((0xC9, "arithmetic"), (0xCA, "arithmetic"), (0xC3, "lossless"), (0xC7, "lossless"), (0xCB, "lossless"),
                         (0xC5, "hierarchical")):
        other = bytearray(base)
        other[sof + 1] = marker
        _refused(other, text)
    wide = bytearray(base)
    wide[sof + 7:sof + 9] = struct.pack(">H", 32769)
    _refused(wide, "above 32768")
    tall = bytearray(base)
    tall[sof + 5:sof + 7] = struct.pack(">H", 40000)
    _refused(tall, "above 32768")
    empty = bytearray(base)
    empty[sof + 5:sof + 7] = b"\0\0"
    _refused(empty, "width or height is 0")
    # a frame of 32768 x 32768 is inside the limit, but this stream cannot hold it
    huge = bytearray(base)
    huge[sof + 5:sof + 9] = struct.pack(">HH", 32768, 32768)
    _refused(huge, "truncated")
    # 2 and 4 components
    two = base[:sof] + b"\xFF\xC0" + struct.pack(">H", 8 + 6) + bytes([8, 0, 8, 0, 8, 2, 1, 0x11, 0, 2, 0x11, 0]) + base[sof + 2 + 17:]
    _refused(two, "1 or 3 components")
    _refused(jf.data("refused_cmyk_17x9"), "1 or 3 components")
    # sampling factors
    five = bytearray(base)
    five[sof + 11] = 0x51
    _refused(five, "outside 1..4")
    odd = bytearray(jf.data("420_8x8_base_q92"))
    odd[_sof(odd) + 11] = 0x32  # h = 3 with chroma h = 1 is fine, v = 2 ... but make the second component h = 2: 3 % 2 != 0
    odd[_sof(odd) + 14] = 0x21
    _refused(odd, "does not divide")
    # truncation, a missing EOI, no SOI, garbage
    _refused(base[:len(base) // 2], "truncated")
    _refused(base[:-2], "truncated")
    _refused(b"\x89PNG\r\n\x1a\n" + bytes(32), "no SOI")
    _refused(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00" + bytes(32), "marker")
    assert lib().szg_jpeg_open(None, 0, None) == abi.SZG_ERR_INVALID_ARGUMENT
    handle = C.c_void_p()
    assert lib().szg_jpeg_open(None, 4, C.byref(handle)) == abi.SZG_ERR_INVALID_ARGUMENT and not handle
    lib().szg_jpeg_destroy(None)
    # nothing of this touches the PNG-only entry point: it still refuses a JPEG stream
    with pytest.raises(assets.AssetError, match="JPEG"):
        assets.decode_image_rgba(jf.data("444_8x8_base_q92"))


# ---------------------------------------------------------------------------------------------------------------
# rule 2: the parser against an independent encoder, coefficient by coefficient
# ---------------------------------------------------------------------------------------------------------------
def _blocks(rng, shape, dense):
    """quantised blocks: DC within +-12000 (differences stay below 2^15), AC up to 15 magnitude bits"""
    bh, bw = shape
    b = np.zeros((bh, bw, 8, 8), np.int64)
    b[..., 0, 0] = rng.integers(-12000, 12001, (bh, bw))
    ac = rng.integers(-32767, 32768, (bh, bw, 8, 8))
    keep = rng.random((bh, bw, 8, 8)) < dense
    keep[..., 0, 0] = False
    b[keep] = ac[keep]
    b[..., 7, 7] = np.where(rng.random((bh, bw)) < 0.5, b[..., 7, 7], 0)  # some blocks end in EOB, some in coefficient 63
    return b


def _check(width, height, factors, tables, scans=None, restart_interval=0, dense=0.2, seed=0, **options):
    rng = np.random.default_rng(seed)
    h_max, v_max = max(f[0] for f in factors), max(f[1] for f in factors)
    components = []
    for k, (h, v) in enumerate(factors):
        bw, bh, _, _ = jm.plane_grid(width, height, h, v, h_max, v_max)
        components.append((h, v, min(k, len(tables) - 1), _blocks(rng, (bh, bw), dense)))
    data = jw.encode(width, height, components, tables, scans=scans, restart_interval=restart_interval, **options)
    masks = jw.coded_mask(width, height, components, scans)
    with jf.Jpeg(data) as j:
        assert j.status == abi.SZG_OK, j.error
        assert (j.frame.width, j.frame.height, j.frame.plane_count) == (width, height, len(factors))
        for k, (h, v, tq, blocks) in enumerate(components):
            q = np.asarray(tables[tq], np.int64).reshape(8, 8)
            want = ((blocks * q) & 0xFFFF).astype(np.uint16).view(np.int16)  # int16(value * q), wrap included
            want = np.where(masks[k][:, :, None, None], want, 0)             # blocks no scan writes are zero
            assert (j.coefficients(k) == want).all(), (k, h, v)
    return data


Q8 = {0: np.arange(1, 65).reshape(8, 8), 1: np.full((8, 8), 255)}
Q16 = {0: np.arange(1, 65).reshape(8, 8) * 1021 % 65535 + 1, 1: np.full((8, 8), 65535)}


def test_parser_returns_the_wrapped_products():
    assert int(np.asarray(Q16[0]).max()) > 255
    for w, h in ((1, 1), (17, 9)):
        _check(w, h, [(1, 1)], Q8, seed=1)
        _check(w, h, [(2, 2), (1, 1), (1, 1)], Q16, seed=2)                                        # 16-bit tables, wrap
        _check(w, h, [(2, 1), (1, 1), (1, 1)], Q8, scans=[[0], [1], [2]], seed=3)                  # non-interleaved
        _check(w, h, [(2, 2), (1, 1), (1, 1)], Q16, scans=[[1, 2], [0]], seed=4)                   # mixed
        _check(w, h, [(3, 1), (1, 1), (1, 1)], Q8, seed=5)                                         # h3v1
        for interval in (1, 3):
            _check(w, h, [(2, 2), (1, 1), (1, 1)], Q8, restart_interval=interval, seed=6)
            _check(w, h, [(1, 1), (1, 1), (1, 1)], Q16, scans=[[0], [1, 2]], restart_interval=interval, seed=7)
        _check(w, h, [(1, 2), (1, 1), (1, 1)], Q8, fill=3, restart_interval=1, seed=8)             # fill bytes before markers
        _check(w, h, [(1, 1), (1, 1), (1, 1)], Q8, ac_bits=13, dc_bits=11, seed=9)                 # codes past the look-up table
    # a 40 x 24 picture: restart markers wrap around RST7
    _check(40, 24, [(1, 1)], Q8, restart_interval=1, seed=10)


def test_stuffed_bytes_are_data():
    # dense 15-bit values put runs of one bits into the stream: FF bytes that the encoder stuffs
    data = _check(17, 9, [(1, 1), (1, 1), (1, 1)], Q16, dense=0.9, seed=11)
    sos = data.index(b"\xFF\xDA")
    assert data.count(b"\xFF\x00", sos) > 10


def test_mutated_streams_never_crash_and_fail_with_a_text():
    rng = np.random.default_rng(5)
    for name in ("420_17x9_base_q92", "444_9x17_prog_q12", "422_33x31_rst_q92"):
        data = jf.data(name)
        for k in range(150):
            m = bytearray(data)
            for _ in range(1 + k % 3):
                m[int(rng.integers(2, len(m)))] ^= 1 << int(rng.integers(0, 8))
            j = jf.Jpeg(bytes(m[:len(m) - (k % 7 == 0) * int(rng.integers(0, len(m) // 2))]))
            if j.status == abi.SZG_OK:
                j.reconstruct_host()
            else:
                assert j.status in (abi.SZG_ERR_PARSE, abi.SZG_ERR_OUT_OF_MEMORY) and j.error.startswith("szg_jpeg_open:")
            j.close()
