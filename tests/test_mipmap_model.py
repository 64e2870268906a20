"""include/szg/mipmaps.h on the CPU: the numpy model of tests/mipmap_model.py against hand-computed values, the C-ABI's size
helpers against the same values, and every refusal of the new entry points, none of which needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from syzygy_amd import abi, lib, library_path
from tests import mipmap_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# (w, h) -> (levels, bytes of levels 1..): written out by hand
#   (3, 5)      5 -> 3 levels: 1x2, 1x1                                   8 + 4
#   (8, 1)      4 levels: 4x1, 2x1, 1x1                                   16 + 8 + 4
#   (257, 129)  9 levels: 128x64, 64x32, 32x16, 16x8, 8x4, 4x2, 2x1, 1x1  32768 + 8192 + 2048 + 512 + 128 + 32 + 8 + 4
#   (4096, 4096) 13 levels: 4 * (4^0 + ... + 4^11) = 4 * (4^12 - 1) / 3
SIZES = {(1, 1): (1, 0), (2, 2): (2, 4), (3, 5): (3, 12), (8, 1): (4, 28), (257, 129): (9, 43692), (4096, 4096): (13, 22369620)}


@pytest.mark.parametrize("size", sorted(SIZES))
def test_level_counts_and_chain_bytes(size):
    levels, nbytes = SIZES[size]
    assert mm.level_count(*size) == levels and mm.chain_bytes(*size) == nbytes
    assert lib().szg_mip_level_count(*size) == levels
    assert lib().szg_mip_chain_bytes(*size) == nbytes
    shapes = mm.level_shapes(*size)
    assert len(shapes) == levels and shapes[0] == size and shapes[-1] == (1, 1)


def test_empty_images_have_no_levels():
    for size in ((0, 0), (0, 7), (7, 0)):
        assert lib().szg_mip_level_count(*size) == 0 and lib().szg_mip_chain_bytes(*size) == 0
        assert mm.level_count(*size) == 0


def test_uniform_srgb_texture_keeps_its_code_at_every_level():
    for code in range(256):
        level0 = np.full((4, 8, 4), code, np.uint8)
        for k, level in enumerate(mm.build_chain(level0, True)):
            assert (level == code).all(), (code, k, level.reshape(-1, 4)[0])


def test_uniform_unorm_texture_keeps_its_code_at_every_level():
    for code in (0, 1, 127, 128, 254, 255):
        for level in mm.build_chain(np.full((5, 3, 4), code, np.uint8), False):
            assert (level == code).all()


def test_unorm_2x2_known_bytes():
    level0 = np.array([[[0, 10, 255, 1], [1, 20, 255, 2]], [[2, 30, 254, 3], [4, 41, 255, 4]]], np.uint8)
    levels = mm.build_chain(level0, False)
    assert len(levels) == 2 and levels[1].shape == (1, 1, 4)
    # (0+1+2+4+2)>>2 = 2, (10+20+30+41+2)>>2 = 25, (255+255+254+255+2)>>2 = 255, (1+2+3+4+2)>>2 = 3
    assert levels[1].reshape(4).tolist() == [2, 25, 255, 3]
    assert mm.pack_chain(levels).tolist() == [2, 25, 255, 3]


def test_odd_sizes_drop_the_last_column_and_duplicate_a_single_row():
    level0 = np.zeros((1, 5, 4), np.uint8)
    level0[0, :, 0] = [10, 20, 30, 40, 250]
    level1 = mm.downsample(level0, False)
    assert level1.shape == (1, 2, 4)
    assert level1[0, :, 0].tolist() == [15, 35]  # the row is used twice, column 4 is never read


def test_srgb_alpha_takes_the_integer_rule_and_colour_averages_in_linear_light():
    level0 = np.zeros((2, 2, 4), np.uint8)
    level0[..., :3] = [[[0] * 3, [255] * 3], [[0] * 3, [255] * 3]]
    level0[..., 3] = [[0, 1], [2, 4]]
    level1 = mm.downsample(level0, True)
    assert level1[0, 0, 3] == 2  # (0 + 1 + 2 + 4 + 2) >> 2
    # half of linear white is sRGB 0.7354 -> code 188, well above the 128 an average of the codes gives
    assert level1[0, 0, 0] == 188 and level1[0, 0, 1] == 188 and level1[0, 0, 2] == 188


def _random_chain(w, h, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (hk, wk, 4), dtype=np.uint8) for wk, hk in mm.level_shapes(w, h)]


def test_lambda_is_exactly_k_for_a_footprint_of_2_to_the_k_texels():
    W, H = 128, 64
    levels = _random_chain(W, H, 1)
    rng = np.random.default_rng(2)
    st = rng.uniform(-3, 3, (64, 2)).astype(F)
    for k in range(7):
        ddx = np.zeros((64, 2), F)
        ddx[:, 0] = F(2.0**k) / F(W)  # 2^k texels per pixel in x, exactly
        ddy = np.zeros((64, 2), F)
        ddy[:, 1] = F(1.0) / F(H)  # one texel per pixel in y
        lam = mm.mip_lambda(W, H, len(levels), mm.MAX_LOD_NONE, ddx, ddy)
        assert (lam == F(k)).all(), (k, lam[0])
        got, read = mm.sample(levels, False, st, ddx, ddy, mm.MAX_LOD_NONE, return_levels=True)
        assert read[:, k].all() and read.sum() == 64, k  # f == 0: level k alone
        assert np.array_equal(got.view(np.uint32), mm.bilinear(levels[k], False, st).view(np.uint32))


def test_max_lod_of_the_reference_never_reads_level_2():
    W, H = 64, 64
    levels = _random_chain(W, H, 3)
    rng = np.random.default_rng(4)
    n = 2048
    st = rng.uniform(-3, 3, (n, 2)).astype(F)
    mag = (2.0 ** rng.uniform(-12, 4, (n, 2))).astype(F)  # texels per pixel
    ddx = (mag * rng.choice([-1, 1], (n, 2)) / F(W)).astype(F)
    ddy = (mag[:, ::-1] / F(H)).astype(F)
    for srgb in (False, True):
        _, read = mm.sample(levels, srgb, st, ddx, ddy, mm.MAX_LOD_REFERENCE, return_levels=True)
        assert not read[:, 2:].any()
        assert read[:, 1].any() and read[:, 0].any()
    _, read = mm.sample(levels, False, st, ddx, ddy, mm.MAX_LOD_NONE, return_levels=True)
    assert read[:, 2:].any()  # the same samples do reach further without the clamp


def test_special_derivatives_select_the_documented_level():
    W, H = 16, 8
    levels = _random_chain(W, H, 5)
    L = len(levels)
    nan, inf, den = F(np.nan), F(np.inf), F(1e-42)
    cases = [((0, 0), (0, 0), 0), ((nan, 0), (0, 0), 0), ((nan, nan), (nan, nan), 0), ((den, 0), (0, den), 0),
             ((inf, 0), (0, 0), L - 1), ((-inf, 0), (0, 0), L - 1), ((nan, 0), (0, 1.0), 3), ((1e30, 0), (0, 0), L - 1)]
    for ddx, ddy, want in cases:
        lam = mm.mip_lambda(W, H, L, mm.MAX_LOD_NONE, np.array([ddx], F), np.array([ddy], F))
        assert lam[0] == F(want), (ddx, ddy, lam)
    st = np.array([[0.3, 0.7]], F)
    out = mm.sample(levels, False, st, np.array([[nan, 0]], F), np.zeros((1, 2), F), mm.MAX_LOD_NONE)
    assert np.array_equal(out, mm.bilinear(levels[0], False, st))


def test_unregistered_and_magnified_samples_equal_the_one_level_rule():
    levels = _random_chain(5, 3, 6)
    rng = np.random.default_rng(7)
    st = rng.uniform(-3, 3, (256, 2)).astype(F)
    small = np.full((256, 2), 2.0**-9, F)
    base = mm.bilinear(levels[0], True, st)
    assert np.array_equal(mm.sample(levels, True, st, small, small, mm.MAX_LOD_NONE), base)
    big = np.full((256, 2), 4.0, F)
    assert np.array_equal(mm.sample(levels, True, st, big, big, mm.MAX_LOD_NONE, level_count_registered=1), base)
    assert np.array_equal(mm.sample(levels, True, st, big, big, 0.0), base)


# ---------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------
def header(name):
    return open(os.path.join(ROOT, "include", "szg", name)).read()


def test_every_symbol_of_mipmaps_h_is_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header("mipmaps.h"), flags=re.S)
    names = sorted(set(re.findall(r"\b(szg_[a-z0-9_]+)\s*\(", text)))
    assert names == ["szg_deferred_set_texture_mips", "szg_mip_chain_bytes", "szg_mip_level_count", "szg_record_generate_mipmaps"]
    handle = C.CDLL(library_path())
    for name in names:
        assert hasattr(handle, name), f"{name} declared in mipmaps.h but not exported"
        assert name in abi.MIPMAP_FUNCTIONS, f"{name} declared in mipmaps.h but has no ctypes signature"
    assert sorted(abi.MIPMAP_FUNCTIONS) == names


def test_constants_and_structs_match_the_header():
    text = header("mipmaps.h")
    assert re.search(r"#define SZG_SAMPLER_MAX_LOD_REFERENCE 1\.0f\b", text) and abi.SZG_SAMPLER_MAX_LOD_REFERENCE == 1.0
    assert re.search(r"#define SZG_SAMPLER_MAX_LOD_NONE 1000\.0f\b", text) and abi.SZG_SAMPLER_MAX_LOD_NONE == 1000.0
    assert "vulkanstructs.cpp:147-183" in text and "material.cpp:115-120" in text and "image.cpp:86" in text
    assert C.sizeof(abi.TextureMips) == 24 and abi.TextureMips.d_chain.offset == 8 and abi.TextureMips.level_count.offset == 16
    # additive: the version and the structs of raster.h stay as they were
    assert abi.SZG_ABI_VERSION == 2 and lib().szg_abi_version() == 2
    assert (C.sizeof(abi.Texture), C.sizeof(abi.Material), C.sizeof(abi.Surface)) == (24, 72, 80)
    assert C.sizeof(abi.MeshInstanced) == 64


def _entries(*rows):
    table = (abi.TextureMips * len(rows))()
    for i, (level0, chain, levels) in enumerate(rows):
        table[i].level0_data, table[i].d_chain, table[i].level_count = level0, chain, levels
    return table


SET_REFUSALS = {
    "null entries": (None, 2, 1000.0, b"NULL entries"),
    "level_count 0": (_entries((0x1000, 0x2000, 0)), 1, 1000.0, b"level_count 0"),
    "null level0": (_entries((None, 0x2000, 2)), 1, 1000.0, b"NULL level0_data"),
    "null chain": (_entries((0x1000, None, 2)), 1, 1000.0, b"NULL d_chain"),
    "duplicate": (_entries((0x1000, 0x2000, 2), (0x3000, 0x4000, 3), (0x1000, 0x5000, 1)), 3, 1000.0, b"duplicate"),
    "misaligned level0": (_entries((0x1002, 0x2000, 2)), 1, 1000.0, b"aligned"),
    "misaligned chain": (_entries((0x1000, 0x2001, 2)), 1, 1000.0, b"aligned"),
    "negative max_lod": (_entries((0x1000, 0x2000, 2)), 1, -0.5, b"max_lod"),
    "nan max_lod": (_entries((0x1000, 0x2000, 2)), 1, float("nan"), b"max_lod"),
    "nan max_lod clearing": (None, 0, float("nan"), b"max_lod"),
    "null pipeline": (_entries((0x1000, 0x2000, 2)), 1, 1.0, b"NULL pipeline"),
}


@pytest.mark.parametrize("name", sorted(SET_REFUSALS))
def test_set_texture_mips_refuses(name):
    """No device: the pipeline handle is NULL, and the arguments are judged before it, each refusal with its own text."""
    entries, count, max_lod, text = SET_REFUSALS[name]
    assert lib().szg_deferred_set_texture_mips(None, entries, count, max_lod) == abi.SZG_ERR_INVALID_ARGUMENT
    message = lib().szg_last_error()
    assert b"szg_deferred_set_texture_mips" in message and text in message, message


@pytest.mark.parametrize("index", range(12))
def test_generate_mipmaps_refuses(index):
    name, level0, chain, nbytes, text = mm.generate_refusals(0x10000, 0x20000)[index]
    status = lib().szg_record_generate_mipmaps(None, C.byref(level0) if level0 is not None else None, chain, nbytes)
    assert status == abi.SZG_ERR_INVALID_ARGUMENT, name
    message = lib().szg_last_error()
    assert b"szg_record_generate_mipmaps" in message and text in message, (name, message)


def test_generate_mipmaps_of_a_single_texel_is_a_no_op():
    level0 = abi.Texture(0x10000, 1, 1, 4, 1)
    assert lib().szg_record_generate_mipmaps(None, C.byref(level0), None, 0) == abi.SZG_OK


def test_the_examples_mipmaps_switch():
    from syzygy_amd import pipelines

    assert pipelines.parse_mipmaps_option("none") == abi.SZG_SAMPLER_MAX_LOD_NONE
    assert pipelines.parse_mipmaps_option("reference") == abi.SZG_SAMPLER_MAX_LOD_REFERENCE == 1.0
    assert pipelines.parse_mipmaps_option("2.5") == 2.5 and pipelines.parse_mipmaps_option("0") == 0.0
    for bad in ("-1", "nan", "many", ""):
        with pytest.raises(ValueError):
            pipelines.parse_mipmaps_option(bad)
    for example in ("render_gltf.py", "frame_loop.py"):
        assert '"--mipmaps"' in open(os.path.join(ROOT, "examples", example)).read()
