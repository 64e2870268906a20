"""include/szg/texture_display.h: every symbol it declares is exported and bound, and the other way round; its constants and
struct; every refusal that needs no device returns its status and a text. No GPU needed."""
import ctypes as C
import os
import re

import pytest

from syzygy_amd import abi, lib
from syzygy_amd._lib import library_path
from tests import texture_display_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = abi.SZG_ERR_INVALID_ARGUMENT


def header(name):
    return open(os.path.join(ROOT, "include", "szg", name)).read()


def test_every_symbol_of_the_header_is_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header("texture_display.h"), flags=re.S)
    names = sorted(set(re.findall(r"\b(szg_[a-z0-9_]+)\s*\(", text)))
    assert names == ["szg_record_clear_color_image", "szg_record_copy_image", "szg_ui_layer_add_texture_view"]
    handle = C.CDLL(library_path())
    for name in names:
        assert hasattr(handle, name), f"{name} declared in texture_display.h but not exported"
        assert name in abi.TEXTURE_DISPLAY_FUNCTIONS, f"{name} declared in texture_display.h but has no ctypes signature"
    assert sorted(abi.TEXTURE_DISPLAY_FUNCTIONS) == names
    for name in names:
        assert getattr(lib(), name).argtypes == abi.TEXTURE_DISPLAY_FUNCTIONS[name][1]


def test_constants_struct_and_the_new_format():
    defines = dict(re.findall(r"#define\s+(SZG_SWIZZLE_[A-Z]+)\s+(\d+)u", header("texture_display.h")))
    assert len(defines) == 7
    for name, value in defines.items():
        assert int(value) == getattr(abi, name), name
    # VkComponentSwizzle
    assert [abi.SZG_SWIZZLE_IDENTITY, abi.SZG_SWIZZLE_ZERO, abi.SZG_SWIZZLE_ONE, abi.SZG_SWIZZLE_R, abi.SZG_SWIZZLE_G,
            abi.SZG_SWIZZLE_B, abi.SZG_SWIZZLE_A] == list(range(7))
    assert C.sizeof(abi.UITextureView) == 16
    assert abi.SZG_FORMAT_RGBA8_SRGB == 8 and abi.TEXEL_BYTES[abi.SZG_FORMAT_RGBA8_SRGB] == 4
    assert re.search(r"SZG_FORMAT_RGBA8_SRGB\s*=\s*SZG_FORMAT_A2B10G10R10_UNORM \+ 1", header("abi.h")) and abi.SZG_FORMAT_A2B10G10R10_UNORM == 7
    # additive: three symbols and one format value behind the old ones
    assert lib().szg_abi_version() == abi.SZG_ABI_VERSION == int(re.search(r"#define SZG_ABI_VERSION (\d+)", header("abi.h")).group(1))


def ref(x):
    return C.byref(x) if x is not None else None


@pytest.mark.parametrize("case", tc.copy_refusals(0x10000000, 0x20000000), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_copy_refusals_are_decided_on_the_host(case):
    name, src, dst, sr, dr = case
    assert lib().szg_record_copy_image(None, ref(src), ref(dst), abi.Rect(*sr), abi.Rect(*dr)) == INV, name
    assert b"szg_record_copy_image" in lib().szg_last_error() and len(lib().szg_last_error()) > 30, name


@pytest.mark.parametrize("case", tc.clear_refusals(0x20000000), ids=lambda c: c[0].replace(" ", "_"))
def test_clear_refusals_are_decided_on_the_host(case):
    name, im, color = case
    cc = (C.c_float * 4)(*color) if color is not None else None
    assert lib().szg_record_clear_color_image(None, ref(im), cc) == INV, name
    assert b"szg_record_clear_color_image" in lib().szg_last_error() and len(lib().szg_last_error()) > 40, name


def test_regions_and_images_without_texels_are_no_ops():
    for fmt in (tc.R8, tc.SRGB8, tc.U16, tc.H16):  # and every accepted source format passes the checks
        src, dst = tc.image(64, 32, fmt, 0x10000000), tc.image(48, 24, tc.H16, 0x20000000)
        for sr, dr in tc.EMPTY_REGIONS:
            assert lib().szg_record_copy_image(None, C.byref(src), C.byref(dst), abi.Rect(*sr), abi.Rect(*dr)) == abi.SZG_OK
    black = (C.c_float * 4)(0, 0, 0, 1)
    for w, h in ((0, 24), (48, 0)):
        assert lib().szg_record_clear_color_image(None, C.byref(tc.image(w, h, tc.U16, 0x20000000)), black) == abi.SZG_OK


def test_add_texture_view_without_a_layer():
    out = C.c_void_p(1)
    im = tc.image(4, 4, tc.H16, 0x10000000)
    assert lib().szg_ui_layer_add_texture_view(None, C.byref(im), abi.UISampler(0, 0), None, C.byref(out)) == INV
    assert b"szg_ui_layer_add_texture_view" in lib().szg_last_error()


def test_the_older_entry_points_refuse_the_new_format():
    srgb = tc.image(64, 32, tc.SRGB8, 0x10000000)
    info = abi.PresentInfo(abi.Rect(0, 0, 64, 32), abi.Rect(0, 0, 64, 32), abi.SZG_FILTER_NEAREST, abi.SZG_PRESENT_ENCODE_NONE)
    assert lib().szg_record_present(None, C.byref(srgb), C.byref(tc.image(64, 32, tc.R8, 0x20000000)), C.byref(info)) == INV
    assert lib().szg_record_present(None, C.byref(tc.image(64, 32, tc.U16, 0x20000000)), C.byref(srgb), C.byref(info)) == INV
    assert lib().szg_record_oetf(None, C.byref(srgb), 64, 32, abi.SZG_OETF_SRGB) == INV
