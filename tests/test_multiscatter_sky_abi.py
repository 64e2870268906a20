"""include/szg/multiscatter_sky.h: every symbol it declares is exported and bound, and the other way round; its constants; the
refusals that need no device. No GPU needed."""
import ctypes as C
import os
import re

from syzygy_amd import abi, lib
from syzygy_amd._lib import library_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = abi.SZG_ERR_INVALID_ARGUMENT


def header(name):
    return open(os.path.join(ROOT, "include", "szg", name)).read()


def test_every_symbol_of_the_header_is_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header("multiscatter_sky.h"), flags=re.S)
    names = sorted(set(re.findall(r"\b(szg_[a-z0-9_]+)\s*\(", text)))
    assert names == ["szg_skyview_get_multiscatter", "szg_skyview_set_multiscatter"]
    handle = C.CDLL(library_path())
    for name in names:
        assert hasattr(handle, name), f"{name} declared in multiscatter_sky.h but not exported"
    assert sorted(abi.MULTISCATTER_SKY_FUNCTIONS) == names
    for name in names:
        assert getattr(lib(), name).argtypes == abi.MULTISCATTER_SKY_FUNCTIONS[name][1]
        assert getattr(lib(), name).restype == abi.MULTISCATTER_SKY_FUNCTIONS[name][0]
    assert any(h == "multiscatter_sky.h" and t is abi.MULTISCATTER_SKY_FUNCTIONS for h, t, _ in abi.BINDINGS)


def test_declarations_match_the_python_table():
    text = re.sub(r"/\*.*?\*/", "", header("multiscatter_sky.h"), flags=re.S)
    ctype = {"szg_skyview_t*": C.c_void_p, "const szg_skyview_t*": C.c_void_p, "uint32_t": C.c_uint32, "uint32_t*": C.POINTER(C.c_uint32)}
    for ret, name, params in re.findall(r"\b(int)\s+(szg_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        types = [ctype[re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*")] for p in params.split(",")]
        assert (C.c_int, types) == abi.MULTISCATTER_SKY_FUNCTIONS[name], name


def test_constants_and_version():
    defines = dict(re.findall(r"#define\s+(SZG_MULTISCATTER_[A-Z]+)\s+(\d+)u", header("multiscatter_sky.h")))
    assert defines == {"SZG_MULTISCATTER_OFF": "0", "SZG_MULTISCATTER_ADD": "1", "SZG_MULTISCATTER_ONLY": "2"}
    for name, value in defines.items():
        assert int(value) == getattr(abi, name), name
    # additive: the version does not move
    assert lib().szg_abi_version() == abi.SZG_ABI_VERSION == int(re.search(r"#define SZG_ABI_VERSION (\d+)", header("abi.h")).group(1))
    # abi.h no longer says that nothing consumes the LUT, and points here
    assert "NOT consumed by any parity pass" not in header("abi.h") and "szg/multiscatter_sky.h" in header("abi.h")
    for phrase in ("OUT OF SCOPE", "sampleGround", "szg_skyview_record_composite_fast", "k_multiscatter"):
        assert phrase in header("multiscatter_sky.h"), phrase


def test_refusals_without_a_pipeline():
    assert lib().szg_skyview_set_multiscatter(None, abi.SZG_MULTISCATTER_ADD) == INV
    assert b"szg_skyview_set_multiscatter" in lib().szg_last_error()
    mode = C.c_uint32(77)
    assert lib().szg_skyview_get_multiscatter(None, C.byref(mode)) == INV and mode.value == 77
    assert b"szg_skyview_get_multiscatter" in lib().szg_last_error()
    assert lib().szg_skyview_set_multiscatter(None, 3) == INV
