"""include/szg/jpeg.h: every symbol it declares is exported and bound, and the other way round (as tests/test_abi.py does for
its headers); struct layouts; the device entry points refuse bad arguments before anything touches a device."""
import ctypes as C
import os
import re

from syzygy_amd import abi, lib, library_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", "szg", name)).read()


def test_every_declared_symbol_is_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header("jpeg.h"), flags=re.S)
    names = sorted(set(re.findall(r"\b(szg_[a-z0-9_]+)\s*\(", text)))
    assert len(names) == 7, names
    handle = C.CDLL(library_path())
    for name in names:
        assert hasattr(handle, name), f"{name} declared in jpeg.h but not exported"
        assert name in abi.JPEG_FUNCTIONS, f"{name} declared in jpeg.h but has no ctypes signature"
    for name in abi.JPEG_FUNCTIONS:
        assert name in names, f"{name} bound in Python but not declared in jpeg.h"
        assert getattr(lib(), name).argtypes is not None


def test_constants_and_layouts():
    text = _header("jpeg.h") + _header("assets.h")
    for name in ("SZG_JPEG_GREY", "SZG_JPEG_YCBCR", "SZG_JPEG_RGB", "SZG_GLTF_DECODE_JPEG", "SZG_GLTF_JPEG_FOR_DEVICE",
                 "SZG_JPEG_MAX_EXTENT"):
        value = re.search(rf"#define {name} (\d+)u", text)
        assert value and int(value.group(1)) == getattr(abi, name), name
    assert abi.SZG_GLTF_DECODE_JPEG == 2 and abi.SZG_GLTF_JPEG_FOR_DEVICE == 4
    # the flags live next to SZG_GLTF_DECODE_BUFFER_VIEW_IMAGES and add no function to assets.h
    declared = re.sub(r"/\*.*?\*/", "", _header("assets.h"), flags=re.S)
    assert re.search(r"#define SZG_GLTF_DECODE_BUFFER_VIEW_IMAGES 1u", declared) and not re.search(r"jpeg\w*\s*\(", declared)
    assert C.sizeof(abi.JpegPlane) == 32 and C.sizeof(abi.JpegFrame) == 28 + 4 + 3 * 32 and C.sizeof(abi.JpegMap) == 32
    assert abi.JpegFrame.planes.offset == 32 and abi.JpegPlane.h.offset == 8
    # additive: the ABI version did not move
    assert lib().szg_abi_version() == abi.SZG_ABI_VERSION == int(re.search(r"#define SZG_ABI_VERSION (\d+)", _header("abi.h")).group(1))


def test_null_and_invalid_arguments_are_refused_without_a_device():
    L = lib()
    frame = abi.JpegFrame()
    assert L.szg_jpeg_get_frame(None, C.byref(frame)) == abi.SZG_ERR_INVALID_ARGUMENT
    assert L.szg_jpeg_scratch_bytes(None) == 0 and L.szg_jpeg_scratch_bytes(C.byref(frame)) == 0
    image = abi.Image()
    assert L.szg_record_jpeg_reconstruct(None, None, None, 0, 0xFFFFFFFF, 0, None) == abi.SZG_ERR_INVALID_ARGUMENT
    assert b"szg_record_jpeg_reconstruct" in L.szg_last_error()
    assert L.szg_record_jpeg_reconstruct(None, C.byref(frame), C.c_void_p(16), 0, 0xFFFFFFFF, 0, C.byref(image)) == abi.SZG_ERR_INVALID_ARGUMENT
    image.data = 16
    assert L.szg_record_jpeg_reconstruct(None, C.byref(frame), C.c_void_p(16), 0, 0xFFFFFFFF, 0, C.byref(image)) == abi.SZG_ERR_INVALID_ARGUMENT
    assert b"plane_count" in L.szg_last_error()
    assert L.szg_jpeg_reconstruct_host(None, 0, 0, None, 0) == abi.SZG_ERR_INVALID_ARGUMENT
