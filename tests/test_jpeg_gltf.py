"""The glTF loader's two JPEG flags (include/szg/jpeg.h): off by default, host decode with SZG_GLTF_DECODE_JPEG, entropy decode
only with SZG_GLTF_JPEG_FOR_DEVICE. CPU only."""
import base64
import ctypes as C
import json

import numpy as np

from syzygy_amd import abi, assets, lib
from tests import gltf_writer as gw
from tests import jpeg_fixtures as jf

COLOR, MR, OCC = "444_17x9_base_q92", "420_9x17_prog_q92", "grey_8x8_rst_q92"


def _uri(data):
    return "data:image/jpeg;base64," + base64.b64encode(data).decode()


def _asset(tmp_path, embed=False):
    b = gw.GltfBuilder()
    png = np.arange(4 * 4 * 4, dtype=np.uint8).reshape(4, 4, 4)
    if embed:
        images = [b.image_view(jf.data(n), name=n) for n in (COLOR, MR, OCC)]
    else:
        images = [b.image_uri(_uri(jf.data(n)), name=n) for n in (COLOR, MR, OCC)]
    images.append(b.image_uri(gw.data_uri_png(gw.png_rgba8(png)), name="png"))
    images.append(b.image_uri(_uri(jf.data(COLOR)[:300]), name="cut"))
    t = [b.texture(i) for i in images]
    b.doc["materials"] = [
        {"name": "full", "pbrMetallicRoughness": {"baseColorTexture": {"index": t[0]}, "metallicRoughnessTexture": {"index": t[1]}},
         "normalTexture": {"index": t[3]}},
        {"name": "occlusion_only", "occlusionTexture": {"index": t[2]}},
        {"name": "cut", "pbrMetallicRoughness": {"baseColorTexture": {"index": t[4]}}},
    ]
    if embed:
        return b.glb(), png
    path = tmp_path / "jpeg.gltf"
    path.write_bytes(json.dumps(b.document()).encode().replace(b'"buffers": [{"byteLength": 0}]', b'"buffers": []'))
    return str(path), png


def test_default_flags_keep_the_default_map_and_the_summary(tmp_path):
    path, png = _asset(tmp_path)
    a = assets.load_gltf(path)
    full, occ, cut = a.materials
    assert full["color"] is None and full["orm"] is None and occ["orm"] is None and cut["color"] is None
    assert (full["normal"][0] == png).all()
    text = "\n".join(a.warnings)
    assert text.count("JPEG streams are not decoded by this build (PNG only)") == 4
    assert "Summary: 4 image(s) of this asset are JPEG streams, which this build does not decode (PNG only); " \
           "the materials that reference them use the default maps." in text
    for kind in ("color", "ORM"):
        assert f"Material full: Failed to upload {kind} texture." in text
    # the resolved material is the library default
    assert (a.material(0)["color"][0] == assets.default_material_map(abi.SZG_MAP_COLOR)).all()


def test_host_flag_decodes_like_a_png_with_the_orm_overrides(tmp_path):
    path, png = _asset(tmp_path)
    a = assets.load_gltf(path, flags=abi.SZG_GLTF_DECODE_JPEG)
    full, occ, cut = a.materials
    assert (full["color"][0] == jf.expected(COLOR)).all() and full["color"][1] is True
    want = jf.expected(MR).copy()
    want[..., 0] = 255
    assert (full["orm"][0] == want).all() and full["orm"][1] is False
    want = jf.expected(OCC).copy()
    want[..., 1:3] = 0
    assert (occ["orm"][0] == want).all()
    assert (full["normal"][0] == png).all()
    assert full["texture_names"]["color"] == "texture_" + COLOR
    # a stream that fails warns and keeps the default map, like any undecodable image; no summary line for decoded images
    assert cut["color"] is None
    text = "\n".join(a.warnings)
    assert "stbi: Failed to convert image. (color map of material 'cut': szg_jpeg_open: truncated" in text
    assert "Material cut: Failed to upload color texture." in text
    assert "Summary:" not in text and "PNG only" not in text


def _device_maps(handle):
    out = {}
    for i in range(lib().szg_gltf_material_count(handle)):
        m = abi.AssetMaterial()
        assert lib().szg_gltf_material(handle, i, C.byref(m)) == abi.SZG_OK
        for key, kind in (("color", abi.SZG_MAP_COLOR), ("normal", abi.SZG_MAP_NORMAL), ("orm", abi.SZG_MAP_ORM)):
            j = abi.JpegMap()
            assert lib().szg_gltf_material_jpeg(handle, i, kind, C.byref(j)) == abi.SZG_OK
            out[i, key] = (getattr(m, key), j)
    return out


def _check_device_flag(handle, png):
    maps = _device_maps(handle)
    for (material, key), name, masks, srgb in (((0, "color"), COLOR, (0xFFFFFFFF, 0), 1), ((0, "orm"), MR, (0xFFFFFF00, 0xFF), 0),
                                               ((1, "orm"), OCC, (0xFF0000FF, 0), 0)):
        tex, j = maps[material, key]
        want = jf.expected(name)
        assert not tex.rgba and (tex.width, tex.height, tex.srgb) == (want.shape[1], want.shape[0], srgb)
        assert j.jpeg and (j.rgba_and, j.rgba_or, j.srgb) == (*masks, srgb) and j.name == b"texture_" + name.encode()
        assert tex.name == j.name
        # the handle is a live szg_jpeg: reconstructing it with the masks gives the host flag's texels
        frame = abi.JpegFrame()
        assert lib().szg_jpeg_get_frame(j.jpeg, C.byref(frame)) == abi.SZG_OK
        got = np.zeros(want.shape, np.uint8)
        assert lib().szg_jpeg_reconstruct_host(C.byref(frame), j.rgba_and, j.rgba_or, got.ctypes.data_as(C.c_void_p), want.shape[1] * 4) == 0
        override = want.copy()
        if key == "orm":
            if material == 0:
                override[..., 0] = 255
            else:
                override[..., 1:3] = 0
        assert (got == override).all()
    # a PNG map is decoded as always and is no JPEG; so are a missing map and a failed one
    tex, j = maps[0, "normal"]
    assert tex.rgba and not j.jpeg and (j.rgba_and, j.rgba_or) == (0xFFFFFFFF, 0)
    assert (np.ctypeslib.as_array(tex.rgba, shape=(4, 4, 4)) == png).all()
    for key in ((1, "color"), (2, "color"), (2, "orm")):
        assert not maps[key][0].rgba and not maps[key][1].jpeg
    assert "szg_jpeg_open: truncated" in lib().szg_gltf_warnings(handle).decode()
    j = abi.JpegMap()
    assert lib().szg_gltf_material_jpeg(handle, 3, abi.SZG_MAP_COLOR, C.byref(j)) == abi.SZG_ERR_INVALID_ARGUMENT
    assert lib().szg_gltf_material_jpeg(handle, 0, 3, C.byref(j)) == abi.SZG_ERR_INVALID_ARGUMENT
    assert lib().szg_gltf_material_jpeg(handle, 0, 0, None) == abi.SZG_ERR_INVALID_ARGUMENT
    assert lib().szg_gltf_material_jpeg(None, 0, 0, C.byref(j)) == abi.SZG_ERR_INVALID_ARGUMENT


def test_device_flag_keeps_the_entropy_decode_only(tmp_path):
    path, png = _asset(tmp_path)
    for flags in (abi.SZG_GLTF_JPEG_FOR_DEVICE, abi.SZG_GLTF_JPEG_FOR_DEVICE | abi.SZG_GLTF_DECODE_JPEG):  # 4 implies 2
        handle = C.c_void_p()
        assert lib().szg_gltf_load_file(path.encode(), flags, C.byref(handle)) == abi.SZG_OK
        try:
            _check_device_flag(handle, png)
        finally:
            lib().szg_gltf_destroy(handle)


def test_buffer_view_images_combine_with_both_flags(tmp_path):
    glb, png = _asset(tmp_path, embed=True)
    # without the buffer-view flag the embedded images are not looked at, whatever the JPEG flags say
    a = assets.load_gltf_bytes(glb, is_glb=True, flags=abi.SZG_GLTF_DECODE_JPEG)
    assert a.materials[0]["color"] is None and any("Unsupported glTF image source found." in w for w in a.warnings)
    a = assets.load_gltf_bytes(glb, is_glb=True, flags=abi.SZG_GLTF_DECODE_BUFFER_VIEW_IMAGES)
    assert a.materials[0]["color"] is None and any("Summary: 4 image(s)" in w for w in a.warnings)
    a = assets.load_gltf_bytes(glb, is_glb=True, flags=abi.SZG_GLTF_DECODE_BUFFER_VIEW_IMAGES | abi.SZG_GLTF_DECODE_JPEG)
    assert (a.materials[0]["color"][0] == jf.expected(COLOR)).all()
    want = jf.expected(OCC).copy()
    want[..., 1:3] = 0
    assert (a.materials[1]["orm"][0] == want).all()
    buf = (C.c_uint8 * len(glb)).from_buffer_copy(glb)
    handle = C.c_void_p()
    flags = abi.SZG_GLTF_DECODE_BUFFER_VIEW_IMAGES | abi.SZG_GLTF_JPEG_FOR_DEVICE
    assert lib().szg_gltf_load_memory(C.cast(buf, C.c_void_p), len(glb), 1, None, flags, C.byref(handle)) == abi.SZG_OK
    try:
        _check_device_flag(handle, png)
    finally:
        lib().szg_gltf_destroy(handle)
