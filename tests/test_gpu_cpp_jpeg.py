"""The C++ mirror of include/szg/jpeg.h (include/szg/assets.hpp) through its own interface, from a program built with hipcc by
tests/Makefile (jpeg/load_jpeg_gltf.cpp): AssetLibrary::loadGLTFFromPath(path, SZG_GLTF_JPEG_FOR_DEVICE) reconstructs the
JPEG maps of a glTF file on the GPU, ORM overrides as masks, with the mip chain behind; loadTextureFromPath decodes a JPEG
file only with setDecodeJPEG."""
import base64
import json
import subprocess

import numpy as np
import pytest

from syzygy_amd import lib
from tests import gltf_writer as gw
from tests import jpeg_fixtures as jf
from tests import mipmap_model as mm
from tests import native

pytestmark = pytest.mark.gpu


def test_asset_library_reconstructs_jpeg_maps_on_the_device(tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    lib()  # built and loadable
    exe = native.build("jpeg/load_jpeg_gltf")
    color, mr, file_name = "420_33x31_prog_q92", "422_17x9_base_q92", "h1v2_33x33_base_q85"
    b = gw.GltfBuilder()
    png = np.random.default_rng(2).integers(0, 256, (5, 6, 4), dtype=np.uint8)
    images = [b.image_uri("data:image/jpeg;base64," + base64.b64encode(jf.data(n)).decode(), name=n) for n in (color, mr)]
    images.append(b.image_uri(gw.data_uri_png(gw.png_rgba8(png)), name="png"))
    t = [b.texture(i) for i in images]
    b.doc["materials"] = [{"name": "m", "pbrMetallicRoughness": {"baseColorTexture": {"index": t[0]}, "metallicRoughnessTexture": {"index": t[1]}},
                           "normalTexture": {"index": t[2]}}]
    gltf = tmp_path / "maps.gltf"
    gltf.write_bytes(json.dumps(b.document()).encode().replace(b'"buffers": [{"byteLength": 0}]', b'"buffers": []'))
    jpg = tmp_path / "file.jpg"
    jpg.write_bytes(jf.data(file_name))
    p = subprocess.run([exe, str(gltf), str(tmp_path / "out"), str(jpg)], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "OK 4", p.stdout
    orm = jf.expected(mr).copy()
    orm[..., 0] = 255
    # the loader brings ORM, colour, normal in this order; then the file
    want = [("texture_" + mr, orm, 0), ("texture_" + color, jf.expected(color), 1), ("texture_png", png, 0),
            ("texture_file", jf.expected(file_name), 1)]
    for k, (name, rgba, srgb) in enumerate(want):
        h, w = rgba.shape[:2]
        assert lines[k] == f"TEX {k} {name} {w} {h} {srgb} {mm.level_count(w, h)}", lines[k]
        got = np.fromfile(f"{tmp_path}/out.{k}.rgba", np.uint8).reshape(h, w, 4)
        assert np.array_equal(got, rgba), name
        chain = np.fromfile(f"{tmp_path}/out.{k}.chain", np.uint8)
        assert np.array_equal(chain, mm.pack_chain(mm.build_chain(rgba, bool(srgb)))), name
