"""The C++ mirror of include/szg/mipmaps.h (include/szg/assets.hpp, pipelines.hpp) through its own interface, from a program
built with hipcc (tests/cpp/asset_library_mips.cpp): an AssetLibrary with the generateMips switch on owns chains for what it
loads, textureMips() lists them, DeferredShadingPipeline::setTextureMips takes them, and the chain of a loaded PNG equals the
model's."""
import subprocess

import numpy as np
import pytest

from syzygy_amd import lib
from tests import gltf_writer
from tests import mipmap_model as mm
from tests import native

pytestmark = pytest.mark.gpu


def test_asset_library_builds_lists_and_registers_chains(tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    lib()  # built and loadable
    exe = native.build("cpp/asset_library_mips")
    w, h = 37, 19
    rgba = np.random.default_rng(9).integers(0, 256, (h, w, 4), dtype=np.uint8)
    png = tmp_path / "noise.png"
    png.write_bytes(gltf_writer.png_rgba8(rgba))
    p = subprocess.run([exe, str(png), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == f"OK {w} {h} {mm.level_count(w, h)}"
    level0 = np.fromfile(tmp_path / "out.level0", np.uint8).reshape(h, w, 4)
    assert np.array_equal(level0, rgba)
    chain = np.fromfile(tmp_path / "out.chain", np.uint8)
    assert np.array_equal(chain, mm.pack_chain(mm.build_chain(rgba, True)))
