"""CPU: the box bound of the lights pass's tile cull never clears a bit the per-pixel early-out would not.

tests/lights_tiles/light_tile_bounds.cpp (plain C++ over syzygy_amd/csrc/szg_light_tiles.hpp, the header k_light_tiles and
k_lights compile) takes the bench scene's ring of 64 spot lights and three sets of the same ring with perturbed poses, and for
every (box, light) whose bit tileMaySkipLight would clear evaluates pairCull - the light loop's own early-out - at the
box's corners, at its point nearest to the light and at 3000 positions inside. Random boxes of every shape, single-point
boxes, boxes around and beside the lights, boxes straddling cw = 0, non-finite boxes, records without flag bit 0. It must
find no position where the early-out fails, and the bound must not be vacuous."""
import os
import re
import subprocess

import numpy as np

from syzygy_amd import scene
from tests import light_tile_model as lt
from tests import native


def test_light_tiles_header_is_exported_and_bound():
    """include/szg/light_tiles.h: every symbol it declares is exported and bound, and the other way round; the tile and batch
    sizes of the Python mirror are the header's."""
    import ctypes as C

    from syzygy_amd import abi, library_path

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "szg", "light_tiles.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(szg_[a-z0-9_]+)\s*\(", text)))
    handle = C.CDLL(library_path())
    assert names == sorted(abi.LIGHT_TILE_FUNCTIONS) and all(hasattr(handle, n) for n in names)
    device = open(os.path.join(root, "syzygy_amd", "csrc", "szg_light_tiles.hpp")).read()
    assert f"LIGHT_TILE_DIM = {abi.LIGHT_TILE_DIM}u" in device and f"LIGHT_TILE_BATCH = {abi.LIGHT_TILE_BATCH}u" in device


def test_a_cleared_bit_means_the_early_out_fires_everywhere_in_the_box(tmp_path):
    exe = native.build("lights_tiles/light_tile_bounds")
    sets = [lt.spot_records(scene.spot_ring(64), 64)] + [lt.spot_records(lt.perturbed_ring(64, seed), 64) for seed in (1, 2, 3)]
    np.concatenate(sets).tofile(tmp_path / "lights.bin")
    done = subprocess.run([exe, str(tmp_path / "lights.bin")], capture_output=True, text=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0, done.stdout + done.stderr
    assert re.search(r"^violations 0$", done.stdout, re.M)
    ground = re.search(r"ground patch away from the ring's targets: (\d+) of 64 bits cleared", done.stdout)
    assert ground and int(ground.group(1)) >= 1
