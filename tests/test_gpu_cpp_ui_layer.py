"""The C++ mirror of the UI layer pass (include/szg/ui_layer.hpp: szg::UILayer) through its own interface, from a program built
with hipcc (tests/cpp/ui_layer_shim.cpp) whose draw data has Dear ImGui's shape: two lists concatenated with global offsets,
a command with a user callback skipped, the scene viewport quad at the editor's UVs - against the CPU model, bit for bit."""
import subprocess

import numpy as np
import pytest

from syzygy_amd import lib
from tests import native
from tests import ui_layer_cases as uc
from tests import ui_layer_model as um

pytestmark = pytest.mark.gpu


def test_uilayer_record_draw_from_cpp(tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    lib()  # built and loadable
    exe = native.build("cpp/ui_layer_shim")
    cap, content, display = (64, 48), (37, 29), (53, 41)
    scene = np.random.default_rng(4).integers(0, 65536, (cap[1], cap[0], 4), dtype=np.uint16)
    scene[..., 3] |= 0xC000  # mostly opaque, so that the scene shows
    scene.tofile(tmp_path / "scene.bin")
    p = subprocess.run([exe, str(tmp_path / "scene.bin"), *map(str, cap + content + display), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout + p.stderr)
    assert p.stdout.strip().splitlines()[-1] == f"OK {cap[0]} {cap[1]}"
    assert "szg_ui_layer_record_draw failed" in p.stderr  # the draw after removeTexture, refused and logged
    got = np.fromfile(tmp_path / "out.bin", np.uint16).reshape(cap[1], cap[0], 4)

    everything = (0.0, 0.0, float(display[0]), float(display[1]))
    bg, tint = 0xFF221E1E, 0xA03C78F0
    uvx, uvy = np.float32(content[0]) / np.float32(cap[0]), np.float32(content[1]) / np.float32(cap[1])
    vertices = [(0, 0, .5, .5, bg), (display[0], 0, .5, .5, bg), (display[0], display[1], .5, .5, bg), (0, display[1], .5, .5, bg),
                (6, 5, 0, 0, uc.OPAQUE), (6 + content[0], 5, uvx, 0, uc.OPAQUE), (6 + content[0], 5 + content[1], uvx, uvy, uc.OPAQUE),
                (6, 5 + content[1], 0, uvy, uc.OPAQUE),
                (10.5, 8.25, .5, .5, tint), (40, 8.25, .5, .5, tint), (40, 30, .5, .5, tint), (10.5, 30, .5, .5, tint)]
    indices = [0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7, 0, 1, 2, 0, 2, 3]
    commands = [(everything, "font", 0, 0, 6), (everything, "scene", 0, 6, 6), ((12.7, 9.2, 33.9, 25.5), "font", 8, 12, 6)]
    draw = uc.flat(vertices, indices, commands, display)
    textures = {"font": um.Texture(np.full((1, 1, 4), 255, np.uint8), um.LINEAR, um.REPEAT),
                "scene": um.Texture(scene, um.NEAREST, um.CLAMP_TO_BORDER)}
    # the output texture is allocated at the capacity and starts zeroed; the render area is the display
    want = um.render(np.zeros((cap[1], cap[0], 4), np.uint16), (0, 0, display[0], display[1]), um.CLEAR, (0, 0, 0, 1), draw, textures)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:5]
    assert (got[display[1]:] == 0).all() and (got[:, display[0]:] == 0).all()
