"""GPU: szg::Renderer::recordDraw with the debug-line pass (include/szg/scene.hpp), through a C++ caller compiled here with
hipcc (tests/cpp/record_draw_debuglines.cpp). With the switch on, the frame is the switch-off frame with the model's
lines drawn over it, the list being the one the Python builders make from the same boxes; with it off (before and after),
the frame is byte-identical and nothing is drawn."""
import subprocess

import numpy as np
import pytest

from syzygy_amd import abi, lib
from tests import debuglines_model as dm
from tests import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    lib()  # built and loadable
    return native.build("cpp/record_draw_debuglines")


def python_list(boxes_raw):
    """The list the Python mirror (pipelines.DebugLines' builders) makes from the same instance transforms, vertex bounds
    and shadow bounds."""
    import ctypes as C

    f = np.frombuffer(boxes_raw, np.float32)
    n = (len(f) - 6) // 15
    out = []
    for k in range(n):
        t = abi.Transform.from_buffer_copy(f[15 * k: 15 * k + 9].tobytes())
        bb = abi.AABB.from_buffer_copy(f[15 * k + 9: 15 * k + 15].tobytes())
        box = (abi.VertexPacked * 48)()
        lib().szg_debug_lines_box_transform(C.byref(t), C.byref(bb), box)
        out.append(bytes(box))
    sb = abi.AABB.from_buffer_copy(f[-6:].tobytes())
    box = (abi.VertexPacked * 48)()
    lib().szg_debug_lines_box(sb.center, abi.f4(0, 0, 0, 1), sb.half_extent, box)
    out.append(bytes(box))
    return b"".join(out), n


@pytest.mark.parametrize("extent,width", [((320, 180), 1.0), ((640, 360), 3.0)])
def test_renderer_record_draw_with_and_without_debug_lines(exe, tmp_path, extent, width):
    W, H = extent
    prefix = str(tmp_path / "frame")
    r = subprocess.run([exe, prefix, str(W), str(H), str(width)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    read = lambda s: np.fromfile(prefix + s, dtype=np.uint16).reshape(H, W, 4)  # noqa: E731
    off, on, off2 = read(".off.bin"), read(".on.bin"), read(".off2.bin")
    lines = open(prefix + ".lines.bin", "rb").read()
    want_list, instances = python_list(open(prefix + ".boxes.bin", "rb").read())
    assert instances == 2  # Scene::defaultScene: the floor and the floating cube (scene.cpp:100-147)
    assert lines == want_list, "the renderer's list differs from the Python builders'"
    nv = len(lines) // 48
    assert f"frame 0 enabled 0 staged {nv} draw 0 0 0" in r.stdout
    assert f"frame 1 enabled 1 staged {nv} draw 1 {nv} {nv}" in r.stdout
    assert f"frame 2 enabled 0 staged {nv} draw 0 0 0" in r.stdout
    assert np.array_equal(off, off2), "the switch-off frame changed"
    cam = abi.CameraPacked.from_buffer_copy(open(prefix + ".camera.bin", "rb").read())
    mask = dm.model(cam, dm.positions_of(np.frombuffer(lines, np.uint8)), W, H, width)
    assert mask.sum() > 200
    want, _ = dm.render(mask, off)
    bad = np.argwhere((on != want).any(axis=-1))
    assert len(bad) == 0, f"{len(bad)} texels differ, first {bad[:5].tolist()}"
    assert not np.array_equal(on, off)
