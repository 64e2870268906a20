#!/usr/bin/env python3
"""Writes tests/golden/debugline_vectors.npz: gl_Position of the reference's COMMITTED debugline.vert.spv, executed
literally by tests/golden/spirv_interp.py (every OpFMul / OpFAdd one binary32 operation, matrix products summed left to
right), on 64 seeded vertices and two cameras, each read as camera 1 of a two-camera buffer. tests/test_debuglines_model.py
requires the CPU model of the debug-line pass (tests/debuglines_model.py) to reproduce them BIT FOR BIT, which pins the
vertex stage of include/szg/debuglines.h to the binary.

    python tests/golden/make_debugline_vectors.py            (needs /root/reference; a few seconds)

The vertices include points behind the camera, points on the near plane and very large coordinates.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden.make_spirv_vectors import REFERENCE, Builtins, _bits, pack_block  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "debugline_vectors.npz")
SHADER = "shaders/debug/debugline.vert.spv"
F32 = np.float32


def available():
    return os.path.exists(os.path.join(REFERENCE, SHADER))


def cameras():
    """The editor's default camera and the frame-loop camera (examples/frame_loop.py), at 16:9."""
    from syzygy_amd import scene

    a = scene.default_camera()
    b = scene.default_camera()
    b.cameraPosition[:] = [-22.0, -18.0, -42.0]
    b.eulerAngles[:] = [float(v) for v in scene.eulers_from_forward((22.0, 11.0, 42.0))]
    return [(c, scene.camera_packed(c, 16.0 / 9.0)) for c in (a, b)]


def vertices(rng, camera):
    """64 positions: 40 in the scene's range, 8 behind the camera, 8 on its near plane, 8 very large."""
    from syzygy_amd import scene

    pos = np.array(camera.cameraPosition, np.float64)
    fwd = np.array(scene.forward_from_eulers(list(camera.eulerAngles)), np.float64)
    out = [rng.uniform(-30, 30, 3) for _ in range(40)]
    out += [pos - fwd * rng.uniform(0.5, 20) + rng.uniform(-3, 3, 3) for _ in range(8)]
    side = np.cross(fwd, [0.0, 1.0, 0.0])
    out += [pos + fwd * camera.near_plane + side * rng.uniform(-0.05, 0.05) for _ in range(8)]
    out += [rng.choice([-1.0, 1.0], 3) * 10.0 ** rng.uniform(6, 30, 3) for _ in range(8)]
    return np.array(out, np.float32)


def generate(log=print):
    from syzygy_amd import abi
    from tests.golden import spirv_interp as si

    m = si.Module(os.path.join(REFERENCE, SHADER))
    (gid,) = [g for g, (pt, sc) in m.globals.items() if sc == si.SC_PUSH_CONSTANT]
    block = m.types[m.globals[gid][0]].pointee
    rng = np.random.default_rng(0xD1A6)
    builtins = Builtins()
    out = {}
    cams = cameras()
    for k, (camera, cam) in enumerate(cams):
        other = cams[1 - k][1]
        pos = vertices(rng, camera)
        verts = (abi.VertexPacked * len(pos))()
        for v, p in zip(verts, pos):
            v.position[:] = [float(x) for x in p]
            v.uv_x, v.uv_y = float(F32(rng.uniform(0, 1))), float(F32(rng.uniform(0, 1)))
            v.color[:] = [1.0, 0.0, 0.0, 1.0]
        mem = si.Memory()
        a_vert = mem.alloc(bytes(verts))
        a_cam = mem.alloc(bytes(other) + bytes(cam))  # camera 1 of its buffer
        it = si.Interpreter(m, mem, builtins, pack_block(m, block, dict(vertexBuffer=a_vert, cameraBuffer=a_cam, cameraIndex=1)), {})
        clip = []
        for i in range(len(pos)):
            it.run(inputs={si.BUILTIN_VERTEX_INDEX: i, si.BUILTIN_INSTANCE_INDEX: 0})
            clip.append(list(it.outputs["gl_PerVertex"][0][0]))
        out[f"camera_{k}"] = np.frombuffer(bytes(cam), np.uint8)
        out[f"vertices_{k}"] = np.frombuffer(bytes(verts), np.uint8)
        out[f"gl_position_{k}"] = _bits(clip)
        log(f"camera {k}: {len(pos)} vertices")
    return out


if __name__ == "__main__":
    if not available():
        sys.exit(f"{os.path.join(REFERENCE, SHADER)} not found")
    vec = generate()
    np.savez_compressed(OUT, **vec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
