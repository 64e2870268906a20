"""Device time of the debug-line pass (include/szg/debuglines.h) at 3840x2160: device events around N records after a
warm-up, ms per record. Cases: the frame loop's 5 boxes (120 lines, the reference's typical load), 500 lines (the
reference's DEBUGLINES_CAPACITY of 1000 vertices), 500 lines whose endpoints lie 10^6 px off-screen (cost follows the
covered pixels, not the unclipped length), 10^5 random lines at width 1 and at width 8.

    python tools/bench_debug_lines.py [--reps 50] [--json out.json]

Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_debug_lines.py`."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from syzygy_amd import abi, lib, meshes, pipelines as pl, scene  # noqa: E402

W, H = 3840, 2160


def frame_loop_camera():
    c = scene.default_camera()
    c.cameraPosition[:] = [-22.0, -18.0, -42.0]
    c.eulerAngles[:] = [float(v) for v in scene.eulers_from_forward((22.0, 11.0, 42.0))]
    return scene.camera_packed(c, W / H)


def identity_camera():
    cam = abi.CameraPacked()
    eye = np.eye(4, dtype=np.float32)
    for name in ("projection", "inverseProjection", "view", "viewInverseTranspose", "rotation", "projViewInverse"):
        setattr(cam, name, abi.Mat4.from_numpy(eye))
    return cam


def editor_boxes():
    """examples/frame_loop.py's instances (two cubes, a small cube, the floor) + the shadow-bounds box: 5 boxes."""
    cv, _ = meshes.cube_mesh()
    pv, _ = meshes.plane_mesh()
    out, casters, keep = [], [], []
    for verts, tr, sc in ((cv, (0, -8, 6), (5, 5, 5)), (cv, (0, -8, -6), (5, 5, 5)), (cv, (14, -6, -2), (2, 2, 2)), (pv, (0, -1, 0), (20, 1, 20))):
        bounds = abi.AABB()
        lib().szg_aabb_create(abi.f3(*verts["position"].min(0)), abi.f3(*verts["position"].max(0)), C.byref(bounds))
        t = (abi.Transform * 1)()
        t[0].translation[:], t[0].eulerAnglesRadians[:], t[0].scale[:] = list(tr), [0.0, 0.0, 0.0], list(sc)
        box = (abi.VertexPacked * 48)()
        lib().szg_debug_lines_box_transform(t, C.byref(bounds), box)
        out.append(bytes(box))
        keep.append(t)
        casters.append(abi.ShadowCaster(bounds, t, 1, 1, 1, 0))
    sb = abi.AABB()
    lib().szg_calculate_shadow_bounds((abi.ShadowCaster * len(casters))(*casters), len(casters), C.byref(sb))
    box = (abi.VertexPacked * 48)()
    lib().szg_debug_lines_box(sb.center, abi.f4(0, 0, 0, 1), sb.half_extent, box)
    out.append(bytes(box))
    return np.frombuffer(b"".join(out), np.float32).reshape(-1, 12)


def vertices(positions):
    v = np.zeros((len(positions), 12), np.float32)
    v[:, 0:3] = positions
    return v


def screen_lines(rng, n, length_mean):
    a = rng.uniform(0, 1, (n, 2)) * [W, H]
    d = rng.normal(size=(n, 2))
    d *= (rng.exponential(length_mean, n) / np.maximum(np.linalg.norm(d, axis=1), 1e-9))[:, None]
    p = np.concatenate([a, a + d], axis=1).reshape(-1, 2)
    return vertices(np.stack([p[:, 0] / (W / 2) - 1, p[:, 1] / (H / 2) - 1, np.full(len(p), 0.5)], axis=1))


def far_lines(rng, n):
    """Endpoints 10^6 px off-screen on both sides, crossing the frame."""
    y0, y1 = rng.uniform(0, H, n), rng.uniform(0, H, n)
    p = np.stack([np.full(n, -1e6), y0, np.full(n, 1e6), y1], axis=1).reshape(-1, 2)
    return vertices(np.stack([p[:, 0] / (W / 2) - 1, p[:, 1] / (H / 2) - 1, np.full(len(p), 0.5)], axis=1))


def world_lines(rng, n):
    p = rng.uniform(-30, 30, (2 * n, 3))
    p[:, 1] = rng.uniform(-20, 0, 2 * n)
    return vertices(p)


def run(name, cam, verts, width, reps):
    cams = torch.from_numpy(np.frombuffer(bytes(cam), np.uint8).copy()).cuda()
    d_v = torch.from_numpy(np.ascontiguousarray(verts).copy()).cuda()
    target = pl.SceneTexture(W, H)
    st = target.abi()
    h = C.c_void_p()
    assert lib().szg_debug_lines_create(C.byref(h), len(verts), 0) == abi.SZG_OK
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def record():
        rc = lib().szg_debug_lines_record(h, stream, C.c_float(width), pl.rect(W, H), None, C.byref(st), 0, C.c_void_p(cams.data_ptr()),
                                          C.c_void_p(d_v.data_ptr()), len(verts))
        assert rc == abi.SZG_OK, lib().szg_last_error()

    for _ in range(3):
        record()
    torch.cuda.synchronize()
    covered = int((target.color[..., 1] != 0).sum())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        record()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    lib().szg_debug_lines_destroy(h)
    r = {"case": name, "lines": len(verts) // 2, "width": width, "covered_pixels": covered, "ms_per_record": round(ms, 5),
         "ns_per_covered_pixel": round(ms * 1e6 / max(covered, 1), 4)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    entry.build(only_if_missing=True)
    rng = np.random.default_rng(2026)
    results = [
        run("editor boxes (frame-loop camera)", frame_loop_camera(), editor_boxes(), 1.0, args.reps),
        run("500 world lines (DEBUGLINES_CAPACITY)", frame_loop_camera(), world_lines(rng, 500), 1.0, args.reps),
        run("500 lines, endpoints 1e6 px off-screen", identity_camera(), far_lines(rng, 500), 1.0, args.reps),
        run("1e5 random lines", identity_camera(), screen_lines(rng, 100_000, 20.0), 1.0, args.reps),
        run("1e5 random lines, width 8", identity_camera(), screen_lines(rng, 100_000, 20.0), 8.0, args.reps),
    ]
    out = {"extent": [W, H], "reps": args.reps, "build_id": entry.build_id(), "source_hash": entry.source_hash("hip"),
           "device": torch.cuda.get_device_name(0), "results": results}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
