"""GPU: the debug-line pass (include/szg/debuglines.h, kernels_debuglines.hip) against the CPU model
(tests/debuglines_model.py), bit for bit on the colour plane and on debug_color; every byte the pass must not touch is
checked against a sentinel pattern (the whole colour / debug / depth buffers, beyond the draw rect included)."""
import ctypes as C

import numpy as np
import pytest

from syzygy_amd import abi, lib
from tests import debuglines_model as dm
from tests import util

pytestmark = pytest.mark.gpu
F32 = np.float32
WIDTHS = [0.0, 1.0, 1.5, 3.0, 8.0, 100.0]


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    from syzygy_amd import pipelines

    class Ctx:
        pass

    c = Ctx()
    c.pl, c.torch = pipelines, torch
    return c


def identity_camera():
    cam = abi.CameraPacked()
    eye = np.eye(4, dtype=np.float32)
    for name in ("projection", "inverseProjection", "view", "viewInverseTranspose", "rotation", "projViewInverse"):
        setattr(cam, name, abi.Mat4.from_numpy(eye))
    return cam


def screen(points, W, H, z=0.5):
    """Pixel coordinates -> positions that the identity camera maps exactly onto them (W, H powers of two)."""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    out = np.empty((len(p), 3), np.float32)
    out[:, 0] = p[:, 0] / (W / 2) - 1
    out[:, 1] = p[:, 1] / (H / 2) - 1
    out[:, 2] = z
    return out


def frame_loop_camera():
    from syzygy_amd import scene

    c = scene.default_camera()
    c.cameraPosition[:] = [-22.0, -18.0, -42.0]
    c.eulerAngles[:] = [float(v) for v in scene.eulers_from_forward((22.0, 11.0, 42.0))]
    return c


def scene_box_positions():
    """Renderer::recordDraw's list for meshes.reference_default_scene(): one box per instance transform from
    Mesh::vertexBounds (renderer.cpp:355-365), then the shadow-bounds box (:417-423)."""
    from syzygy_amd import meshes

    cv, _ = meshes.cube_mesh()
    pv, _ = meshes.plane_mesh()
    out = []
    casters = []
    keep = []
    for verts, (tr, sc) in ((cv, ((0, -8, 6), (5, 5, 5))), (cv, ((0, -8, -6), (5, 5, 5))), (pv, ((0, -1, 0), (20, 1, 20)))):
        bounds = abi.AABB()
        lib().szg_aabb_create(abi.f3(*verts["position"].min(0)), abi.f3(*verts["position"].max(0)), C.byref(bounds))
        t = (abi.Transform * 1)()
        t[0].translation[:], t[0].eulerAnglesRadians[:], t[0].scale[:] = list(tr), [0.0, 0.0, 0.0], list(sc)
        box = (abi.VertexPacked * 48)()
        lib().szg_debug_lines_box_transform(t, C.byref(bounds), box)
        out.append(dm.positions_of(box))
        keep.append(t)
        casters.append(abi.ShadowCaster(bounds, t, 1, 1, 1, 0))
    sb = abi.AABB()
    lib().szg_calculate_shadow_bounds((abi.ShadowCaster * 3)(*casters), 3, C.byref(sb))
    box = (abi.VertexPacked * 48)()
    lib().szg_debug_lines_box(sb.center, abi.f4(0, 0, 0, 1), sb.half_extent, box)
    out.append(dm.positions_of(box))
    return np.concatenate(out)


class Target:
    """Colour / depth / debug planes of (W + pad_x) x (rows + pad_y) texels filled with a sentinel pattern."""

    def __init__(self, gpu, W, rows, debug=True, pad=(7, 5), seed=1):
        rng = np.random.default_rng(seed)
        self.iw, self.ih = W + pad[0], rows + pad[1]
        self.color0 = rng.integers(0, 65536, (self.ih, self.iw, 4), dtype=np.uint16)
        self.depth0 = rng.integers(0, 2 ** 32, (self.ih, self.iw), dtype=np.uint32)
        self.debug0 = rng.uniform(-2, 2, (self.ih, self.iw, 4)).astype(np.float32) if debug else None
        t = gpu.torch
        self.color = t.from_numpy(self.color0.view(np.int16).copy()).cuda()
        self.depth = t.from_numpy(self.depth0.view(np.int32).copy()).cuda()
        self.debug = t.from_numpy(self.debug0.copy()).cuda() if debug else None

    def abi(self):
        st = abi.SceneTexture()
        st.color = abi.Image(self.color.data_ptr(), self.iw, self.ih, self.iw * 8, abi.SZG_FORMAT_RGBA16_UNORM)
        st.depth = abi.Image(self.depth.data_ptr(), self.iw, self.ih, self.iw * 4, abi.SZG_FORMAT_D32_SFLOAT)
        if self.debug is not None:
            st.debug_color = abi.Image(self.debug.data_ptr(), self.iw, self.ih, self.iw * 16, abi.SZG_FORMAT_RGBA32_SFLOAT)
        return st

    def read(self, gpu):
        gpu.torch.cuda.synchronize()
        c = self.color.cpu().numpy().view(np.uint16)
        d = self.depth.cpu().numpy().view(np.uint32)
        g = self.debug.cpu().numpy() if self.debug is not None else None
        return c, d, g

    def expect(self, mask, rows=None):
        """The sentinel planes with the model's mask applied (rows: global rows of a tile's local rows)."""
        m = mask if rows is None else mask[rows]
        c, g = dm.render(m, self.color0, self.debug0)
        return c, self.depth0, g


class Pass:
    def __init__(self, gpu, capacity):
        self.gpu = gpu
        self.h = C.c_void_p()
        assert lib().szg_debug_lines_create(C.byref(self.h), capacity, 0) == abi.SZG_OK, lib().szg_last_error()

    def record(self, target, cam, positions, W, H, width, tile=None, count=None, rect=None, debug_override=None):
        t = self.gpu.torch
        cams = np.frombuffer(b"\xff" * C.sizeof(abi.CameraPacked) + bytes(cam), np.uint8)  # camera 1 of the buffer
        d_cam = t.from_numpy(cams.copy()).cuda()
        v = np.zeros((max(len(positions), 1), 12), np.float32)
        v[: len(positions), 0:3] = positions
        v[: len(positions), 8:12] = [1, 0, 0, 1]
        d_v = t.from_numpy(v).cuda()
        st = target.abi()
        if debug_override is not None:
            debug_override(st)
        n = len(positions) if count is None else count
        status = lib().szg_debug_lines_record(self.h, None, C.c_float(width), rect or abi.Rect(0, 0, W, H),
                                              C.byref(tile) if tile is not None else None, C.byref(st), 1,
                                              C.c_void_p(d_cam.data_ptr()), C.c_void_p(d_v.data_ptr()), n)
        t.cuda.synchronize()
        return status

    def close(self):
        lib().szg_debug_lines_destroy(self.h)


def check(gpu, cam, positions, W, H, width, brute=False, debug=True, seed=1):
    p = Pass(gpu, max(len(positions), 2))
    target = Target(gpu, W, H, debug=debug, seed=seed)
    assert p.record(target, cam, positions, W, H, width) == abi.SZG_OK, lib().szg_last_error()
    p.close()
    got = target.read(gpu)
    mask = dm.model(cam, positions, W, H, width, brute=brute)
    want = target.expect(mask)
    assert np.array_equal(got[1], want[1]), "depth touched"
    bad = np.argwhere((got[0] != want[0]).any(axis=-1))
    assert len(bad) == 0, f"{len(bad)} colour texels differ, first {bad[:5].tolist()}; model covers {mask.sum()}"
    if debug:
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "debug_color differs"
    return mask


@pytest.mark.parametrize("extent", [(1280, 720), (3840, 2160)])
@pytest.mark.parametrize("camera", ["default", "frame_loop"])
@pytest.mark.parametrize("width", WIDTHS)
def test_scene_boxes_bit_exact(gpu, extent, camera, width):
    from syzygy_amd import scene

    W, H = extent
    c = scene.default_camera() if camera == "default" else frame_loop_camera()
    cam = scene.camera_packed(c, W / H)
    mask = check(gpu, cam, scene_box_positions(), W, H, width, debug=(width != 3.0))
    if width >= 1.0:
        assert mask.sum() > 100


def special_lines(W, H):
    """Screen-space segments (pixel coordinates) for the identity camera."""
    return np.array([
        [10, 20, 100, 20], [10.5, 30.5, 100.5, 30.5], [40, 2, 40, 60], [44.5, 1.5, 44.5, 61.5],  # horizontal / vertical, on edges
        [3, 3, 3, 3], [70.5, 12.5, 70.5, 12.5],  # zero length
        [5, 5, 120, 59], [5.5, 58.5, 120.5, 3.5], [0, 0, 128, 64], [64, 0, 64, 64],  # diagonals, corner to corner
        [-1e6, 17.25, 1e6, 19.75], [33.5, -1e6, 35.5, 1e6], [-1e6, -1e6, 1e6, 1e6],  # endpoints 10^6 px off-screen
        [-3e6, 40, 50, 41], [12, 13, 13, 40], [100, 50, 101, 50.5], [20, 44, 20.5, 44],
    ], np.float64)


@pytest.mark.parametrize("width", WIDTHS)
def test_special_lines_bit_exact_and_never_dropped_by_the_candidate_interval(gpu, width):
    W, H = 128, 64
    seg = special_lines(W, H)
    pos = screen(seg.reshape(-1, 2), W, H)
    check(gpu, identity_camera(), pos, W, H, width, brute=True)


def test_near_plane_and_behind_the_camera(gpu):
    from syzygy_amd import scene

    W, H = 320, 180
    c = scene.default_camera()
    cam = scene.camera_packed(c, W / H)
    pos = np.array(c.cameraPosition, np.float32)
    fwd = np.array(scene.forward_from_eulers(list(c.eulerAngles)), np.float32)
    side = np.cross(fwd, [0, 1, 0]).astype(np.float32)
    rng = np.random.default_rng(5)
    pts = []
    for _ in range(40):  # crossing the near plane
        pts += [pos - fwd * rng.uniform(0.1, 10) + side * rng.uniform(-3, 3), pos + fwd * rng.uniform(1, 50) + side * rng.uniform(-20, 20)]
    for _ in range(20):  # entirely behind
        pts += [pos - fwd * rng.uniform(0.5, 10) + side * rng.uniform(-3, 3), pos - fwd * rng.uniform(0.5, 10) - side * rng.uniform(-3, 3)]
    for _ in range(10):  # on the near plane
        p = pos + fwd * c.near_plane
        pts += [p + side * rng.uniform(-0.1, 0.1), pos + fwd * rng.uniform(1, 30)]
    positions = np.array(pts, np.float32)
    for width in (1.0, 8.0):
        mask = check(gpu, cam, positions, W, H, width, brute=True)
        assert mask.any()
    # the behind-the-camera half alone draws nothing
    assert not dm.model(cam, positions[80:120], W, H, 8.0).any()


@pytest.mark.parametrize("width", [1.0, 8.0])
def test_random_sweep_of_100k_lines(gpu, width):
    W, H = 2048, 1024
    rng = np.random.default_rng(int(width))
    n = 100_000
    a = rng.uniform(-0.25, 1.25, (n, 2)) * [W, H]
    d = rng.normal(size=(n, 2))
    # mostly short, some long (up to across the frame and beyond)
    length = np.where(rng.uniform(size=n) < 0.99, rng.exponential(6, n), rng.uniform(100, 4000, n))
    d *= (length / np.maximum(np.linalg.norm(d, axis=1), 1e-9))[:, None]
    seg = np.concatenate([a, a + d], axis=1)
    pos = screen(seg.reshape(-1, 2), W, H, z=0.25)
    mask = check(gpu, identity_camera(), pos, W, H, width, debug=False, seed=7)
    assert 0.05 < mask.mean() < 0.98


def test_odd_vertex_count(gpu):
    W, H = 128, 64
    seg = special_lines(W, H)[:5]
    pos = screen(seg.reshape(-1, 2), W, H)
    extra = screen([[1, 1]], W, H)
    p = Pass(gpu, 16)
    target = Target(gpu, W, H)
    allpos = np.concatenate([pos, extra])
    assert p.record(target, identity_camera(), allpos, W, H, 2.0) == abi.SZG_OK
    p.close()
    got = target.read(gpu)
    want = target.expect(dm.model(identity_camera(), allpos, W, H, 2.0))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(want[0], target.expect(dm.model(identity_camera(), pos, W, H, 2.0))[0])


@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_row_tiles_compose_to_the_full_frame(gpu, nranks):
    from syzygy_amd import scene

    W, H, block = 1280, 720, 16
    cam = scene.camera_packed(frame_loop_camera(), W / H)
    positions = scene_box_positions()
    full = dm.model(cam, positions, W, H, 3.0)
    composed = np.zeros((H, W, 4), np.uint16)
    p = Pass(gpu, len(positions))
    for rank in range(nranks):
        tile = util.rowtile(H, block, rank, nranks)
        rows = util.global_rows(H, block, rank, nranks)
        target = Target(gpu, W, tile.local_rows, pad=(0, 0), seed=rank)
        target.color0[:] = 0
        target.color.zero_()
        assert p.record(target, cam, positions, W, H, 3.0, tile=tile) == abi.SZG_OK, lib().szg_last_error()
        got = target.read(gpu)
        want = target.expect(full, rows)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
        composed[rows] = got[0][: len(rows)]
    p.close()
    assert np.array_equal(composed, dm.render(full, np.zeros((H, W, 4), np.uint16))[0])


def test_refusals_leave_the_image_untouched(gpu):
    W, H = 64, 32
    pos = screen([[1, 1], [60, 30], [2, 30], [60, 2]], W, H)
    p = Pass(gpu, 4)
    cam = identity_camera()
    cases = [
        (dict(rect=abi.Rect(1, 0, W, H)), "offset"),
        (dict(width=float("nan")), "line_width"),
        (dict(width=float("inf")), "line_width"),
        (dict(width=-1.0), "line_width"),
        (dict(width=abi.SZG_DEBUG_LINES_MAX_WIDTH * 1.01), "line_width"),
        (dict(count=6), "capacity"),
        (dict(debug_override=lambda st: setattr(st.color, "data", None)), "color"),
    ]
    for kw, word in cases:
        target = Target(gpu, W, H)
        width = kw.pop("width", 1.0)
        status = p.record(target, cam, pos if "count" not in kw else np.concatenate([pos, pos[:2]]), W, H, width, **kw)
        assert status != abi.SZG_OK, word
        assert word in lib().szg_last_error().decode(), (word, lib().szg_last_error())
        got = target.read(gpu)
        assert np.array_equal(got[0], target.color0) and np.array_equal(got[1], target.depth0), word
        assert np.array_equal(got[2], target.debug0), word
    # fewer than two vertices: accepted, nothing drawn
    target = Target(gpu, W, H)
    assert p.record(target, cam, pos[:1], W, H, 1.0) == abi.SZG_OK
    assert np.array_equal(target.read(gpu)[0], target.color0)
    # the cap itself is accepted
    assert p.record(Target(gpu, W, H), cam, pos, W, H, abi.SZG_DEBUG_LINES_MAX_WIDTH) == abi.SZG_OK
    p.close()


def test_python_debug_lines_mirror(gpu):
    """pipelines.DebugLines: push* through the C builders, capacity enforced, recordDraw only when enabled."""
    from syzygy_amd import scene

    pl = gpu.pl
    W, H = 320, 180
    lines = pl.DebugLines()
    cams = pl.TStagedBuffer(abi.CameraPacked, 1)
    c = frame_loop_camera()
    cam = scene.camera_packed(c, W / H)
    cams.push(cam)
    cams.recordCopyToDevice()
    lines.pushBox((0, -8, 6), (0, 0, 0, 1), (5, 5, 5))
    lines.push((0, 0, 0), (10, -10, 10))
    target = pl.SceneTexture(W, H, debug=True)
    res = lines.recordDraw(None, 0, target, pl.rect(W, H), cams)
    gpu.torch.cuda.synchronize()
    assert res == (0, 0, 0) and not target.color.any().item()  # off by default: nothing launched
    lines.enabled, lines.lineWidth = True, 2.0
    res = lines.recordDraw(None, 0, target, pl.rect(W, H), cams)
    assert res == (1, 50, 50)
    staged = np.concatenate([dm.positions_of((abi.VertexPacked * 50)(*lines.vertices.readValidStaged()))])
    mask = dm.model(cam, staged, W, H, 2.0)
    want, _ = dm.render(mask, np.zeros((H, W, 4), np.uint16))
    assert np.array_equal(target.color_numpy(), want) and mask.sum() > 100
    with pytest.raises(ValueError):
        for _ in range(25):
            lines.pushBox((0, 0, 0), (0, 0, 0, 1), (1, 1, 1))
    lines.cleanup()
