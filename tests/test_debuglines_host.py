"""The DebugLines list builders of szg/host.h (renderer/pipelines/debuglines.cpp:23-124) against a numpy restatement of
the same glm formulas, bit for bit (there is no glm here: both sides restate glm 1.0.1's published formulas), and the
vertex fields and box topology they promise. No GPU needed."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from syzygy_amd import abi, lib

F32 = np.float32
RIGHT, FORWARD, UP = (np.array(v, np.float32) for v in ((1, 0, 0), (0, 0, 1), (0, -1, 0)))  # geometrystatics.hpp:7-9


def fa(v):
    v = [float(x) for x in v]
    return (C.c_float * len(v))(*v)


def positions(out):
    return np.frombuffer(bytes(out), np.float32).reshape(-1, 12)[:, 0:3]


def cross(x, y):  # glm::cross
    return np.array([x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]], np.float32)


def rotate(q, v):  # glm qua * vec3
    qv = np.asarray(q[:3], np.float32)
    uv = cross(qv, v)
    uuv = cross(qv, uv)
    return v + ((uv * F32(q[3])) + uuv) * F32(2.0)


def quad(a, b, c, d):
    return [a, b, b, c, c, d, d, a]


def rect_axes(c, A, B):
    return quad(c + A + B, c + A - B, c - A - B, c - A + B)


def box(c, r, f, u):
    return (rect_axes(c - u, r, f) + rect_axes(c + u, r, f) + rect_axes(c - r, f, u) + rect_axes(c + r, f, u) +
            rect_axes(c - f, u, r) + rect_axes(c + f, u, r))


def mat_vec(m, v):  # glm mat4 * vec4: (m0*x + m1*y) + (m2*z + m3*w)
    M = np.array(m.m, np.float32).reshape(4, 4)  # rows = columns of the matrix
    return (M[0] * v[0] + M[1] * v[1]) + (M[2] * v[2] + M[3] * v[3])


def same(out, want):
    got = positions(out)
    want = np.array(want, np.float32)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]


def quats(rng, n):
    for i in range(n):
        q = rng.normal(size=4)
        if i % 2 == 0:
            q /= np.linalg.norm(q)  # unit
        else:
            q *= rng.uniform(0.2, 3.0)  # non-unit: glm does not normalise
        yield np.array(q, np.float32)


def v3(rng, lo=-50, hi=50):
    return np.array(rng.uniform(lo, hi, 3), np.float32)


def test_vertex_fields():
    out = (abi.VertexPacked * 2)()
    lib().szg_debug_lines_segment(fa([1, 2, 3]), fa([4, 5, 6]), out)
    raw = np.frombuffer(bytes(out), np.float32).reshape(2, 12)
    # position, uv_x, normal, uv_y, color
    assert raw[0].tolist() == [1, 2, 3, 0, 0, 0, 0, 0, 1, 0, 0, 1]
    assert raw[1].tolist() == [4, 5, 6, 1, 0, 0, 0, 0, 0, 0, 1, 1]


def test_segment_quad_and_rectangle_axes():
    rng = np.random.default_rng(11)
    for _ in range(50):
        a, b, c, d = (v3(rng) for _ in range(4))
        out = (abi.VertexPacked * 8)()
        lib().szg_debug_lines_quad(fa(a), fa(b), fa(c), fa(d), out)
        same(out, quad(a, b, c, d))
        lib().szg_debug_lines_rectangle_axes(fa(a), fa(b), fa(c), out)
        same(out, rect_axes(a, b, c))


def test_rectangle_oriented():
    rng = np.random.default_rng(12)
    for q in quats(rng, 60):
        c, e = v3(rng), np.array(rng.uniform(-10, 10, 2), np.float32)
        out = (abi.VertexPacked * 8)()
        lib().szg_debug_lines_rectangle_oriented(fa(c), fa(q), fa(e), out)
        scale = np.array([e[0], 1.0, e[1]], np.float32)
        same(out, rect_axes(c, rotate(q, scale * RIGHT), rotate(q, scale * FORWARD)))


def test_box_center_quat_extents():
    rng = np.random.default_rng(13)
    for q in quats(rng, 60):
        c, e = v3(rng), np.array(rng.uniform(0.01, 20, 3), np.float32)
        out = (abi.VertexPacked * 48)()
        lib().szg_debug_lines_box(fa(c), fa(q), fa(e), out)
        same(out, box(c, rotate(q, e * RIGHT), rotate(q, e * FORWARD), rotate(q, e * UP)))


def test_box_transform():
    rng = np.random.default_rng(14)
    for _ in range(60):
        t = abi.Transform()
        t.translation[:] = [float(x) for x in v3(rng)]
        t.eulerAnglesRadians[:] = [float(x) for x in rng.uniform(-np.pi, np.pi, 3)]
        t.scale[:] = [float(x) for x in rng.uniform(0.1, 6, 3)]
        bb = abi.AABB()
        bb.center[:] = [float(x) for x in v3(rng, -3, 3)]
        bb.half_extent[:] = [float(x) for x in rng.uniform(0.01, 4, 3)]
        out = (abi.VertexPacked * 48)()
        lib().szg_debug_lines_box_transform(C.byref(t), C.byref(bb), out)
        m = abi.Mat4()
        lib().szg_transform_matrix(t.translation, t.eulerAnglesRadians, t.scale, C.byref(m))  # Transform::toMatrix
        h = np.array(bb.half_extent, np.float32)
        axes = [mat_vec(m, np.append(h * a, F32(0)))[:3] for a in (RIGHT, FORWARD, UP)]
        centre = mat_vec(m, np.append(np.array(bb.center, np.float32), F32(1)))[:3]
        same(out, box(centre, *axes))


@pytest.mark.parametrize("use_transform", [False, True])
def test_box_is_24_segments_over_the_8_corners(use_transform):
    out = (abi.VertexPacked * 48)()
    if use_transform:
        t = abi.Transform()
        t.translation[:], t.eulerAnglesRadians[:], t.scale[:] = [1, 2, 3], [0, 0, 0], [1, 1, 1]
        bb = abi.AABB()
        bb.center[:], bb.half_extent[:] = [0, 0, 0], [1, 2, 4]
        lib().szg_debug_lines_box_transform(C.byref(t), C.byref(bb), out)
        centre, ext = np.array([1, 2, 3], np.float32), np.array([1, 2, 4], np.float32)
    else:
        lib().szg_debug_lines_box(fa([1, 2, 3]), fa([0, 0, 0, 1]), fa([1, 2, 4]), out)
        centre, ext = np.array([1, 2, 3], np.float32), np.array([1, 2, 4], np.float32)
    p = positions(out)
    corners = {tuple(centre + ext * np.array(s, np.float32)) for s in np.array(np.meshgrid([-1, 1], [-1, 1], [-1, 1])).T.reshape(-1, 3)}
    assert {tuple(x) for x in p} == corners
    # each corner: 3 edges, each edge drawn by the 2 faces that share it, so 6 endpoints
    assert set(Counter(tuple(x) for x in p).values()) == {6}
    # every segment is one box edge: exactly one coordinate differs
    seg = p.reshape(24, 2, 3)
    assert ((seg[:, 0] != seg[:, 1]).sum(axis=1) == 1).all()
    edges = Counter(frozenset((tuple(s[0]), tuple(s[1]))) for s in seg)
    assert len(edges) == 12 and set(edges.values()) == {2}
