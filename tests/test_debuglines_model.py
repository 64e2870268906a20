"""The CPU model of the debug-line pass (tests/debuglines_model.py) against the reference's committed debugline.vert.spv
(tests/golden/debugline_vectors.npz, bit for bit), its two candidate enumerations against each other, and the C-ABI of
include/szg/debuglines.h (exported, bound, versioned). No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from syzygy_amd import abi, lib, library_path
from tests import debuglines_model as dm
from tests.golden import make_debugline_vectors as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def vec():
    return np.load(os.path.join(ROOT, "tests", "golden", "debugline_vectors.npz"))


def test_vertex_stage_reproduces_the_committed_spirv_bit_for_bit(vec):
    for k in range(2):
        cam = abi.CameraPacked.from_buffer_copy(vec[f"camera_{k}"].tobytes())
        pos = dm.positions_of(vec[f"vertices_{k}"])
        got = dm.clip_positions(cam, pos).view(np.uint32)
        want = vec[f"gl_position_{k}"]
        assert got.shape == want.shape
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_vectors_cover_the_cases_the_rules_name(vec):
    clip = np.concatenate([vec[f"gl_position_{k}"].view(np.float32) for k in range(2)])
    assert (clip[:, 3] < 0).sum() >= 8          # behind the camera
    assert (np.abs(clip[:, 2] - clip[:, 3]) <= 1e-3 * np.abs(clip[:, 3])).sum() >= 8  # on the near plane (z = w)
    assert (np.abs(clip) > 1e20).any(axis=1).sum() >= 8  # very large


@pytest.mark.skipif(not gen.available(), reason="the reference's committed SPIR-V is only present in the build container")
def test_committed_vectors_are_what_the_reference_binary_produces(vec):
    live = gen.generate(log=lambda *_: None)
    assert sorted(live) == sorted(vec.files)
    for name in vec.files:
        assert np.array_equal(np.asarray(live[name]), vec[name]), name


def _lines(rng, n, W, H, spread, length):
    a = rng.uniform(-spread, 1 + spread, (n, 2)) * [W, H]
    d = rng.normal(size=(n, 2))
    d *= (rng.uniform(0, length, n) / np.maximum(np.linalg.norm(d, axis=1), 1e-9))[:, None]
    b = a + d
    return tuple(np.asarray(v, np.float32) for v in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))


@pytest.mark.parametrize("width", [0.0, 1.0, 1.5, 3.0, 8.0, 100.0])
def test_band_enumeration_equals_the_bounding_box(width):
    """The fast enumeration drops no pixel of the exact test: random, axis-aligned, half-integer and far-off lines."""
    W, H = 96, 64
    rng = np.random.default_rng(int(width * 10) + 3)
    xa, ya, xb, yb = _lines(rng, 120, W, H, 0.3, 80)
    special = np.array([[10, 20.5, 70, 20.5], [30.5, 5, 30.5, 60], [10, 10, 10, 10], [0, 0, 96, 64], [-1e6, 31, 1e6, 33],
                        [48, -1e6, 49, 1e6], [12, 12, 13, 40], [5.5, 5.5, 90.5, 5.5], [20, 30, 20, 30.25]], np.float32)
    lines = tuple(np.concatenate([v, special[:, i]]) for i, v in enumerate((xa, ya, xb, yb)))
    band = dm.coverage_band(lines, W, H, width)
    brute = dm.coverage_brute(lines, W, H, width)
    assert np.array_equal(band, brute), np.argwhere(band != brute)[:5]
    assert band.any()


def test_clipping_drops_lines_behind_the_camera_and_keeps_crossing_ones():
    from syzygy_amd import scene

    cam = scene.camera_packed(scene.default_camera(), 16 / 9)
    c = scene.default_camera()
    pos = np.array(c.cameraPosition, np.float32)
    fwd = np.array(scene.forward_from_eulers(list(c.eulerAngles)), np.float32)
    behind = np.stack([pos - fwd * 5, pos - fwd * 9 + 1])
    crossing = np.stack([pos - fwd * 5 + [0.5, 0.2, 0], pos + fwd * 20])
    assert len(dm.setup(cam, behind, 160, 90)[0]) == 0
    xa, ya, xb, yb = dm.setup(cam, crossing, 160, 90)
    assert len(xa) == 1 and np.isfinite([xa, ya, xb, yb]).all()
    # an odd last vertex draws nothing
    assert len(dm.setup(cam, np.concatenate([crossing, crossing[:1]]), 160, 90)[0]) == 1


def test_debuglines_header_is_exported_bound_and_versioned():
    text = open(os.path.join(ROOT, "include", "szg", "debuglines.h")).read()
    names = sorted(set(re.findall(r"\b(szg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert names == sorted(abi.DEBUGLINE_FUNCTIONS)
    handle = C.CDLL(library_path())
    for name in names:
        assert hasattr(handle, name)
    assert lib().szg_abi_version() == abi.SZG_ABI_VERSION == 2
    for macro, value in (("SZG_DEBUG_LINES_CAPACITY", 1000), ("SZG_DEBUG_LINES_MAX_WIDTH", 256.0),
                         ("SZG_DEBUG_LINES_GUARD_BAND", 16777216.0)):
        m = re.search(rf"#define {macro} ([0-9.]+)", text)
        assert m and float(m.group(1)) == value == getattr(abi, macro)


def test_create_without_a_device_fails_loudly_and_bad_capacities_are_refused():
    h = C.c_void_p()
    for cap in (0, abi.SZG_DEBUG_LINES_MAX_CAPACITY + 1):
        assert lib().szg_debug_lines_create(C.byref(h), cap, 0) == abi.SZG_ERR_INVALID_ARGUMENT
        assert b"capacity" in lib().szg_last_error()
    assert lib().szg_debug_lines_record(None, None, 1.0, abi.Rect(0, 0, 8, 8), None, None, 0, None, None, 0) == \
        abi.SZG_ERR_INVALID_ARGUMENT
