"""GPU: the fast composite (szg_skyview_record_composite_fast, k_composite<true>) against the oracle's fast composite, which
evaluates the fetch include/szg/abi.h states ("THE FETCH of the fast composite") on the same volume - bit for bit: the debug
plane with its NaN pattern, the UNORM16 colour, and the sky pixels against the exact GPU composite.

The frames are those of tests/aerial_model.py (fill scene, default camera, sun at 35 degrees, 70 x 37, small LUTs):
tests/test_aerial_model.py proves on the CPU that their geometry pixels, over the max distances used here, lie in the ramp
below the first slice, between every pair of slices and behind the last one."""
import functools

import numpy as np
import pytest

from tests import aerial_model as am
from tests import util
from tests.test_gpu_parity import gpu, run_composite_case, staged  # noqa: F401  (gpu is a fixture; staged is run_composite_case's)

pytestmark = pytest.mark.gpu

F = np.float32
ELEVATION, SPOTS, LUT = am.COVERAGE_ELEVATION, am.COVERAGE_SPOTS, am.LUT
W0, H0 = am.COVERAGE_EXTENTS[0]


def assert_bit_identical(got, got_q, frame, what):
    want = frame.debug
    assert got.shape == want.shape, what
    assert (np.isnan(got) == np.isnan(want)).all(), f"{what}: NaN pattern differs at {int((np.isnan(got) != np.isnan(want)).sum())} values"
    ok = ~np.isnan(want)
    differing = int((got.view(np.uint32)[ok] != want.view(np.uint32)[ok]).sum())
    print(f"{what}: {differing} of {ok.sum()} values differ, colour differs at {int((got_q != frame.color).sum())}")
    assert differing == 0, what
    assert (got_q == frame.color).all(), what


def fast_case(gpu, W=W0, H=H0, max_distance=am.COVERAGE_MAX_DISTANCES[0], volume=None, **kw):
    return run_composite_case(gpu, W, H, ELEVATION, spots=SPOTS, lut=LUT, aerial=(max_distance, volume), **kw)


@functools.lru_cache(maxsize=None)
def exact_frame(gpu):
    """The exact GPU composite of the 70 x 37 frame (shared, read-only)."""
    got, got_q, frame = run_composite_case(gpu, W0, H0, ELEVATION, spots=SPOTS, lut=LUT)
    got.setflags(write=False)
    return got, frame.depth > 0


# ---------------------------------------------------------------------------
# the volume the GPU recorded
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_distance", am.COVERAGE_MAX_DISTANCES)
def test_recorded_volume(gpu, max_distance):
    got, got_q, frame = fast_case(gpu, max_distance=max_distance)
    assert_bit_identical(got, got_q, frame, f"fast composite, max distance {max_distance}")
    exact, geometry = exact_frame(gpu)
    assert geometry.any() and (~geometry).any()
    assert (got[~geometry].view(np.uint32) == exact[~geometry].view(np.uint32)).all(), "sky pixels are the exact composite's"
    assert (got[geometry].view(np.uint32) != exact[geometry].view(np.uint32)).any(), "the fast mode was not taken"


# ---------------------------------------------------------------------------
# volumes written by the caller
# ---------------------------------------------------------------------------
def index_revealing_volume():
    k, j, i = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    vol = np.ones((32, 32, 32, 4), F)
    vol[..., :3] = ((i + 32 * j + 1024 * k).astype(F) * F(1.0e-3 / 32768.0))[..., None]
    return vol.reshape(32 * 32, 32, 4)


def random_poisoned_volume():
    rng = np.random.default_rng(0xF0C5)
    vol = (10.0 ** rng.uniform(-5.0, -2.0, (32 * 32 * 32, 4))).astype(F)
    vol[:, 3] = 1.0
    for value, count in ((np.nan, 400), (np.inf, 200)):
        vol[rng.choice(len(vol), count, replace=False), rng.integers(0, 3, count)] = value
    return vol.reshape(32 * 32, 32, 4)


@pytest.mark.parametrize("max_distance", [am.COVERAGE_MAX_DISTANCES[1], am.COVERAGE_MAX_DISTANCES[4]])
@pytest.mark.parametrize("make", [index_revealing_volume, random_poisoned_volume])
def test_uploaded_volume(gpu, make, max_distance):
    volume = make()
    got, got_q, frame = fast_case(gpu, max_distance=max_distance, volume=volume)
    assert frame.aerial_volume is volume
    geometry = frame.depth > 0
    if make is random_poisoned_volume:
        poisoned = ~np.isfinite(frame.debug[geometry][:, :3]).all(axis=-1)
        print(f"{int(poisoned.sum())} of {int(geometry.sum())} geometry pixels are NaN or inf through a froxel")
        assert 32 <= poisoned.sum() < geometry.sum() / 2, "the volume's NaN / inf froxels reach some pixels and spare most"
    else:
        assert np.isfinite(frame.debug).all()
    assert_bit_identical(got, got_q, frame, f"fast composite, {make.__name__}, max distance {max_distance}")


# ---------------------------------------------------------------------------
# distances an ordinary frame never has
# ---------------------------------------------------------------------------
def test_poisoned_positions(gpu):
    """Geometry pixels AT the camera (dist 0), a denormal and an ulp beside it, so close that the squared distance underflows,
    1e30 m away (the squared distance overflows: dist = +inf), at inf and at NaN. Only the position plane changes; y stays at
    or below 0 (+y is down), so the pixels stay geometry. Every fourth poisoned pixel is metal as well.

    What this can and cannot see: with dist = 0 (also after the underflow of its square), +inf or NaN the pixel is NaN whatever
    the fetch returns - the transmittance to the surface normalises a zero or non-finite vector - so for those cases only the
    NaN pattern is compared here; the rule's clauses for dist = 0, +inf and NaN are pinned by the CPU comparison of oracle and
    model (tests/test_aerial_model.py). The offsets of 1e-12 .. 1e-3 m give FINITE pixels deep in the ramp, compared bit for
    bit."""
    picked = {}

    def poison(frame, inp):
        cam = np.array(inp.cam.position[:3], F)
        assert cam[0] == 0.0 and cam[1] < 0.0  # a denormal offset in x is representable
        geometry = np.argwhere(frame.depth > 0)
        rng = np.random.default_rng(31)
        picks = geometry[rng.choice(len(geometry), 96, replace=False)]
        cases = [cam,
                 cam + np.array([1.0e-40, 0.0, 0.0], F),                                  # a denormal away
                 np.array([cam[0], cam[1], np.nextafter(cam[2], F(0.0))], F),              # one ulp away
                 cam + np.array([3.0e-17, 0.0, 0.0], F),                                  # dist^2 ~ 1e-45 Mm^2: underflows
                 cam + np.array([1.0e-12, 0.0, 0.0], F),                                  # deep in the ramp, finite pixels
                 cam + np.array([1.0e-9, 0.0, 0.0], F), cam + np.array([1.0e-6, 0.0, 0.0], F), cam + np.array([1.0e-3, 0.0, 0.0], F),
                 np.array([1.0e30, cam[1], cam[2]], F), np.array([cam[0], -1.0e30, cam[2]], F),
                 np.array([np.inf, cam[1], cam[2]], F), np.array([cam[0], cam[1], -np.inf], F), np.array([cam[0], -np.inf, cam[2]], F),
                 np.array([np.nan, cam[1], cam[2]], F), np.array([cam[0], cam[1], np.nan], F)]
        for n, (y, x) in enumerate(picks):
            frame.position[y, x, :3] = cases[n % len(cases)]
            if n % 4 == 0:
                frame.orm[y, x, 2] = np.float16(1.0)
        picked["pixels"] = picks

    for max_distance, volume in ((am.COVERAGE_MAX_DISTANCES[2], None), (am.COVERAGE_MAX_DISTANCES[2], random_poisoned_volume())):
        got, got_q, frame = fast_case(gpu, max_distance=max_distance, volume=volume, poison=poison)
        ys, xs = picked["pixels"].T
        assert (frame.depth[ys, xs] > 0).all() and not (frame.position[ys, xs, 1] > 0).any()
        assert np.isnan(frame.debug[ys, xs]).any()
        if volume is None:
            assert np.isfinite(frame.debug[ys, xs]).all(axis=-1).sum() >= 4 * (96 // 15), "the small offsets give finite pixels"
        assert_bit_identical(got, got_q, frame, "fast composite, poisoned positions" + (", poisoned volume" if volume is not None else ""))


# ---------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------
# 64 x 64: odd pixels sit on froxel centres (both bilinear weights 0 or 1); 33 x 9: one texel past a workgroup in each axis
@pytest.mark.parametrize("size", [(64, 64), (33, 9)])
def test_extents(gpu, size):
    for max_distance in (am.COVERAGE_MAX_DISTANCES[2], am.COVERAGE_MAX_DISTANCES[5]):
        got, got_q, frame = fast_case(gpu, size[0], size[1], max_distance=max_distance)
        assert (frame.depth > 0).any()
        assert_bit_identical(got, got_q, frame, f"fast composite {size[0]}x{size[1]}, max distance {max_distance}")


def test_one_geometry_pixel(gpu):
    """1 x 1: sx = sy = 0, both axes clamp to the edge: only froxel column 0, row 0 may show."""
    def poison(frame, inp):
        frame.depth[0, 0] = 0.5
        frame.position[0, 0] = [3.0, -1.0, 40.0, 1.0]  # ~ 54 m from the camera, above the ground
        frame.normal[0, 0] = [0.0, -1.0, 0.0, 0.0]
        frame.diffuse[0, 0] = frame.specular[0, 0] = [0.5, 0.5, 0.5, 1.0]
        frame.orm[0, 0] = [1.0, 0.5, 0.0, 1.0]

    volume = np.full((32, 32, 32, 4), np.nan, F)
    volume[:, 0, 0] = index_revealing_volume().reshape(32, 32, 32, 4)[:, 0, 0]
    for v in (None, volume.reshape(32 * 32, 32, 4)):
        got, got_q, frame = fast_case(gpu, 1, 1, max_distance=am.COVERAGE_MAX_DISTANCES[3], volume=v, poison=poison)
        assert frame.depth[0, 0] > 0 and np.isfinite(frame.debug).all()
        assert_bit_identical(got, got_q, frame, "fast composite 1x1")


@pytest.mark.parametrize("nranks,block_rows", [(2, 8), (3, 4)])
def test_row_tiles_equal_the_untiled_fast_frame(gpu, nranks, block_rows):
    """Each rank's tile is its rows of the untiled fast frame, bit for bit: sy comes from the GLOBAL row."""
    max_distance = am.COVERAGE_MAX_DISTANCES[4]
    full, full_q, full_frame = fast_case(gpu, max_distance=max_distance)
    assert_bit_identical(full, full_q, full_frame, "untiled fast frame")
    for rank in range(nranks):
        tile = util.rowtile(H0, block_rows, rank, nranks)
        rows = util.global_rows(H0, block_rows, rank, nranks)
        assert 0 < tile.local_rows == len(rows) < H0
        got, got_q, frame = fast_case(gpu, max_distance=max_distance, tile=tile, volume=full_frame.aerial_volume)
        assert (got.view(np.uint32) == full[rows].view(np.uint32)).all() or \
            ((np.isnan(got) == np.isnan(full[rows])).all() and (got.view(np.uint32) == full[rows].view(np.uint32))[~np.isnan(got)].all())
        assert (got_q == full_q[rows]).all()
        assert_bit_identical(got, got_q, frame, f"fast composite, tile {rank} of {nranks}, blocks of {block_rows} rows")
