"""The composite keeps its two march requests per pixel (primary ray, metal reflection that hits the ground), their results, the
three flags and what phase C wants back in a per-thread queue in LDS (kernels_composite.hip, phase B). Frames that queue
could get wrong - threads that leave before it, slots that stay empty, slots that are all full, row-tiled launches - each bit
for bit against the oracle: the debug image (with its NaN pattern) and the UNORM16 colour."""
import numpy as np
import pytest

from tests import literal_pair as lp
from tests import util
from tests.test_gpu_parity import gpu, run_composite_case  # noqa: F401  (gpu is a fixture)

pytestmark = pytest.mark.gpu

SMALL_LUTS = ((256, 64), (128, 64))


def assert_bit_identical(got, got_q, frame, what):
    want = frame.debug
    assert got.shape == want.shape and got_q.shape == frame.color.shape, what
    lp.compared(want.size + frame.color.size)
    assert (np.isnan(got) == np.isnan(want)).all(), f"{what}: NaN pattern differs"
    ok = ~np.isnan(want)
    differing = int((got.view(np.uint32)[ok] != want.view(np.uint32)[ok]).sum())
    print(f"{what}: {differing} of {ok.sum()} values differ, colour differs at {int((got_q != frame.color).sum())}")
    assert differing == 0, what
    assert (got_q == frame.color).all(), what


# A workgroup covers 32 x 8 pixels, a wave 8 x 8 of them: extents that leave partly filled waves and workgroups in x, in y and
# in both, one narrower than a wave's 8 columns, one lower than its 8 rows, and one single pixel.
@pytest.mark.parametrize("size", [(70, 37), (33, 9), (5, 13), (45, 3), (1, 1)])
def test_extents_that_are_not_multiples_of_the_workgroup(gpu, size):
    W, H = size
    got, got_q, frame = run_composite_case(gpu, W, H, 25.0, lut=SMALL_LUTS)
    assert_bit_identical(got, got_q, frame, f"composite {W}x{H}")


def pixel_directions(cam, W, H):
    """camera.comp:324-328 in float64: the view direction of every pixel in the atmosphere's frame (+y up)."""
    inverse_projection = np.array(list(cam.inverseProjection.m), np.float64).reshape(4, 4).T  # column-major
    rotation = np.array(list(cam.rotation.m), np.float64).reshape(4, 4).T
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    clip = np.stack([(x / W - 0.5) * 2.0, (y / H - 0.5) * 2.0, np.ones_like(x, float), np.ones_like(x, float)], axis=-1)
    rot = clip @ inverse_projection.T @ rotation.T
    d = rot[..., :3] / np.linalg.norm(rot[..., :3], axis=-1, keepdims=True)
    d[..., 1] *= -1.0
    return d


def camera_above(pitch):
    from syzygy_amd import scene

    cam = scene.default_camera()
    cam.cameraPosition[:] = [0.0, -300.0, -13.0]  # engine frame, +y down: 300 m above the ground
    cam.eulerAngles[:] = [pitch, 0.0, 0.3]
    return cam


def test_every_pixel_needs_both_marches(gpu):
    """Metal seen from above: every pixel is geometry 40-60 m above the ground (slot 0: aerial perspective) whose normal is
    horizontal, so the reflection of the downward view ray keeps going down and hits the ground (slot 1)."""
    W, H = 96, 40
    cam = camera_above(-0.9)
    probe = util.Inputs(W, H, elevation_degrees=30.0, spots=8, camera=cam)
    directions = pixel_directions(probe.cam, W, H)
    assert (directions[..., 1] < -0.05).all(), "the camera does not look down at every pixel"

    def poison(frame, inp):
        rng = np.random.default_rng(11)
        frame.depth[:] = 0.5
        frame.position[..., 0] = rng.uniform(-200.0, 200.0, (H, W)).astype(np.float32)
        frame.position[..., 1] = rng.uniform(-60.0, -40.0, (H, W)).astype(np.float32)  # +y is down: above the ground
        frame.position[..., 2] = rng.uniform(-200.0, 200.0, (H, W)).astype(np.float32)
        frame.position[..., 3] = 1.0
        angle = rng.uniform(0.0, 2.0 * np.pi, (H, W))
        frame.normal[..., 0] = np.cos(angle).astype(np.float16)
        frame.normal[..., 1] = 0.0
        frame.normal[..., 2] = np.sin(angle).astype(np.float16)
        frame.diffuse[..., :3] = np.float16(0.5)
        frame.specular[..., :3] = np.float16(0.7)
        frame.orm[..., 0] = np.float16(1.0)
        frame.orm[..., 1] = np.float16(0.4)
        frame.orm[..., 2] = np.float16(1.0)  # metallic: the reflection term is evaluated
        # reflect(d, n) = d - 2 (d.n) n with n.y = 0 keeps d.y: downwards from a few tens of metres up, it meets the ground
        n = np.stack([frame.normal[..., 0], frame.normal[..., 1], frame.normal[..., 2]], axis=-1).astype(np.float64)
        reflected = directions - 2.0 * (directions * n).sum(-1, keepdims=True) * n
        assert (reflected[..., 1] < -0.04).all()

    got, got_q, frame = run_composite_case(gpu, W, H, 30.0, camera=cam, lut=SMALL_LUTS, poison=poison)
    assert (frame.depth > 0).all()
    assert_bit_identical(got, got_q, frame, "composite, both marches at every pixel")


def test_no_pixel_needs_a_march(gpu):
    """Sky alone, seen from below the horizon line upwards: no primary ray hits the ground, no geometry: both slots of every
    thread stay empty and phase C must not read a result."""
    W, H = 96, 40
    cam = camera_above(0.9)
    probe = util.Inputs(W, H, elevation_degrees=30.0, spots=8, camera=cam)
    assert (pixel_directions(probe.cam, W, H)[..., 1] > 0.05).all(), "the camera does not look up at every pixel"

    def poison(frame, inp):
        frame.depth[:] = 0.0

    got, got_q, frame = run_composite_case(gpu, W, H, 30.0, camera=cam, lut=SMALL_LUTS, poison=poison)
    assert_bit_identical(got, got_q, frame, "composite, no march")


@pytest.mark.parametrize("nranks,block_rows,rank", [(3, 4, 1), (2, 8, 0)])
def test_row_tiled_frame(gpu, nranks, block_rows, rank):
    """One rank's tile of a row-tiled frame (local rows map to global rows in blocks; 50 rows leave a partial block)."""
    W, H = 72, 50
    tile = util.rowtile(H, block_rows, rank, nranks)
    assert 0 < tile.local_rows < H
    got, got_q, frame = run_composite_case(gpu, W, H, 25.0, tile=tile, lut=SMALL_LUTS)
    assert got.shape[0] == tile.local_rows
    assert_bit_identical(got, got_q, frame, f"composite tile {rank} of {nranks}, blocks of {block_rows} rows")
