"""The composite reads the frame's constants again for each of the two march slots (kernels_composite.hip, phase B). That must
not depend on which slots a wave runs: one 40 x 12 frame, no multiple of the 32 x 8 workgroup, seen from above, in which the
lanes of every 8 x 8 wave alternate between four kinds of pixel:

  0  sky (the view ray meets the ground: slot 0)
  1  non-metal geometry (slot 0 only)
  2  metal whose reflection meets the ground (both slots)
  3  metal whose reflection leaves for the sky (slot 0; the reflection samples the sky-view LUT)

Both images bit for bit against the oracle, the debug image with its NaN pattern and the UNORM16 colour, with a sun shadow
map bound and with none."""
import numpy as np
import pytest

from tests import util
from tests.test_gpu_composite_march_queue import SMALL_LUTS, assert_bit_identical, camera_above, pixel_directions
from tests.test_gpu_parity import gpu, run_composite_case  # noqa: F401  (gpu is a fixture)

pytestmark = pytest.mark.gpu

W, H = 40, 12


def kinds():
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    return (x + y) % 4


@pytest.mark.parametrize("shadow", [False, True])
def test_four_kinds_of_pixel_in_every_wave(gpu, shadow):
    cam = camera_above(-0.9)
    probe = util.Inputs(W, H, elevation_degrees=30.0, spots=8, camera=cam)
    directions = pixel_directions(probe.cam, W, H)
    assert (directions[..., 1] < -0.05).all(), "the camera does not look down at every pixel"
    kind = kinds()
    for wy in range(0, H, 8):
        for wx in range(0, W, 8):
            assert set(kind[wy:wy + 8, wx:wx + 8].ravel()) == {0, 1, 2, 3}

    def poison(frame, inp):
        rng = np.random.default_rng(17)
        frame.depth[:] = np.where(kind == 0, 0.0, 0.5).astype(np.float32)
        frame.position[..., 0] = rng.uniform(-200.0, 200.0, (H, W)).astype(np.float32)
        frame.position[..., 1] = rng.uniform(-60.0, -40.0, (H, W)).astype(np.float32)  # +y is down: above the ground
        frame.position[..., 2] = rng.uniform(-200.0, 200.0, (H, W)).astype(np.float32)
        frame.position[..., 3] = 1.0
        angle = rng.uniform(0.0, 2.0 * np.pi, (H, W))
        up = kind == 3
        # horizontal normals keep the reflection going down; a normal that points up (engine frame: -y) turns it to the sky
        frame.normal[..., 0] = np.where(up, 0.0, np.cos(angle)).astype(np.float16)
        frame.normal[..., 1] = np.where(up, -1.0, 0.0).astype(np.float16)
        frame.normal[..., 2] = np.where(up, 0.0, np.sin(angle)).astype(np.float16)
        frame.diffuse[..., :3] = np.float16(0.5)
        frame.specular[..., :3] = np.float16(0.7)
        frame.orm[..., 0] = np.float16(1.0)
        frame.orm[..., 1] = np.float16(0.4)
        frame.orm[..., 2] = np.where(kind >= 2, 1.0, 0.0).astype(np.float16)  # metallic
        n = np.stack([frame.normal[..., 0], -frame.normal[..., 1].astype(np.float64), frame.normal[..., 2]], axis=-1).astype(np.float64)
        reflected = directions - 2.0 * (directions * n).sum(-1, keepdims=True) * n
        assert (reflected[..., 1][kind == 2] < -0.04).all() and (reflected[..., 1][kind == 3] > 0.04).all()

    sun_shadow = np.random.default_rng(7).random((96, 96), dtype=np.float32) if shadow else None
    got, got_q, frame = run_composite_case(gpu, W, H, 30.0, camera=cam, lut=SMALL_LUTS, poison=poison, sun_shadow=sun_shadow)
    assert ((frame.depth == 0) == (kind == 0)).all()
    # the kinds differ in the image: no two of them share all their values
    assert len({frame.debug[kind == k].tobytes() for k in range(4)}) == 4
    assert_bit_identical(got, got_q, frame, "composite, four kinds of pixel per wave, %s sun shadow map" % ("with a" if shadow else "no"))
