"""GPU: the hand-made frames of tests/composite_pixel_cases.py through recordComposite against the CPU oracle, bit for bit with
no value excluded.

k_composite forms the view direction, the material, the surface position, the BRDF's two pow() and the tonemap with the lean
exact operators wherever a wave-uniform gate proves their operand domain, and reads what depends on the camera, the
atmosphere and the draw extent alone from the block k_frame_prep writes once per record call. None of it may change a bit of
camera.comp's result. Every gate has waves with all lanes inside its domain, all outside, and a single lane outside; the frames
are one workgroup (32x8), 40x16 (partial workgroups) or one pixel wide, the LUTs 64x16 and 128x64 (the oracle's, uploaded).

The convertPBR frames also run through the lights pass (recordLights against oracle.lights) at 0, 1 and 3 spot lights: the two
passes share the function."""
import functools

import numpy as np
import pytest

from syzygy_amd import abi
from tests import composite_pixel_cases as cp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    from syzygy_amd import pipelines

    class Ctx:
        pass

    c = Ctx()
    c.torch, c.pl = torch, pipelines
    return c


@functools.lru_cache(maxsize=None)
def frames():
    return {f.name: f for f in cp.build()}


def staged(pl, f):
    cameras = pl.TStagedBuffer(abi.CameraPacked, 1)
    atmospheres = pl.TStagedBuffer(abi.AtmospherePacked, 1)
    lights = pl.TStagedBuffer(abi.DirectionalLightPacked, 2)
    cameras.push(f.cam)
    atmospheres.push(f.atm)
    lights.push([f.dirs[0], f.dirs[1]])
    for b in (cameras, atmospheres, lights):
        b.recordCopyToDevice()
    return cameras, atmospheres, lights


def run_composite(gpu, frame):
    torch, pl = gpu.torch, gpu.pl
    f = cp.frame_inputs(frame)
    cameras, atmospheres, lights = staged(pl, f)
    target = pl.SceneTexture(f.width, f.height, debug=True)
    target.color.copy_(torch.from_numpy(f.prior.copy().view(np.int16)))
    target.depth.copy_(torch.from_numpy(f.depth.copy()))
    deferred = pl.DeferredShadingPipeline((f.width, f.height), max_spot_lights=1, max_shadow_maps=0)
    sky = pl.SkyViewComputePipeline.create(transmittance_extent=cp.TLUT_EXTENT, skyview_extent=cp.SLUT_EXTENT)
    try:
        deferred.upload_gbuffer({k: v.copy() for k, v in f.planes.items()})
        sky.upload_lut(sky.transmittanceLUT(), f.tlut.copy())
        sky.upload_lut(sky.skyviewLUT(), f.slut.copy())
        sky.recordComposite(None, target, f.rect, deferred.gbuffer(), deferred.shadowMaps(), 0, atmospheres, 0, cameras, 0, lights)
        torch.cuda.synchronize()
        debug, color = target.debug.cpu().numpy(), target.color_numpy()
    finally:
        deferred.cleanup()
        sky.destroy()
    want_debug, want_color = cp.oracle_composite(frame)
    cp.assert_same(frame, debug, color, want_debug, want_color, f"{frame.name} (composite)")


@pytest.mark.parametrize("name", [f.name for f in cp.build()])
def test_composite_frame_is_bit_identical_to_the_oracle(gpu, name):
    run_composite(gpu, frames()[name])


def test_every_gate_has_frames_on_both_sides_and_with_a_single_lane_outside():
    for gate in cp.GATES:
        sides = {f.side for f in frames().values() if f.gate == gate}
        assert sides & {"both", "lane"} and sides & {"both", "out"}, (gate, sides)


@pytest.mark.parametrize("spots", [0, 1, 3])
@pytest.mark.parametrize("name", cp.MATERIAL_FRAMES)
def test_lights_pass_on_the_material_frames_is_bit_identical_to_the_oracle(gpu, name, spots):
    torch, pl = gpu.torch, gpu.pl
    frame = frames()[name]
    f = cp.frame_inputs(frame)
    cameras, atmospheres, lights = staged(pl, f)
    spot = cp.spot_lights(spots)
    target = pl.SceneTexture(f.width, f.height, debug=True)
    target.depth.copy_(torch.from_numpy(f.depth.copy()))
    deferred = pl.DeferredShadingPipeline((f.width, f.height), max_spot_lights=max(spots, 1), max_shadow_maps=0)
    try:
        deferred.upload_gbuffer({k: v.copy() for k, v in f.planes.items()})
        deferred.recordLights(None, f.rect, target, 1, lights, spot, 0, cameras)
        torch.cuda.synchronize()
        debug, color = target.debug.cpu().numpy(), target.color_numpy()
    finally:
        deferred.cleanup()
    want_debug, want_color = cp.oracle_lights(frame, spot, spots)
    cp.assert_same(frame, debug, color, want_debug, want_color, f"{name} (lights, {spots} spot lights)")
