"""GPU: the hand-made pixels of tests/composite_gate_cases.py through recordComposite and recordCompositeFast, against the CPU
oracle bit for bit.

k_composite claims that none of its lean switches, nor the skip of a non-metal's reflection, changes a bit of camera.comp's
result. Each test runs the groups of one gate family - every pixel placed on a threshold, on both sides of it and at its
float32 neighbours, in uniform, mixed and partial waves - and requires the fp32 debug image to equal the oracle's in every bit
(NaN for NaN) and the UNORM16 colour to be identical: the suite's own rule for this kernel (assert_bit_identical of
tests/test_gpu_composite_march_queue.py). No pixel is left out. A mismatch names the group, the scenario, its family and form,
the lane, both values in hex and the census's verdict for the lane.

Every group is uploaded as run_composite_case of tests/test_gpu_parity.py does it: G-buffer, depth and prior colour uploaded,
both LUTs uploaded through the pipeline's own images (which re-scans their status words), the sun's shadow map - rows wider than
the map - set with setShadowMap. The fast composite fetches from the aerial volume recorded on the GPU; the oracle gets the
download of that same volume."""
import functools

import numpy as np
import pytest

from syzygy_amd import abi
from tests import composite_gate_cases as cg
from tests import literal_pair as lp
from tests import padded_images as pi

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
def built():
    return cg.build()


def groups_of(family):
    return [g for g in built() if any(sc.family == family for sc in g.scenarios)]


def hex_of(values):
    return "[" + " ".join(f"{int(v):08x}" for v in np.asarray(values).view(np.uint32 if np.asarray(values).dtype == np.float32 else np.uint16)) + "]"


def describe_mismatch(group, y, x, got, want):
    k = group.scenario_at(x, y)
    lane = (y % 8) * 8 + x % 8
    if k is None:
        return f"group {group.name}, texel ({x}, {y}) of an empty (sky) tile, lane {lane}: kernel {got} {hex_of(got)}, oracle {want} {hex_of(want)}"
    sc = group.scenarios[k]
    return (f"group {group.name}, scenario {sc.name} ({sc.family}, {sc.form}), lane {lane} (texel {x}, {y}): kernel {got} {hex_of(got)}, "
            f"oracle {want} {hex_of(want)}\n  census: {cg.verdict(group, k, lane)}")


def assert_same_image(group, debug, color, want_debug, want_color, what):
    assert debug.shape == want_debug.shape and color.shape == want_color.shape
    lp.compared(want_debug.size + want_color.size)
    same = (debug.view(np.uint32) == want_debug.view(np.uint32)) | (np.isnan(debug) & np.isnan(want_debug))
    bad = np.argwhere(~same.all(axis=-1))
    if len(bad):
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} texels of the debug image differ from the oracle; first:\n" +
                             describe_mismatch(group, int(y), int(x), debug[y, x, :3], want_debug[y, x, :3]))
    bad = np.argwhere((color != want_color).any(axis=-1))
    if len(bad):
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} texels of the UNORM16 colour differ from the oracle; first:\n" +
                             describe_mismatch(group, int(y), int(x), color[y, x], want_color[y, x]))


def run_group(gpu, group, fast):
    torch, pl = gpu.torch, gpu.pl
    f = cg.frame_inputs(group)
    W, H = f.width, f.height
    cameras = pl.TStagedBuffer(abi.CameraPacked, 1)
    atmospheres = pl.TStagedBuffer(abi.AtmospherePacked, 1)
    lights = pl.TStagedBuffer(abi.DirectionalLightPacked, 2)
    cameras.push(f.cam)
    atmospheres.push(f.atm)
    lights.push([f.dirs[0], f.dirs[1]])
    for b in (cameras, atmospheres, lights):
        b.recordCopyToDevice()
    target = pl.SceneTexture(W, H, debug=True)
    target.color.copy_(torch.from_numpy(f.prior.copy().view(np.int16)))
    target.depth.copy_(torch.from_numpy(f.depth.copy()))
    deferred = pl.DeferredShadingPipeline((W, H), max_spot_lights=1, max_shadow_maps=1)
    sky = pl.SkyViewComputePipeline.create(transmittance_extent=cg.TLUT_EXTENT, skyview_extent=cg.SLUT_EXTENT)
    try:
        deferred.upload_gbuffer({k: v.copy() for k, v in f.planes.items()})
        shadow = None
        if f.shadow is not None:
            shadow = pi.PaddedImage(abi.SZG_FORMAT_D32_SFLOAT, cg.MAP_W, cg.MAP_H, cg.MAP_PAD, pi.NEAREST_OCCLUDER).to_device(torch)
            shadow.write_inside(np.ascontiguousarray(f.shadow))
            deferred.setShadowMap(0, shadow.device.view(torch.float32)[:, : shadow.cap_w])
        sky.upload_lut(sky.transmittanceLUT(), f.tlut.copy())
        sky.upload_lut(sky.skyviewLUT(), f.slut.copy())
        record, aerial = sky.recordComposite, None
        if fast:
            sky.recordAerialLUT(None, 0, atmospheres, 0, cameras, cg.AERIAL_MAX_DISTANCE)
            torch.cuda.synchronize()
            aerial = (sky.download_lut(sky.aerialLUT()[0]), cg.AERIAL_MAX_DISTANCE)
            record = sky.recordCompositeFast
        record(None, target, f.rect, deferred.gbuffer(), deferred.shadowMaps(), 0, atmospheres, 0, cameras, 0, lights)
        torch.cuda.synchronize()
        debug, color = target.debug.cpu().numpy(), target.color_numpy()
        if shadow is not None:
            shadow.assert_untouched(f"{group.name}: shadow map")
    finally:
        deferred.cleanup()
        sky.destroy()
    want_debug, want_color = cg.oracle_frame(group, aerial=aerial)
    assert_same_image(group, debug, color, want_debug, want_color, f"{group.name} ({'fast' if fast else 'exact'} composite)")


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("family", cg.FAMILIES)
def test_gate_family_is_bit_identical_to_the_oracle(gpu, family, fast):
    groups = groups_of(family)
    assert groups
    for g in groups:
        run_group(gpu, g, fast)
