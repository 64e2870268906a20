"""GPU: the hand-made pixel-light pairs of tests/lights_gate_cases.py through recordLights, against the CPU oracle bit for bit.

k_lights claims that none of its culls, flags and lean paths changes a bit of lights.comp's sum. Each test runs the groups of
one gate family - every pair placed on a threshold, on both sides of it and at its float32 neighbours, in uniform, mixed and
partial waves - and requires the fp32 debug image to equal the oracle's in every bit (NaN for NaN) and the UNORM16 colour to be
identical. A mismatch names the scenario, the lane, the light and the census's verdict for the pair. Every group runs twice:
into tight images, and into a scene texture and a G-buffer allocated larger than the draw extent with padded pitches
(tests/padded_images.py), whose texels outside the extent must keep their sentinels. Shadow maps always have rows wider than
the map."""
import functools

import numpy as np
import pytest

from syzygy_amd import abi
from tests import lights_gate_cases as lg
from tests import literal_pair as lp
from tests import padded_images as pi

pytestmark = pytest.mark.gpu

CAPACITY_EXTRA = (11, 5)  # the padded run's scene texture and G-buffer are this much larger than the draw extent
SCENE_PADS = (3, 5, 1)


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
    return lg.build()


def groups_of(family):
    L, G = built()
    return [g for g in G if any(sc.family == family for sc in g.scenarios)]


def describe_mismatch(group, L, y, x, got, want):
    cols = min(lg.COLS, group.tiles)
    k = (y // 8) * cols + x // 8
    lane = (y % 8) * 8 + x % 8
    sc = group.scenarios[k]
    lines = [f"group {group.name}, scenario {sc.name} ({sc.family}, {sc.form}), lane {lane} (texel {x}, {y}): kernel {got} "
             f"({got.view(np.uint32)}), oracle {want} ({want.view(np.uint32)})"]
    for name in group.light_names[:6]:
        lines.append(f"  light {name}: {lg.verdict(group, k, lane, L[name])}")
    return "\n".join(lines)


def assert_same_image(group, L, debug, color, what):
    want_debug, want_color = lg.oracle_frame(group, L)
    assert debug.shape == want_debug.shape and color.shape == want_color.shape
    lp.compared(want_debug.size + want_color.size)
    same = (debug.view(np.uint32) == want_debug.view(np.uint32)) | (np.isnan(debug) & np.isnan(want_debug))
    bad = np.argwhere(~same.all(axis=-1))
    if len(bad):
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} texels of the debug image differ from the oracle; first:\n" +
                             describe_mismatch(group, L, int(y), int(x), debug[y, x, :3], want_debug[y, x, :3]))
    bad = np.argwhere((color != want_color).any(axis=-1))
    if len(bad):
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} texels of the UNORM16 colour differ from the oracle; first:\n" +
                             describe_mismatch(group, L, int(y), int(x), color[y, x], want_color[y, x]))


def run_group(gpu, group, L, padded):
    W, H = group.extent
    inp, spots, maps, planes = lg.frame_inputs(group, L)
    cameras = gpu.pl.TStagedBuffer(abi.CameraPacked, 1)
    dirs = gpu.pl.TStagedBuffer(abi.DirectionalLightPacked, 2)
    cameras.push(inp.cam)
    dirs.push([inp.sun, inp.moon])
    cameras.recordCopyToDevice()
    dirs.recordCopyToDevice()
    capacity = (W + CAPACITY_EXTRA[0], H + CAPACITY_EXTRA[1]) if padded else (W, H)
    deferred = gpu.pl.DeferredShadingPipeline(capacity, max_spot_lights=len(group.light_names), max_shadow_maps=group.slot_count)
    try:
        if padded:
            deferred.upload_gbuffer(pi.gbuffer_poison(*capacity))
        deferred.upload_gbuffer(planes)
        keep = []
        for slot, m in maps.items():
            im = pi.PaddedImage(abi.SZG_FORMAT_D32_SFLOAT, lg.MAP_W, lg.MAP_H, lg.MAP_PAD, pi.NEAREST_OCCLUDER).to_device(gpu.torch)
            im.write_inside(np.ascontiguousarray(m))
            deferred.setShadowMap(slot, im.device.view(gpu.torch.float32)[:, : im.cap_w])
            keep.append(im)
        if padded:
            target = pi.PaddedScene(gpu.torch, capacity[0], capacity[1], SCENE_PADS)
        else:
            target = gpu.pl.SceneTexture(W, H, debug=True)
        deferred.recordLights(None, inp.rect, target, group.skip, dirs, spots, 0, cameras)
        gpu.torch.cuda.synchronize()
        if padded:
            debug, color = target.debug.inside((W, H)), target.color.inside((W, H))
            target.debug.assert_outside_untouched((W, H), f"{group.name}: debug colour")
            target.color.assert_outside_untouched((W, H), f"{group.name}: colour")
            target.depth.assert_untouched(f"{group.name}: depth (not an output of this pass)")
            got = deferred.download_gbuffer(*capacity)
            poison = pi.gbuffer_poison(*capacity)
            for name, plane in got.items():  # the pass only reads the G-buffer
                want = poison[name]
                want[:H, :W] = planes[name]
                assert (np.ascontiguousarray(plane).view(np.uint8) == want.view(np.uint8)).all(), f"{group.name}: gbuffer.{name} changed"
        else:
            debug, color = target.debug.cpu().numpy(), target.color_numpy()
        for im in keep:
            im.assert_untouched(f"{group.name}: shadow map")
        assert_same_image(group, L, debug, color, f"{group.name}{' (padded images)' if padded else ''}")
    finally:
        deferred.cleanup()


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("family", lg.FAMILIES)
def test_gate_family_is_bit_identical_to_the_oracle(gpu, family, padded):
    L, _ = built()
    groups = groups_of(family)
    assert groups
    for g in groups:
        run_group(gpu, g, L, padded)

