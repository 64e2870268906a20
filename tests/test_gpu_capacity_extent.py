"""GPU: every pass of the deferred path on images allocated LARGER than the draw extent - the engine's normal configuration
(the reference allocates its scene texture and G-buffer at 4096^2 and draws into the top-left drawExtent of them;
include/szg/abi.h: szg_image.width / height are the allocated extent, pitch_bytes is explicit, szg_deferred_desc is a capacity).

For each pass: one run into tight images as every other test does, one run from the same inputs into capacity / pitch-padded
images (tests/padded_images.py) through the same library. Then
  * inside the draw rect the padded run equals the tight run bit for bit (the allocated size cannot change a value:
    tests/test_padded_images.py checks the reference's (texel + 0.5) / allocatedExtent in float32),
  * the tight run carries the oracle / model assertions of the pass's own parity test, which pins both,
  * outside the draw rect every byte of every image the pass may write or only reads, pitch padding included, still holds its
    sentinel. The sentinels are hostile when read (NaN geometry, nearest-occluder shadow padding), so a read past the rect or
    with a wrong pitch shows inside it.
The last part: malformed images are refused with SZG_ERR_INVALID_ARGUMENT before anything is written."""
import ctypes as C
import functools

import numpy as np
import pytest

from syzygy_amd import abi, lib
from tests import debuglines_model as dm
from tests import padded_images as pi
from tests import raster_scenes as rs
from tests import util
from tests.util import assert_close

pytestmark = pytest.mark.gpu

LUT = ((128, 32), (128, 64))
# (draw rect, scene-texture capacity, G-buffer capacity, scene pitches padded)
SHAPES = [
    ((70, 37), (96, 48), (80, 40), True),   # ragged in both axes; whole extra workgroups fit in the capacity; capacities differ
    ((33, 9), (64, 16), (64, 16), False),   # one texel past a 32x8 workgroup in each axis
    ((32, 8), (40, 9), (40, 9), False),     # exactly one workgroup; capacity not a multiple of anything
    ((1, 1), (16, 16), (16, 16), True),     # one live lane
    ((70, 37), (70, 37), (70, 37), True),   # extent = capacity, every pitch padded by a different odd number of texels
]
SHAPE_IDS = [f"{r[0]}x{r[1]}-in-{s[0]}x{s[1]}" + ("-padded" if p else "") for r, s, _, p in SHAPES]
SCENE_PADS = (3, 5, 1)  # colour, depth, debug colour: texels of row padding
shapes = pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    from oracle import binding as ob
    from syzygy_amd import pipelines

    class Ctx:
        pass

    c = Ctx()
    c.torch, c.pl, c.ob = torch, pipelines, ob
    return c


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def staged(gpu, inp):
    cameras = gpu.pl.TStagedBuffer(abi.CameraPacked, 1)
    atmospheres = gpu.pl.TStagedBuffer(abi.AtmospherePacked, 1)
    lights = gpu.pl.TStagedBuffer(abi.DirectionalLightPacked, 2)
    cameras.push(inp.cam)
    atmospheres.push(inp.atm)
    lights.push([inp.sun, inp.moon])
    for b in (cameras, atmospheres, lights):
        b.recordCopyToDevice()
    return cameras, atmospheres, lights


def padded_scene(gpu, shape):
    _, scap, _, padded = shape
    return pi.PaddedScene(gpu.torch, scap[0], scap[1], SCENE_PADS if padded else (0, 0, 0))


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got.view(np.uint8) != want.view(np.uint8))
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ from the tight run, first {bad[:4].tolist()}"


def tight_scene_arrays(gpu, target):
    gpu.torch.cuda.synchronize()
    return {"color": target.color_numpy(), "depth": target.depth.cpu().numpy(),
            "debug_color": target.debug.cpu().numpy() if target.debug is not None else None}


def check_scene(scene, tight, extent, written, what):
    """Images in `written`: inside the rect bit-equal to the tight run's, outside untouched. The others: untouched."""
    for name, im in scene.images().items():
        if name in written:
            same_bits(im.inside(extent), tight[name], f"{what}: {name}")
            im.assert_outside_untouched(extent, f"{what}: {name}")
        else:
            im.assert_untouched(f"{what}: {name} (not an output of this pass)")


def poison_pipeline_gbuffer(deferred, gcap):
    deferred.upload_gbuffer(pi.gbuffer_poison(gcap[0], gcap[1]))


def check_pipeline_gbuffer(deferred, gcap, tight, extent, what):
    """The planes a pipeline owns (tight pitch at its capacity `gcap`): inside `extent` bit-equal to `tight` (the planes of the
    tight run, or the planes uploaded for a pass that only reads them), outside still the poison."""
    got = deferred.download_gbuffer(gcap[0], gcap[1])
    poison = pi.gbuffer_poison(gcap[0], gcap[1])
    w, h = extent
    for name, plane in got.items():
        same_bits(plane[:h, :w], tight[name][:h, :w], f"{what}: gbuffer.{name}")
        outside = np.ones((gcap[1], gcap[0]), bool)
        outside[:h, :w] = False
        bits = np.uint16 if plane.dtype == np.float16 else np.uint32
        changed = np.argwhere((plane.view(bits) != poison[name].view(bits)).any(axis=-1) & outside)
        assert len(changed) == 0, f"{what}: gbuffer.{name}: {len(changed)} texels outside the draw rect changed, first {changed[:4].tolist()}"


def oracle_planes_equal(got, want, what):
    for name, a in got.items():
        b = want[name]
        bits = np.uint16 if a.dtype == np.float16 else np.uint32
        same = (a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))
        assert same.all(), f"{what}: {name} differs from the oracle at {(~same).sum()} values"


@functools.lru_cache(maxsize=None)
def oracle_luts(elevation, extent):
    from oracle import binding as ob

    inp = util.Inputs(extent[0], extent[1], elevation_degrees=elevation)
    tlut = ob.transmittance_lut(inp.atm, LUT[0][0], LUT[0][1], threads=8)
    slut = ob.skyview_lut(inp.atm, inp.cam, tlut, LUT[1][0], LUT[1][1], threads=8)
    tlut.setflags(write=False)
    slut.setflags(write=False)
    return tlut, slut


def padded_shadow_map(gpu, depth_map, pad):
    """A caller-owned D32F map whose rows are `pad` texels wider than the map, the padding filled with 1.0 - the nearest
    possible occluder, so a sampler that takes the width for the pitch (or the pitch for the width) darkens pixels."""
    h, w = depth_map.shape
    im = pi.PaddedImage(abi.SZG_FORMAT_D32_SFLOAT, w, h, pad, pi.NEAREST_OCCLUDER).to_device(gpu.torch)
    im.write_inside(depth_map)
    return im


def strided_tensor(im):
    """The [h, w] float32 view of a padded D32F image: what DeferredShadingPipeline.setShadowMap takes."""
    return im.device.view(im.torch.float32)[:, : im.cap_w]


# ---------------------------------------------------------------------------
# 1. recordGBufferFill: five planes + depth
# ---------------------------------------------------------------------------
@shapes
def test_gbuffer_fill(gpu, shape):
    (W, H), scap, gcap, _ = shape
    inp = util.Inputs(W, H)
    cameras, _, _ = staged(gpu, inp)
    target = gpu.pl.SceneTexture(W, H, debug=True)
    deferred = gpu.pl.DeferredShadingPipeline((W, H), max_spot_lights=1, max_shadow_maps=0)
    deferred.recordGBufferFill(None, inp.rect, target, 0, cameras, inp.synthetic.fill)
    tight = tight_scene_arrays(gpu, target)
    tight_planes = deferred.download_gbuffer(W, H)
    deferred.cleanup()
    frame = gpu.ob.HostFrame(W, H)  # tests/test_gpu_parity.py test_gbuffer_fill_bit_exact
    gpu.ob.gbuffer_fill(frame, inp.rect, None, inp.cam, inp.synthetic.fill, threads=4)
    for name, want in frame.planes().items():
        assert (tight_planes[name].view(np.uint8) == want.view(np.uint8)).all(), name
    assert (tight["depth"].view(np.uint32) == frame.depth.view(np.uint32)).all()

    scene = padded_scene(gpu, shape)
    deferred = gpu.pl.DeferredShadingPipeline(gcap, max_spot_lights=1, max_shadow_maps=0)
    poison_pipeline_gbuffer(deferred, gcap)
    deferred.recordGBufferFill(None, inp.rect, scene, 0, cameras, inp.synthetic.fill)
    check_scene(scene, tight, (W, H), {"depth"}, "G-buffer fill")
    check_pipeline_gbuffer(deferred, gcap, tight_planes, (W, H), "G-buffer fill")
    deferred.cleanup()


# ---------------------------------------------------------------------------
# 2. recordGBufferRaster: triangles that extend past the right and bottom edges of the draw rect, inside the capacity
# ---------------------------------------------------------------------------
def raster_meshes(W, H, scap):
    """A seeded soup (ordinary, sliver, sub-pixel and far-outside triangles, tests/raster_scenes.py) for the exact
    perspective camera (clip = (x, y, 1/4, z)), plus two triangles whose far corners lie at the last column / row of the
    CAPACITY image: without the scissor at the draw rect (deferred.cpp:493-713) they would fill columns W.. and rows H.. ."""
    soup = rs.soup(41, 18, W, H).reshape(-1, 3, 3)
    soup = soup[np.arange(len(soup)) % 6 != 4].reshape(-1, 3)  # without the viewport-filling ones: background texels stay
    xr, yb = 2.0 * (scap[0] - 0.5) / W - 1.0, 2.0 * (scap[1] - 0.5) / H - 1.0
    past = np.array([[-0.6, -0.7, 1.0], [xr, -0.3, 1.0], [-0.2, yb, 1.0],
                     [0.1, 0.2, 2.0], [xr * 2.0, yb * 2.0, 2.0], [-0.9 * 2.0, yb * 2.0, 2.0]], np.float32)
    pos = np.concatenate([soup, past])
    idx = np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)
    idx = np.concatenate([idx, idx[:, ::-1]])  # both windings
    return [rs.mesh_of(pos, idx)]


@shapes
def test_gbuffer_raster(gpu, shape):
    (W, H), scap, gcap, _ = shape
    cam = rs.exact_perspective_camera()
    cameras = gpu.pl.TStagedBuffer(abi.CameraPacked, 1)
    cameras.push(cam)
    cameras.recordCopyToDevice()
    ms = raster_meshes(W, H, scap)
    rect = abi.Rect(0, 0, W, H)
    target = gpu.pl.SceneTexture(W, H, debug=True)
    deferred = gpu.pl.DeferredShadingPipeline((W, H), max_spot_lights=1, max_shadow_maps=0)
    deferred.recordGBufferRaster(None, rect, target, 0, cameras, ms)
    tight = tight_scene_arrays(gpu, target)
    tight_planes = deferred.download_gbuffer(W, H)
    deferred.cleanup()
    frame = gpu.ob.HostFrame(W, H, debug=False)  # tests/test_gpu_raster_exact.py KernelBackend.gbuffer
    gpu.ob.gbuffer_raster(frame, rect, None, cam, ms, threads=1)
    assert (tight["depth"].view(np.uint32) == frame.depth.view(np.uint32)).all(), "kernel depth differs from the oracle"
    oracle_planes_equal(tight_planes, frame.planes(), "G-buffer raster")
    assert W * H == 1 or (tight["depth"] > 0).any()
    if (scap[0] > W or scap[1] > H) and W > 1:
        # the case does what it is for: the last column and the last row of the draw rect are covered, so the triangles go on past them
        assert (tight["depth"][:, W - 1] > 0).any() and (tight["depth"][H - 1, :] > 0).any()

    scene = padded_scene(gpu, shape)
    deferred = gpu.pl.DeferredShadingPipeline(gcap, max_spot_lights=1, max_shadow_maps=0)
    poison_pipeline_gbuffer(deferred, gcap)
    deferred.recordGBufferRaster(None, rect, scene, 0, cameras, ms)
    check_scene(scene, tight, (W, H), {"depth"}, "G-buffer raster")
    check_pipeline_gbuffer(deferred, gcap, tight_planes, (W, H), "G-buffer raster")
    deferred.cleanup()


# ---------------------------------------------------------------------------
# 3. recordLights: 0, 1 and 24 spots, caller-owned non-square shadow maps with padded rows
# ---------------------------------------------------------------------------
def light_shadow_maps(spots):
    rng = np.random.default_rng(0x5A2C + spots)
    maps = {1: rng.random((33, 47), dtype=np.float32)}  # the moon
    if spots >= 1:
        maps[2] = (rng.random((40, 64), dtype=np.float32) > 0.5).astype(np.float32) * np.float32(0.9999)
    if spots >= 24:
        maps[9] = rng.random((21, 9), dtype=np.float32)
        maps[25] = rng.random((64, 31), dtype=np.float32)
    return maps


@pytest.mark.parametrize("spots", [0, 1, 24])
@shapes
def test_lights(gpu, shape, spots):
    (W, H), scap, gcap, _ = shape
    skip = 1
    inp = util.Inputs(W, H, spots=spots)
    cameras, _, lights = staged(gpu, inp)
    frame = gpu.ob.HostFrame(W, H)
    gpu.ob.gbuffer_fill(frame, inp.rect, None, inp.cam, inp.synthetic.fill, threads=8)
    planes = {k: v.copy() for k, v in frame.planes().items()}
    maps = light_shadow_maps(spots)
    images = (abi.Image * (spots + 2))()
    for slot, m in maps.items():
        images[slot] = gpu.ob.host_image(m, abi.SZG_FORMAT_D32_SFLOAT)
    shadow_host = abi.ShadowMaps(spots + 2, 0, C.cast(images, C.POINTER(abi.Image)))
    gpu.ob.lights(frame, inp.rect, None, shadow_host, inp.cam, inp.dirs, 2, skip, inp.spots, spots, threads=8)

    def run(target, capacity, attach):
        deferred = gpu.pl.DeferredShadingPipeline(capacity, max_spot_lights=max(spots, 1), max_shadow_maps=spots + 2)
        if capacity != (W, H):
            poison_pipeline_gbuffer(deferred, capacity)
        deferred.upload_gbuffer(planes)
        keep = [attach(deferred, slot, m) for slot, m in maps.items()]
        deferred.recordLights(None, inp.rect, target, skip, lights, inp.spots if spots else None, 0, cameras)
        gpu.torch.cuda.synchronize()
        return deferred, keep

    def attach_tight(deferred, slot, m):
        t = gpu.torch.from_numpy(m).cuda()
        deferred.setShadowMap(slot, t)
        return t

    target = gpu.pl.SceneTexture(W, H, debug=True)
    deferred, _ = run(target, (W, H), attach_tight)
    tight = tight_scene_arrays(gpu, target)
    deferred.cleanup()
    # tests/test_gpu_parity.py test_lights_match_oracle / test_lights_with_shadow_maps
    assert_close(tight["debug_color"], frame.debug, what=f"lights {W}x{H} spots={spots}")
    assert np.abs(tight["color"].astype(np.int32) - frame.color.astype(np.int32)).max() <= 1
    assert (tight["color"][..., 3] == 65535).all()

    def attach_padded(deferred, slot, m):
        im = padded_shadow_map(gpu, m, pad=2 * slot + 3)
        deferred.setShadowMap(slot, strided_tensor(im))
        return im

    scene = padded_scene(gpu, shape)
    deferred, padded_maps = run(scene, gcap, attach_padded)
    sm = deferred.shadowMaps()
    for im, (slot, m) in zip(padded_maps, maps.items()):  # setShadowMap passed the row stride on as the pitch
        got = sm.maps[slot]
        assert (got.width, got.height, got.pitch_bytes, got.data) == (m.shape[1], m.shape[0], im.pitch_bytes, im.device.data_ptr())
    check_scene(scene, tight, (W, H), {"color", "debug_color"}, f"lights spots={spots}")
    if gcap != (W, H):
        check_pipeline_gbuffer(deferred, gcap, planes, (W, H), f"lights spots={spots}")
    for im in padded_maps:
        im.assert_untouched("lights: shadow map")
    deferred.cleanup()


def test_set_shadow_map_of_a_tight_tensor_is_the_image_it_always_was(gpu):
    deferred = gpu.pl.DeferredShadingPipeline((8, 8), max_spot_lights=1, max_shadow_maps=3)
    for slot, (h, w) in enumerate([(33, 47), (1, 5), (6, 1)]):
        t = gpu.torch.zeros((h, w), dtype=gpu.torch.float32, device="cuda")
        deferred.setShadowMap(slot, t)
        im = deferred.shadowMaps().maps[slot]
        assert (im.data, im.width, im.height, im.pitch_bytes, im.format) == (t.data_ptr(), w, h, w * 4, abi.SZG_FORMAT_D32_SFLOAT)
    wide = gpu.torch.zeros((6, 10), dtype=gpu.torch.float32, device="cuda")
    deferred.setShadowMap(0, wide[:, :7])
    im = deferred.shadowMaps().maps[0]
    assert (im.width, im.height, im.pitch_bytes) == (7, 6, 40)
    with pytest.raises(ValueError):
        deferred.setShadowMap(0, wide[:, ::2])  # texels of a row must be contiguous
    deferred.setShadowMap(0, None)
    assert not deferred.shadowMaps().maps[0].data
    deferred.cleanup()


# ---------------------------------------------------------------------------
# 4. recordComposite / recordCompositeFast: caller-built G-buffer (five pitches, its own capacity), padded sun shadow map,
#    prior colour read from the padded colour image
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@shapes
def test_composite(gpu, shape, fast):
    (W, H), scap, gcap, _ = shape
    elevation, spots = 35.0, 8  # the conditions of tests/test_gpu_parity.py test_fast_composite_is_close_to_the_exact_one
    inp = util.Inputs(W, H, elevation_degrees=elevation, spots=spots)
    cameras, atmospheres, lights = staged(gpu, inp)
    frame = gpu.ob.HostFrame(W, H)
    gpu.ob.gbuffer_fill(frame, inp.rect, None, inp.cam, inp.synthetic.fill, threads=8)
    gpu.ob.lights(frame, inp.rect, None, None, inp.cam, inp.dirs, 2, 1, inp.spots, spots, threads=8)
    prior, depth = frame.color.copy(), frame.depth.copy()
    planes = {k: v.copy() for k, v in frame.planes().items()}
    tlut, slut = oracle_luts(elevation, (W, H))
    sun_map = np.random.default_rng(7).random((31, 48), dtype=np.float32)

    sky = gpu.pl.SkyViewComputePipeline.create(transmittance_extent=LUT[0], skyview_extent=LUT[1])
    sky.upload_lut(sky.transmittanceLUT(), tlut)
    sky.upload_lut(sky.skyviewLUT(), slut)
    if fast:
        sky.recordAerialLUT(None, 0, atmospheres, 0, cameras, 10.0e-3)  # 10 km
    record = sky.recordCompositeFast if fast else sky.recordComposite

    # tight: the pipeline's own G-buffer and a tight map, as tests/test_gpu_parity.py run_composite_case does
    deferred = gpu.pl.DeferredShadingPipeline((W, H), max_spot_lights=1, max_shadow_maps=1)
    deferred.upload_gbuffer(planes)
    t = gpu.torch.from_numpy(sun_map).cuda()
    deferred.setShadowMap(0, t)

    def tight_run(call):
        target = gpu.pl.SceneTexture(W, H, debug=True)
        target.color.copy_(gpu.torch.from_numpy(prior.view(np.int16)))
        target.depth.copy_(gpu.torch.from_numpy(depth))
        call(None, target, inp.rect, deferred.gbuffer(), deferred.shadowMaps(), 0, atmospheres, 0, cameras, 0, lights)
        return tight_scene_arrays(gpu, target)

    tight = tight_run(record)
    if fast:
        # The fast mode is approximate by design: its tight run is held to the EXACT composite's tight run (which the other half of
        # this test pins to the oracle) with the bounds of test_fast_composite_is_close_to_the_exact_one. Bit for bit it is
        # pinned to the oracle's fast composite by tests/test_gpu_fast_composite.py.
        a, b = tight_run(sky.recordComposite)["debug_color"], tight["debug_color"]
        geo = depth > 0
        assert (a[~geo].view(np.uint32) == b[~geo].view(np.uint32)).all(), "sky pixels must be untouched by the fast mode"
        if geo.any():
            rel = util.rel_err(a[geo][:, :3], b[geo][:, :3], util.ATOL_COLOR)
            print(f"fast composite vs exact at {W}x{H}: max rel {rel.max():.3e}, mean rel {rel.mean():.3e} over {geo.sum()} geometry pixels")
            assert rel.max() < 5e-2 and rel.mean() < 5e-3
    deferred.cleanup()
    if not fast:  # test_composite_matches_oracle / test_composite_with_sun_shadow_map (the fast mode: tests/test_gpu_fast_composite.py)
        images = (abi.Image * 1)(gpu.ob.host_image(sun_map, abi.SZG_FORMAT_D32_SFLOAT))
        gpu.ob.composite(frame, inp.rect, None, abi.ShadowMaps(1, 0, C.cast(images, C.POINTER(abi.Image))), inp.atm, inp.cam, inp.dirs, 0,
                         tlut, slut, threads=8)
        assert_close(tight["debug_color"], frame.debug, what=f"composite {W}x{H}")
        assert np.abs(tight["color"].astype(np.int32) - frame.color.astype(np.int32)).max() <= 1

    scene = padded_scene(gpu, shape)
    scene.color.write_inside(prior)
    scene.depth.write_inside(depth)
    gbuffer = pi.PaddedGBuffer(gpu.torch, gcap[0], gcap[1])
    gbuffer.write_inside(planes)
    assert len({im.pitch_bytes // im.texel for im in gbuffer.planes.values()}) == 5
    sun = padded_shadow_map(gpu, sun_map, pad=5)
    sun_images = (abi.Image * 1)(sun.image())
    record(None, scene, inp.rect, gbuffer.abi(), abi.ShadowMaps(1, 0, C.cast(sun_images, C.POINTER(abi.Image))), 0, atmospheres, 0, cameras,
           0, lights)
    check_scene(scene, tight, (W, H), {"color", "debug_color"}, "composite")
    for name, im in gbuffer.planes.items():
        im.assert_untouched(f"composite: gbuffer.{name}")
    sun.assert_untouched("composite: sun shadow map")
    sky.destroy()


# ---------------------------------------------------------------------------
# 5. the chained frame with GPU LUTs, whole and row-tiled (3 ranks, blocks of 4 rows) into targets taller than the tile
# ---------------------------------------------------------------------------
def chain(gpu, inp, target, capacity, tile):
    cameras, atmospheres, lights = staged(gpu, inp)
    deferred = gpu.pl.DeferredShadingPipeline(capacity, max_spot_lights=max(inp.spot_count, 1), max_shadow_maps=0)
    poison_pipeline_gbuffer(deferred, capacity)
    sky = gpu.pl.SkyViewComputePipeline.create(transmittance_extent=LUT[0], skyview_extent=LUT[1])
    deferred.recordDrawCommands(None, inp.rect, target, 1, lights, inp.spots if inp.spot_count else None, 0, cameras,
                                inp.synthetic.fill, tile=tile)
    sky.recordDrawCommands(None, target, inp.rect, deferred.gbuffer(), deferred.shadowMaps(), 0, atmospheres, 0, cameras, 0, lights,
                           tile=tile)
    gpu.torch.cuda.synchronize()
    sky.destroy()
    return deferred


@pytest.mark.parametrize("tiled", [False, True], ids=["whole", "3-ranks"])
@shapes
def test_chained_frame(gpu, shape, tiled):
    (W, H), scap, gcap, _ = shape
    elevation = 25.0
    inp = util.Inputs(W, H, elevation_degrees=elevation, spots=8)
    # the whole frame, tight, against the oracle: tests/test_gpu_parity.py test_generic_path_unusual_atmospheres' assertions
    full_target = gpu.pl.SceneTexture(W, H, debug=True)
    chain(gpu, inp, full_target, (W, H), None).cleanup()
    full = tight_scene_arrays(gpu, full_target)
    frame = gpu.ob.HostFrame(W, H)
    gpu.ob.gbuffer_fill(frame, inp.rect, None, inp.cam, inp.synthetic.fill, threads=8)
    gpu.ob.lights(frame, inp.rect, None, None, inp.cam, inp.dirs, 2, 1, inp.spots, inp.spot_count, threads=8)
    tlut, slut = oracle_luts(elevation, (W, H))
    gpu.ob.composite(frame, inp.rect, None, None, inp.atm, inp.cam, inp.dirs, 0, tlut, slut, threads=8)
    assert_close(full["debug_color"], frame.debug, what=f"full frame {W}x{H}")
    assert np.abs(full["color"].astype(np.int32) - frame.color.astype(np.int32)).max() <= 1

    for rank in range(3 if tiled else 1):
        tile = util.rowtile(H, 4, rank, 3) if tiled else None
        rows = util.global_rows(H, 4, rank, 3) if tiled else np.arange(H)
        n = len(rows)
        what = f"chained frame, rank {rank} of 3" if tiled else "chained frame"
        tight_planes = None
        if n > 0:
            target = gpu.pl.SceneTexture(W, n, debug=True)
            deferred = chain(gpu, inp, target, (W, n), tile)
            tight = tight_scene_arrays(gpu, target)
            tight_planes = deferred.download_gbuffer(W, n)
            deferred.cleanup()
            # test_rowtiles_equal_full_frame_bit_exact: a rank's tile is its rows of the whole frame
            assert (tight["color"] == full["color"][rows]).all()
            assert (tight["debug_color"].view(np.uint32) == full["debug_color"][rows].view(np.uint32)).all()
        scene = padded_scene(gpu, shape)  # taller than the tile's local rows, wider than the draw
        assert not tiled or scene.color.cap_h > n or H == 1
        deferred = chain(gpu, inp, scene, gcap, tile)
        if n > 0:
            check_scene(scene, tight, (W, n), {"color", "depth", "debug_color"}, what)
            check_pipeline_gbuffer(deferred, gcap, tight_planes, (W, n), what)
        else:  # more ranks than row blocks: this rank holds nothing and writes nothing
            check_scene(scene, None, (W, 0), set(), what)
            check_pipeline_gbuffer(deferred, gcap, pi.gbuffer_poison(*gcap), (0, 0), what)
        deferred.cleanup()


# ---------------------------------------------------------------------------
# 6. debug lines whose pixels would fall in columns W .. cap_w - 1 and rows H .. cap_h - 1
# ---------------------------------------------------------------------------
def lines_past_the_rect(W, H, scap):
    cw, ch = scap
    seg = np.array([
        [0.5, 0.5, cw - 0.5, ch - 0.5],               # the diagonal of the CAPACITY image
        [-3.0, H - 0.5, cw + 3.0, H - 0.5],           # along the last row of the rect and on through the capacity columns
        [W - 0.5, -3.0, W - 0.5, ch + 3.0],           # down the last column and on through the capacity rows
        [W + 0.5, 0.5, cw - 0.5, max(H - 1.5, 0.5)],  # entirely right of the rect
        [0.5, H + 0.5, max(W - 1.5, 0.5), ch - 0.5],  # entirely below it
        [W - 2.0, H - 2.0, W + 2.0, H + 2.0],         # across the corner
        [0.25, 0.75, W * 0.5, H * 0.5],
    ], np.float64)
    p = seg.reshape(-1, 2)
    out = np.empty((len(p), 3), np.float32)
    out[:, 0], out[:, 1], out[:, 2] = p[:, 0] / (W / 2) - 1, p[:, 1] / (H / 2) - 1, 0.5
    return out


def identity_camera():
    cam = abi.CameraPacked()
    eye = np.eye(4, dtype=np.float32)
    for name in ("projection", "inverseProjection", "view", "viewInverseTranspose", "rotation", "projViewInverse"):
        setattr(cam, name, abi.Mat4.from_numpy(eye))
    return cam


def record_debug_lines(gpu, scene_texture, positions, W, H, width):
    handle = C.c_void_p()
    assert lib().szg_debug_lines_create(C.byref(handle), max(len(positions), 2), 0) == abi.SZG_OK, lib().szg_last_error()
    d_cam = gpu.torch.from_numpy(np.frombuffer(bytes(identity_camera()), np.uint8).copy()).cuda()
    v = np.zeros((len(positions), 12), np.float32)
    v[:, 0:3] = positions
    v[:, 8:12] = [1, 0, 0, 1]
    d_v = gpu.torch.from_numpy(v).cuda()
    status = lib().szg_debug_lines_record(handle, None, C.c_float(width), abi.Rect(0, 0, W, H), None, C.byref(scene_texture), 0,
                                          C.c_void_p(d_cam.data_ptr()), C.c_void_p(d_v.data_ptr()), len(positions))
    gpu.torch.cuda.synchronize()
    lib().szg_debug_lines_destroy(handle)
    return status


@pytest.mark.parametrize("width", [1.0, 3.0])
@shapes
def test_debug_lines(gpu, shape, width):
    (W, H), scap, _, _ = shape
    positions = lines_past_the_rect(W, H, scap)
    scene = padded_scene(gpu, shape)
    # the tight run draws over the same prior colour: the sentinel
    color0 = scene.color.typed(scene.color.host, scap)[:H, :W].copy()
    debug0 = scene.debug.typed(scene.debug.host, scap)[:H, :W].copy()
    target = gpu.pl.SceneTexture(W, H, debug=True)
    target.color.copy_(gpu.torch.from_numpy(color0.view(np.int16)))
    target.debug.copy_(gpu.torch.from_numpy(debug0))
    assert record_debug_lines(gpu, target.abi(), positions, W, H, width) == abi.SZG_OK, lib().szg_last_error()
    tight = tight_scene_arrays(gpu, target)
    mask = dm.model(identity_camera(), positions, W, H, width, brute=True)  # tests/test_gpu_debuglines.py check()
    want_color, want_debug = dm.render(mask, color0, debug0)
    assert np.array_equal(tight["color"], want_color), f"{(tight['color'] != want_color).any(axis=-1).sum()} texels differ from the model"
    assert np.array_equal(tight["debug_color"].view(np.uint32), want_debug.view(np.uint32))
    assert W == 1 or (mask[H - 1].any() and mask[:, W - 1].any())  # the lines do reach the last row and column of the rect
    assert (tight["depth"] == 0).all()

    assert record_debug_lines(gpu, scene.abi(), positions, W, H, width) == abi.SZG_OK, lib().szg_last_error()
    check_scene(scene, tight, (W, H), {"color", "debug_color"}, f"debug lines, width {width}")


# ---------------------------------------------------------------------------
# 7. szg_compose_rowtiles into a destination wider and taller than the frame, pitch padded to another multiple of 16 bytes
# ---------------------------------------------------------------------------
@shapes
def test_compose_rowtiles(gpu, shape):
    """The compose kernel copies 16 bytes per lane and szg_compose_rowtiles refuses a frame whose rows are no multiple of 16
    bytes, i.e. an odd width (api_core.cpp). At the two odd-width shapes of the table, 33x9 and 1x1, this pass therefore has
    no inside-the-rect comparison: what is asserted there is that the tight and the padded call are both refused and that the
    padded destination keeps every byte. The even-width shapes carry the full comparison."""
    (W, H), scap, _, _ = shape
    nranks, block_rows = 3, 4
    rng = np.random.default_rng(W * 100 + H)
    full = rng.integers(0, 65536, (H, W, 4), dtype=np.uint16)
    stride_rows = max(len(util.global_rows(H, block_rows, r, nranks)) for r in range(nranks))
    buf = np.zeros((nranks, stride_rows, W, 4), np.uint16)
    for r in range(nranks):
        rows = util.global_rows(H, block_rows, r, nranks)
        buf[r, : len(rows)] = full[rows]
    d_buf = gpu.torch.from_numpy(buf.view(np.int16)).cuda()
    dst = pi.PaddedImage(abi.SZG_FORMAT_RGBA16_UNORM, scap[0], scap[1], 2 + scap[0] % 2, pi.POISON_COLOR).to_device(gpu.torch)
    assert dst.pitch_bytes % 16 == 0 and dst.pitch_bytes > scap[0] * 8
    tight = gpu.torch.zeros((H, W, 4), dtype=gpu.torch.int16, device="cuda")

    def compose(image):
        status = lib().szg_compose_rowtiles(None, C.c_void_p(d_buf.data_ptr()), stride_rows * W * 8, nranks, block_rows, C.byref(image), W, H)
        gpu.torch.cuda.synchronize()
        return status

    tight_status = compose(abi.Image(tight.data_ptr(), W, H, W * 8, abi.SZG_FORMAT_RGBA16_UNORM))
    status = compose(dst.image())
    if W % 2:  # rows of the frame must be multiples of 16 bytes (api_core.cpp): an odd width is refused, whatever the allocation
        assert tight_status == status == abi.SZG_ERR_INVALID_ARGUMENT
        dst.assert_untouched("compose, refused")
        return
    assert tight_status == status == abi.SZG_OK, lib().szg_last_error()
    got_tight = tight.cpu().numpy().view(np.uint16)
    assert (got_tight == full).all()  # test_rowtiles_equal_full_frame_bit_exact's last assertion
    same_bits(dst.inside((W, H)), got_tight, "compose")
    dst.assert_outside_untouched((W, H), "compose")


# ---------------------------------------------------------------------------
# Refusals write nothing
# ---------------------------------------------------------------------------
class Described:
    """What the pipelines' record methods take as scene texture: anything with abi()."""

    def __init__(self, st):
        self.st = st

    def abi(self):
        return self.st


def shrink(image, width=None, height=None):
    if width is not None:
        image.width = width
    if height is not None:
        image.height = height


def off_by_two(image):
    image.data = image.data + 2


# (name, mutation of (scene texture, caller G-buffer), word of the error text, applies to)
W0, H0 = 70, 37
REFUSALS = [
    ("colour pitch of the draw width on a capacity-wide image", lambda st, g: setattr(st.color, "pitch_bytes", W0 * 8), "scene_texture.color", "color"),
    ("colour pitch one texel short of the allocated width", lambda st, g: setattr(st.color, "pitch_bytes", (st.color.width - 1) * 8), "scene_texture.color", "color"),
    ("colour pitch not a multiple of the texel size", lambda st, g: setattr(st.color, "pitch_bytes", st.color.pitch_bytes + 4), "scene_texture.color", "color"),
    ("debug pitch not a multiple of the texel size", lambda st, g: setattr(st.debug_color, "pitch_bytes", st.debug_color.pitch_bytes + 8), "scene_texture.debug_color", "color"),
    ("colour pointer off by 2 bytes", lambda st, g: off_by_two(st.color), "scene_texture.color", "color"),
    ("debug pointer off by 2 bytes", lambda st, g: off_by_two(st.debug_color), "scene_texture.debug_color", "color"),
    ("debug_color narrower than the rect", lambda st, g: shrink(st.debug_color, width=W0 - 1), "scene_texture.debug_color", "color"),
    ("debug_color shorter than the rect", lambda st, g: shrink(st.debug_color, height=H0 - 1), "scene_texture.debug_color", "color"),
    ("depth narrower than the rect", lambda st, g: shrink(st.depth, width=W0 - 1), "scene_texture.depth", "depth"),
    ("depth shorter than the rect", lambda st, g: shrink(st.depth, height=H0 - 1), "scene_texture.depth", "depth"),
    ("depth pitch smaller than its width", lambda st, g: setattr(st.depth, "pitch_bytes", W0 * 4), "scene_texture.depth", "depth"),
    ("depth pointer off by 2 bytes", lambda st, g: off_by_two(st.depth), "scene_texture.depth", "depth"),
    ("normal plane narrower than the rect", lambda st, g: shrink(g.normal, width=W0 - 1), "gbuffer.normal", "gbuffer"),
    ("position plane shorter than the rect", lambda st, g: shrink(g.worldPosition, height=H0 - 1), "gbuffer.worldPosition", "gbuffer"),
    ("ORM plane pitch of the draw width", lambda st, g: setattr(g.occlusionRoughnessMetallic, "pitch_bytes", W0 * 8), "gbuffer.occlusionRoughnessMetallic", "gbuffer"),
    ("diffuse pointer off by 2 bytes", lambda st, g: off_by_two(g.diffuse), "gbuffer.diffuse", "gbuffer"),
]


def test_refusals_write_nothing(gpu):
    """Every record entry point with one malformed image at a time: SZG_ERR_INVALID_ARGUMENT that names the image, and every
    byte of every image - scene texture, caller G-buffer, the pipeline's own planes - still at its sentinel, also for the
    calls that chain passes (a frame whose lights pass is refused must not have had its G-buffer and depth rewritten first).

    The images are allocated 4 rows taller than they are declared, so that every malformed description still points
    inside its allocation. The G-buffer of the deferred pipeline is its own (one capacity for all planes): for its entry
    points the G-buffer case is the draw rect one texel wider / taller than that capacity while the scene texture fits."""
    from syzygy_amd import SzgError

    scap, gcap = (96, 48), (80, 40)
    inp = util.Inputs(W0, H0, spots=1)
    cameras, atmospheres, lights = staged(gpu, inp)
    scene = pi.PaddedScene(gpu.torch, scap[0], scap[1] + 4, SCENE_PADS)
    gbuffer = pi.PaddedGBuffer(gpu.torch, gcap[0], gcap[1] + 4)
    deferred = gpu.pl.DeferredShadingPipeline(gcap, max_spot_lights=1, max_shadow_maps=0)
    poison_pipeline_gbuffer(deferred, gcap)
    sky = gpu.pl.SkyViewComputePipeline.create(transmittance_extent=LUT[0], skyview_extent=LUT[1])
    sky.recordTransmittance(None, 0, atmospheres)
    sky.recordSkyViewLUT(None, 0, atmospheres, 0, cameras)
    sky.recordAerialLUT(None, 0, atmospheres, 0, cameras, 10.0e-3)
    ms = raster_meshes(W0, H0, scap)
    positions = lines_past_the_rect(W0, H0, scap)
    lines = gpu.pl.DebugLineGraphicsPipeline(len(positions))
    endpoints = gpu.pl.TStagedBuffer(abi.VertexPacked, len(positions))
    vertices = (abi.VertexPacked * len(positions))()
    for v, p in zip(vertices, positions):
        v.position[:] = [float(c) for c in p]
    endpoints.push(list(vertices))
    endpoints.recordCopyToDevice()

    def descriptions():
        st = abi.SceneTexture()
        st.color, st.depth, st.debug_color = (im.image(height=scap[1]) for im in (scene.color, scene.depth, scene.debug))
        g = abi.GBuffer()
        for name, im in gbuffer.planes.items():
            setattr(g, name, im.image(height=gcap[1]))
        return st, g

    rect = inp.rect
    spots = inp.spots
    fill = inp.synthetic.fill
    # name -> (call(scene texture, G-buffer, rect), the kinds of image the entry point looks at)
    entries = {
        "recordGBufferFill": (lambda st, g, r: deferred.recordGBufferFill(None, r, Described(st), 0, cameras, fill), {"color", "depth", "own"}),
        "recordGBufferRaster": (lambda st, g, r: deferred.recordGBufferRaster(None, r, Described(st), 0, cameras, ms), {"color", "depth", "own"}),
        "recordLights": (lambda st, g, r: deferred.recordLights(None, r, Described(st), 1, lights, spots, 0, cameras), {"color", "own"}),
        "deferred.recordDrawCommands": (lambda st, g, r: deferred.recordDrawCommands(None, r, Described(st), 1, lights, spots, 0, cameras, fill),
                                        {"color", "depth", "own"}),
        "deferred.recordDrawCommandsMeshes": (lambda st, g, r: deferred.recordDrawCommandsMeshes(None, r, Described(st), 1, lights, spots, 0,
                                                                                                 cameras, ms), {"color", "depth", "own"}),
        "recordComposite": (lambda st, g, r: sky.recordComposite(None, Described(st), r, g, None, 0, atmospheres, 0, cameras, 0, lights),
                            {"color", "depth", "gbuffer"}),
        "recordCompositeFast": (lambda st, g, r: sky.recordCompositeFast(None, Described(st), r, g, None, 0, atmospheres, 0, cameras, 0, lights),
                                {"color", "depth", "gbuffer"}),
        "sky.recordDrawCommands": (lambda st, g, r: sky.recordDrawCommands(None, Described(st), r, g, None, 0, atmospheres, 0, cameras, 0, lights),
                                   {"color", "depth", "gbuffer"}),
        "debug lines": (lambda st, g, r: lines.recordDrawCommands(None, 2.0, r, Described(st), 0, cameras, endpoints), {"color"}),
    }

    def nothing_written(what):
        gpu.torch.cuda.synchronize()
        for name, im in scene.images().items():
            im.assert_untouched(f"{what}: {name}")
        for name, im in gbuffer.planes.items():
            im.assert_untouched(f"{what}: caller gbuffer.{name}")
        check_pipeline_gbuffer(deferred, gcap, pi.gbuffer_poison(*gcap), (0, 0), what)

    def refused(call, st, g, r, word, what):
        with pytest.raises(SzgError) as e:
            call(st, g, r)
        assert e.value.code == abi.SZG_ERR_INVALID_ARGUMENT, (what, str(e.value))
        assert word in str(e.value), (what, str(e.value))

    tried = 0
    for entry, (call, looks_at) in entries.items():
        for case, mutate, word, kind in REFUSALS:
            if kind not in looks_at:
                continue
            st, g = descriptions()
            mutate(st, g)
            refused(call, st, g, rect, word, f"{entry}: {case}")
            tried += 1
        if "own" in looks_at:
            for r in (abi.Rect(0, 0, gcap[0] + 1, H0), abi.Rect(0, 0, W0, gcap[1] + 1)):
                st, g = descriptions()
                refused(call, st, g, r, "gbuffer.diffuse", f"{entry}: draw rect {r.width}x{r.height} on a {gcap} G-buffer")
                tried += 1
        nothing_written(entry)
    assert tried == 4 * (12 + 2) + (8 + 2) + 3 * 16 + 8  # fill, raster and the two chained calls; lights; the sky's three; lines

    # the same descriptions unharmed are accepted by every entry point: the refusals above were about the one malformed image
    for entry, (call, _) in entries.items():
        st, g = descriptions()
        call(st, g, rect)
    gpu.torch.cuda.synchronize()
    deferred.cleanup()
    lines.cleanup()
    sky.destroy()


def test_compose_refusals_write_nothing(gpu):
    W, H, nranks, block_rows = 70, 37, 3, 4
    stride_rows = max(len(util.global_rows(H, block_rows, r, nranks)) for r in range(nranks))
    d_buf = gpu.torch.zeros((nranks, stride_rows, W, 4), dtype=gpu.torch.int16, device="cuda")
    dst = pi.PaddedImage(abi.SZG_FORMAT_RGBA16_UNORM, 96, 48 + 4, 2, pi.POISON_COLOR).to_device(gpu.torch)
    cases = [
        ("pitch of the frame width on a wider image", lambda im: setattr(im, "pitch_bytes", W * 8)),
        ("pitch not a multiple of the texel size", lambda im: setattr(im, "pitch_bytes", im.pitch_bytes + 4)),
        ("pitch not a multiple of 16 bytes", lambda im: setattr(im, "pitch_bytes", im.pitch_bytes + 8)),
        ("pointer off by 2 bytes", off_by_two),
        ("pointer off by 8 bytes", lambda im: setattr(im, "data", im.data + 8)),
        ("narrower than the frame", lambda im: shrink(im, width=W - 1)),
        ("shorter than the frame", lambda im: shrink(im, height=H - 1)),
    ]
    for case, mutate in cases:
        im = dst.image(height=48)
        mutate(im)
        status = lib().szg_compose_rowtiles(None, C.c_void_p(d_buf.data_ptr()), stride_rows * W * 8, nranks, block_rows, C.byref(im), W, H)
        assert status == abi.SZG_ERR_INVALID_ARGUMENT, case
        dst.assert_untouched(f"compose: {case}")
    im = dst.image(height=48)
    assert lib().szg_compose_rowtiles(None, C.c_void_p(d_buf.data_ptr()), stride_rows * W * 8, nranks, block_rows, C.byref(im), W, H) == abi.SZG_OK
    gpu.torch.cuda.synchronize()
