"""GPU: every pass on a non-blocking stream, behind and beside a blocker (tests/stream_order.py has the two arrangements and
why they are conclusive). A case uses the input builders, oracles and models of the pass's own test, at the smallest shapes
that still reach every launch of the pass, and compares as that test compares: bit-identical, or the chained frame's <= 1
UNORM16 step. Caller-owned images are allocated larger than the draw extent with padded pitches, and nothing outside the
extent may change. The three runs of a case (warm, behind, beside) have different inputs and share the pipeline objects: what
a run leaves in the pipeline's constant blocks, records, LUTs and raster buffers is the stale state the next run must not see.

Then the state that outlives a call: frames in flight on one stream with real meshes, UI draw lists and debug lines (below and
above the slot count of the staging rings), raster buffers that grow between two frames in flight, the LUT passes on a second
stream as the STREAM RULE allows, and the process-global OETF table across two streams in a fresh child process."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from syzygy_amd import abi, lib
from tests import padded_images as pi
from tests import raster_scenes as rs
from tests import stream_order as so
from tests import util
from tests.util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TLUT, SLUT = (64, 16), (64, 32)
W, H = 64, 48              # draw extent of the frame passes
SCENE_CAP = (72, 52)       # caller-owned scene texture: larger than the extent, every pitch padded
GBUF_CAP = (70, 50)        # G-buffer capacity (pipeline-owned or caller-built)
SCENE_PADS = (3, 5, 1)
ELEVATIONS = (35.0, 12.0, 55.0, 70.0, 5.0, 25.0)  # the sun of the warm, behind and beside run; of the frames of a sequence
SPOT_SEEDS = (11, 23, 37, 41, 53, 67)


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    from oracle import binding as ob
    from syzygy_amd import pipelines, scene

    c = types.SimpleNamespace(torch=torch, pl=pipelines, ob=ob, scene=scene)
    c.blocker = so.Blocker(torch)
    yield c
    del c.blocker
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# shared pieces of the cases
# ---------------------------------------------------------------------------
class Params:
    """The three staged parameter buffers of a frame. Their device addresses stay the same over the runs of a case: what a
    run uploaded is what an early read of the next run finds."""

    def __init__(self, gpu):
        self.cameras = gpu.pl.TStagedBuffer(abi.CameraPacked, 1)
        self.atmospheres = gpu.pl.TStagedBuffer(abi.AtmospherePacked, 1)
        self.lights = gpu.pl.TStagedBuffer(abi.DirectionalLightPacked, 2)

    def stage(self, inp):
        self.cameras.stage([inp.cam])
        self.atmospheres.stage([inp.atm])
        self.lights.stage([inp.sun, inp.moon])

    def upload(self, S):
        for b in (self.cameras, self.atmospheres, self.lights):
            b.recordCopyToDevice(S)


def inputs(gpu, variant, spots=8, extent=(W, H), edit=None, grid=None):
    inp = util.Inputs(extent[0], extent[1], elevation_degrees=ELEVATIONS[variant], spots=spots,
                      grid=grid or (6 - variant % 3, 4 - variant // 3), atmosphere_edit=edit)
    if spots:
        inp.spots = gpu.scene.spot_ring(spots, seed=SPOT_SEEDS[variant])
    return inp


def absorbing(variant):
    """An atmosphere that differs between the runs in what the transmittance LUT depends on."""
    def edit(a):
        a.absorptionRayleighPerMegameter[:] = [0.25 * variant, 0.5 * variant, 0.125 * variant]
    return edit


def lut_bytes(gpu, array):
    a = np.ascontiguousarray(array, np.float32)
    return so.staged_tensor(gpu.torch, a.view(np.uint8).reshape(a.shape[0], -1))


def status_word(image):
    """The status dword behind a LUT's texels as a 1 x 1 image (tests/test_gpu_parity.py _slut_status_word)."""
    word = abi.Image()
    word.data = image.data + image.width * image.height * 16
    word.width, word.height, word.pitch_bytes, word.format = 1, 1, 16, image.format
    return word


def nan_like(gpu, image):
    """Sentinel texels for a LUT the library owns."""
    return lut_bytes(gpu, np.full((image.height, image.width, 4), np.nan, np.float32))


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = {2: np.uint16, 4: np.uint32, 1: np.uint8}[got.dtype.itemsize]
    same = got.view(bits) == want.view(bits)
    if got.dtype.kind == "f":
        same |= np.isnan(got) & np.isnan(want)
    bad = np.argwhere(~same)
    assert len(bad) == 0, f"{what}: {len(bad)} of {same.size} values differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


def check_owned_planes(deferred, cap, want, extent, what):
    """The planes a pipeline owns: inside `extent` the oracle's bits, outside still the poison."""
    got = deferred.download_gbuffer(cap[0], cap[1])
    poison = pi.gbuffer_poison(cap[0], cap[1])
    w, h = extent
    for name, plane in got.items():
        full = poison[name]
        full[:h, :w] = want[name][:h, :w]
        same_bits(plane, full, f"{what}: gbuffer.{name}")


def poisoned_planes(cap, planes=None):
    full = pi.gbuffer_poison(cap[0], cap[1])
    if planes is not None:
        for name, a in planes.items():
            full[name][: a.shape[0], : a.shape[1]] = a
    return full


def padded_scene(gpu):
    return pi.PaddedScene(gpu.torch, SCENE_CAP[0], SCENE_CAP[1], SCENE_PADS)


def check_frame_images(scene, frame, extent, written, what, exact_color=False):
    """Colour within one UNORM16 step of the oracle (the existing bound of a frame pass) or identical, debug colour within the
    parity tolerance, depth identical; outside the extent and in images the pass does not write, the sentinels."""
    for name, im in scene.images().items():
        if name not in written:
            im.assert_untouched(f"{what}: {name} (not an output of this pass)")
            continue
        got = im.inside(extent)
        if name == "depth":
            same_bits(got, frame.depth, f"{what}: depth")
        elif name == "color":
            if exact_color:
                same_bits(got, frame.color, f"{what}: colour")
            else:
                d = np.abs(got.astype(np.int32) - frame.color.astype(np.int32))
                assert d.max() <= 1, f"{what}: colour differs from the oracle by up to {d.max()} UNORM16 steps at {(d > 1).sum()} values"
        else:
            assert_close(got, frame.debug, what=f"{what}: debug colour")
        im.assert_outside_untouched(extent, f"{what}: {name}")


class Case:
    conditions = True

    def __init__(self, id, **kw):
        self.id = id
        self.__dict__.update(kw)

    def setup(self, gpu):
        return types.SimpleNamespace()

    def restage(self, gpu, state, run):
        """Sequences only (so.run_sequence): put the run's values back into the pipeline-side host staging that the run
        recorded before it has overwritten."""

    def teardown(self, gpu, state):
        for v in vars(state).values():
            for name in ("cleanup", "destroy"):
                if hasattr(v, name):
                    getattr(v, name)()


def new_sky(gpu):
    sky = gpu.pl.SkyViewComputePipeline.create(transmittance_extent=TLUT, skyview_extent=SLUT)
    assert sky is not None
    return sky


# ---------------------------------------------------------------------------
# the LUT passes
# ---------------------------------------------------------------------------
class LutCase(Case):
    """One LUT pass of the sky-view pipeline. `which`: transmittance, multiscatter, skyview, skyview-rows, aerial. The
    passes that read the transmittance LUT get the oracle's, written in stream order into the pipeline's texels."""

    def setup(self, gpu):
        s = types.SimpleNamespace(sky=new_sky(gpu), params=Params(gpu))
        s.t_image, s.s_image = s.sky.transmittanceLUT(), s.sky.skyviewLUT()
        s.m_image = s.sky.multiScatterLUT() if self.which == "multiscatter" else None
        return s

    def prepare(self, gpu, s, v):
        r = types.SimpleNamespace()
        r.inp = inputs(gpu, v, spots=0, edit=absorbing(v))
        if v == 2:
            r.inp.camera.cameraPosition[1] = -300.0
            r.inp.cam = gpu.scene.camera_packed(r.inp.camera, W / H)
        s.params.stage(r.inp)
        r.tlut = gpu.ob.transmittance_lut(r.inp.atm, TLUT[0], TLUT[1], threads=8)
        r.tlut_dev = lut_bytes(gpu, r.tlut)
        r.max_distance = (0.032, 0.05, 0.2)[v]
        if self.which == "transmittance":
            r.out, r.want = [s.t_image], [r.tlut]
        elif self.which == "multiscatter":
            r.out, r.want = [s.m_image], [gpu.ob.multiscatter_lut(r.inp.atm, r.tlut)[0]]
        elif self.which in ("skyview", "skyview-rows"):
            r.out, r.want = [s.s_image], [gpu.ob.skyview_lut(r.inp.atm, r.inp.cam, r.tlut, SLUT[0], SLUT[1], threads=8)]
        else:
            r.out = list(s.sky.aerialLUT())
            r.want = list(gpu.ob.aerial_lut(r.inp.atm, r.inp.cam, r.tlut, r.max_distance, threads=8))
        r.sentinels = [nan_like(gpu, im) for im in r.out]
        # the status dword behind the texels of the transmittance and the sky-view LUT ("a texel is out of range"): the pass
        # clears it in stream order and, with these atmospheres, no texel sets it again
        r.status = [status_word(im) for im in r.out] if self.which in ("transmittance", "skyview", "skyview-rows") else []
        r.status_set = so.staged_tensor(gpu.torch, np.array([[1, 0, 0, 0]], np.uint8))
        return r

    def enqueue(self, gpu, s, r, S):
        s.params.upload(S)
        for im, sentinel in zip(r.out, r.sentinels):
            so.copy2d_async(S, im, sentinel)
        for word in r.status:
            so.copy2d_async(S, word, r.status_set)
        if self.which != "transmittance":
            so.copy2d_async(S, s.t_image, r.tlut_dev)
        p = s.params
        if self.which == "transmittance":
            s.sky.recordTransmittance(S, 0, p.atmospheres)
        elif self.which == "multiscatter":
            s.sky.recordMultiScatterLUT(S, 0, p.atmospheres)
        elif self.which == "skyview":
            s.sky.recordSkyViewLUT(S, 0, p.atmospheres, 0, p.cameras)
        elif self.which == "skyview-rows":
            from syzygy_amd import rowtile

            for rank in (2, 0, 3, 1):
                b, e = rowtile.lut_rows(SLUT[1], rank, 4)
                s.sky.recordSkyViewLUTRows(S, 0, p.atmospheres, 0, p.cameras, b, e)
        else:
            s.sky.recordAerialLUT(S, 0, p.atmospheres, 0, p.cameras, r.max_distance)

    def check(self, gpu, s, r, what):
        for im, want in zip(r.out, r.want):
            got = s.sky.download_lut(im)
            if self.which.startswith("skyview"):  # tests/test_gpu_parity.py test_skyview_lut_matches_oracle
                assert_close(got[..., :3], want[..., :3], atol=1e-9, what=what)
                assert (got[..., 3] == 1.0).all(), what
            else:  # test_transmittance_lut_matches_oracle, test_multiscatter_lut_matches_its_oracle, test_aerial_lut_matches_oracle
                assert_close(got, want, atol=1e-12, what=what)
        for word in r.status:
            value = int(gpu.pl._memcpy2d_from(word, 4, 1).cpu().numpy().view(np.uint32).ravel()[0])
            assert value == 0, f"{what}: the LUT's status dword is {value:#x}: it was set before the pass and the pass must clear it in stream order"


# ---------------------------------------------------------------------------
# composite, exact and fast, on caller-built images with a padded sun shadow map
# ---------------------------------------------------------------------------
class CompositeCase(Case):
    def setup(self, gpu):
        s = types.SimpleNamespace(sky=new_sky(gpu), params=Params(gpu))
        s.t_image, s.s_image = s.sky.transmittanceLUT(), s.sky.skyviewLUT()
        return s

    def prepare(self, gpu, s, v):
        r = types.SimpleNamespace(inp=inputs(gpu, v))
        inp = r.inp
        s.params.stage(inp)
        frame = gpu.ob.HostFrame(W, H)
        gpu.ob.gbuffer_fill(frame, inp.rect, None, inp.cam, inp.synthetic.fill, threads=8)
        gpu.ob.lights(frame, inp.rect, None, None, inp.cam, inp.dirs, 2, 1, inp.spots, inp.spot_count, threads=8)
        tlut = gpu.ob.transmittance_lut(inp.atm, TLUT[0], TLUT[1], threads=8)
        slut = gpu.ob.skyview_lut(inp.atm, inp.cam, tlut, SLUT[0], SLUT[1], threads=8)
        r.tlut_dev, r.slut_dev = lut_bytes(gpu, tlut), lut_bytes(gpu, slut)
        sun_map = np.random.default_rng(7 + v).random((32, 32), dtype=np.float32)
        r.scene = padded_scene(gpu)
        r.scene.color.write_inside(frame.color)
        r.scene.depth.write_inside(frame.depth)
        r.gbuffer = pi.PaddedGBuffer(gpu.torch, GBUF_CAP[0], GBUF_CAP[1])
        r.gbuffer.write_inside({k: a.copy() for k, a in frame.planes().items()})
        r.sun = pi.PaddedImage(abi.SZG_FORMAT_D32_SFLOAT, 32, 32, 5, pi.NEAREST_OCCLUDER).to_device(gpu.torch)
        r.sun.write_inside(sun_map)
        so.stage_scene(r.scene)
        for im in list(r.gbuffer.planes.values()) + [r.sun]:
            so.stage_image(im)
        r.sun_images = (abi.Image * 1)(r.sun.image())
        r.shadow = abi.ShadowMaps(1, 0, C.cast(r.sun_images, C.POINTER(abi.Image)))
        host_images = (abi.Image * 1)(gpu.ob.host_image(sun_map, abi.SZG_FORMAT_D32_SFLOAT))
        host_shadow = abi.ShadowMaps(1, 0, C.cast(host_images, C.POINTER(abi.Image)))
        r.max_distance = (10.0e-3, 20.0e-3, 5.0e-3)[v]
        aerial = None
        if self.fast:  # tests/test_gpu_fast_composite.py: the oracle fetches from the volume the pass recorded
            r.volume = gpu.ob.aerial_lut(inp.atm, inp.cam, tlut, r.max_distance, threads=8)[0]
            aerial = (r.volume, r.max_distance)
        gpu.ob.composite(frame, inp.rect, None, host_shadow, inp.atm, inp.cam, inp.dirs, 0, tlut, slut, threads=8,
                         **({"aerial": aerial} if aerial else {}))
        r.frame = frame
        return r

    def enqueue(self, gpu, s, r, S):
        p = s.params
        p.upload(S)
        so.copy2d_async(S, s.t_image, r.tlut_dev)
        so.copy2d_async(S, s.s_image, r.slut_dev)
        so.write_scene(r.scene)
        for im in list(r.gbuffer.planes.values()) + [r.sun]:
            so.write_image(im)
        args = (S, r.scene, r.inp.rect, r.gbuffer.abi(), r.shadow, 0, p.atmospheres, 0, p.cameras, 0, p.lights)
        if self.fast:
            s.sky.recordAerialLUT(S, 0, p.atmospheres, 0, p.cameras, r.max_distance)
            s.sky.recordCompositeFast(*args)
        else:
            s.sky.recordComposite(*args)

    def check(self, gpu, s, r, what):
        check_frame_images(r.scene, r.frame, (W, H), {"color", "debug_color"}, what)
        r.scene.depth.assert_outside_untouched((W, H), what)
        same_bits(r.scene.depth.inside((W, H)), r.frame.depth, f"{what}: depth is only read")
        for name, im in r.gbuffer.planes.items():
            same_bits(im.read(), im.host, f"{what}: gbuffer.{name} is only read")
        same_bits(r.sun.read(), r.sun.host, f"{what}: the sun shadow map is only read")


# ---------------------------------------------------------------------------
# the deferred pipeline's passes on the analytic scene
# ---------------------------------------------------------------------------
class FillCase(Case):
    def setup(self, gpu):
        return types.SimpleNamespace(deferred=gpu.pl.DeferredShadingPipeline(GBUF_CAP, max_spot_lights=1, max_shadow_maps=0), params=Params(gpu))

    def prepare(self, gpu, s, v):
        r = types.SimpleNamespace(inp=inputs(gpu, v, spots=0))
        s.params.stage(r.inp)
        r.frame = gpu.ob.HostFrame(W, H)
        gpu.ob.gbuffer_fill(r.frame, r.inp.rect, None, r.inp.cam, r.inp.synthetic.fill, threads=8)
        r.scene = so.stage_scene(padded_scene(gpu))
        r.poison = so.stage_planes(gpu.torch, poisoned_planes(GBUF_CAP))
        return r

    def enqueue(self, gpu, s, r, S):
        s.params.upload(S)
        so.write_scene(r.scene)
        so.write_planes(S, s.deferred.gbuffer(), r.poison)
        s.deferred.recordGBufferFill(S, r.inp.rect, r.scene, 0, s.params.cameras, r.inp.synthetic.fill)

    def check(self, gpu, s, r, what):
        check_frame_images(r.scene, r.frame, (W, H), {"depth"}, what)
        check_owned_planes(s.deferred, GBUF_CAP, r.frame.planes(), (W, H), what)


class LightsCase(Case):
    """8 spots, caller-owned shadow maps with padded rows in the moon's slot and two spot slots; the G-buffer planes are the
    oracle's fill, written into the pipeline's planes in stream order."""
    SPOTS = 8
    MAPS = {1: (33, 47), 2: (40, 64), 9: (21, 9)}

    def setup(self, gpu):
        return types.SimpleNamespace(deferred=gpu.pl.DeferredShadingPipeline(GBUF_CAP, max_spot_lights=self.SPOTS, max_shadow_maps=self.SPOTS + 2),
                                     params=Params(gpu))

    def prepare(self, gpu, s, v):
        r = types.SimpleNamespace(inp=inputs(gpu, v, spots=self.SPOTS))
        inp = r.inp
        s.params.stage(inp)
        frame = gpu.ob.HostFrame(W, H)
        gpu.ob.gbuffer_fill(frame, inp.rect, None, inp.cam, inp.synthetic.fill, threads=8)
        r.planes = {k: a.copy() for k, a in frame.planes().items()}
        r.planes_dev = so.stage_planes(gpu.torch, poisoned_planes(GBUF_CAP, r.planes))
        rng = np.random.default_rng(0x5A2C + v)
        r.maps, images = {}, (abi.Image * (self.SPOTS + 2))()
        for slot, shape in self.MAPS.items():
            m = rng.random(shape, dtype=np.float32) if slot != 2 else (rng.random(shape, dtype=np.float32) > 0.5).astype(np.float32) * np.float32(0.9999)
            im = pi.PaddedImage(abi.SZG_FORMAT_D32_SFLOAT, shape[1], shape[0], 2 * slot + 3, pi.NEAREST_OCCLUDER).to_device(gpu.torch)
            im.write_inside(m)
            r.maps[slot] = so.stage_image(im)
            images[slot] = gpu.ob.host_image(m, abi.SZG_FORMAT_D32_SFLOAT)
            r.__dict__[f"keep{slot}"] = m
        gpu.ob.lights(frame, inp.rect, None, abi.ShadowMaps(self.SPOTS + 2, 0, C.cast(images, C.POINTER(abi.Image))), inp.cam, inp.dirs, 2, 1,
                      inp.spots, self.SPOTS, threads=8)
        r.frame = frame
        r.scene = so.stage_scene(padded_scene(gpu))
        return r

    def enqueue(self, gpu, s, r, S):
        s.params.upload(S)
        so.write_scene(r.scene)
        so.write_planes(S, s.deferred.gbuffer(), r.planes_dev)
        for slot, im in r.maps.items():
            so.write_image(im)
            s.deferred.setShadowMap(slot, im.device.view(gpu.torch.float32)[:, : im.cap_w])
        s.deferred.recordLights(S, r.inp.rect, r.scene, 1, s.params.lights, r.inp.spots, 0, s.params.cameras)

    def check(self, gpu, s, r, what):
        check_frame_images(r.scene, r.frame, (W, H), {"color", "debug_color"}, what)
        assert (r.scene.color.inside((W, H))[..., 3] == 65535).all()
        check_owned_planes(s.deferred, GBUF_CAP, r.planes, (W, H), f"{what}: only read")
        for slot, im in r.maps.items():
            same_bits(im.read(), im.host, f"{what}: shadow map {slot} is only read")


class ShadowMapsCase(Case):
    """recordShadowMaps of the analytic scene into the maps the pipeline owns (tests/test_gpu_parity.py
    test_shadow_maps_match_oracle_and_shade_the_frame)."""
    SPOTS, DIM = 3, 64

    def setup(self, gpu):
        return types.SimpleNamespace(deferred=gpu.pl.DeferredShadingPipeline((8, 8), max_spot_lights=self.SPOTS, max_shadow_maps=2 + self.SPOTS,
                                                                             shadow_map_dim=self.DIM), params=Params(gpu))

    def prepare(self, gpu, s, v):
        r = types.SimpleNamespace(inp=inputs(gpu, v, spots=self.SPOTS))
        s.params.stage(r.inp)
        packed = [r.inp.sun, r.inp.moon] + [r.inp.spots[i] for i in range(self.SPOTS)]
        r.want = [gpu.ob.shadow_map(light, self.DIM, r.inp.synthetic.fill, threads=8) for light in packed]
        r.sentinel = so.staged_tensor(gpu.torch, np.full((self.DIM, self.DIM), 0.75, np.float32).view(np.uint8))
        return r

    def enqueue(self, gpu, s, r, S):
        s.params.upload(S)
        sm = s.deferred.shadowMaps()
        for slot in range(2 + self.SPOTS):
            so.copy2d_async(S, sm.maps[slot], r.sentinel)
        s.deferred.recordShadowMaps(S, s.params.lights, r.inp.spots, r.inp.synthetic.fill)

    def check(self, gpu, s, r, what):
        for slot, want in enumerate(r.want):
            same_bits(read_shadow_map(gpu, s.deferred, slot, self.DIM), want, f"{what}: shadow map {slot}")
        assert (r.want[0] > 0).any() and (r.want[2] > 0).any()


# ---------------------------------------------------------------------------
# the compute rasteriser
# ---------------------------------------------------------------------------
def soup_meshes(seed, count):
    """A seeded soup for the exact perspective camera, both windings, without the viewport-filling triangles (background
    texels stay): 2 * (count - count / 6) primitives."""
    soup = rs.soup(seed, count, W, H).reshape(-1, 3, 3)
    soup = soup[np.arange(len(soup)) % 6 != 4].reshape(-1, 3)
    idx = np.arange(len(soup), dtype=np.uint32).reshape(-1, 3)
    return [rs.mesh_of(soup, np.concatenate([idx, idx[:, ::-1]]))]


def upload_meshes(ms):
    """Geometry and textures are assets: on the device before the frame is recorded (syzygy_amd.meshes caches the copies)."""
    from syzygy_amd.meshes import mesh_array

    mesh_array(ms, "cuda")


class RasterCase(Case):
    """recordGBufferRaster. `scenes(variant)` -> (camera, meshes, expected primitive count or None)."""

    def setup(self, gpu):
        s = types.SimpleNamespace(deferred=gpu.pl.DeferredShadingPipeline(GBUF_CAP, max_spot_lights=1, max_shadow_maps=0))
        s.cameras = gpu.pl.TStagedBuffer(abi.CameraPacked, 1)
        return s

    def prepare(self, gpu, s, v):
        r = types.SimpleNamespace()
        r.cam, r.meshes = self.scenes(v)
        upload_meshes(r.meshes)
        s.cameras.stage([r.cam])
        r.rect = abi.Rect(0, 0, W, H)
        r.frame = gpu.ob.HostFrame(W, H, debug=False)
        gpu.ob.gbuffer_raster(r.frame, r.rect, None, r.cam, r.meshes, threads=4)
        assert (r.frame.depth > 0).any()
        r.scene = so.stage_scene(padded_scene(gpu))
        r.poison = so.stage_planes(gpu.torch, poisoned_planes(GBUF_CAP))
        return r

    def restage(self, gpu, s, r):
        s.cameras.stage([r.cam])

    def enqueue(self, gpu, s, r, S):
        s.cameras.recordCopyToDevice(S)
        so.write_scene(r.scene)
        so.write_planes(S, s.deferred.gbuffer(), r.poison)
        s.deferred.recordGBufferRaster(S, r.rect, r.scene, 0, s.cameras, r.meshes)

    def check(self, gpu, s, r, what):
        check_frame_images(r.scene, r.frame, (W, H), {"depth"}, what)
        if getattr(r, "last", True):  # the planes the pipeline owns hold the last frame recorded
            check_owned_planes(s.deferred, GBUF_CAP, r.frame.planes(), (W, H), what)


def small_soup(v):
    return rs.exact_perspective_camera(), soup_meshes(41 + v, 60)  # 100 primitives


def tie_scene(v):
    """test_raster_exact's tie case above RASTER_SORT_THRESHOLD: 16 layers of 12 x 12 quads = 4608 primitives, the radix
    sort over two super-chunks. Another seed per run: other colours and instance depths."""
    scene = rs.tie_layers(seed=1612 + v, quads=12)
    assert scene["primitives"] == 4608
    return scene["camera"], scene["meshes"]


def shadow_raster_oracle(gpu, light, dim, ms):
    pv = abi.Mat4()
    lib().szg_mat4_mul(C.byref(light.projection), C.byref(light.view), C.byref(pv))
    return gpu.ob.shadow_raster(pv, dim, ms, threads=8)


def read_shadow_map(gpu, deferred, slot, dim):
    im = deferred.shadowMaps().maps[slot]
    return gpu.pl._memcpy2d_from(im, dim * 4, dim).cpu().numpy().view(np.float32).reshape(dim, dim)


def box_meshes(inp):
    """The analytic scene as real meshes (tests/test_raster.py test_shadow_raster_matches_oracle_and_the_analytic_maps)."""
    from syzygy_amd import meshes

    return meshes.meshes_of_fill_scene(inp.synthetic.fill)


class ShadowRasterCase(Case):
    """recordShadowRaster into two owned slots (sun and moon), which reuse the primitive buffers."""
    DIM = 64

    def setup(self, gpu):
        s = types.SimpleNamespace(deferred=gpu.pl.DeferredShadingPipeline((8, 8), max_spot_lights=1, max_shadow_maps=2, shadow_map_dim=self.DIM))
        s.lights = gpu.pl.TStagedBuffer(abi.DirectionalLightPacked, 2)
        return s

    def prepare(self, gpu, s, v):
        r = types.SimpleNamespace(inp=inputs(gpu, v, spots=0))
        r.meshes = box_meshes(r.inp)
        upload_meshes(r.meshes)
        s.lights.stage([r.inp.sun, r.inp.moon])
        r.want = [shadow_raster_oracle(gpu, light, self.DIM, r.meshes) for light in (r.inp.sun, r.inp.moon)]
        r.sentinel = so.staged_tensor(gpu.torch, np.full((self.DIM, self.DIM), 0.75, np.float32).view(np.uint8))
        return r

    def enqueue(self, gpu, s, r, S):
        s.lights.recordCopyToDevice(S)
        sm = s.deferred.shadowMaps()
        for slot in range(2):
            so.copy2d_async(S, sm.maps[slot], r.sentinel)
        s.deferred.recordShadowRaster(S, s.lights, None, r.meshes)

    def check(self, gpu, s, r, what):
        for slot, want in enumerate(r.want):
            same_bits(read_shadow_map(gpu, s.deferred, slot, self.DIM), want, f"{what}: shadow map {slot}")
        assert (r.want[0] > 0).any() and not np.array_equal(r.want[0], r.want[1])


def mesh_frame_oracle(gpu, inp, ms, dim, spots, lut=None):
    """The oracle chain of tests/test_raster.py test_frame_from_real_meshes_matches_oracle_chain: shadow raster of every
    light (dim > 0), G-buffer raster, lights, and with `lut` = (transmittance extent, sky-view extent) the atmosphere on top."""
    host_maps, maps = None, []
    if dim:
        packed = [inp.sun, inp.moon] + [inp.spots[i] for i in range(spots)]
        maps = [shadow_raster_oracle(gpu, light, dim, ms) for light in packed]
        images = (abi.Image * len(maps))(*[gpu.ob.host_image(m, abi.SZG_FORMAT_D32_SFLOAT) for m in maps])
        host_maps = abi.ShadowMaps(len(maps), 0, C.cast(images, C.POINTER(abi.Image)))
    frame = gpu.ob.HostFrame(inp.width, inp.height)
    gpu.ob.gbuffer_raster(frame, inp.rect, None, inp.cam, ms, threads=8)
    gpu.ob.lights(frame, inp.rect, None, host_maps, inp.cam, inp.dirs, 2, 1, inp.spots, spots, threads=8)
    if lut is not None:
        tlut = gpu.ob.transmittance_lut(inp.atm, lut[0][0], lut[0][1], threads=8)
        slut = gpu.ob.skyview_lut(inp.atm, inp.cam, tlut, lut[1][0], lut[1][1], threads=8)
        gpu.ob.composite(frame, inp.rect, None, host_maps, inp.atm, inp.cam, inp.dirs, 0, tlut, slut, threads=8)
    frame.maps = maps
    return frame


class MeshFrameCase(Case):
    """A frame from real meshes. SPOTS > 0: szg_deferred_record_draw_commands_meshes as one call - shadow raster into the
    owned maps, G-buffer raster, lights; 5 uploads through the pipeline's staging ring. SPOTS == 0: G-buffer raster and a
    lights pass with the directional lights only on a pipeline without shadow maps; 1 upload (the draw records). With `sky`
    the sky-view pipeline's frame on top (transmittance LUT, sky-view LUT, composite)."""
    SPOTS, DIM, sky = 3, 64, False

    def setup(self, gpu):
        s = types.SimpleNamespace(params=Params(gpu), deferred=gpu.pl.DeferredShadingPipeline(
            GBUF_CAP, max_spot_lights=max(self.SPOTS, 1), max_shadow_maps=(2 + self.SPOTS) if self.DIM else 0, shadow_map_dim=self.DIM))
        if self.sky:
            s.sky = new_sky(gpu)
        return s

    def prepare(self, gpu, s, v):
        # more boxes in every later run: another draw list per frame, and the instance counts only grow
        r = types.SimpleNamespace(inp=inputs(gpu, v, spots=self.SPOTS, grid=(3 + v, 4)))
        s.params.stage(r.inp)
        r.meshes = box_meshes(r.inp)
        upload_meshes(r.meshes)
        r.frame = mesh_frame_oracle(gpu, r.inp, r.meshes, self.DIM, self.SPOTS, (TLUT, SLUT) if self.sky else None)
        assert (r.frame.depth > 0).mean() > 0.1
        r.planes = {k: a.copy() for k, a in r.frame.planes().items()}
        r.scene = so.stage_scene(padded_scene(gpu))
        r.poison = so.stage_planes(gpu.torch, poisoned_planes(GBUF_CAP))
        return r

    def restage(self, gpu, s, r):
        s.params.stage(r.inp)

    def enqueue(self, gpu, s, r, S):
        p = s.params
        p.upload(S)
        so.write_scene(r.scene)
        so.write_planes(S, s.deferred.gbuffer(), r.poison)
        if self.SPOTS:
            s.deferred.recordDrawCommandsMeshes(S, r.inp.rect, r.scene, 1, p.lights, r.inp.spots, 0, p.cameras, r.meshes)
        else:
            s.deferred.recordGBufferRaster(S, r.inp.rect, r.scene, 0, p.cameras, r.meshes)
            s.deferred.recordLights(S, r.inp.rect, r.scene, 1, p.lights, None, 0, p.cameras)
        if self.sky:
            s.sky.recordDrawCommands(S, r.scene, r.inp.rect, s.deferred.gbuffer(), s.deferred.shadowMaps(), 0, p.atmospheres, 0, p.cameras,
                                     0, p.lights)

    def check(self, gpu, s, r, what):
        check_frame_images(r.scene, r.frame, (W, H), {"color", "depth", "debug_color"}, what)
        if getattr(r, "last", True):  # what the pipeline owns holds the last frame recorded
            for slot, want in enumerate(r.frame.maps):
                same_bits(read_shadow_map(gpu, s.deferred, slot, self.DIM), want, f"{what}: shadow map {slot}")
            check_owned_planes(s.deferred, GBUF_CAP, r.planes, (W, H), what)


class ChainCase(Case):
    """The chained frame with GPU LUTs: deferred.recordDrawCommands (analytic fill, lights) then sky.recordDrawCommands
    (transmittance LUT, sky-view LUT, composite). With `reuse` every run records the frame twice with equal inputs before its
    own: two frames with equal inputs, then - in the next run - one with changed inputs, on a pipeline that compares the
    reuse key on the device."""
    reuse = False

    def setup(self, gpu):
        s = types.SimpleNamespace(params=Params(gpu), sky=new_sky(gpu),
                                  deferred=gpu.pl.DeferredShadingPipeline(GBUF_CAP, max_spot_lights=8, max_shadow_maps=0))
        s.sky.setLUTReuse(self.reuse)
        return s

    def prepare(self, gpu, s, v):
        r = types.SimpleNamespace(inp=inputs(gpu, v))
        inp = r.inp
        s.params.stage(inp)
        frame = gpu.ob.HostFrame(W, H)
        gpu.ob.gbuffer_fill(frame, inp.rect, None, inp.cam, inp.synthetic.fill, threads=8)
        gpu.ob.lights(frame, inp.rect, None, None, inp.cam, inp.dirs, 2, 1, inp.spots, inp.spot_count, threads=8)
        tlut = gpu.ob.transmittance_lut(inp.atm, TLUT[0], TLUT[1], threads=8)
        slut = gpu.ob.skyview_lut(inp.atm, inp.cam, tlut, SLUT[0], SLUT[1], threads=8)
        gpu.ob.composite(frame, inp.rect, None, None, inp.atm, inp.cam, inp.dirs, 0, tlut, slut, threads=8)
        r.frame = frame
        r.scene = so.stage_scene(padded_scene(gpu))
        r.poison = so.stage_planes(gpu.torch, poisoned_planes(GBUF_CAP))
        return r

    def enqueue(self, gpu, s, r, S):
        p = s.params
        p.upload(S)
        for _ in range(3 if self.reuse else 1):
            so.write_scene(r.scene)
            so.write_planes(S, s.deferred.gbuffer(), r.poison)
            s.deferred.recordDrawCommands(S, r.inp.rect, r.scene, 1, p.lights, r.inp.spots, 0, p.cameras, r.inp.synthetic.fill)
            s.sky.recordDrawCommands(S, r.scene, r.inp.rect, s.deferred.gbuffer(), s.deferred.shadowMaps(), 0, p.atmospheres, 0, p.cameras,
                                     0, p.lights)

    def check(self, gpu, s, r, what):
        check_frame_images(r.scene, r.frame, (W, H), {"color", "depth", "debug_color"}, what)
        check_owned_planes(s.deferred, GBUF_CAP, r.frame.planes(), (W, H), what)


# ---------------------------------------------------------------------------
# the passes over one image
# ---------------------------------------------------------------------------
class OetfCase(Case):
    """szg_record_oetf at 131 x 7 inside a larger image (tests/test_gpu_parity.py test_oetf_bit_exact)."""
    EXTENT = (131, 7)

    def prepare(self, gpu, s, v):
        w, h = self.EXTENT
        r = types.SimpleNamespace()
        rng = np.random.default_rng(w * 31 + self.function + 1000 * v)
        r.img = rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)
        r.img[0, 0] = [0, 205, 206, 65535]  # around the sRGB cutoff
        r.target = pi.PaddedImage(abi.SZG_FORMAT_RGBA16_UNORM, w + 6, h + 3, 1, pi.POISON_COLOR).to_device(gpu.torch)
        assert r.target.pitch_bytes % 16 == 0
        r.target.write_inside(r.img)
        so.stage_image(r.target)
        r.want = gpu.ob.oetf(r.img.copy(), self.function)
        return r

    def enqueue(self, gpu, s, r, S):
        so.write_image(r.target)
        im = r.target.image()
        assert lib().szg_record_oetf(C.c_void_p(S.cuda_stream), C.byref(im), self.EXTENT[0], self.EXTENT[1], self.function) == abi.SZG_OK, \
            lib().szg_last_error()

    def check(self, gpu, s, r, what):
        same_bits(r.target.inside(self.EXTENT), r.want, what)
        r.target.assert_outside_untouched(self.EXTENT, what)


class ComposeCase(Case):
    """szg_compose_rowtiles (3 ranks, blocks of 4 rows) into a destination larger than the frame."""
    RANKS, BLOCK = 3, 4

    def prepare(self, gpu, s, v):
        r = types.SimpleNamespace()
        rng = np.random.default_rng(W * 100 + H + v)
        r.full = rng.integers(0, 65536, (H, W, 4), dtype=np.uint16)
        r.stride_rows = max(len(util.global_rows(H, self.BLOCK, k, self.RANKS)) for k in range(self.RANKS))
        buf = np.zeros((self.RANKS, r.stride_rows, W, 4), np.uint16)
        for k in range(self.RANKS):
            rows = util.global_rows(H, self.BLOCK, k, self.RANKS)
            buf[k, : len(rows)] = r.full[rows]
        r.source = so.staged_tensor(gpu.torch, buf.view(np.int16))
        r.live = gpu.torch.zeros_like(r.source)
        r.dst = pi.PaddedImage(abi.SZG_FORMAT_RGBA16_UNORM, SCENE_CAP[0], SCENE_CAP[1], 2, pi.POISON_COLOR).to_device(gpu.torch)
        assert r.dst.pitch_bytes % 16 == 0
        so.stage_image(r.dst)
        return r

    def enqueue(self, gpu, s, r, S):
        r.live.copy_(r.source)
        so.write_image(r.dst)
        im = r.dst.image()
        rc = lib().szg_compose_rowtiles(C.c_void_p(S.cuda_stream), C.c_void_p(r.live.data_ptr()), r.stride_rows * W * 8, self.RANKS, self.BLOCK,
                                        C.byref(im), W, H)
        assert rc == abi.SZG_OK, lib().szg_last_error()

    def check(self, gpu, s, r, what):
        same_bits(r.dst.inside((W, H)), r.full, what)
        r.dst.assert_outside_untouched((W, H), what)


def byte_pattern(count):
    """`count` bytes that differ from their neighbours and from zero (tests/test_gpu_present.py)."""
    return np.resize(((np.arange(251, dtype=np.int64) * 37 + 11) % 251 + 1).astype(np.uint8), count)


class PresentCase(Case):
    """szg_record_present, LINEAR, 33 x 17 -> 40 x 20 inside a 44 x 23 destination of format `fmt`; the three runs use no
    encode, the sRGB and the pure-gamma encode. With `in_place`: pipelines.record_present, whose OETF rewrites the source."""
    SRC, DST, DST_CAP = (33, 17), (40, 20), (44, 23)
    in_place = False

    def prepare(self, gpu, s, v):
        from tests import present_model as pm

        (sw, sh), (dw, dh), (cw, ch) = self.SRC, self.DST, self.DST_CAP
        r = types.SimpleNamespace()
        r.src = np.random.default_rng(100 * self.fmt + v).integers(0, 65536, (sh, sw, 4), dtype=np.uint16)
        r.encode = (abi.SZG_PRESENT_ENCODE_NONE, abi.SZG_OETF_SRGB, abi.SZG_OETF_PURE_GAMMA)[v]
        # one more column than the image: szg_record_oetf wants rows of a multiple of 16 bytes, and 33 texels are 264
        r.src_buffer = np.full((sh, sw + 1, 4), 0xBEEF, np.uint16)
        r.src_buffer[:, :sw] = r.src
        r.src_staged = so.staged_tensor(gpu.torch, r.src_buffer.view(np.int16))
        r.src_live = gpu.torch.zeros_like(r.src_staged)
        if self.in_place:
            cw, ch = dw, dh
            r.function = (abi.SZG_OETF_SRGB, abi.SZG_OETF_PURE_GAMMA, abi.SZG_OETF_SRGB)[v]
        dst0 = byte_pattern(cw * ch * 4 + v)[v:].reshape(ch, cw, 4)
        r.dst_staged = so.staged_tensor(gpu.torch, dst0)
        r.dst_live = gpu.torch.zeros_like(r.dst_staged)
        host_dst = dst0.copy().view(np.uint32).reshape(ch, cw) if self.fmt == pm.A2B10G10R10 else dst0.copy()
        if self.in_place:
            r.want_src = gpu.ob.oetf(r.src.copy(), r.function)
            r.want = pm.present(r.want_src, (0, 0, sw, sh), host_dst, (0, 0, dw, dh), self.fmt, pm.LINEAR)
        else:
            r.want_src = r.src
            table = None if r.encode == abi.SZG_PRESENT_ENCODE_NONE else pm.oetf_table(r.encode)
            r.want = pm.present(r.src, (0, 0, sw, sh), host_dst, (0, 0, dw, dh), self.fmt, pm.LINEAR, table)
        return r

    def enqueue(self, gpu, s, r, S):
        from tests import present_model as pm

        (sw, sh), (dw, dh) = self.SRC, self.DST
        r.src_live.copy_(r.src_staged)
        r.dst_live.copy_(r.dst_staged)
        if self.in_place:
            dst = r.dst_live.view(gpu.torch.int32).reshape(dh, dw) if self.fmt == pm.A2B10G10R10 else r.dst_live
            gpu.pl.record_present(S, r.src_live[:, :sw], (0, 0, sw, sh), dst, r.function, False, None if self.fmt == pm.A2B10G10R10 else self.fmt)
            return
        ch, cw = r.dst_live.shape[:2]
        src = abi.Image(r.src_live.data_ptr(), sw, sh, (sw + 1) * 8, abi.SZG_FORMAT_RGBA16_UNORM)
        dst = abi.Image(r.dst_live.data_ptr(), cw, ch, cw * 4, self.fmt)
        info = abi.PresentInfo(abi.Rect(0, 0, sw, sh), abi.Rect(0, 0, dw, dh), abi.SZG_FILTER_LINEAR, r.encode)
        assert lib().szg_record_present(C.c_void_p(S.cuda_stream), C.byref(src), C.byref(dst), C.byref(info)) == abi.SZG_OK, lib().szg_last_error()

    def check(self, gpu, s, r, what):
        got = r.dst_live.cpu().numpy()
        same_bits(got, r.want.view(np.uint8).reshape(got.shape), what)
        want_buffer = r.src_buffer.copy()
        want_buffer[:, : self.SRC[0]] = r.want_src
        same_bits(r.src_live.cpu().numpy().view(np.uint16), want_buffer, f"{what}: the source")


class ComputeCollectionCase(Case):
    """One program of the compute collection at 17 x 5 in a 32 x 16 image with a padded pitch, one texel into its buffer
    (tests/gpu_compute_collection_child.py "padded_pitch"); the three runs push the ordinary, special and example blocks."""
    EXTENT, IMAGE, PITCH, OFFSET = (17, 5), (32, 16), 37, 1

    def prepare(self, gpu, s, v):
        from tests import gpu_compute_collection_child as child
        from tests import test_gpu_compute_collection as tcc

        r = types.SimpleNamespace()
        r.block = child.blocks()[(self.shader, child.KINDS[v])]
        count = child.buffer_bytes(self.IMAGE, self.PITCH, self.OFFSET)
        initial = byte_pattern(count + v)[v:].copy()
        r.staged = so.staged_tensor(gpu.torch, initial)
        r.live = gpu.torch.zeros_like(r.staged)
        r.want = tcc.expected_buffer(initial, self.shader, r.block, self.EXTENT, self.IMAGE, self.PITCH, self.OFFSET)
        r.index = child.SHADERS.index(self.shader)
        return r

    def enqueue(self, gpu, s, r, S):
        r.live.copy_(r.staged)
        im = abi.Image(r.live.data_ptr() + self.OFFSET * 8, self.IMAGE[0], self.IMAGE[1], self.PITCH * 8, abi.SZG_FORMAT_RGBA16_UNORM)
        raw = C.create_string_buffer(r.block, len(r.block))
        rc = lib().szg_record_compute_collection(C.c_void_p(S.cuda_stream), r.index, raw, len(r.block), C.byref(im), self.EXTENT[0], self.EXTENT[1])
        C.memset(raw, 0xEE, len(r.block))  # the block was copied before the call returned
        assert rc == abi.SZG_OK, lib().szg_last_error()

    def check(self, gpu, s, r, what):
        same_bits(r.live.cpu().numpy(), r.want, what)


def two_boxes(lines, v):
    lines.clear()
    lines.pushBox((0.0 + 3.0 * v, -8.0, 20.0), (0.0, 0.0, 0.0, 1.0), (5.0, 5.0 + v, 5.0))
    lines.pushBox((-12.0, -6.0 - v, 30.0), (0.0, 0.3826834, 0.0, 0.9238795), (4.0, 3.0, 6.0 + 2.0 * v))


class DebugLinesCase(Case):
    """pipelines.DebugLines.recordDraw: the list's staged copy and the line rasteriser, two boxes (96 vertices), over a
    padded scene texture; tests/debuglines_model.py gives the covered pixels."""

    def setup(self, gpu):
        s = types.SimpleNamespace(lines=gpu.pl.DebugLines(capacity=96), params=Params(gpu))
        s.lines.enabled = True
        return s

    def prepare(self, gpu, s, v):
        from tests import debuglines_model as dm

        r = types.SimpleNamespace(inp=inputs(gpu, v, spots=0))
        s.params.stage(r.inp)
        r.variant = v
        two_boxes(s.lines, v)
        r.width = (1.0, 3.0, 2.0)[v % 3]
        positions = dm.positions_of(b"".join(bytes(x) for x in s.lines.vertices.readValidStaged()))
        r.scene = padded_scene(gpu)
        color0, debug0 = r.scene.color.inside((W, H)), r.scene.debug.inside((W, H))
        mask = dm.model(r.inp.cam, positions, W, H, r.width)
        assert mask.sum() > 40
        r.want_color, r.want_debug = dm.render(mask, color0, debug0)
        so.stage_scene(r.scene)
        return r

    def restage(self, gpu, s, r):
        s.params.stage(r.inp)
        two_boxes(s.lines, r.variant)

    def enqueue(self, gpu, s, r, S):
        s.params.upload(S)
        so.write_scene(r.scene)
        s.lines.lineWidth = r.width
        s.lines.recordDraw(S, 0, r.scene, r.inp.rect, s.params.cameras)
        assert s.lines.lastFrameDrawResults[1] == 96

    def check(self, gpu, s, r, what):
        same_bits(r.scene.color.inside((W, H)), r.want_color, f"{what}: colour")
        same_bits(r.scene.debug.inside((W, H)), r.want_debug, f"{what}: debug colour")
        for name, im in r.scene.images().items():
            im.assert_outside_untouched((W, H) if name != "depth" else (0, 0), f"{what}: {name}")

    def teardown(self, gpu, s):
        s.lines.cleanup()


UI_EXTENT = (48, 36)


def ui_draw(v, white, image, quads=65):
    """`quads` translucent quads on a 48 x 36 frame, alternately filled (the white texel) and textured (the second texture with
    uv beyond [0, 1]): 130 triangles, more than one chunk of 64."""
    from syzygy_amd import ui

    rng = np.random.default_rng(900 + v)
    dl = ui.DrawList(white)
    for k in range(quads):
        x0, y0 = rng.uniform(-4, UI_EXTENT[0] - 4), rng.uniform(-4, UI_EXTENT[1] - 4)
        x1, y1 = x0 + rng.uniform(1, 24), y0 + rng.uniform(1, 18)
        col = ui.col32(*(int(c) for c in rng.integers(0, 256, 3)), int(rng.integers(13, 243)))
        if k % 2 == 0:
            dl.add_rect_filled((x0, y0), (x1, y1), col)
        else:
            dl.add_image(image, (x0, y0), (x1, y1), (-0.5, -0.25), (1.5, 1.75), col)
    return ui.DrawData((0, 0), UI_EXTENT, (1, 1), [dl]).flatten()


def ui_textures(gpu, layer):
    """(handles, model textures by handle): the white texel and a 9 x 7 RGBA16 texture under LINEAR / REPEAT."""
    from tests import ui_layer_cases as uc
    from tests import ui_layer_model as um

    white = um.Texture(np.full((1, 1, 4), 255, np.uint8), um.NEAREST, um.REPEAT)
    image = um.Texture(uc.sampler_texture(np.uint16), um.LINEAR, um.REPEAT)
    hw = layer.addTexture(gpu.torch.from_numpy(white.data).cuda(), white.filter, white.address)
    hi = layer.addTexture(gpu.torch.from_numpy(image.data.view(np.int16)).cuda(), image.filter, image.address)
    return (hw, hi), {hw: white, hi: image}


class UILayerCase(Case):
    """pipelines.UILayer.recordDraw with LOAD: vertex and index staging, the command upload and the rasteriser; the output
    texture is prefilled in stream order and is an input of the blend."""

    def setup(self, gpu):
        s = types.SimpleNamespace(layer=gpu.pl.UILayer(UI_EXTENT, triangleCapacity=1024, commandCapacity=256))
        s.handles, s.textures = ui_textures(gpu, s.layer)
        gpu.torch.cuda.synchronize()
        return s

    def prepare(self, gpu, s, v):
        from tests import ui_layer_model as um

        r = types.SimpleNamespace(draw=ui_draw(v, *s.handles))
        assert sum(c.elem_count for c in r.draw.commands) == 65 * 6 and len({c.texture for c in r.draw.commands}) == 2
        r.image0 = np.random.default_rng(77 + v).integers(0, 65536, (UI_EXTENT[1], UI_EXTENT[0], 4), dtype=np.uint16)
        r.prefill = so.staged_tensor(gpu.torch, r.image0.view(np.int16))
        r.output = gpu.pl.SceneTexture(*UI_EXTENT)
        r.clear = (0.1, 0.2, 0.3, 0.9)
        r.want = um.render(r.image0, (0, 0) + UI_EXTENT, um.LOAD, r.clear, r.draw, s.textures)
        return r

    def enqueue(self, gpu, s, r, S):
        s.layer._output = r.output
        r.output.color.copy_(r.prefill)
        s.layer.recordDraw(S, r.draw, abi.SZG_UI_LOAD_OP_LOAD, r.clear)

    def check(self, gpu, s, r, what):
        same_bits(r.output.color_numpy(), r.want, what)
        assert (r.want != r.image0).any(axis=2).mean() > 0.5


def receding_plane(v):
    """A ground plane one unit below the eye from z = 1 to 64 whose 33 x 17 sRGB colour map repeats many times: minified almost
    everywhere, so the sampler reads the generated levels (tests/test_gpu_raster_mipmaps.py has the geometry)."""
    from syzygy_amd import meshes

    corners = [(-64.0, 1.0, 1.0), (64.0, 1.0, 1.0), (64.0, 1.0, 64.0), (-64.0, 1.0, 64.0)]
    uv = [(0.375 * x, 0.375 * z) for x, _, z in corners]
    colour = np.random.default_rng(330 + v).integers(0, 256, (17, 33, 4), dtype=np.uint8)
    material = {"color": (colour, True), "normal": (meshes.constant_texture((127, 127, 255, 0), 16), False),
                "orm": (meshes.constant_texture((255, 60, 0, 0), 8), False)}
    mesh = rs.mesh_of(corners, [0, 1, 2, 0, 2, 3, 2, 1, 0, 3, 2, 0], material=material, uv=uv, normal=(0.0, -1.0, 0.0))
    projection = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0.25], [0, 0, 1, 0]], np.float32)
    return mesh, colour, rs.camera(projection)


class MipCase(Case):
    """szg_record_generate_mipmaps of a 33 x 17 sRGB map against tests/mipmap_model.py, and in the same stream order a G-buffer
    raster that samples the chain just generated. The raster's reference is the same call recorded and synchronised on the
    null stream beforehand, on a pipeline of its own, from a chain generated there (and checked against the model): the
    oracle has no mip sampler, and what is asked here is that the stream-ordered frame is the serial frame, bit for bit."""
    EXTENT = (64, 48)

    def setup(self, gpu):
        s = types.SimpleNamespace(deferred=gpu.pl.DeferredShadingPipeline(self.EXTENT, max_spot_lights=1, max_shadow_maps=0),
                                  serial=gpu.pl.DeferredShadingPipeline(self.EXTENT, max_spot_lights=1, max_shadow_maps=0))
        s.cameras = gpu.pl.TStagedBuffer(abi.CameraPacked, 1)
        return s

    def prepare(self, gpu, s, v):
        from tests import mipmap_model as mm

        torch = gpu.torch
        w, h = self.EXTENT
        r = types.SimpleNamespace()
        r.mesh, colour, r.cam = receding_plane(v)
        upload_meshes([r.mesh])
        r.rect = abi.Rect(0, 0, w, h)
        r.level0 = r.mesh.device_texture(colour).view(17, 33, 4)
        r.levels = mm.level_count(33, 17)
        r.want_chain = mm.pack_chain(mm.build_chain(colour, True))
        # the serial frame
        cameras = gpu.pl.TStagedBuffer(abi.CameraPacked, 1)
        cameras.push(r.cam)
        cameras.recordCopyToDevice()
        r.serial_chain = gpu.pl.generate_mipmaps(r.level0, True)
        s.serial.setTextureMips([(r.level0, r.serial_chain, r.levels)])
        r.serial_target = gpu.pl.SceneTexture(w, h)
        s.serial.recordGBufferRaster(None, r.rect, r.serial_target, 0, cameras, [r.mesh])
        torch.cuda.synchronize()
        same_bits(r.serial_chain.cpu().numpy(), r.want_chain, "the serial chain")
        r.want_planes = s.serial.download_gbuffer(w, h)
        r.want_depth = r.serial_target.depth.cpu().numpy()
        frame = gpu.ob.HostFrame(w, h, debug=False)
        gpu.ob.gbuffer_raster(frame, r.rect, None, r.cam, [r.mesh], threads=4)
        same_bits(r.want_depth, frame.depth, "the serial frame's depth against the oracle")
        same_bits(r.want_planes["worldPosition"], frame.planes()["worldPosition"], "the serial frame's positions against the oracle")
        assert not np.array_equal(r.want_planes["diffuse"], frame.planes()["diffuse"]), "the chain is not sampled: the case checks nothing"
        s.serial.setTextureMips([])
        # what the stream-ordered run writes
        s.cameras.stage([r.cam])
        r.chain = torch.zeros(len(r.want_chain), dtype=torch.uint8, device="cuda")
        r.target = gpu.pl.SceneTexture(w, h)
        r.depth_sentinel = torch.full((h, w), 0.75, dtype=torch.float32, device="cuda")
        r.poison = so.stage_planes(torch, poisoned_planes(self.EXTENT))
        return r

    def enqueue(self, gpu, s, r, S):
        s.cameras.recordCopyToDevice(S)
        r.target.depth.copy_(r.depth_sentinel)
        so.write_planes(S, s.deferred.gbuffer(), r.poison)
        level0 = abi.Texture(r.level0.data_ptr(), 33, 17, 33 * 4, 1)
        rc = lib().szg_record_generate_mipmaps(C.c_void_p(S.cuda_stream), C.byref(level0), C.c_void_p(r.chain.data_ptr()), r.chain.numel())
        assert rc == abi.SZG_OK, lib().szg_last_error()
        s.deferred.setTextureMips([(r.level0, r.chain, r.levels)])
        s.deferred.recordGBufferRaster(S, r.rect, r.target, 0, s.cameras, [r.mesh])

    def check(self, gpu, s, r, what):
        same_bits(r.chain.cpu().numpy(), r.want_chain, f"{what}: the generated chain")
        same_bits(r.target.depth.cpu().numpy(), r.want_depth, f"{what}: depth")
        got = s.deferred.download_gbuffer(*self.EXTENT)
        for name, want in r.want_planes.items():
            same_bits(got[name], want, f"{what}: gbuffer.{name}")


class JpegCase(Case):
    """szg_record_jpeg_reconstruct of a 17 x 9 4:2:0 frame from random coefficient planes into the top-left of a larger, padded
    RGBA8 image (tests/test_gpu_jpeg.py, tests/jpeg_model.py); coefficients and sentinels arrive in stream order."""
    EXTENT, FACTORS = (17, 9), [(2, 2), (1, 1), (1, 1)]

    def prepare(self, gpu, s, v):
        from tests import jpeg_fixtures as jf
        from tests import test_gpu_jpeg as tj

        torch = gpu.torch
        w, h = self.EXTENT
        r = types.SimpleNamespace()
        planes = tj._planes(w, h, self.FACTORS, tj.RANGES[v], seed=170 + v)
        r.staged = [so.staged_tensor(torch, p.reshape(-1)) for p in planes]
        r.live = [torch.zeros_like(t) for t in r.staged]
        r.frame = jf.make_frame(w, h, self.FACTORS, abi.SZG_JPEG_YCBCR, [t.data_ptr() for t in r.live])
        need = lib().szg_jpeg_scratch_bytes(C.byref(r.frame))
        r.scratch = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
        r.sentinel = torch.full((h + 3, w + 5, 4), 0xEE, dtype=torch.uint8, device="cuda")
        r.dst = torch.zeros_like(r.sentinel)
        r.want = np.full((h + 3, w + 5, 4), 0xEE, np.uint8)
        r.want[:h, :w] = tj._model(w, h, self.FACTORS, abi.SZG_JPEG_YCBCR, planes)
        return r

    def enqueue(self, gpu, s, r, S):
        w, h = self.EXTENT
        for live, staged in zip(r.live, r.staged):
            live.copy_(staged)
        r.dst.copy_(r.sentinel)
        gpu.pl.record_jpeg_reconstruct(r.frame, r.dst[:h, :w], cmd=S, scratch=r.scratch)

    def check(self, gpu, s, r, what):
        same_bits(r.dst.cpu().numpy(), r.want, what)


CASES = [
    LutCase("transmittance-lut", which="transmittance"),
    LutCase("multiscatter-lut", which="multiscatter"),
    LutCase("skyview-lut", which="skyview"),
    LutCase("skyview-lut-row-slices", which="skyview-rows"),
    LutCase("aerial-lut", which="aerial"),
    CompositeCase("composite", fast=False),
    CompositeCase("composite-fast", fast=True),
    ChainCase("chained-frame"),
    ChainCase("chained-frame-lut-reuse", reuse=True),
    FillCase("gbuffer-fill"),
    LightsCase("lights-8-spots-shadow-maps"),
    ShadowMapsCase("shadow-maps-analytic"),
    RasterCase("gbuffer-raster-100", scenes=small_soup),
    RasterCase("gbuffer-raster-4608-sorted", scenes=tie_scene),
    ShadowRasterCase("shadow-raster-two-slots"),
    MeshFrameCase("draw-commands-meshes"),
    OetfCase("oetf-srgb", function=abi.SZG_OETF_SRGB),
    OetfCase("oetf-1", function=1),
    ComposeCase("compose-rowtiles"),
    PresentCase("present-rgba8", fmt=abi.SZG_FORMAT_RGBA8_UNORM),
    PresentCase("present-bgra8", fmt=abi.SZG_FORMAT_BGRA8_UNORM),
    PresentCase("present-a2b10g10r10", fmt=abi.SZG_FORMAT_A2B10G10R10_UNORM),
    PresentCase("record-present-oetf-in-place", fmt=abi.SZG_FORMAT_RGBA8_UNORM, in_place=True),
    ComputeCollectionCase("compute-collection-booleanpush", shader="booleanpush"),
    ComputeCollectionCase("compute-collection-gradient_color", shader="gradient_color"),
    ComputeCollectionCase("compute-collection-sparse_push_constant", shader="sparse_push_constant"),
    ComputeCollectionCase("compute-collection-matrix_color", shader="matrix_color"),
    DebugLinesCase("debug-lines-two-boxes"),
    UILayerCase("ui-layer-65-quads-two-textures"),
    MipCase("mip-chain-33x17-and-the-raster-sampling-it"),
    JpegCase("jpeg-reconstruct-17x9-420"),
]


def test_case_table_is_well_formed():
    """What can be checked without a GPU: the helpers import, ids are unique, every case has the five steps, the blocker rule
    keeps its floor, ceiling and the factor of at least four on the host time."""
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        for step in ("setup", "prepare", "enqueue", "check", "teardown"):
            assert callable(getattr(c, step)), (c.id, step)
        assert isinstance(c.conditions, bool)
    assert so.MULTIPLIER >= 4.0 and so.CEILING_MS == 250.0 and so.MAX_STREAMS_PER_CASE == 3
    assert so.blocker_length_ms(0.0, 0.0) == so.FLOOR_MS
    assert so.blocker_length_ms(0.004, 0.005) == so.MULTIPLIER * 5.0 >= 4 * 4.0
    assert so.blocker_length_ms(0.5, 1.0) == so.CEILING_MS
    assert [name for _, name in so.VARIANTS] == ["warm", "behind", "beside"]
    assert len({c.id for c, _, _ in SEQUENCES}) == len(SEQUENCES)
    for c, frames, conditions in SEQUENCES:
        assert callable(c.restage) and 2 <= frames < len(ELEVATIONS) and isinstance(conditions, bool), c.id
    assert len(ELEVATIONS) == len(SPOT_SEEDS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_pass_behind_and_beside_a_blocker(gpu, case):
    so.run_case(gpu, case)


# ---------------------------------------------------------------------------
# state that outlives a call
# ---------------------------------------------------------------------------
def growth_scenes(v):
    """Warm run and frame 1: about 100 primitives (the raster buffers are allocated for 4096). Frame 2: 4608 primitives in more
    draws than before, which grows the draw records and every per-primitive buffer while frame 1 is still in flight."""
    return small_soup(v) if v < 2 else tie_scene(v)


# (case, frames in flight, condition A asserted). The pipeline's staging ring has 8 slots and pipelines.TStagedBuffer 3; a
# slot is rewritten only after its copy has run, so a sequence with more uploads in flight than slots waits in a record call
# by design: those sequences, and the one that grows the raster buffers (include/szg/raster.h "HOST WAITS"), assert the
# images only.
SEQUENCES = [
    (MeshFrameCase("mesh-frames-1-ring-upload-each", SPOTS=0, DIM=0, sky=True), 3, True),   # 3 of 8 ring slots, 3 of 3 staged-buffer slots
    (MeshFrameCase("mesh-frames-5-ring-uploads-each", sky=True), 3, False),                 # 15 uploads through 8 ring slots
    (UILayerCase("ui-draw-lists"), 3, True),
    (UILayerCase("ui-draw-lists-above-the-slot-count"), 5, False),                           # 5 vertex uploads through 3 slots
    (DebugLinesCase("debug-line-sets"), 3, True),
    (DebugLinesCase("debug-line-sets-above-the-slot-count"), 5, False),
    (RasterCase("raster-buffers-grow-in-flight", scenes=growth_scenes), 2, False),           # the wait in ensure_raster_capacity
]


@pytest.mark.gpu
@pytest.mark.parametrize("case,frames,conditions", SEQUENCES, ids=[c.id for c, _, _ in SEQUENCES])
def test_frames_in_flight_behind_one_blocker(gpu, case, frames, conditions):
    report = so.run_sequence(gpu, case, frames, conditions)
    if case.id == "raster-buffers-grow-in-flight":
        # the case does what it is for: the growing call waited for the stream, blocker included
        assert not report["pending_at_return"]


class TwoStreamFrame:
    """One frame of the chained path with the LUT passes on stream `L` and everything else on stream `Cs`, ordered by events
    as the STREAM RULE (include/szg/abi.h) allows and syzygy_amd/rowtile.py does. Parameter buffers and targets are the
    frame's own; the two pipeline objects are shared between the frames."""

    def __init__(self, gpu, inp):
        self.inp, self.params = inp, Params(gpu)
        self.params.stage(inp)
        self.scene = so.stage_scene(padded_scene(gpu))

    def oracle(self, gpu):
        inp = self.inp
        frame = gpu.ob.HostFrame(W, H)
        gpu.ob.gbuffer_fill(frame, inp.rect, None, inp.cam, inp.synthetic.fill, threads=8)
        gpu.ob.lights(frame, inp.rect, None, None, inp.cam, inp.dirs, 2, 1, inp.spots, inp.spot_count, threads=8)
        tlut = gpu.ob.transmittance_lut(inp.atm, TLUT[0], TLUT[1], threads=8)
        slut = gpu.ob.skyview_lut(inp.atm, inp.cam, tlut, SLUT[0], SLUT[1], threads=8)
        gpu.ob.composite(frame, inp.rect, None, None, inp.atm, inp.cam, inp.dirs, 0, tlut, slut, threads=8)
        return frame

    def record(self, gpu, deferred, sky, L, Cs, texels_free=None):
        """`texels_free`: the event behind the composite that last read the LUT texels (None: nothing reads them)."""
        torch, p, inp = gpu.torch, self.params, self.inp
        with torch.cuda.stream(L):
            p.upload(L)
            uploaded = torch.cuda.Event()
            uploaded.record()
        with torch.cuda.stream(Cs):
            Cs.wait_event(uploaded)
            so.write_scene(self.scene)
            deferred.recordDrawCommands(Cs, inp.rect, self.scene, 1, p.lights, inp.spots, 0, p.cameras, inp.synthetic.fill)
        with torch.cuda.stream(L):
            if texels_free is not None:
                L.wait_event(texels_free)
            sky.recordTransmittance(L, 0, p.atmospheres)
            sky.recordSkyViewLUT(L, 0, p.atmospheres, 0, p.cameras)
            luts = torch.cuda.Event()
            luts.record()
        with torch.cuda.stream(Cs):
            Cs.wait_event(luts)
            sky.recordComposite(Cs, self.scene, inp.rect, deferred.gbuffer(), deferred.shadowMaps(), 0, p.atmospheres, 0, p.cameras, 0, p.lights)
            composed = torch.cuda.Event()
            composed.record()
        return composed

    def images(self):
        return {name: im.read() for name, im in self.scene.images().items()}


def _two_streams(gpu, L, Cs):
    import time

    torch = gpu.torch
    deferred = gpu.pl.DeferredShadingPipeline(GBUF_CAP, max_spot_lights=8, max_shadow_maps=0)
    sky = new_sky(gpu)
    try:
        # the single-stream frame of inputs X, then a frame of other inputs that leaves other state in both pipelines
        single = TwoStreamFrame(gpu, inputs(gpu, 0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        single.record(gpu, deferred, sky, Cs, Cs)
        host_s = time.perf_counter() - t0
        Cs.synchronize()
        total_s = time.perf_counter() - t0
        check_frame_images(single.scene, single.oracle(gpu), (W, H), {"color", "depth", "debug_color"}, "single-stream frame")
        want = single.images()
        other = TwoStreamFrame(gpu, inputs(gpu, 3))
        torch.cuda.synchronize()
        other.record(gpu, deferred, sky, Cs, Cs)
        Cs.synchronize()

        # behind a blocker on L: the frame of X again on two streams, then two more frames whose LUT passes are recorded while
        # the composite before them is still queued
        frames = [TwoStreamFrame(gpu, inputs(gpu, v)) for v in (0, 1, 2)]
        ms = so.blocker_length_ms(3 * host_s, 3 * total_s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = gpu.blocker.enqueue(L, ms)
        composed = None
        for f in frames:
            composed = f.record(gpu, deferred, sky, L, Cs, texels_free=composed)
        pending = not done.query()
        returned_ms = (time.perf_counter() - t0) * 1e3
        L.synchronize()
        Cs.synchronize()
        print(f"stream-order two-streams warm_host_ms={host_s * 1e3:.2f} warm_total_ms={total_s * 1e3:.2f} blocker_ms={ms:.2f} "
              f"behind_returned_ms={returned_ms:.2f}")
        assert pending, f"inconclusive: blocker ended before the last record call returned ({ms:.1f} ms blocker, the calls took {returned_ms:.2f} ms)"
        for name, got in frames[0].images().items():
            same_bits(got, want[name], f"two-stream frame against the single-stream frame: {name}")
        for k, f in enumerate(frames[1:]):
            check_frame_images(f.scene, f.oracle(gpu), (W, H), {"color", "depth", "debug_color"}, f"two-stream frame {k + 1} of inputs of its own")
    finally:
        torch.cuda.synchronize()
        deferred.cleanup()
        sky.destroy()


@pytest.mark.gpu
def test_lut_passes_on_a_second_stream_ordered_by_events(gpu):
    import gc

    failure = None
    with so.side_streams(gpu.torch, 2) as (L, Cs):
        try:
            _two_streams(gpu, L, Cs)
        except Exception as e:  # (tests/stream_order.py run_case: what the frames hold must go before the streams do)
            failure = so.failure_text(e)
        gc.collect()
        gpu.torch.cuda.synchronize()
    if failure is not None:
        pytest.fail(failure, pytrace=False)


@pytest.mark.gpu
def test_oetf_table_is_ordered_across_streams_in_a_fresh_process():
    """The transfer tables live for the life of the process (api_image_passes.cpp oetf_table), so the first use has to happen in
    a process of its own: tests/gpu_stream_order_child.py."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_stream_order_child.py")], capture_output=True, text=True, timeout=120)
    lines = [line for line in r.stdout.strip().split("\n") if line.startswith("{")]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(lines[-1])
    print(lines[-1])
    assert r.returncode == 0, (out, r.stderr[-2000:])
    assert sorted(out["functions"]) == ["0", "1"]
    for function, result in out["functions"].items():
        assert result["blocker_pending_when_both_calls_had_returned"], f"inconclusive: blocker ended before the second call returned ({result})"
        assert result["first_stream_equals_model"] and result["second_stream_equals_model"], (function, result)
