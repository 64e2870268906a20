"""Mip-mapped material textures through szg_deferred_record_gbuffer_raster (include/szg/mipmaps.h): the table changes nothing
until a chain with more than one level is registered, and the level of detail the kernel picks on a receding ground plane is
the one float64 geometry predicts."""
import ctypes as C

import numpy as np
import pytest

from syzygy_amd import abi, lib, meshes
from tests import mipmap_model as mm
from tests import raster_scenes as rs
from tests import util
from tests.test_raster import _planes_equal, _soup

pytestmark = pytest.mark.gpu
PLANES = ("diffuse", "specular", "normal", "worldPosition", "occlusionRoughnessMetallic")


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    from syzygy_amd import pipelines

    class Ctx:
        pass

    c = Ctx()
    c.pl, c.torch = pipelines, torch
    return c


def _cameras(gpu, cam):
    cameras = gpu.pl.TStagedBuffer(abi.CameraPacked, 1)
    cameras.push(cam)
    cameras.recordCopyToDevice()
    return cameras


class Raster:
    """One pipeline and its target; record(ms) rasters and downloads (planes, depth)."""

    def __init__(self, gpu, W, H, cam, tile=None):
        self.gpu, self.W, self.H, self.tile = gpu, W, H, tile
        self.rows = H if tile is None else tile.local_rows
        self.target = gpu.pl.SceneTexture(W, self.rows)
        self.deferred = gpu.pl.DeferredShadingPipeline((W, self.rows), max_spot_lights=1, max_shadow_maps=0)
        self.cameras = _cameras(gpu, cam)

    def record(self, ms):
        self.deferred.recordGBufferRaster(None, abi.Rect(0, 0, self.W, self.H), self.target, 0, self.cameras, ms, tile=self.tile)
        self.gpu.torch.cuda.synchronize()
        return self.deferred.download_gbuffer(self.W, self.rows), self.target.depth.cpu().numpy().copy()

    def close(self):
        self.deferred.cleanup()


def _assert_same_frame(a, b):
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "depth differs"
    _planes_equal(a[0], b[0])


# ---------------------------------------------------------------------------
# plumbing: a table without a second level, or with max_lod 0, changes no bit
# ---------------------------------------------------------------------------
def _textures_of(ms):
    """[(mesh, texture array, srgb)] once per (mesh, array)."""
    out, seen = [], set()
    for m in ms:
        for _, _, material in m.surfaces:
            for tex, srgb in material.values():
                if (id(m), id(tex)) not in seen:
                    seen.add((id(m), id(tex)))
                    out.append((m, tex, srgb))
    return out


SCENES = {
    "reference_default": meshes.reference_default_scene,
    "soup": lambda: _soup(11, 300),
    "all": lambda: meshes.reference_default_scene() + _soup(3, 120) + meshes.meshes_of_fill_scene(util.Inputs(8, 8).synthetic.fill),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_tables_without_a_reachable_second_level_change_nothing(gpu, name):
    W, H = 97, 61
    inp = util.Inputs(W, H)
    ms = SCENES[name]()
    r = Raster(gpu, W, H, inp.cam)
    base = r.record(ms)
    assert (base[1] > 0).mean() > 0.05
    textures = _textures_of(ms)
    level0 = [m.device_texture(tex) for m, tex, _ in textures]
    # entries that all say "one level"
    r.deferred.setTextureMips([(t, 0, 1) for t in level0], mm.MAX_LOD_NONE)
    _assert_same_frame(r.record(ms), base)
    # full chains, max_lod = 0
    chains = [gpu.pl.generate_mipmaps(t.view(tex.shape[0], tex.shape[1], 4), srgb) for t, (_, tex, srgb) in zip(level0, textures)]
    full = [(t, c if c.numel() else 0, mm.level_count(tex.shape[1], tex.shape[0])) for t, c, (_, tex, _) in zip(level0, chains, textures)]
    full = [(t, c, n if n > 1 else 1) for t, c, n in full]
    assert any(n > 1 for _, _, n in full)
    r.deferred.setTextureMips(full, 0.0)
    _assert_same_frame(r.record(ms), base)
    # the same chains with the clamp lifted: coverage and depth do not depend on the table (what the colour then reads is the
    # subject of the plane tests below; these scenes' small maps are magnified almost everywhere)
    r.deferred.setTextureMips(full, mm.MAX_LOD_NONE)
    lifted = r.record(ms)
    assert np.array_equal(lifted[1].view(np.uint32), base[1].view(np.uint32))
    assert np.array_equal(lifted[0]["worldPosition"].view(np.uint32), base[0]["worldPosition"].view(np.uint32))
    # and clearing the table brings the base image back
    r.deferred.setTextureMips([])
    _assert_same_frame(r.record(ms), base)
    r.close()


def test_a_level_count_above_the_textures_own_is_refused_at_record_time(gpu):
    W, H = 32, 16
    inp = util.Inputs(W, H)
    ms = meshes.reference_default_scene()  # 64 x 64 maps: 7 levels
    r = Raster(gpu, W, H, inp.cam)
    r.record(ms)
    tex = ms[0].surfaces[0][2]["color"][0]
    chain = gpu.torch.zeros(mm.chain_bytes(64, 64), dtype=gpu.torch.uint8, device="cuda")
    r.deferred.setTextureMips([(ms[0].device_texture(tex), chain, 8)])
    arr = meshes.mesh_array(ms, "cuda")
    st = r.target.abi()
    status = lib().szg_deferred_record_gbuffer_raster(r.deferred._h, None, abi.Rect(0, 0, W, H), None, C.byref(st), 0,
                                                      C.c_void_p(r.cameras.deviceAddress()), arr, len(ms))
    assert status == abi.SZG_ERR_INVALID_ARGUMENT
    assert b"level_count 8" in lib().szg_last_error() and b"7 levels" in lib().szg_last_error()
    r.deferred.setTextureMips([(ms[0].device_texture(tex), chain, 7)])
    r.record(ms)
    r.close()


# ---------------------------------------------------------------------------
# LOD end to end: a receding ground plane whose colour chain is colour-coded by level
# ---------------------------------------------------------------------------
W, H = 128, 96
TEX = 128                 # colour map 128 x 128, 8 levels, level k uniform with byte 32 k
Z_NEAR, Z_FAR = 1.0, 64.0  # the plane y = 1 (one unit below the eye; +y is down the screen), z from 1 to 64, |x| <= 64
UV_SCALE = 0.375          # u = 0.375 x, v = 0.375 z: exactly representable at the four vertices
# clip = (x, y, 0.25, z): a pinhole along +z, depth 0.25 / z inside (0, 1]
PROJECTION = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0.25], [0, 0, 1, 0]], np.float32)


def _plane_scene():
    corners = [(-64.0, 1.0, Z_NEAR), (64.0, 1.0, Z_NEAR), (64.0, 1.0, Z_FAR), (-64.0, 1.0, Z_FAR)]
    uv = [(UV_SCALE * x, UV_SCALE * z) for x, _, z in corners]
    colour = np.zeros((TEX, TEX, 4), np.uint8)
    material = {"color": (colour, False), "normal": (meshes.constant_texture((127, 127, 255, 0), 16), False),
                "orm": (meshes.constant_texture((255, 60, 0, 0), 8), False)}
    # both windings: back-face culling keeps the one that faces the eye
    return rs.mesh_of(corners, [0, 1, 2, 0, 2, 3, 2, 1, 0, 3, 2, 0], material=material, uv=uv, normal=(0.0, -1.0, 0.0)), material


def _coded_chain():
    return np.concatenate([np.full(wk * hk * 4, 32 * k, np.uint8) for k, (wk, hk) in enumerate(mm.level_shapes(TEX, TEX))][1:])


def _expected_lambda():
    """float64: uv at every pixel centre by intersecting its ray with the plane, the quad differences the kernel takes (right
    minus left, bottom minus top), and lambda from them. Returns lam, on_plane, whole_quad (every pixel of the 2x2 quad on
    the plane), uv [H, W, 2] and the per-pixel uv step lambda is made of."""
    px = (np.arange(W) + 0.5)[None, :] * np.ones((H, 1))
    py = (np.arange(H) + 0.5)[:, None] * np.ones((1, W))
    ndc_x, ndc_y = 2.0 * px / W - 1.0, 2.0 * py / H - 1.0
    # the ray through (ndc_x, ndc_y) is (ndc_x, ndc_y, 1) t; it meets y = 1 at t = z = 1 / ndc_y
    with np.errstate(divide="ignore"):
        z = np.where(ndc_y > 0, 1.0 / np.where(ndc_y > 0, ndc_y, 1.0), np.inf)
    x = ndc_x * z
    on_plane = (z >= Z_NEAR) & (z <= Z_FAR) & (np.abs(x) <= 64.0)
    uv = np.stack([UV_SCALE * x, UV_SCALE * z], axis=-1)
    left, right = uv[:, 0::2], uv[:, 1::2]
    top, bottom = uv[0::2], uv[1::2]
    with np.errstate(invalid="ignore", divide="ignore"):  # pixels above the horizon carry inf; they are never compared
        ddx = np.repeat(right - left, 2, axis=1)
        ddy = np.repeat(bottom - top, 2, axis=0)
        r2 = np.maximum((ddx[..., 0] * TEX) ** 2 + (ddx[..., 1] * TEX) ** 2, (ddy[..., 0] * TEX) ** 2 + (ddy[..., 1] * TEX) ** 2)
        lam = 0.5 * np.log2(r2)
    quad = on_plane[0::2, 0::2] & on_plane[0::2, 1::2] & on_plane[1::2, 0::2] & on_plane[1::2, 1::2]
    whole_quad = np.repeat(np.repeat(quad, 2, axis=0), 2, axis=1)
    step = np.sqrt(r2) / TEX  # the per-pixel uv step lambda is made of
    return lam, on_plane, whole_quad, uv, step


@pytest.fixture(scope="module")
def plane(gpu):
    """The plane rastered once per configuration, shared by the tests below."""
    mesh, material = _plane_scene()
    cam = rs.camera(PROJECTION)
    ms = [mesh]
    r = Raster(gpu, W, H, cam)
    t = gpu.torch
    colour_chain = t.from_numpy(_coded_chain()).cuda()
    entries = [(mesh.device_texture(material["color"][0]), colour_chain, 8)]
    for key in ("normal", "orm"):  # uniform at every level: their LOD does not show
        tex = material[key][0]
        level0 = mesh.device_texture(tex)
        chain = gpu.pl.generate_mipmaps(level0.view(tex.shape[0], tex.shape[1], 4), False)
        want = np.concatenate([np.tile(tex[0, 0], wk * hk) for wk, hk in mm.level_shapes(tex.shape[1], tex.shape[0])[1:]])
        assert np.array_equal(chain.cpu().numpy(), want)
        entries.append((level0, chain, mm.level_count(tex.shape[1], tex.shape[0])))
    out = {"mesh": ms, "cam": cam, "entries": entries}
    out["base"] = r.record(ms)
    r.deferred.setTextureMips(entries, mm.MAX_LOD_NONE)
    out["mips"] = r.record(ms)
    r.deferred.setTextureMips(entries, mm.MAX_LOD_REFERENCE)
    out["reference"] = r.record(ms)
    r.deferred.setTextureMips([])
    out["cleared"] = r.record(ms)
    r.close()
    return out


def test_lod_on_a_receding_plane_is_the_one_geometry_predicts(plane):
    planes, depth = plane["mips"]
    lam, on_plane, whole_quad, uv, step = _expected_lambda()
    assert np.array_equal(depth > 0, on_plane), "coverage differs from the geometry"
    compare = on_plane & whole_quad
    share = compare.sum() / on_plane.sum()
    print(f"plane pixels {on_plane.sum()}, compared {compare.sum()} ({share:.3f})")
    assert share >= 0.9
    want = np.clip(lam, 0.0, 7.0)
    got = planes["diffuse"][..., 0].astype(np.float64) * 255.0 / 32.0
    # tolerance, in levels, from the scene's numbers:
    #   the fp16 store of a value below 1 moves it by at most 2^-12, times 255 / 32
    store = 2.0**-12 * 255.0 / 32.0
    #   the fp32 interpolation of uv moves a quad difference by about 2^-23 |uv|max; relative to the smallest per-pixel
    #   uv step that is the relative error of the footprint, and so (up to 1 / ln 2 against the factor 2 below) of lambda
    interpolation = 2.0**-23 * np.abs(uv[compare]).max() / step[compare].min()
    print(f"|uv|max {np.abs(uv[compare]).max():.3f}, smallest step {step[compare].min():.6f}: store {store:.3e}, interpolation {interpolation:.3e}")
    assert store < 2.0**-9 and interpolation < 2.0**-9
    tolerance = 2.0 * (store + interpolation)
    err = np.abs(got - want)[compare]
    print(f"lambda spans {want[compare].min():.3f} .. {want[compare].max():.3f}; max |lam_gpu - lam| {err.max():.3e}, tolerance {tolerance:.3e}")
    assert err.max() <= tolerance
    assert want[compare].min() <= 0.5 and want[compare].max() >= 4.0
    blended = (want[compare] % 1.0 > 0.05) & (want[compare] % 1.0 < 0.95)
    assert blended.mean() > 0.5  # most pixels lie between two levels
    # green and blue carry the same codes; specular repeats diffuse (offscreen.frag:72-75)
    assert np.array_equal(planes["diffuse"][..., 1].view(np.uint16), planes["diffuse"][..., 0].view(np.uint16))
    assert np.array_equal(planes["specular"].view(np.uint16), planes["diffuse"].view(np.uint16))


def test_only_the_colour_changes_on_the_plane(plane):
    (base, base_depth), (mips, depth) = plane["base"], plane["mips"]
    assert np.array_equal(base_depth.view(np.uint32), depth.view(np.uint32))
    assert np.array_equal(base["worldPosition"].view(np.uint32), mips["worldPosition"].view(np.uint32))
    # The normal and ORM maps are uniform at every level, but the bilinear weights of two levels differ, so a blended value
    # is the level-0 value up to a few fp32 roundings (2^-22 relative): far below an fp16 step, so a stored code moves by at
    # most one step (2^-10 relative), and only where the value sits on a rounding boundary.
    for name in ("normal", "occlusionRoughnessMetallic"):
        a, b = base[name].astype(np.float64), mips[name].astype(np.float64)
        assert (np.abs(a - b) <= 2.0**-10 * np.abs(a) + 2.0**-20).all(), name  # (+ the fp32 perturbation itself, near 0)
        assert (base[name] != mips[name]).mean() < 0.01, name
    assert (base["diffuse"][..., :3] == 0).all()  # level 0 is black


def test_reference_max_lod_never_passes_level_1(plane):
    planes, _ = plane["reference"]
    code = np.float16(np.float32(32.0) / np.float32(255.0))
    assert planes["diffuse"][..., :3].max() <= code
    lam = _expected_lambda()[0]
    far = (plane["reference"][1] > 0) & (lam > 1.5)
    assert far.any() and (planes["diffuse"][..., 0][far] == code).all()


def test_clearing_the_table_restores_the_base_image(plane):
    _assert_same_frame(plane["cleared"], plane["base"])


def test_row_tiles_equal_the_untiled_frame(gpu, plane):
    full_planes, full_depth = plane["mips"]
    for rank in range(3):
        tile = util.rowtile(H, 8, rank, 3)
        rows = util.global_rows(H, 8, rank, 3)
        r = Raster(gpu, W, H, plane["cam"], tile=tile)
        r.deferred.setTextureMips(plane["entries"], mm.MAX_LOD_NONE)
        planes, depth = r.record(plane["mesh"])
        r.close()
        assert np.array_equal(depth.view(np.uint32), full_depth[rows].view(np.uint32))
        _planes_equal(planes, {name: full_planes[name][rows] for name in PLANES})
