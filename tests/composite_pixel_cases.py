"""Hand-made frames for the composite's per-pixel path outside the march (k_composite phases A and C, atmosphere/camera.comp).

tests/composite_gate_cases.py places pixels on the gates of the geometry branch's transmittance samples. This module does the
same for what lies around them: the frame constants k_frame_prep forms once per record call (camera position and radius, the
horizon angles, the sun's projected direction, the draw extent's reciprocals) and the wave-uniform gates of the lean operators
at the per-pixel sites:

  view       |rotation * inverseProjection * clip|^2 in [2^-60, 2^60]                 (normalize of the view direction)
  material   convertPBRLeanOK: max(specular) in [2^-60, 2^60], the numerators of the quotients by it and by pi zero or moderate,
             pow(160, 1 - roughness) inside powLean's domain
  pows       both bases of brdfMix positive normal numbers, the exponents moderate    (the two pow of the BRDF)
  tonemap    the three values in front of pow(., 1.2) positive normal numbers         (phase C)

Every gate has frames with all lanes of a wave inside the domain, all outside, and one lane outside among 63 inside (and the
reverse). One 8x8 tile of a frame is one wave (lane = (y % 8) * 8 + x % 8). Frames are 32x8 (one workgroup), 40x16 (partial
workgroups) or, for the draw extent's own cases, 1x8. numpy and syzygy_amd.abi only; the texel and block builders are those of
tests/composite_gate_cases.py."""
import numpy as np

from syzygy_amd import abi
from tests import composite_gate_cases as cg
from tests import literal_pair as lp

f32 = np.float32
TLUT_EXTENT, SLUT_EXTENT = (64, 16), (128, 64)
px, ORDINARY, METAL = cg.px, cg.ORDINARY, cg.METAL
SKY = px(depth=0.0)
ODD_LANES = (27, 0, 63)


def wave(base, odd=None, lane=27):
    v = [base] * 64
    if odd is not None:
        v[lane] = odd
    return v


def crossing(inside, outside):
    """The four waves of a 32x8 frame: all inside, all outside, one lane outside, one lane inside."""
    return [wave(inside), wave(outside), wave(inside, outside, 27), wave(outside, inside, 27)]


def crossing10(inside, outside):
    """The ten waves of a 40x16 frame: the four of crossing(), the odd lane at both ends of a wave, and ordinary company."""
    return crossing(inside, outside) + [wave(inside, outside, 0), wave(inside, outside, 63), wave(ORDINARY), wave(METAL), wave(SKY),
                                        wave(METAL, outside, 5)]


STANDARD = [wave(ORDINARY), wave(METAL), wave(SKY), wave(ORDINARY, METAL, 27)]
MIXED_SKY = [wave(SKY), wave(SKY, ORDINARY, 27), wave(ORDINARY, SKY, 0), wave(METAL, SKY, 63)]


class Frame:
    def __init__(self, name, waves, extent=(32, 8), camera=cg.CAMERA, inverse_projection=cg.INVERSE_PROJECTION, rotation=None, atm=None,
                 gate=None, side=None):
        self.name, self.waves, self.extent = name, waves, extent
        self.camera, self.inverse_projection, self.rotation, self.atm_edits = camera, inverse_projection, rotation, dict(atm or {})
        self.gate, self.side = gate, side  # which gate the frame is about and where its waves lie: "in", "out", "both", "lane"

    @property
    def atm(self):
        return cg.atmosphere(**self.atm_edits)

    @property
    def cam(self):
        return cg.camera_block(self.camera, self.inverse_projection, self.rotation)

    def images(self):
        """G-buffer planes, depth and prior colour of the draw extent. Tiles past the list are sky."""
        W, H = self.extent
        cols = (W + 7) // 8
        planes = {"diffuse": np.zeros((H, W, 4), np.float16), "specular": np.zeros((H, W, 4), np.float16), "normal": np.zeros((H, W, 4), np.float16),
                  "worldPosition": np.zeros((H, W, 4), f32), "occlusionRoughnessMetallic": np.zeros((H, W, 4), np.float16)}
        depth, prior = np.zeros((H, W), f32), np.zeros((H, W, 4), np.uint16)
        prior[..., 3] = 65535
        ys, xs = np.mgrid[0:H, 0:W]
        prior[..., 0], prior[..., 1], prior[..., 2] = (xs * 977 + ys * 131 + 7) % 20000, (xs * 313 + ys * 71 + 11) % 20000, (xs * 5 + ys * 3 + 1) % 20000
        for y in range(H):
            for x in range(W):
                k = (y // 8) * cols + x // 8
                if k >= len(self.waves):
                    continue
                t = self.waves[k][(y % 8) * 8 + x % 8]
                for plane, key in (("diffuse", "d"), ("specular", "s"), ("normal", "n"), ("worldPosition", "p"), ("occlusionRoughnessMetallic", "o")):
                    planes[plane][y, x, :3] = t[key]
                    planes[plane][y, x, 3] = 1.0
                depth[y, x] = t["depth"]
                if "prior" in t:
                    prior[y, x, :3] = t["prior"]
        return planes, depth, prior


def with_prior(texel, prior):
    t = dict(texel)
    t["prior"] = np.array(prior, np.uint16)
    return t


def zero_at(extent, pixel, a, z):
    """cg._zero_at for a bare extent: the unrotated view vector is (a (cx - cx0), a (cy - cy0), z), the zero vector at `pixel`
    when z is 0."""
    (W, H), (x, y) = extent, pixel
    cx0 = ((f32(x) / f32(W)) - f32(0.5)) * f32(2.0)
    cy0 = ((f32(y) / f32(H)) - f32(0.5)) * f32(2.0)
    return np.array([(a, 0, 0, -f32(a) * cx0), (0, a, 0, -f32(a) * cy0), (0, 0, 0, z), (0, 0, 9.9999008, 9.9999997e-05)], f32)


def looking(y, z):
    """A rotation (rows) that turns the view vector (0, 0, 1, w) of scaled_projection(0, 0) into (0, y, z); the kernel then negates y."""
    return ((1, 0, 0, 0), (0, 0, y, 0), (0, 0, z, 0), (0, 0, 0, 1))


E61 = float(2.0 ** 61)
NIGHT = {"incidentDirectionSun": (0.0, 0.8, -0.6)}


def build():
    F = []
    add = lambda *a, **k: F.append(Frame(*a, **k))
    # --- the frame constants: camera position, altitude, the draw extent
    add("camera_default_zero_x", STANDARD)
    add("camera_zero_z", STANDARD, camera=(5.0, -10.0, 0.0))
    add("camera_x_2^61", STANDARD, camera=(E61, -10.0, -13.0))
    add("camera_y_2^61", STANDARD, camera=(0.0, -E61, -13.0))
    add("camera_half_metre", STANDARD, camera=(0.0, -0.5, 0.0))
    add("camera_30_km", STANDARD, camera=(0.0, -30000.0, 0.0))
    add("camera_30_km_sky", MIXED_SKY, camera=(3.0, -30000.0, 4.0))
    add("camera_underground", STANDARD, camera=(0.0, 20.0, 0.0))
    add("draw_width_1", [wave(ORDINARY)], extent=(1, 8))
    add("draw_width_1_sky", [wave(SKY)], extent=(1, 8))
    add("draw_40x16", STANDARD + MIXED_SKY + [wave(METAL), wave(SKY)], extent=(40, 16))
    # --- view: one pixel's vector exactly zero (a lane outside), every vector overflowing / underflowing (all outside)
    add("view_zero_lane_27", STANDARD, inverse_projection=zero_at((32, 8), (3, 3), 1.0, 0.0), gate="view", side="lane")
    add("view_zero_lane_sky", STANDARD, inverse_projection=zero_at((32, 8), (19, 3), 1.0, 0.0), gate="view", side="lane")
    add("view_overflow", STANDARD, inverse_projection=zero_at((32, 8), (1, 1), 2.0 ** 70, 2.0 ** 70), gate="view", side="out")
    add("view_underflow", STANDARD, inverse_projection=zero_at((32, 8), (1, 1), 2.0 ** -80, 2.0 ** -80), gate="view", side="out")
    # (a squared length that is a denormal number: the generic normalize() still returns a unit vector)
    add("view_denormal_length", STANDARD, inverse_projection=zero_at((32, 8), (1, 1), 2.0 ** -68, 2.0 ** -68), gate="view", side="out")
    add("view_2^-35", STANDARD, inverse_projection=zero_at((32, 8), (1, 1), 2.0 ** -35, 2.0 ** -35), gate="view", side="out")
    add("view_2^31", STANDARD, inverse_projection=zero_at((32, 8), (1, 1), 2.0 ** 31, 2.0 ** 31), gate="view", side="out")
    # --- material
    add("specular_black", crossing10(ORDINARY, px(s=(0.0, 0.0, 0.0))), extent=(40, 16), gate="material", side="both")
    add("specular_black_metal", crossing(METAL, px(s=(0.0, 0.0, 0.0), o=(1.0, 0.25, 1.0))), gate="material", side="both")
    add("specular_half_denormal", crossing(px(s=(cg.HALF_MIN, 0.25, 0.125)), px(s=(0.0, 0.0, -0.0))), gate="material", side="both")
    add("specular_negative_max", crossing(ORDINARY, px(s=(-0.5, -0.25, -1.0))), gate="material", side="both")
    add("specular_nan_component", crossing(ORDINARY, px(s=(0.5, np.nan, 0.125))), gate="material", side="both")
    add("specular_minus_zero_component", crossing(px(s=(0.5, -0.0, 0.125)), px(s=(0.0, 0.0, 0.0))), gate="material", side="both")
    add("roughness_one", crossing10(px(o=(1.0, 60.0 / 255.0, 0.0)), px(o=(1.0, 1.0, 0.0))), extent=(40, 16), gate="material", side="both")
    add("roughness_zero", crossing(px(o=(1.0, 0.0, 0.0)), px(o=(1.0, 1.0, 1.0))), gate="material", side="both")
    add("roughness_inf", crossing(ORDINARY, px(o=(1.0, np.inf, 0.0))), gate="material", side="both")
    add("roughness_nan", crossing(ORDINARY, px(o=(1.0, np.nan, 0.0))), gate="material", side="both")
    add("specular_inf_component", crossing(METAL, px(s=(np.inf, 0.25, 0.125), o=(1.0, 0.25, 1.0))), gate="material", side="both")
    add("diffuse_zero_and_inf", crossing(px(d=(0.0, 0.0, 0.0)), px(d=(np.inf, 0.375, 0.25))), gate="material", side="both")
    add("diffuse_nan", crossing(px(d=(0.5, -0.0, 0.25)), px(d=(0.5, 0.375, np.nan))), gate="material", side="both")
    # --- the surface position (its quotient by 10^6 is the generic one: no gate)
    add("position_2^61", crossing10(px((0.0, -2.0, 5.0)), px((E61, -2.0, 5.0))), extent=(40, 16))
    add("position_y_2^61", crossing(px((1.0, -2.0, 0.0)), px((1.0, -E61, 5.0))))
    add("position_denormal", crossing(px((1.0, -0.0, 5.0)), px((1e-40, -2.0, 5.0))))
    add("position_nan_inf", crossing(ORDINARY, px((np.inf, -2.0, np.nan))))
    # --- the two pow of the BRDF: a normal that faces away from the half vector makes the specular base 0; a NaN normal likewise
    away = px(n=(0.0, 1.0, 0.0))
    add("brdf_base_zero", crossing10(ORDINARY, away), extent=(40, 16), gate="pows", side="both")
    # (a roughness beyond 1 makes the specular exponent 160^(1 - roughness) small: pow(0, .) = 0 and exp(. * log) differ visibly.
    # This normal faces the sun and away from the half vector on part of the wave: the base is 0 on some lanes only.)
    add("brdf_base_zero_small_exponent", crossing(px(o=(1.0, 2.0, 0.0)), px(n=(0.0, 0.25, 1.0), o=(1.0, 2.0, 0.0))), gate="pows", side="both")
    add("brdf_nan_normal", crossing(ORDINARY, px(n=(0.0, np.nan, 0.0))), gate="pows", side="both")
    add("brdf_nan_normal_metal", crossing(METAL, px(n=(np.nan, -1.0, 0.0), o=(1.0, 0.25, 1.0))), gate="pows", side="both")
    # --- phase C: a zero or denormal value in front of pow(., 1.2). With a zero red sun intensity red is the prior colour alone.
    lit, black = with_prior(ORDINARY, (500, 600, 700)), with_prior(ORDINARY, (0, 600, 700))
    add("tonemap_black_red", crossing10(lit, black), extent=(40, 16), atm={"sunIntensitySpectrum": (0.0, 1.0, 1.0)}, gate="tonemap", side="both")
    add("tonemap_denormal_red", crossing(lit, black), atm={"sunIntensitySpectrum": (1e-40, 1.0, 1.0)}, gate="tonemap", side="both")
    add("tonemap_night", crossing(with_prior(ORDINARY, (500, 600, 700)), with_prior(ORDINARY, (0, 0, 0))), atm=NIGHT, gate="tonemap", side="both")
    add("tonemap_negative_intensity", STANDARD, atm={"sunIntensitySpectrum": (1.0, -1.0, 1.0)}, gate="tonemap", side="out")
    # --- reflections of a metal: into the ground, into the sky, exactly vertical (a camera that looks straight down on a level mirror)
    mirror = lambda n: px(n=n, o=(1.0, 0.25, 1.0))
    add("metal_reflection_ground_and_sky", [wave(mirror((1.0, 0.0, 0.0))), wave(mirror((0.0, -1.0, 0.0))), wave(mirror((1.0, 0.0, 0.0)), mirror((0.0, -1.0, 0.0)), 27),
                                            wave(mirror((0.0, -1.0, 0.0)), mirror((0.0, 1.0, 0.0)), 27)])
    down = dict(inverse_projection=cg.scaled_projection(0.0, 0.0), rotation=looking(1.0, 0.0))
    up = dict(inverse_projection=cg.scaled_projection(0.0, 0.0), rotation=looking(-1.0, 0.0))
    level = dict(inverse_projection=cg.scaled_projection(0.0, 0.0))
    add("metal_reflection_vertical", [wave(mirror((0.0, -1.0, 0.0))), wave(ORDINARY), wave(ORDINARY, mirror((0.0, -1.0, 0.0)), 27), wave(SKY)], **down)
    # --- the same three as sky pixels: the view straight down (the ground), level (the sky), straight up (normalize(0, 0))
    add("sky_view_down", MIXED_SKY, **down)
    add("sky_view_up", MIXED_SKY, **up)
    add("sky_view_level", MIXED_SKY, **level)
    add("sky_view_down_30_km", MIXED_SKY, camera=(0.0, -30000.0, 0.0), **down)
    # (sky rays from the camera use the frame's horizon angles and projected sun direction: ordinary cameras; a column of pixels
    # whose view has a horizontal part of exactly 0, of denormal and of small squared length; cameras under the ground)
    all_sky = [wave(SKY)] * 4
    add("sky_ordinary", all_sky, camera=(0.0, -2000.0, 0.0))
    add("sky_ordinary_40x16", [wave(SKY)] * 10, extent=(40, 16), camera=(0.0, -30000.0, 0.0))
    steep = lambda sx: dict(inverse_projection=cg.scaled_projection(sx, 0.0), rotation=looking(-1.0, 0.0))
    add("sky_up_column_vertical", all_sky, **steep(1.0))
    add("sky_up_denormal_horizontal", all_sky, **steep(2.0 ** -70))
    add("sky_up_horizontal_2^-35", all_sky, **steep(2.0 ** -35))
    add("sky_camera_underground", all_sky, camera=(0.0, 20.0, 0.0))
    add("sky_camera_below_lean_floor", all_sky, camera=(0.0, 100000.0, 0.0))
    add("sky_sun_2^-31", all_sky, atm={"incidentDirectionSun": (0.0, 0.0, -(2.0 ** -31))}, **level)
    # --- the view exactly towards and exactly away from the sun (level view along +z), and a quarter turn from it
    for tag, sun in (("towards", (0.0, 0.0, -1.0)), ("away", (0.0, 0.0, 1.0)), ("across", (-1.0, 0.0, 0.0)), ("towards_1%_long", (0.0, 0.0, -1.01))):
        add(f"sun_{tag}", MIXED_SKY, atm={"incidentDirectionSun": sun}, **level)
    add("sun_disc_edge", MIXED_SKY, atm={"incidentDirectionSun": (0.0, -0.009308, -0.99995667)}, **level)
    names = [f.name for f in F]
    assert len(set(names)) == len(names)
    return F


GATES = ("view", "material", "pows", "tonemap")

# the convertPBR cases again for the lights pass, which shares the function
MATERIAL_FRAMES = ("specular_black", "specular_half_denormal", "specular_negative_max", "roughness_one", "roughness_zero", "diffuse_zero_and_inf")

_INPUTS, _ORACLE, _LUTS = {}, {}, {}


class Inputs:
    pass


def luts(atm, cam):
    from oracle import binding as ob

    key = (bytes(atm), bytes(cam))
    if key not in _LUTS:
        tlut = ob.transmittance_lut(atm, TLUT_EXTENT[0], TLUT_EXTENT[1], threads=8)
        slut = ob.skyview_lut(atm, cam, tlut, SLUT_EXTENT[0], SLUT_EXTENT[1], threads=8)
        tlut.setflags(write=False)
        slut.setflags(write=False)
        _LUTS[key] = (tlut, slut)
    return _LUTS[key]


def frame_inputs(frame):
    if frame.name not in _INPUTS:
        f = Inputs()
        f.width, f.height = frame.extent
        f.rect = abi.Rect(0, 0, f.width, f.height)
        f.atm, f.cam = frame.atm, frame.cam
        f.dirs = (abi.DirectionalLightPacked * 2)(cg.shadow_sun(), abi.DirectionalLightPacked())
        f.planes, f.depth, f.prior = frame.images()
        f.tlut, f.slut = luts(f.atm, f.cam)
        for a in (f.depth, f.prior) + tuple(f.planes.values()):
            a.setflags(write=False)
        _INPUTS[frame.name] = f
    return _INPUTS[frame.name]


def host_frame(f):
    from oracle import binding as ob

    frame = ob.HostFrame(f.width, f.height)
    frame.diffuse[:], frame.specular[:], frame.normal[:] = f.planes["diffuse"], f.planes["specular"], f.planes["normal"]
    frame.position[:], frame.orm[:] = f.planes["worldPosition"], f.planes["occlusionRoughnessMetallic"]
    frame.depth[:], frame.color[:] = f.depth, f.prior
    return frame


def oracle_composite(frame):
    """(debug [H, W, 4] float32, colour [H, W, 4] uint16) of oracle.composite over the frame; computed once, read-only."""
    if frame.name not in _ORACLE:
        from oracle import binding as ob

        f = frame_inputs(frame)
        h = host_frame(f)
        ob.composite(h, f.rect, None, None, f.atm, f.cam, f.dirs, 0, f.tlut, f.slut, threads=8)
        h.debug.setflags(write=False)
        h.color.setflags(write=False)
        _ORACLE[frame.name] = (h.debug, h.color)
    return _ORACLE[frame.name]


def spot_lights(count):
    from syzygy_amd import scene

    return scene.spot_ring(count) if count else None


def oracle_lights(frame, spots, count):
    from oracle import binding as ob

    f = frame_inputs(frame)
    h = host_frame(f)
    h.color[:] = 0
    ob.lights(h, f.rect, None, None, f.cam, f.dirs, 2, 1, spots, count, threads=8)
    return h.debug, h.color


def describe(frame, y, x, got, want):
    cols = (frame.extent[0] + 7) // 8
    h = lambda v: "[" + " ".join(f"{int(b):08x}" for b in np.asarray(v, f32).view(np.uint32)) + "]" if np.asarray(v).dtype == f32 else str(list(v))
    return (f"frame {frame.name} (gate {frame.gate}, {frame.side}), texel ({x}, {y}) = wave {(y // 8) * cols + x // 8} lane {(y % 8) * 8 + x % 8}: "
            f"kernel {got} {h(got)}, oracle {want} {h(want)}")


def assert_same(frame, debug, color, want_debug, want_color, what):
    """Bit for bit with no value excluded: the fp32 debug image (NaN for NaN) and the UNORM16 colour."""
    assert debug.shape == want_debug.shape and color.shape == want_color.shape
    lp.compared(want_debug.size + want_color.size)
    same = (debug.view(np.uint32) == want_debug.view(np.uint32)) | (np.isnan(debug) & np.isnan(want_debug))
    bad = np.argwhere(~same.all(axis=-1))
    if len(bad):
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} texels of the debug image differ; first: " + describe(frame, int(y), int(x), debug[y, x, :3], want_debug[y, x, :3]))
    bad = np.argwhere((color != want_color).any(axis=-1))
    if len(bad):
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} texels of the UNORM16 colour differ; first: " + describe(frame, int(y), int(x), color[y, x], want_color[y, x]))
