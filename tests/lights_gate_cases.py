"""Hand-made pixel-light pairs for the lights pass (k_light_prep / k_lights, deferred/lights.comp) and a census of its gates.

k_lights decides for every pixel-light pair whether it is evaluated and by which arithmetic; every decision is a threshold,
several are taken per wave. This module places pairs ON those thresholds, on both sides of them and at their float32
neighbours, and says - by a float64 model written from lights.comp and the kernel's comments, not by calling the oracle - on
which side of which gate each pair lies. numpy only; tests/test_lights_gate_cases.py checks the coverage and the oracle against
the census without a GPU, tests/test_gpu_lights_gates.py runs the same cases through recordLights.

LIGHTS are SpotLightPacked records written field by field. Their matrices hold powers of two, so the clip coordinates of a
chosen position are known: for the plain light at the origin, cw = p.z, cx = 0.5 p.x + 0.5 p.z, cy = 0.5 p.y + 0.5 p.z; the
cone's rim q = 0.25 is x^2 + y^2 = z^2. `forward` is (0, 0, 1), so the light direction is (0, 0, -1) and N.L = -normal.z,
one half-precision component. The `position` field (which only enters the distance) and the view matrix's translation
(which only enters the clip coordinates) are independent fields of the record; one light uses that to move d^2 away from cw.

PIXELS are G-buffer texels laid out in 8x8 tiles, one tile = one wave of k_lights (pixel_of_thread_bottom_up: lane =
(y % 8) * 8 + x % 8) = one SCENARIO. A scenario has a form:
  uniform   all 64 lanes hold one variant,
  mixed<k>  lane k (0, 63 or the interior lane 27) holds another variant than the other 63,
  partial   as mixed with the odd lane at 34, every third lane background (diffuse.w < 1); the tiles of the last column and the
            last row of a group's image are cut by the draw extent as well.
A GROUP is one recordLights call: lights, shadow maps, skip count, camera position, and a grid of scenarios.
"""
import ctypes as C

import numpy as np

from syzygy_amd import abi

f32, f64 = np.float32, np.float64
LANES = 64
MIXED_LANES = (0, 63, 27)
PARTIAL_LANE = 34  # row 4, column 2: inside the draw extent in a cut tile too
FORMS = ("uniform", "mixed0", "mixed63", "mixed27", "partial")
BAND = 2.0 ** -20  # "near a threshold": within this relative distance
COLS = 16          # tiles per row of a group's image
CUT = (3, 2)       # the draw extent ends this many texels before the last tile column / row does
HALF_MIN = 2.0 ** -24  # smallest half denormal


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def dn(x):
    return np.nextafter(f32(x), f32(-np.inf))


def rel(x, k):
    """x * (1 + k 2^-22): four float32 steps from x per unit of k. A quantity derived from x, linearly or as its square, is then
    still inside the 2^-20 band for |k| <= 1 and further from the threshold than its own float32 rounding."""
    return f32(f64(f32(x)) * (1.0 + k * 2.0 ** -22))


# ---------------------------------------------------------------------------------------------------------------------------
# lights
# ---------------------------------------------------------------------------------------------------------------------------
class Light:
    def __init__(self, name, position=(0, 0, 0), distance_position=None, xrow=(1, 0, 0, 0), yrow=(0, 1, 0, 0), zrow=(0, 0, 0.25, 0.125),
                 wscale=1.0, color=(1, 1, 1), strength=1.0, factor=1.0, distance=1.0, shadow=None, unit=1.0):
        self.name, self.shadow, self.unit = name, shadow, f64(unit)
        self.center = np.array(position, f32)  # the apex of the cone (translation of the view matrix)
        proj = np.zeros((4, 4), f32)
        proj[0], proj[1], proj[2], proj[3] = xrow, yrow, zrow, (0, 0, wscale, 0)
        view = np.eye(4, dtype=f32)
        view[:3, 3] = -self.center
        p = abi.SpotLightPacked()
        p.projection, p.view = abi.Mat4.from_numpy(proj), abi.Mat4.from_numpy(view)
        p.color[:] = [float(f32(c)) for c in color] + [1.0]
        p.forward[:] = [0.0, 0.0, 1.0, 0.0]
        p.position[:] = [float(v) for v in (self.center if distance_position is None else np.array(distance_position, f32))] + [1.0]
        p.strength, p.falloffFactor, p.falloffDistance = float(f32(strength)), float(f32(factor)), float(f32(distance))
        self.packed = p
        # --- the record as k_light_prep forms it
        to_tex = np.array([[0.5, 0, 0, 0.5], [0, 0.5, 0, 0.5], [0, 0, 1, 0], [0, 0, 0, 1]], f64)
        self.rows = (to_tex @ proj.astype(f64) @ view.astype(f64)).astype(f32)  # exact for the records below: powers of two
        self.position = np.array(p.position[:3], f32)
        self.dir = np.array([0.0, 0.0, -1.0])
        self.cs = np.array(p.color[:3], f32) * f32(p.strength)
        self.factor, self.distance = f32(p.falloffFactor), f32(p.falloffDistance)
        lo, hi = f32(2.0 ** -30), f32(2.0 ** 30)
        cs_ok = all(c == 0 or lo <= abs(c) <= hi for c in self.cs)
        rows_ok = bool((np.abs(self.rows) <= f32(2.0 ** 28)).all())
        lean = cs_ok and rows_ok and bool((np.abs(self.position) <= hi).all()) and lo <= self.distance <= hi and lo <= self.factor <= hi
        with np.errstate(all="ignore"):
            rcp = f32(1.0) / self.distance                 # rcpN: the correctly rounded reciprocal
            self.fb_raw = f32(f32(self.factor * rcp) * rcp)  # falloffFactor * rcp * rcp, float32, before leanOK clears it
        if lean and not (lo <= self.fb_raw <= hi):
            lean = False
        self.lean = lean
        self.falloff_bound = self.fb_raw if lean else f32(0.0)
        self.tight = lean and bool((np.abs(self.position) <= f32(4096.0)).all()) and f32(2.0 ** -20) <= self.fb_raw <= f32(2.0 ** 20) and \
            bool((np.abs(self.rows) <= f32(2.0 ** 14)).all())

    def at(self, x, y, z):
        """A world position given relative to the cone's apex, x and y in units of the cone's half width at depth 1."""
        return (self.center.astype(f64) + np.array([x * self.unit, y * self.unit, z], f64)).astype(f32)


def lights():
    """name -> Light. The comment says which flag of k_light_prep the record is for and by which single criterion."""
    P12, P14, P20, P28, P30 = 2.0 ** 12, 2.0 ** 14, 2.0 ** 20, 2.0 ** 28, 2.0 ** 30
    pcf = (0, 0, 0.25, 0.125)  # sz = (0.25 z + 0.125) / z: 0.3125 at z = 2
    L = [
        Light("tight"),                                                          # tight
        Light("tight_shift", xrow=(1, 0, -1, 0), yrow=(0, 1, -1, 0)),            # tight; cx = 0.5 x, cy = 0.5 y, cw = z
        Light("tight_cz", zrow=(0, 1, 0, 0), shadow="random"),                   # tight, with a map; cz = y
        Light("tight_cz_denormal", zrow=(0, 1, 0, 0), shadow="denormal"),        # tight, cz = y; the map holds the depth 2^-130
        Light("tight_far_d2", distance_position=(0, 0, -1)),                     # tight; d^2 ~ 1 whatever cw = z is
        Light("lean_w20", wscale=P20),                                           # leanOK, not tight (row 2^20); cw = 2^20 z
        Light("tight_pos_on", position=(P12, 0, 0)),                             # tight: position exactly 2^12
        Light("lean_pos_above", position=(up(P12), 0, 0)),                       # not tight: position just above 2^12
        # not tight by its position alone, as far out as leanOK admits, nothing a power of two: d^2 ~ 2^61, falloff ~ 2^81
        Light("lean_pos_2^30", distance_position=(2.0 ** 30, -0.75 * 2.0 ** 30, 1.1 * 2.0 ** 29), factor=1.7 * 2.0 ** 19, color=(1.3 * 2.0 ** -30, 1, 1.9)),
        Light("tight_row_on", xrow=(2 * P14, 0, 0, 0), unit=1 / (2 * P14)),      # tight: a row entry of exactly 2^14
        Light("lean_row_above", xrow=(up(2 * P14), 0, 0, 0), unit=1 / (2 * P14)),  # not tight: a row entry just above 2^14
        Light("tight_fb_hi_on", factor=P20), Light("lean_fb_hi_above", factor=up(P20)),          # falloffBound at 2^20
        Light("tight_fb_lo_on", factor=1 / P20), Light("lean_fb_lo_below", factor=dn(1 / P20)),  # falloffBound at 2^-20
        Light("lean_cs_on", color=(1 / P30, 1, 1)),                              # leanOK: a colour * strength component of exactly 2^-30
        Light("generic_cs_below", color=(dn(1 / P30), 1, 1)),                    # not leanOK: a component just below 2^-30
        Light("lean_cs_zero", color=(0, 1, 1)),                                  # a component exactly 0: k_light_prep accepts it (numerator())
        Light("lean_row_on", xrow=(2 * P28, 0, 0, 0), unit=1 / (2 * P28)),       # leanOK: a row entry of exactly 2^28
        Light("generic_row_above", xrow=(up(2 * P28), 0, 0, 0), unit=1 / (2 * P28)),  # not leanOK: a row entry just above 2^28
        # falloffBound = factor / distance^2 just outside 2^+-30 with factor and distance each inside their own range
        Light("lean_fb30_hi_on", factor=P20, distance=2.0 ** -5), Light("generic_fb30_hi_above", factor=P20, distance=dn(2.0 ** -5)),
        Light("lean_fb30_lo_on", factor=1 / P20, distance=2.0 ** 5), Light("generic_fb30_lo_below", factor=1 / P20, distance=up(2.0 ** 5)),
        # shadow PCF: maps of 12 x 6 texels
        Light("pcf_random", zrow=pcf, shadow="random"), Light("pcf_equal", zrow=pcf, shadow="equal"),
        Light("pcf_zero", zrow=pcf, shadow="zero"), Light("pcf_nearer", zrow=pcf, shadow="nearer"),
    ]
    return {l.name: l for l in L}


LIGHT_FLAGS = {  # what the census must find for each record: (leanOK, tight)
    "tight": (1, 1), "tight_shift": (1, 1), "tight_cz": (1, 1), "tight_cz_denormal": (1, 1), "lean_pos_2^30": (1, 0), "tight_far_d2": (1, 1), "lean_w20": (1, 0), "tight_pos_on": (1, 1),
    "lean_pos_above": (1, 0), "tight_row_on": (1, 1), "lean_row_above": (1, 0), "tight_fb_hi_on": (1, 1), "lean_fb_hi_above": (1, 0),
    "tight_fb_lo_on": (1, 1), "lean_fb_lo_below": (1, 0), "lean_cs_on": (1, 1), "generic_cs_below": (0, 0), "lean_cs_zero": (1, 1),
    "lean_row_on": (1, 0), "generic_row_above": (0, 0), "lean_fb30_hi_on": (1, 0), "generic_fb30_hi_above": (0, 0),
    "lean_fb30_lo_on": (1, 0), "generic_fb30_lo_below": (0, 0), "pcf_random": (1, 1), "pcf_equal": (1, 1), "pcf_zero": (1, 1),
    "pcf_nearer": (1, 1),
}
MAP_W, MAP_H, MAP_PAD = 12, 6, 5  # not powers of two; rows 5 texels wider than the map


def shadow_map(kind):
    """[MAP_H, MAP_W] float32 view of a buffer with MAP_PAD more texels per row, the padding holding the nearest occluder."""
    buf = np.ones((MAP_H, MAP_W + MAP_PAD), f32)
    m = buf[:, :MAP_W]
    if kind == "random":
        m[:] = np.random.default_rng(0x6A7E).random((MAP_H, MAP_W), dtype=f32)
    elif kind == "equal":
        m[:] = f32(0.3125)       # the fragment depth of a pixel at z = 2
    elif kind == "zero":
        m[:] = 0.0               # "no occluder" (shadowmap.glinl: occluderDepth > 0)
    elif kind == "denormal":
        m[:] = f32(2.0 ** -130)
    elif kind == "nearer":
        m[:] = up(0.3125)
    else:
        raise KeyError(kind)
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# pixels, scenarios, groups
# ---------------------------------------------------------------------------------------------------------------------------
def px(p, n=(0, 0, -1), d=(0.5, 0.375, 0.25), s=(0.5, 0.25, 0.125), o=(1.0, 0.5, 0.25), a=1.0):
    """One G-buffer texel: position, normal, diffuse rgb, specular rgb, (occlusion, roughness, metallic), diffuse alpha."""
    return {"p": np.array(p, f32), "n": np.array(n, np.float16), "d": np.array(d, np.float16), "s": np.array(s, np.float16),
            "o": np.array(o, np.float16), "a": np.float16(a)}


class Scenario:
    def __init__(self, group, family, name, form, base, odd=None, odd_lane=None):
        self.group, self.family, self.name, self.form, self.odd_lane = group, family, name, form, odd_lane
        v = [base] * LANES
        if odd is not None:
            v[odd_lane] = odd
        self.planes = {k: np.stack([t[k] for t in v]) for k in ("p", "n", "d", "s", "o")}
        self.alpha = np.array([t["a"] for t in v], np.float16)
        if form == "partial":
            background = (np.arange(LANES) % 3 == 0)
            self.alpha = np.where(background, np.float16(0.5), self.alpha).astype(np.float16)


class Group:
    def __init__(self, name, light_names, skip=2, camera=(3, 0, -2), maps_on_directional=()):
        self.name, self.light_names, self.skip, self.camera = name, list(light_names), skip, np.array(camera, f32)
        self.maps_on_directional, self.scenarios = tuple(maps_on_directional), []

    def add(self, family, name, near, far, on=None):
        """Every form of one crossing of a gate: `near` and `far` lie on its two sides, `on` exactly on it where that exists."""
        S = lambda *a, **k: self.scenarios.append(Scenario(self, family, *a, **k))
        variants = [("near", near), ("far", far)] + ([("on", on)] if on is not None else [])
        for tag, v in variants:
            S(f"{name}/uniform-{tag}", "uniform", v)
        for lane in MIXED_LANES:
            S(f"{name}/mixed{lane}-far-among-near", f"mixed{lane}", near, far, lane)
            S(f"{name}/mixed{lane}-near-among-far", f"mixed{lane}", far, near, lane)
            if on is not None:
                S(f"{name}/mixed{lane}-on-among-near", f"mixed{lane}", near, on, lane)
        S(f"{name}/partial-far-among-near", "partial", near, far, PARTIAL_LANE)
        S(f"{name}/partial-near-among-far", "partial", far, near, PARTIAL_LANE)
        if on is not None:
            S(f"{name}/partial-on-among-near", "partial", near, on, PARTIAL_LANE)

    # -- geometry of the image
    @property
    def tiles(self):
        return len(self.scenarios)

    @property
    def extent(self):
        cols = min(COLS, self.tiles)
        rows = (self.tiles + cols - 1) // cols
        return cols * 8 - CUT[0], rows * 8 - CUT[1]

    def origin(self, k):
        cols = min(COLS, self.tiles)
        return (k % cols) * 8, (k // cols) * 8

    def slot(self, j, dir_count=2):
        """Shadow-map slot of spot light j (lights.comp:138-161): counted from the skip count over the directional lights that
        are evaluated, then the spot lights."""
        return self.skip + max(0, dir_count - self.skip) + j

    def planes(self):
        """The five G-buffer planes [H8, W8, 4] at whole tiles (the draw extent is smaller: `extent`)."""
        cols = min(COLS, self.tiles)
        rows = (self.tiles + cols - 1) // cols
        H, W = rows * 8, cols * 8
        out = {"diffuse": np.zeros((H, W, 4), np.float16), "specular": np.zeros((H, W, 4), np.float16), "normal": np.zeros((H, W, 4), np.float16),
               "worldPosition": np.zeros((H, W, 4), f32), "occlusionRoughnessMetallic": np.zeros((H, W, 4), np.float16)}
        for k, sc in enumerate(self.scenarios):
            x0, y0 = self.origin(k)
            tile = lambda a: a.reshape(8, 8, -1)
            out["diffuse"][y0:y0 + 8, x0:x0 + 8, :3] = tile(sc.planes["d"])
            out["diffuse"][y0:y0 + 8, x0:x0 + 8, 3] = sc.alpha.reshape(8, 8)
            out["specular"][y0:y0 + 8, x0:x0 + 8, :3] = tile(sc.planes["s"])
            out["specular"][y0:y0 + 8, x0:x0 + 8, 3] = 1.0
            out["normal"][y0:y0 + 8, x0:x0 + 8, :3] = tile(sc.planes["n"])
            out["worldPosition"][y0:y0 + 8, x0:x0 + 8, :3] = tile(sc.planes["p"])
            out["worldPosition"][y0:y0 + 8, x0:x0 + 8, 3] = 1.0
            out["occlusionRoughnessMetallic"][y0:y0 + 8, x0:x0 + 8, :3] = tile(sc.planes["o"])
            out["occlusionRoughnessMetallic"][y0:y0 + 8, x0:x0 + 8, 3] = 1.0
        return out

    def active(self, k):
        """bool [64]: the lanes of scenario k's wave that evaluate lights: inside the draw extent and not background."""
        x0, y0 = self.origin(k)
        W, H = self.extent
        lane = np.arange(LANES)
        inside = (x0 + lane % 8 < W) & (y0 + lane // 8 < H)
        return inside & ~(self.scenarios[k].alpha.astype(f32) < 1.0)

    def spot_array(self, L):
        arr = (abi.SpotLightPacked * len(self.light_names))()
        for i, n in enumerate(self.light_names):
            arr[i] = L[n].packed
        return arr

    def shadow_maps(self, L):
        """slot -> map view, for the spot lights that have one and the directional slots asked for."""
        maps = {self.slot(j): shadow_map(L[n].shadow) for j, n in enumerate(self.light_names) if L[n].shadow is not None}
        for slot in self.maps_on_directional:
            maps[slot] = shadow_map("random")
        return maps

    @property
    def slot_count(self):
        return self.slot(len(self.light_names)) + 1


FAMILIES = ("cone_exact", "cone_reject", "clip_w", "guard", "back_face", "pixel_flags", "half_vector", "track", "shadow_pcf",
            "light_flags", "slots")


def build():
    """(lights, groups). Deterministic; a few thousand tiles in all."""
    L = lights()
    G = []

    def group(*a, **k):
        g = Group(*a, **k)
        G.append(g)
        return g

    T = L["tight"]
    inside = px(T.at(0.25, 0.125, 2))
    outside = px(T.at(5, 0.5, 2))
    P12, P30 = 2.0 ** 12, 2.0 ** 30

    # --- cone, exact cull q >= 0.25: the rim is x^2 + y^2 = z^2
    g = group("cone_exact", ["tight"])
    g.add("cone_exact", "rim-x-step", px((dn(2), 0, 2)), px((up(2), 0, 2)), px((2, 0, 2)))
    g.add("cone_exact", "rim-x-band", px((rel(2, -1), 0, 2)), px((rel(2, 1), 0, 2)))
    g.add("cone_exact", "rim-negx-step", px((-dn(2), 0, 2)), px((-up(2), 0, 2)), px((-2, 0, 2)))
    g.add("cone_exact", "rim-y-step", px((0, dn(2), 2)), px((0, up(2), 2)), px((0, 2, 2)))
    g.add("cone_exact", "rim-y-band", px((0, rel(2, -1), 2)), px((0, rel(2, 1), 2)))
    g.add("cone_exact", "rim-345-step", px((dn(1.5), 2, 2.5)), px((up(1.5), 2, 2.5)), px((1.5, 2, 2.5)))
    g.add("cone_exact", "rim-345-band", px((rel(1.5, -1), rel(2, -1), 2.5)), px((rel(1.5, 1), rel(2, 1), 2.5)))
    g.add("cone_exact", "far-from-rim", inside, outside)

    # --- cone, conservative reject |s - 0.5| > 0.505: 0.5 |x| > 0.505 |z| for the plain light
    g = group("cone_reject", ["tight"])
    x505 = f32(4.0) * f32(0.505)  # z = 2: the reject's threshold in x, exact
    for tag, other in (("", 0.5), ("-other-axis-0", 0.0)):
        g.add("cone_reject", "x-step" + tag, px((dn(x505), other, 2)), px((up(x505), other, 2)), px((x505, other, 2)))
        g.add("cone_reject", "x-band" + tag, px((rel(x505, -1), other, 2)), px((rel(x505, 1), other, 2)))
        g.add("cone_reject", "y-band" + tag, px((other, rel(x505, -1), 2)), px((other, rel(x505, 1), 2)))
        g.add("cone_reject", "between-rim-and-reject" + tag, px((0.25, other, 2)), px((2.012, other, 2)))  # 0.503: only the exact cull
    g.add("cone_reject", "negx-band", px((-rel(x505, -1), 0.5, 2)), px((-rel(x505, 1), 0.5, 2)))

    # --- clip w
    g = group("clip_w_sign", ["tight"])
    g.add("clip_w", "behind-inside-mirrored-cone", inside, px((0.25, 0.125, -2)))
    g.add("clip_w", "behind-outside-mirrored-cone", inside, px((5, 0.5, -2)))
    g.add("clip_w", "w-zero", inside, px((0.25, 0.125, -0.0)), px((0.25, 0.125, 0.0)))
    g.add("clip_w", "w-zero-on-axis", inside, px((0, 0, -0.0)), px((0, 0, 0.0)))
    g.add("clip_w", "w-denormal", px((0, 0, 2.0 ** -140)), px((0, 0, -2.0 ** -140)))
    g.add("clip_w", "w-denormal-off-axis", inside, px((2.0 ** -139, 0, 2.0 ** -140)))
    g = group("clip_w_small", ["tight_far_d2"])  # |cw| at 2^-30 with d^2 ~ 1
    F = L["tight_far_d2"]
    g.add("clip_w", "w-2^-30-step", px((0, 0, up(2.0 ** -30))), px((0, 0, dn(2.0 ** -30))), px((0, 0, 2.0 ** -30)))
    g.add("clip_w", "w-2^-30-among-ordinary", px(F.at(0.25, 0.125, 2)), px((0, 0, dn(2.0 ** -30))), px((0, 0, 2.0 ** -30)))
    g.add("clip_w", "w-minus-2^-30-step", px((0, 0, -up(2.0 ** -30))), px((0, 0, -dn(2.0 ** -30))), px((0, 0, -2.0 ** -30)))
    g = group("clip_w_large", ["lean_w20"])  # |cw| = 2^20 z at 2^30 with d^2 = 2^20
    g.add("clip_w", "w-2^30-step", px((0, 0, dn(1024))), px((0, 0, up(1024))), px((0, 0, 1024)))
    g.add("clip_w", "w-2^30-among-ordinary", px((0.25 * 2.0 ** -20, 0, 2)), px((0, 0, up(1024))), px((0, 0, 1024)))

    # --- guard falloffBound * d^2 >= 2^-28 (falloffBound = 1): d^2 = z^2 (+ x^2); a pair it protects is outside the cone or back-facing
    g = group("guard", ["tight"])
    z0 = 2.0 ** -14
    for tag, make in (("outside", lambda z: px((2 * f64(z), 0, z))), ("backface", lambda z: px((0, 0, z), n=(0, 0, 1))),
                      ("lit", lambda z: px((0, 0, z)))):
        if tag == "outside":  # d^2 = 5 z^2
            z28 = f32(2.0 ** -14 / np.sqrt(5.0))
            g.add("guard", "guard-band-" + tag, make(rel(z28, 1)), make(rel(z28, -1)))
        else:
            g.add("guard", "guard-step-" + tag, make(up(z0)), make(dn(z0)), make(z0))
            g.add("guard", "guard-band-" + tag, make(rel(z0, 1)), make(rel(z0, -1)))
        g.add("guard", "guard-far-" + tag, make(2.0), make(2.0 ** -20))
        g.add("guard", "quotient-overflows-" + tag, make(2.0), make(2.0 ** -75))  # falloff 2^-148: colour / falloff = inf
    g.add("guard", "d2-2^-30-step", px((0, 0, up(2.0 ** -15))), px((0, 0, dn(2.0 ** -15))), px((0, 0, 2.0 ** -15)))
    g.add("guard", "d2-2^30-step", px((0, 0, dn(2.0 ** 15))), px((0, 0, up(2.0 ** 15))), px((0, 0, 2.0 ** 15)))
    g.add("guard", "d2-2^30-among-ordinary", inside, px((0, 0, up(2.0 ** 15))), px((0, 0, 2.0 ** 15)))

    # --- back face: N.L = -normal.z
    g = group("back_face", ["tight"])
    materials = (("moderate", {}), ("metallic16", {"o": (1.0, 0.5, 16.0)}), ("roughness-1", {"o": (1.0, -1.0, 0.25)}))
    for gtag, p in (("guarded", (0.25, 0.125, 2)), ("unguarded", (0.25 * 2.0 ** -16, 0, 2.0 ** -15))):
        for mtag, m in materials:
            t = f"{gtag}-{mtag}"
            g.add("back_face", "ndl-denormal-" + t, px(p, n=(0, 0, -HALF_MIN), **m), px(p, n=(0, 0, HALF_MIN), **m), px(p, n=(0, 0, -0.0), **m))
            g.add("back_face", "ndl-one-" + t, px(p, n=(0, 0, -1), **m), px(p, n=(0, 0, 1), **m), px(p, n=(0, 0, 0.0), **m))
            g.add("back_face", "ndl-nan-" + t, px(p, n=(0, 0, -1), **m), px(p, n=(0, 0, np.nan), **m))
            g.add("back_face", "ndl-tilted-" + t, px(p, n=(1, 0, -HALF_MIN), **m), px(p, n=(1, 0, HALF_MIN), **m), px(p, n=(1, 0, 0.0), **m))

    # --- per-pixel flags
    g = group("pixel_flags", ["tight"])
    for axis in range(3):
        for bound, btag in ((P12, "2^12"), (P30, "2^30")):
            def at(v, axis=axis):
                p = [0.25, 0.125, 2.0]
                p[axis] = v
                return px(p)
            g.add("pixel_flags", f"position-{'xyz'[axis]}-{btag}", at(dn(bound)), at(up(bound)), at(bound))
            g.add("pixel_flags", f"position-{'xyz'[axis]}-minus-{btag}", at(-dn(bound)), at(-up(bound)), at(-bound))
        g.add("pixel_flags", f"position-{'xyz'[axis]}-2^12-among-ordinary", inside, at(up(P12)), at(P12))
    for z, ztag in ((1.37 * 2.0 ** 13, "2^13"), (1.37 * 2.0 ** 21, "2^21"), (1.37 * 2.0 ** 29, "2^29")):  # lit pixels between the two bounds
        g.add("pixel_flags", f"position-{ztag}-lit-among-ordinary", inside, px((0.1 * z, 0.05 * z, z)))
    # specularPower = 160^(1 - roughness) around 2^20: roughness -1.7314 / -1.7324, the two half values that enclose it
    r20 = np.float16(1.0 - 20.0 * np.log(2.0) / np.log(160.0))
    r_lo, r_hi = (r20, np.nextafter(r20, np.float16(-np.inf))) if 160.0 ** (1.0 - f64(r20)) <= 2.0 ** 20 else (np.nextafter(r20, np.float16(np.inf)), r20)
    g.add("pixel_flags", "specular-power-2^20", px(inside["p"], o=(1.0, r_lo, 0.25)), px(inside["p"], o=(1.0, r_hi, 0.25)))
    g.add("pixel_flags", "specular-power-2^20-among-ordinary", inside, px(inside["p"], o=(1.0, r_hi, 0.25)))
    for value, vtag in ((np.inf, "inf"), (-np.inf, "minus-inf"), (np.nan, "nan")):
        for plane in ("n", "s", "o", "d"):
            for where, base in (("inside", inside), ("outside", outside)):
                bad = dict(base)
                bad[plane] = np.array([value] * 3, np.float16)
                g.add("pixel_flags", f"{vtag}-in-{plane}-{where}-cone", base, bad)

    # --- half vector: camera on the light's axis behind the pixels, view direction (e, 0, 1): |light + view|^2 = e^2
    g = group("half_vector", ["tight"], camera=(0, 0, 6))
    e = 2.0 ** -20
    # (H = (1, 0, 0) there and the Fresnel factor is 1: the normal (0.5, 0, -1) gives N.H = 0.5 - below the clamp, so that a
    # half vector of the wrong length shows - and N.L = 1: a term that is not zero)
    hv = lambda e: px((-4 * f64(e), 0, 2), n=(0.5, 0, -1))
    g.add("half_vector", "hd-2^-40-step", hv(up(e)), hv(dn(e)), hv(e))
    g.add("half_vector", "hd-2^-40-band", hv(rel(e, 1)), hv(rel(e, -1)))
    g.add("half_vector", "hd-zero", hv(2.0 ** -3), hv(0.0))
    g.add("half_vector", "hd-zero-among-2^-40", hv(e), hv(0.0))
    for m, ex in ((1.37, -21), (1.1, -30), (1.9, -45), (1.23, -52), (1.61, -60)):  # nothing a power of two: the square root is rounded
        g.add("half_vector", f"hd-{m}^2-2^{2 * ex}-among-ordinary", hv(2.0 ** -3), hv(m * 2.0 ** ex))
    for deep in (-50, -64, -70):  # far below the bound, down to denormal squared lengths: where a lean square root would go wrong
        g.add("half_vector", f"hd-2^{2 * deep}-among-ordinary", hv(2.0 ** -3), hv(2.0 ** deep))
    # view direction (t, t, 1): light + view = (t, t, 0), H = (1, 1, 0) / sqrt 2 and N.H = 0 exactly for the normal
    # (1, -1, -2^-24), which faces the light (N.L = 2^-24): a pow base of 0 on a pair whose term is NOT zero. With a specular
    # power of 1 / 160 (roughness 2) or 1 a pow that mistakes the base shows in the sum.
    t = 2.0 ** -20
    for rough in (2.0, 1.0, 0.5):
        lit = px((-0.5, -0.25, 2), o=(1.0, rough, 0.25))
        g.add("track", f"specular-base-zero-lit-roughness-{rough}", lit, px((-4 * t, -4 * t, 2), n=(1, -1, -HALF_MIN), o=(1.0, rough, 0.25)))
    # (hd >= 8 cannot be reached by two unit vectors; its largest value, 4, is the view direction ALONG the light direction:)
    g = group("half_vector_max", ["tight"], camera=(0, 0, -3))
    g.add("half_vector", "hd-4-fresnel-base-0", px((0.25, 0, 2)), px((0, 0, 2)))

    # --- the optimistic pass's running minimum: one term at a time
    g = group("track_cxy", ["tight_shift"])  # cx = 0.5 x, cy = 0.5 y, cw = z: the cone's axis is x = y = z
    ok = px((2.25, 2.125, 2))
    c = 2.0 ** -59
    g.add("track", "cx-2^-60-step", px((up(c), 2, 2)), px((dn(c), 2, 2)), px((c, 2, 2)))
    g.add("track", "cx-2^-60-among-lit", ok, px((dn(c), 2, 2)), px((c, 2, 2)))
    g.add("track", "cx-zero-among-lit", ok, px((0.0, 2, 2)))
    g.add("track", "cx-minus-2^-60-among-lit", ok, px((-dn(c), 2, 2)), px((-c, 2, 2)))
    g.add("track", "cy-2^-60-step", px((2, up(c), 2)), px((2, dn(c), 2)), px((2, c, 2)))
    g.add("track", "cy-2^-60-among-lit", ok, px((2, dn(c), 2)), px((2, c, 2)))
    g.add("track", "cy-zero-among-lit", ok, px((2, 0.0, 2)))
    # the same pixels so close to the light that the cone culls do not apply (guard) and the quotients are formed
    near = lambda x, y: px((x, y, 2.0 ** -15))
    g.add("track", "cx-2^-60-unguarded", near(2.0 ** -15, 2.0 ** -15), near(dn(c), 2.0 ** -15), near(c, 2.0 ** -15))
    g.add("track", "cy-zero-unguarded", near(2.0 ** -15, 2.0 ** -15), near(2.0 ** -15, 0.0))
    g = group("track_cz", ["tight_cz"])  # cz = y, with a map
    c = 2.0 ** -60
    g.add("track", "cz-2^-60-step", px((0.25, up(c), 2)), px((0.25, dn(c), 2)), px((0.25, c, 2)))
    g.add("track", "cz-2^-60-among-lit", px((0.25, 0.125, 2)), px((0.25, dn(c), 2)), px((0.25, c, 2)))
    g.add("track", "cz-zero-among-lit", px((0.25, 0.125, 2)), px((0.25, 0.0, 2)))
    g.add("track", "cz-minus-2^-60-among-lit", px((0.25, 0.125, 2)), px((0.25, -dn(c), 2)), px((0.25, -c, 2)))
    # fragment depths cz / 2 in the denormal range against occluders of 2^-130: a quotient that is wrong there changes the shade
    g = group("track_cz_denormal", ["tight_cz_denormal"])
    c = 2.0 ** -129
    g.add("track", "depth-2^-130-step", px((0.25, c + 2.0 ** -148, 2)), px((0.25, c - 2.0 ** -148, 2)), px((0.25, c, 2)))  # one step of the quotient
    g.add("track", "depth-denormal-among-lit", px((0.25, 0.125, 2)), px((0.25, 1.7 * 2.0 ** -131, 2)), px((0.25, 1.3 * 2.0 ** -129, 2)))
    g.add("track", "depth-denormal-other-w", px((0.25, 0.125, 3)), px((0.25, 1.7 * 2.0 ** -131, 3)), px((0.25, 2.9 * 2.0 ** -130, 3)))
    # pow bases. View direction (0.6, d / 5, -0.8), normal (0, 2^-24, 0): N.H = 2^-24 (d / 5) / |light + view|, N.L = 0; the
    # back-face cull is off for these pixels (metallic 16: reflectance above 4), so the BRDF of the pair is evaluated.
    g = group("track_pow", ["tight"])
    hs = np.sqrt(0.36 + 3.24)
    d126 = 5.0 * hs * 2.0 ** -102  # N.H = 2^-126, the smallest normal number
    spec = lambda d: px((0, -f64(d), 2), n=(0, HALF_MIN, 0), o=(1.0, 0.5, 16.0))
    lit = px((0, -0.25, 2), n=(0, 0.5, -1), o=(1.0, 0.5, 16.0))
    g.add("track", "specular-base-smallest-normal-band", spec(rel(d126, 2)), spec(rel(d126, -2)))
    g.add("track", "specular-base-smallest-normal-among-lit", lit, spec(rel(d126, -2)), spec(rel(d126, 2)))
    g.add("track", "specular-base-denormal-among-lit", lit, spec(d126 * 2.0 ** -8))
    g.add("track", "specular-base-zero-among-lit", lit, spec(0.0))
    g = group("track_fresnel", ["tight"], camera=(0, 0, -3))  # view direction = light direction: the Fresnel base 1 - H.L is 0
    g.add("track", "fresnel-base-zero-among-lit", px((0.5, 0.25, 2)), px((0, 0, 2)))

    # --- shadow PCF: 12 x 6 maps; normal (1, 1, -1) projects to (0, 0): the taps are 1.5 texels apart in both axes
    for kind in ("random", "equal", "zero", "nearer"):
        g = group("pcf_" + kind, ["pcf_" + kind])
        n = (1, 1, -1)
        centre = px((0.25, 0.125, 2), n=n)
        # s = 0.5 + 0.25 x, t = 0.5 + 0.25 y at z = 2
        g.add("shadow_pcf", "tap-on-column-0-and-row-0", centre, px((-1, -1, 2), n=n))        # s W = 3, t H = 1.5
        g.add("shadow_pcf", "tap-on-column-W-and-row-H", centre, px((1, 1, 2), n=n))          # s W = 9, t H = 4.5
        g.add("shadow_pcf", "centre-tap-on-s-0", centre, px((-dn(2), 0, 2), n=n), px((-2, 0, 2), n=n))  # the rim: s = 0
        g.add("shadow_pcf", "centre-tap-on-s-1", centre, px((dn(2), 0, 2), n=n), px((2, 0, 2), n=n))
        g.add("shadow_pcf", "centre-tap-on-t-0-and-t-1", px((0, -dn(2), 2), n=n), px((0, dn(2), 2), n=n))
        g.add("shadow_pcf", "depth-steps", px((0.25, 0.125, up(2)), n=n), px((0.25, 0.125, dn(2)), n=n), centre)
        g.add("shadow_pcf", "facing-normal", px((0.25, 0.125, 2)), px((-1, 1, 2)))

    # --- the per-light flags: every record alone, then all of them in one loop beside the moon
    probes = lambda l: (px(l.at(-0.25, 0.125, 2)), px(l.at(-5, 0.5, 2)), px(l.at(-2, 0, 2)))
    for name in LIGHT_FLAGS:
        if name.startswith("pcf_") or name in ("tight", "tight_shift", "tight_cz", "tight_cz_denormal", "tight_far_d2"):
            continue
        g = group("light_" + name, [name])
        a, b, c = probes(L[name])
        g.add("light_flags", "cone", a, b, c)
        g.add("light_flags", "back-face", a, px(a["p"], n=(0, 0, 1)), px(a["p"], n=(0, 0, 0.0)))
        g.add("light_flags", "close", a, px(L[name].at(0, 0, 2.0 ** -15)), px(L[name].at(0, 0, 2.0 ** -14)))
    names = [n for n in LIGHT_FLAGS if not n.startswith("pcf_")] + ["pcf_random"]
    g = group("light_all_with_moon", names, skip=1)
    for name in ("tight", "lean_row_above", "generic_cs_below", "lean_pos_above", "pcf_random"):
        a, b, c = (px(t["p"], n=(0, -1, -1)) for t in probes(L[name]))  # world +y is down: the moon lights normals with y < 0
        g.add("light_flags", "cone-of-" + name, a, b, c)

    # --- slot numbering: the same lights and pixels under every skip count; maps on directional slots too
    for skip in (0, 1, 2, 3):
        g = group(f"slots_skip{skip}", ["tight", "pcf_random", "tight_shift", "pcf_nearer"], skip=skip, maps_on_directional=(0, 1))
        g.add("slots", "cones", px((0.25, 0.125, 2), n=(1, -1, -1)), px((2.25, 2.125, 2), n=(0, -1, -1)), px((2, 0, 2)))
    return L, G


# ---------------------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------------------
# gate -> (threshold, what it switches). Sides: 1 = value >= threshold (for "back_face", "cw_sign": value > 0), 0 = below,
# -1 = the value is NaN. A threshold of 0 has no relative band; `near` is then |value| <= the smallest step of the input.
GATES = {
    "cone_exact": (0.25, "q >= 0.25: the exact rim cull"),
    "cone_reject": (float(f32(0.505)), "max |s - 0.5| |cw| > 0.505 |cw|: surelyOutsideCone"),
    "cw_sign": (0.0, "cw > 0; surelyOutsideCone needs |cw| > 0"),
    "cw_lo": (2.0 ** -30, "lean: |cw| >= 2^-30"), "cw_hi": (2.0 ** 30, "lean: |cw| <= 2^30"),
    "guard": (2.0 ** -28, "falloffBound * d^2 >= 2^-28: the three culls"),
    "d2_lo": (2.0 ** -30, "lean: d^2 >= 2^-30"), "d2_hi": (2.0 ** 30, "lean: d^2 <= 2^30"),
    "back_face": (0.0, "N.L > 0"),
    "hd_lo": (2.0 ** -40, "lean: |light + view|^2 >= 2^-40"),
    "track_cx": (2.0 ** -60, "|cx| >= 2^-60"), "track_cy": (2.0 ** -60, "|cy| >= 2^-60"), "track_cz": (2.0 ** -60, "|cz| >= 2^-60, map present"),
    "track_pow": (2.0 ** -126, "min(N.H, 1 - H.L) clamped >= 2^-126"),
    "pos_tight": (2.0 ** 12, "tightPixel: max |p| <= 2^12"), "pos_moderate": (2.0 ** 30, "positionModerate: max |p| <= 2^30"),
    "specular_power": (2.0 ** 20, "tightPixel: specularPower <= 2^20"),
}
PIXEL_BOOLS = ("pixel_finite", "pixel_moderate")
# gates whose threshold is an upper bound: value <= threshold is the lean side, so "on" belongs below
UPPER = ("cw_hi", "d2_hi", "pos_tight", "pos_moderate", "specular_power", "cone_reject")
# gates for which the cases can sit exactly on the threshold in every form (the others are derived through a rounding)
EXACT_REACHABLE = ("cone_exact", "cone_reject", "cw_sign", "cw_lo", "cw_hi", "guard", "d2_lo", "d2_hi", "back_face", "hd_lo", "track_cx",
                   "track_cy", "track_cz", "pos_tight", "pos_moderate")
# gates whose input is too coarse to come within 2^-20 of the threshold: the roughness is a half (steps of 2^-10 move
# 160^(1 - r) by half a percent). The two half values that enclose 2^20 are used; only the sides are required.
COARSE = ("specular_power",)


def material(sc):
    """float64 PBR quantities of a scenario's 64 texels (pbrFunctions.glinl:3-20)."""
    with np.errstate(all="ignore"):
        s, o = sc.planes["s"].astype(f64), sc.planes["o"].astype(f64)
        metallic = o[:, 2:3]
        refl = 0.04 * (1.0 - metallic) + (0.5 * s / s.max(axis=1, keepdims=True)) * metallic
        power = 160.0 ** (1.0 - o[:, 1])
        return {"normal": sc.planes["n"].astype(f64), "diffuse": sc.planes["d"].astype(f64) / 3.14159265359, "reflectance": refl,
                "occlusion": o[:, 0], "power": power, "normalization": (power + 2.0) / 8.0}


def view_direction(group, sc):
    """normalize(camera - position) as the float32 vector the shader holds (v * (1 / sqrt(dot(v, v))), each operation rounded
    to float32), returned as float64. The census starts from this stored vector like it starts from the stored G-buffer values:
    whether light + view cancels exactly depends on its rounding, not on the real direction."""
    with np.errstate(all="ignore"):
        v = group.camera - sc.planes["p"]
        dot = f32(v[:, 2] * v[:, 2] + f32(v[:, 1] * v[:, 1] + f32(v[:, 0] * v[:, 0])))
        return (v * (f32(1.0) / np.sqrt(dot))[:, None]).astype(f64)


def census(group, k, light):
    """The gate quantities of the 64 pairs (lane of scenario k, light), in float64 from the float32 / half inputs.
    Returns {"value": {gate: [64]}, "side": {gate: int8 [64]}, "near": {gate: bool [64]}, "exact": {gate: bool [64]},
    "flags": {name: bool [64]}, "active": bool [64], "zero": bool [64], "nan": bool [64], "interior": bool [64]}."""
    sc = group.scenarios[k]
    m = material(sc)
    with np.errstate(all="ignore"):
        p = sc.planes["p"].astype(f64)
        R = light.rows.astype(f64)
        clip = p @ R[:, :3].T + R[:, 3]
        cx, cy, cz, cw = clip.T
        ddx, ddy = cx / cw - 0.5, cy / cw - 0.5
        q = ddx * ddx + ddy * ddy
        to_light = light.position.astype(f64) - p
        d2 = (to_light * to_light).sum(axis=1)
        fb = f64(light.falloff_bound)
        ndl = m["normal"] @ light.dir
        view = view_direction(group, sc)
        hs = light.dir + view
        hd = (hs * hs).sum(axis=1)
        h = hs / np.sqrt(hd)[:, None]
        base_spec = np.clip((h * m["normal"]).sum(axis=1), 0.0, 1.0)
        base_fres = 1.0 - np.clip(h @ light.dir, 0.0, 1.0)
        pmax = np.abs(p).max(axis=1)
        value = {
            "cone_exact": q, "cone_reject": np.maximum(np.abs(cx - 0.5 * cw), np.abs(cy - 0.5 * cw)) / np.abs(cw), "cw_sign": cw,
            "cw_lo": np.abs(cw), "cw_hi": np.abs(cw), "guard": fb * d2, "d2_lo": d2, "d2_hi": d2, "back_face": ndl, "hd_lo": hd,
            "track_cx": np.abs(cx), "track_cy": np.abs(cy), "track_cz": np.abs(cz) if light.shadow is not None else np.full(LANES, np.inf),
            "track_pow": np.minimum(base_spec, base_fres), "pos_tight": pmax, "pos_moderate": pmax, "specular_power": np.abs(m["power"]),
        }
        side, near, exact = {}, {}, {}
        for gate, (thr, _) in GATES.items():
            x = value[gate]
            if thr == 0.0:
                s = x > 0.0
                near[gate] = np.abs(x) <= (HALF_MIN if gate == "back_face" else 2.0 ** -126)
            else:
                s = x > thr if gate in UPPER else x >= thr
                near[gate] = np.abs(x - thr) <= BAND * thr
            side[gate] = np.where(np.isnan(x), -1, s.astype(np.int8)).astype(np.int8)
            exact[gate] = x == thr
        big = 2.0 ** 120
        fin = lambda a, b=big: (np.abs(a) <= b).reshape(LANES, -1).all(axis=1)
        pixel_finite = (pmax <= 2.0 ** 30) & fin(view, 2.0) & fin(m["normal"]) & fin(m["diffuse"]) & fin(m["reflectance"]) & \
            fin(m["occlusion"]) & fin(m["normalization"]) & fin(m["power"])
        pixel_moderate = pixel_finite & fin(m["diffuse"], 2.0 ** 16) & fin(m["reflectance"], 4.0) & fin(m["occlusion"], 2.0 ** 16) & \
            fin(m["normalization"], 2.0 ** 8) & fin(m["normal"], 2.0 ** 16)
        tight_pixel = pixel_finite & (pmax <= 2.0 ** 12) & (np.abs(m["power"]) >= 2.0 ** -100) & (np.abs(m["power"]) <= 2.0 ** 20)
        flags = {"pixel_finite": pixel_finite, "pixel_moderate": pixel_moderate, "tight_pixel": tight_pixel,
                 "light_lean": np.full(LANES, light.lean), "light_tight": np.full(LANES, light.tight)}
        # --- what the reference's arithmetic must give for the pair, where the census can tell without rounding questions
        falloff = f64(light.factor) * d2 / (f64(light.distance) ** 2)
        quotient = np.abs(light.cs.astype(f64)).max() / falloff
        quotient_min = np.abs(light.cs.astype(f64)).min() / falloff
        clear = lambda g: ~near[g] | exact[g]
        outside = (side["cone_exact"] == 1) & clear("cone_exact") & np.isfinite(q)
        unlit = (side["back_face"] == 0) | (side["back_face"] == -1)  # clamp(N.L) = 0 also for a NaN
        ordinary = pixel_moderate & (hd > 0.0) & np.isfinite(cz / cw)
        zero = (outside | unlit) & ordinary & (quotient < 2.0 ** 100) & (falloff > 0) & np.isfinite(q)
        nan = outside & ordinary & (quotient_min > 2.0 ** 130)
        gates_clear = np.all([~near[g] for g in GATES], axis=0)
        interior = gates_clear & (q <= 0.2) & pixel_moderate & (quotient < 2.0 ** 100) & (quotient > 2.0 ** -100) & (hd > 2.0 ** -30) & \
            (np.abs(cw) > 2.0 ** -100) & (light.shadow is None)
    return {"value": value, "side": side, "near": near, "exact": exact, "flags": flags, "active": group.active(k), "zero": zero, "nan": nan,
            "interior": interior}


def term64(group, k, light):
    """float64 value [64, 3] of the single pair's term (lights.comp:73-108), without a shadow map."""
    sc = group.scenarios[k]
    m = material(sc)
    with np.errstate(all="ignore"):
        p = sc.planes["p"].astype(f64)
        R = light.rows.astype(f64)
        clip = p @ R[:, :3].T + R[:, 3]
        st = clip[:, :2] / clip[:, 3:4]
        duv = np.clip(np.sqrt(((st - 0.5) ** 2).sum(axis=1)) / 0.5, 0.0, 1.0)
        edge = 1.0 - duv * duv
        nd = np.sqrt(((light.position.astype(f64) - p) ** 2).sum(axis=1)) / f64(light.distance)
        falloff = f64(light.factor) * nd * nd
        spectral = light.cs.astype(f64)[None, :] / falloff[:, None] * edge[:, None]
        view = view_direction(group, sc)
        hs = light.dir + view
        h = hs / np.sqrt((hs * hs).sum(axis=1, keepdims=True))
        micro = np.clip((h * m["normal"]).sum(axis=1), 0.0, 1.0) ** m["power"]
        specular = (m["normalization"] * micro)[:, None]
        fres = m["reflectance"] + (1.0 - m["reflectance"]) * ((1.0 - np.clip(h @ light.dir, 0.0, 1.0)) ** 5.0)[:, None]
        brdf = m["diffuse"] * (1.0 - fres) + specular * fres
        return m["occlusion"][:, None] * brdf * spectral * np.clip(m["normal"] @ light.dir, 0.0, 1.0)[:, None]


def verdict(group, k, lane, light):
    """One line for a failure message: the side of every gate for one pair, the near ones marked."""
    c = census(group, k, light)
    parts = []
    for gate in GATES:
        mark = "=" if c["exact"][gate][lane] else ("~" if c["near"][gate][lane] else "")
        parts.append(f"{gate}:{ {-1: 'nan', 0: 'below', 1: 'above'}[int(c['side'][gate][lane])]}{mark}")
    flags = ",".join(n for n, f in c["flags"].items() if f[lane])
    return f"[{' '.join(parts)} | {flags} | active lanes {int(c['active'].sum())}]"


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's frame of a group (computed once per process, read-only)
# ---------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def frame_inputs(group, L):
    """(rect, camera block, directional lights, spot array, {slot: map view}, planes cut to the draw extent)."""
    from tests import util

    W, H = group.extent
    inp = util.Inputs(W, H, spots=0)
    inp.cam.position[:3] = [float(v) for v in group.camera]
    planes = {k: np.ascontiguousarray(v[:H, :W]) for k, v in group.planes().items()}
    return inp, group.spot_array(L), group.shadow_maps(L), planes


def oracle_frame(group, L):
    """(debug [H, W, 4] float32, colour [H, W, 4] uint16) of oracle.lights over the group."""
    if group.name not in _ORACLE:
        from oracle import binding as ob

        W, H = group.extent
        inp, spots, maps, planes = frame_inputs(group, L)
        frame = ob.HostFrame(W, H)
        frame.diffuse[:], frame.specular[:], frame.normal[:] = planes["diffuse"], planes["specular"], planes["normal"]
        frame.position[:], frame.orm[:] = planes["worldPosition"], planes["occlusionRoughnessMetallic"]
        images = (abi.Image * group.slot_count)()
        for slot, m in maps.items():
            images[slot] = ob.host_image(m, abi.SZG_FORMAT_D32_SFLOAT)
        shadow = abi.ShadowMaps(group.slot_count, 0, C.cast(images, C.POINTER(abi.Image)))
        ob.lights(frame, inp.rect, None, shadow, inp.cam, inp.dirs, 2, group.skip, spots, len(group.light_names), threads=8)
        frame.debug.setflags(write=False)
        frame.color.setflags(write=False)
        _ORACLE[group.name] = (frame.debug, frame.color)
    return _ORACLE[group.name]


def tile_of(group, k, image):
    """[64, c] lanes of scenario k cut from an [H, W, c] image of the draw extent; lanes outside the extent are 0."""
    x0, y0 = group.origin(k)
    out = np.zeros((8, 8) + image.shape[2:], image.dtype)
    part = image[y0:y0 + 8, x0:x0 + 8]
    out[:part.shape[0], :part.shape[1]] = part
    return out.reshape((LANES,) + image.shape[2:])
