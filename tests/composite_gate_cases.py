"""Hand-made pixels for the composite (k_composite, atmosphere/camera.comp) and a census of the gates of its phase A.

k_composite takes several decisions camera.comp does not take: four wave-uniform lean switches in the geometry branch
(samplesLean, vectorsLean, brdfLean), the per-pixel skip of the reflection term of a non-metal (environmentFinite), and it
shares camera.comp's pixel classification and sun shadow lookup. Every decision is a threshold. This module places pixels ON
those thresholds, on both sides of them and at their float32 neighbours, and says - by a float64 model written from
camera.comp and the kernel's comments, not by calling the oracle - on which side of which gate each lane lies, and which
lanes the reference's arithmetic must poison with a NaN. numpy and syzygy_amd.abi only; tests/test_composite_gate_cases.py
checks the coverage and the oracle against the census without a GPU, tests/test_gpu_composite_gates.py runs the same cases
through recordComposite and recordCompositeFast.

PIXELS are G-buffer texels written field by field (fp32 worldPosition in engine space: metres, +y down; fp16 normal, diffuse,
specular, occlusion / roughness / metallic) with a depth and a prior UNORM16 colour, laid out in aligned 8x8 tiles. One tile
is one wave of k_composite (lane = (y % 8) * 8 + x % 8) = one SCENARIO. A scenario has a form:
  uniform   all 64 lanes hold one variant,
  mixed<k>  lane k (0, 63 or the interior lane 27) holds another variant than the other 63,
  partial   as mixed with the odd lane at 34, every third lane a sky pixel (depth 0) whose G-buffer texel is hostile (NaN
            position, inf normal): under waveAll such a lane may neither open nor close a gate nor leak into the result.
The tiles of the last column and the last row of a group's image are cut by the draw extent.
A GROUP is one recordComposite call: camera block, atmosphere block, both LUTs (with texels poked), the sun's shadow map or
none, and a grid of scenarios. Frame-level gates (camera radius, sun length, the atmosphere's flags, the LUT status words)
take one group per value; the group then holds one crossing of ordinary pixels in every form.

What cannot be reached is written down in UNREACHABLE instead of being faked.
"""
import copy
import ctypes as C
import math
import zlib

import numpy as np

from syzygy_amd import abi

f32, f64 = np.float32, np.float64
LANES = 64
MIXED_LANES = (0, 63, 27)
PARTIAL_LANE = 34  # row 4, column 2: inside the draw extent in a cut tile too
FORMS = ("uniform", "mixed0", "mixed63", "mixed27", "partial")
BAND = 2.0 ** -20  # "near a threshold": within this relative distance (the band of tests/lights_gate_cases.py)
COLS = 12          # tiles per row of a group's image at most: 93 texels
CUT = (3, 2)       # the draw extent ends this many texels before the last tile column / row does
HALF_MIN = 2.0 ** -24  # smallest half denormal
TLUT_EXTENT, SLUT_EXTENT = (128, 32), (64, 32)
AERIAL_MAX_DISTANCE = 0.05  # Mm, the recorded 32^3 volume of the fast composite

EARTH = dict(  # scene.cpp:52-75 as the packed block holds it; the sun 30 degrees up
    scatteringRayleighPerMm=(5.802, 13.558, 33.1), densityScaleRayleighMm=0.008, absorptionRayleighPerMm=(0.0, 0.0, 0.0),
    planetRadiusMm=6.36, scatteringMiePerMm=(3.996, 3.996, 3.996), densityScaleMieMm=0.0012, absorptionMiePerMm=(4.4, 4.4, 4.4),
    atmosphereRadiusMm=6.42, incidentDirectionSun=(0.0, -0.4999999701976776, -0.8660253882408142),
    scatteringOzonePerMm=(0.0, 0.0, 0.0), absorptionOzonePerMm=(0.65, 1.881, 0.085), sunIntensitySpectrum=(1.0, 1.0, 1.0),
    sunAngularRadius=0.009308422915637493)
INVERSE_PROJECTION = ((2.2406642, 0, 0, 0), (0, 0.70020753, 0, 0), (0, 0, 0, 1), (0, 0, 9.9999008, 9.9999997e-05))
CAMERA = (0.0, -10.0, -13.0)  # engine metres


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def dn(x):
    return np.nextafter(f32(x), f32(-np.inf))


def metres(mm):
    """The float32 number of metres m with float32(m / 1e6f) == float32(mm) where one exists, else the nearest."""
    target = f32(mm)
    m = f32(f64(target) * 1e6)
    candidates = [m]
    for _ in range(4):
        candidates = [dn(candidates[0])] + candidates + [up(candidates[-1])]
    for cand in sorted(candidates, key=lambda c: abs(f64(c) - f64(m))):
        if f32(cand / f32(1e6)) == target:
            return cand
    return m


def atmosphere(**edits):
    a = abi.AtmospherePacked()
    fields = dict(EARTH)
    fields.update(edits)
    for k, v in fields.items():
        if isinstance(v, (tuple, list, np.ndarray)):
            getattr(a, k)[:] = [float(f32(x)) for x in v]
        else:
            setattr(a, k, float(f32(v)))
    return a


def camera_block(position=CAMERA, inverse_projection=INVERSE_PROJECTION, rotation=None):
    c = abi.CameraPacked()
    eye = np.eye(4, dtype=f32)
    for name in ("projection", "view", "viewInverseTranspose", "projViewInverse"):
        setattr(c, name, abi.Mat4.from_numpy(eye))
    c.inverseProjection = abi.Mat4.from_numpy(np.array(inverse_projection, f32))
    c.rotation = abi.Mat4.from_numpy(eye if rotation is None else np.array(rotation, f32))
    c.forwardWorld[:] = [0.0, 0.0, 1.0, 0.0]
    c.position[:] = [float(f32(v)) for v in position] + [1.0]
    return c


def scaled_projection(sx, sy):
    return ((sx, 0, 0, 0), (0, sy, 0, 0), (0, 0, 0, 1), (0, 0, 9.9999008, 9.9999997e-05))


class Bounds:
    """The constants load_atm() derives from a packed block, in float64 (tests/march_rays.Bounds holds the radius bounds and is
    checked against the device's own values; tests/test_composite_gate_cases.py holds the two equal)."""

    def __init__(self, atm):
        self.Rp, self.Ra = float(atm.planetRadiusMm), float(atm.atmosphereRadiusMm)
        hmin = min(float(atm.densityScaleRayleighMm), float(atm.densityScaleMieMm))
        self.sun = np.array(list(atm.incidentDirectionSun), f64)
        self.sun2 = float(self.sun @ self.sun)
        self.leanFloor = max(0.9 * self.Rp, self.Rp - 80.0 * hmin)
        self.extFloor = max(0.9 * self.Rp, self.Rp - 27.0 * hmin)
        self.extCeil = self.Ra + (self.Ra - self.Rp) * 0.005
        coefficients = [list(getattr(atm, n)) for n in ("scatteringRayleighPerMm", "absorptionRayleighPerMm", "scatteringMiePerMm",
                                                         "scatteringOzonePerMm", "absorptionOzonePerMm")]
        flat = np.array(coefficients, f64).ravel()
        sign_clear = not np.signbit(flat).any()
        shell = self.Ra - self.Rp
        thinnest = math.exp(-1.02 * shell / float(atm.densityScaleRayleighMm)) * 0.5
        lean = all(2.0 ** -30 <= v <= 2.0 ** 30 for v in (self.Rp, self.Ra, hmin)) and bool((np.abs(flat) <= 2.0 ** 30).all()) and \
            hmin >= self.Rp * 2.0 ** -18
        self.lean = lean
        self.extModerate = lean and sign_clear and bool((flat <= 2.0 ** 10).all()) and min(coefficients[0]) * thinnest >= 2.0 ** -40
        horizontal2 = self.sun[0] ** 2 + self.sun[2] ** 2
        self.sunSane = 0.98 <= self.sun2 <= 1.02 and 2.0 ** -30 <= float(atm.sunAngularRadius) <= 1.5 and horizontal2 >= 2.0 ** -100


# ---------------------------------------------------------------------------------------------------------------------------
# pixels, scenarios, groups
# ---------------------------------------------------------------------------------------------------------------------------
def px(p=(1.0, -2.0, 5.0), n=(0.25, -1.0, -0.25), d=(0.5, 0.375, 0.25), s=(0.5, 0.25, 0.125), o=(1.0, 0.5, 0.0), depth=0.5):
    """One texel: engine-space position (metres, +y down), normal, diffuse, specular, (occlusion, roughness, metallic), depth.
    The defaults are the ordinary pixel: a rough non-metal 2 m above the ground that faces the sun."""
    return {"p": np.array(p, f32), "n": np.array(n, np.float16), "d": np.array(d, np.float16), "s": np.array(s, np.float16),
            "o": np.array(o, np.float16), "depth": f32(depth)}


ORDINARY = px()
METAL = px(o=(1.0, 0.25, 1.0))
HOSTILE_SKY = px(p=(np.nan, np.nan, np.nan), n=(np.inf, -np.inf, np.inf), depth=0.0)


class Scenario:
    def __init__(self, group, family, name, form, base, odd=None, odd_lane=None):
        self.group, self.family, self.name, self.form, self.odd_lane = group, family, name, form, odd_lane
        v = [base] * LANES
        if odd is not None:
            v[odd_lane] = odd
        if form == "partial":
            v = [HOSTILE_SKY if (lane % 3 == 0 and lane != odd_lane) else t for lane, t in enumerate(v)]
        self.planes = {k: np.stack([t[k] for t in v]) for k in ("p", "n", "d", "s", "o")}
        self.depth = np.array([t["depth"] for t in v], f32)
        rng = np.random.default_rng(zlib.crc32(f"{group.name}/{name}".encode()))
        self.prior = rng.integers(0, 20000, (LANES, 3)).astype(np.uint16)  # the lights pass's colour, dim: 0 .. 0.3


class Group:
    """One recordComposite call. `tlut_poke` / `slut_pokes`: (row, column, channel, value) written over the oracle's LUTs;
    `slut_target`: "tap" puts the sky-view poke under the reflection tap of one odd lane (resolved by finish())."""

    def __init__(self, name, camera=CAMERA, inverse_projection=INVERSE_PROJECTION, atm=None, tlut_poke=None, slut_value=None,
                 slut_target=None, shadow=None, note=""):
        self.name, self.base_name, self.note = name, name, note
        self.camera, self.inverse_projection = np.array(camera, f32), np.array(inverse_projection, f32)
        self.atm_edits = dict(atm or {})
        self.tlut_poke, self.slut_value, self.slut_target, self.slut_poke = tlut_poke, slut_value, slut_target, None
        self.shadow = shadow  # kind of shadow_map() or None
        self.scenarios, self._cells = [], None

    # -- blocks
    @property
    def atm(self):
        return atmosphere(**self.atm_edits)

    @property
    def cam(self):
        return camera_block(self.camera, self.inverse_projection)

    def bounds(self):
        return Bounds(self.atm)

    def add(self, family, name, near, far, on=None):
        """Every form of one crossing of a gate: `near` and `far` lie on its two sides, `on` exactly on it where that exists."""
        self._cells = None
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

    # -- geometry of the image: a mixed63 tile never lies in the cut column or row
    def _layout(self):
        if self._cells is None:
            n = len(self.scenarios)
            need = sum(sc.form == "mixed63" for sc in self.scenarios)
            cols = min(COLS, max(2, (n + 1) // 2))
            rows = max(2, (n + cols - 1) // cols)
            while (cols - 1) * (rows - 1) < need or cols * rows < n:
                rows += 1
            interior = [(r, c) for r in range(rows - 1) for c in range(cols - 1)]
            taken = interior[:need]
            rest = [(r, c) for r in range(rows) for c in range(cols) if (r, c) not in set(taken)]
            rest.sort(key=lambda rc: not (rc[0] == rows - 1 or rc[1] == cols - 1))  # the cut tiles are used first
            cells, it63, itrest = [], iter(taken), iter(rest)
            for sc in self.scenarios:
                cells.append(next(it63) if sc.form == "mixed63" else next(itrest))
            self._cells = (cols, rows, cells)
        return self._cells

    @property
    def tiles(self):
        return len(self.scenarios)

    @property
    def extent(self):
        cols, rows, _ = self._layout()
        return cols * 8 - CUT[0], rows * 8 - CUT[1]

    def origin(self, k):
        r, c = self._layout()[2][k]
        return c * 8, r * 8

    def scenario_at(self, x, y):
        cells = self._layout()[2]
        return cells.index((y // 8, x // 8)) if (y // 8, x // 8) in cells else None

    def images(self):
        """The G-buffer planes [H8, W8, 4], depth [H8, W8] and prior colour [H8, W8, 4] at whole tiles. Cells without a scenario
        are sky (depth 0)."""
        cols, rows, _ = self._layout()
        H, W = rows * 8, cols * 8
        out = {"diffuse": np.zeros((H, W, 4), np.float16), "specular": np.zeros((H, W, 4), np.float16), "normal": np.zeros((H, W, 4), np.float16),
               "worldPosition": np.zeros((H, W, 4), f32), "occlusionRoughnessMetallic": np.zeros((H, W, 4), np.float16)}
        depth, prior = np.zeros((H, W), f32), np.zeros((H, W, 4), np.uint16)
        prior[..., 3] = 65535
        for k, sc in enumerate(self.scenarios):
            x0, y0 = self.origin(k)
            tile = lambda a: a.reshape(8, 8, -1)
            for plane, key in (("diffuse", "d"), ("specular", "s"), ("normal", "n"), ("worldPosition", "p"), ("occlusionRoughnessMetallic", "o")):
                out[plane][y0:y0 + 8, x0:x0 + 8, :3] = tile(sc.planes[key])
                out[plane][y0:y0 + 8, x0:x0 + 8, 3] = 1.0
            depth[y0:y0 + 8, x0:x0 + 8] = sc.depth.reshape(8, 8)
            prior[y0:y0 + 8, x0:x0 + 8, :3] = tile(sc.prior)
        return out, depth, prior

    def active(self, k):
        """bool [64]: the lanes of scenario k's wave inside the draw extent (the others have left the kernel)."""
        x0, y0 = self.origin(k)
        W, H = self.extent
        lane = np.arange(LANES)
        return (x0 + lane % 8 < W) & (y0 + lane // 8 < H)

    def odd_pixel(self, form):
        """(x, y, k) of the odd lane of the first scenario of `form` whose odd lane is inside the draw extent."""
        for k, sc in enumerate(self.scenarios):
            if sc.form == form and sc.odd_lane is not None and self.active(k)[sc.odd_lane]:
                x0, y0 = self.origin(k)
                return x0 + sc.odd_lane % 8, y0 + sc.odd_lane // 8, k
        raise KeyError(form)

    # -- the per-pixel view direction as the kernel forms it (float32, camera.comp:324-328)
    def directions(self):
        """[H8, W8, 3] float32: normalize((rotation * inverseProjection * clip).xyz) with y negated; rotation is the identity."""
        cols, rows, _ = self._layout()
        W, H = self.extent
        key = (cols, rows, self.inverse_projection.tobytes())
        if getattr(self, "_directions", (None,))[0] == key:
            return self._directions[1]
        with np.errstate(all="ignore"):
            xs, ys = np.arange(cols * 8, dtype=f32), np.arange(rows * 8, dtype=f32)
            clipx = ((xs / f32(W)) - f32(0.5)) * f32(2.0)
            clipy = ((ys / f32(H)) - f32(0.5)) * f32(2.0)
            cx, cy = np.meshgrid(clipx, clipy)
            M = self.inverse_projection
            v = [f32(f32(f32(M[r, 0] * cx) + f32(M[r, 1] * cy)) + M[r, 2]) + M[r, 3] for r in range(3)]
            v = [c.astype(f32) for c in v]
            dot = f32(v[2] * v[2]) + (f32(v[1] * v[1]) + f32(v[0] * v[0]))
            s = f32(1.0) / np.sqrt(dot.astype(f32))
            d = np.stack([v[0] * s, -(v[1] * s), v[2] * s], axis=-1).astype(f32)
        self._directions = (key, d)
        return d


STANDARD = "ordinary-and-metal"


def standard(g, family):
    """One crossing of ordinary pixels in every form, for a group whose gate is a frame-level one."""
    g.add(family, STANDARD, ORDINARY, METAL)
    return g


MAP_W, MAP_H, MAP_PAD = 12, 6, 5  # not square, not powers of two; rows 5 texels wider than the map
SHADOW_DEPTH = 0.3125            # the fragment depth of a pixel at engine z = 2 under SHADOW_SUN


def shadow_sun():
    """The directional light whose matrices give, for an engine position p: clip w = p.z, s = 0.5 + 0.5 p.x / p.z,
    t = -p.y / p.z (0 .. 1 for p.y in -2 .. 0 at p.z = 2: geometry has p.y <= 0), depth (0.25 p.z + 0.125) / p.z. Powers of
    two throughout, so TO_TEX * projection * view is exact. The normal (1, -0.5, -1) projects to (0, 0): taps 1.5 texels apart."""
    l = abi.DirectionalLightPacked()
    proj = np.array([(1, 0, 0, 0), (0, -2, -1, 0), (0, 0, 0.25, 0.125), (0, 0, 1, 0)], f32)
    l.projection, l.view = abi.Mat4.from_numpy(proj), abi.Mat4.from_numpy(np.eye(4, dtype=f32))
    l.color[:] = [1.0, 1.0, 1.0, 1.0]
    l.forward[:] = [0.0, 0.5, -0.866, 0.0]
    l.strength = 1.0
    return l


def shadow_map(kind):
    """[MAP_H, MAP_W] float32 view of a buffer with MAP_PAD more texels per row, the padding holding the nearest occluder."""
    buf = np.ones((MAP_H, MAP_W + MAP_PAD), f32)
    m = buf[:, :MAP_W]
    if kind == "random":
        m[:] = np.random.default_rng(0xC0A5).random((MAP_H, MAP_W), dtype=f32)
    elif kind == "equal":
        m[:] = f32(SHADOW_DEPTH)
    elif kind == "zero":
        m[:] = 0.0
    elif kind == "nearer":
        m[:] = up(SHADOW_DEPTH)
    else:
        raise KeyError(kind)
    return m


FAMILIES = ("surface_length", "surface_radius", "camera_radius", "sun_length", "view_length", "half_vector", "planet_shadow",
            "reflection_skip", "classification", "sun_shadow")
METALLIC = (("plus-zero", 0.0), ("minus-zero", -0.0), ("half-denormal", HALF_MIN), ("one", 1.0), ("nan", np.nan))
CAMERA_SWEEP = tuple(0.25 * k for k in range(-8, 9))  # metres around the lean floor: float32 steps of the radius are 0.48 m


def _large_coefficient():
    return {"scatteringMiePerMm": (1500.0, 1500.0, 1500.0)}  # tests/test_gpu_parity._large_coefficient on the packed block


def build():
    """The groups. Deterministic."""
    G = []

    def group(*a, **k):
        g = Group(*a, **k)
        G.append(g)
        return g

    B = Bounds(atmosphere())
    cam = np.array(CAMERA, f32)
    at = lambda x=cam[0], y=cam[1], z=cam[2], **k: px((x, y, z), **k)

    # --- |surface - camera|^2 against 2^-60 and 2^60 (samplesLean). The camera's x is 0: an x offset is the whole segment.
    g = group("surface_length")
    e = 2.0 ** -30
    g.add("surface_length", "zero-segment", ORDINARY, at())                       # normalize(0) = NaN in the reference
    g.add("surface_length", "zero-segment-metal", METAL, at(o=(1.0, 0.25, 1.0)))
    g.add("surface_length", "x-2^-30-step", at(x=metres(up(e))), at(x=metres(dn(e))), at(x=metres(e)))
    g.add("surface_length", "x-2^-31-among-ordinary", ORDINARY, at(x=metres(e / 2)), at(x=metres(e)))
    g.add("surface_length", "z-2^-31-among-ordinary", ORDINARY, at(z=f32(f64(cam[2]) + 4.66e-4)))
    g.add("surface_length", "x-minus-2^-30-step", at(x=-metres(up(e))), at(x=-metres(dn(e))), at(x=-metres(e)))
    E = 2.0 ** 30
    g.add("surface_length", "x-2^30-step", at(x=metres(dn(E))), at(x=metres(up(E))), at(x=metres(E)))
    g.add("surface_length", "x-2^30-among-ordinary", ORDINARY, at(x=metres(up(E))), at(x=metres(E)))

    # --- surface r^2 against 2^60: straight up, where the radius is the y coordinate alone
    g = group("surface_radius")
    g.add("surface_radius", "y-2^30-step", px((0, -metres(dn(E)), 0)), px((0, -metres(up(E)), 0)), px((0, -metres(E), 0)))
    g.add("surface_radius", "y-2^30-among-ordinary", ORDINARY, px((0, -metres(up(E)), 0)), px((0, -metres(E), 0)))
    g.add("surface_radius", "y-2^31-among-ordinary", ORDINARY, px((0, -metres(2 * E), 0)))

    # --- camera r^2 against leanFloor2 (Earth: Rp - 80 Hm, 96 km underground) and 2^60: one group per camera depth
    floor_depth = (B.Rp - B.leanFloor) * 1e6
    for k, delta in enumerate(CAMERA_SWEEP):
        standard(group(f"camera_floor_{k:02d}", camera=(0.0, floor_depth + delta, 0.0)), "camera_radius")
    for tag, r in (("below", dn(E)), ("on", E), ("above", up(E)), ("far-above", 1.5 * E)):
        standard(group(f"camera_2^30_{tag}", camera=(0.0, -metres(r), 0.0)), "camera_radius")

    # --- |incidentDirectionSun|^2 against 2^-60 and 2^60: a horizontal sun (0, 0, -s), whose squared length s^2 is exact
    for tag, s in (("zero", 0.0), ("lo-below", dn(e)), ("lo-on", e), ("lo-above", up(e)), ("one", 1.0), ("hi-below", dn(E)), ("hi-on", E),
                   ("hi-above", up(E))):
        standard(group(f"sun_length_{tag}", atm={"incidentDirectionSun": (0.0, 0.0, -f32(s))}), "sun_length")

    # --- |direction|^2 (vectorsLean): normalize() returns a unit vector, 0, inf or NaN, nothing in between. The camera's
    # inverseProjection maps clip (cx, cy) to a (cx - cx0, cy - cy0, 0): the zero vector, hence NaN, at ONE pixel; with a = 2^70
    # the dot product overflows everywhere else (direction 0), with a = 2^-80 it underflows (direction inf).
    for form in FORMS[1:]:
        g = standard(group(f"view_length_{form}"), "view_length")
        g.inverse_projection = _zero_at(g, g.odd_pixel(form)[:2], 1.0, 0.0)
    # (z = a here: the vector (a dx, a dy, a) is 0 nowhere. A lane of a uniform wave has dx = dy = 0.)
    for tag, a in (("overflow", 2.0 ** 70), ("underflow", 2.0 ** -80)):
        g = standard(group(f"view_length_{tag}"), "view_length")
        g.inverse_projection = _zero_at(g, (g.origin(0)[0] + 1, g.origin(0)[1] + 1), a, a)

    # --- |l + v|^2 against 2^-40 (brdfLean). All pixels share the direction (0, -0, 1) under a projection whose x / y scale is 0;
    # the sun (0, -a, -1) then gives l + v = (0, a, 0) up to the rounding of normalize(): a = 0 cancels exactly.
    a0 = 2.0 ** -20
    for tag, a in (("cancelled", 0.0), ("half", a0 / 2), ("below", dn(a0)), ("on", a0), ("above", up(a0)), ("twice", 2 * a0), ("2^-10", 2.0 ** -10)):
        standard(group(f"half_vector_{tag}", inverse_projection=scaled_projection(0.0, 0.0),
                       atm={"incidentDirectionSun": (0.0, -f32(a), -1.0)}), "half_vector")
    standard(group("half_vector_scale_2^-80", inverse_projection=scaled_projection(2.0 ** -80, 2.0 ** -80),
                   atm={"incidentDirectionSun": (0.0, 0.0, -1.0)}), "half_vector")
    # with an ordinary camera the sun against ONE pixel's direction puts one lane of one wave below the threshold
    for form in FORMS[1:]:
        g = standard(group(f"half_vector_{form}"), "half_vector")
        x, y, _ = g.odd_pixel(form)
        d = g.directions()[y, x]
        g.atm_edits["incidentDirectionSun"] = tuple(-d)

    # --- shadowedByPlanet: a hit of the planet along the sun direction with pt0 > 0
    g = group("planet_shadow_day")  # sun 30 degrees up
    g.add("planet_shadow", "ground-against-above", px((0, -0.5, 0)), px((0, -50.0, 0)), px((0, 0.0, 0)))  # pt0 = 0 at r = Rp exactly
    g.add("planet_shadow", "miss-among-ordinary", ORDINARY, px((2.0e7, -2.0, 0)))
    night = {"incidentDirectionSun": (0.0, 0.8, -0.6)}  # the sun 53 degrees under the horizon
    g = group("planet_shadow_night", atm=night)
    g.add("planet_shadow", "ground-against-above", px((0, -0.5, 0)), px((0, -50.0, 0)), px((0, 0.0, 0)))
    g.add("planet_shadow", "miss-among-shadowed", ORDINARY, px((0, -6.0e6, 0)))  # 6000 km up: the ray passes the planet
    g.add("planet_shadow", "metal-shadowed", ORDINARY, METAL)

    # --- the reflection skip: every factor of environmentFinite false in turn, under every metallic value
    def metallic_crossings(g, base=None, label=""):
        base = base or {}
        for mtag, mv in METALLIC[1:]:
            g.add("reflection_skip", f"{label}metallic-{mtag}", px(**base), px(**{**base, "o": (1.0, 0.5, mv)}))
        return g

    metallic_crossings(group("skip_all_true"))
    metallic_crossings(group("skip_ext_moderate", atm=_large_coefficient()))
    metallic_crossings(group("skip_sun_radius_2", atm={"sunAngularRadius": 2.0}))
    metallic_crossings(group("skip_sun_vertical", atm={"incidentDirectionSun": (0.0, -1.0, 0.0)}))
    metallic_crossings(group("skip_tlut_texel_2^-60", tlut_poke=(9, 14, 1, 2.0 ** -60)))
    for vtag, value in (("nan", np.nan), ("inf", np.inf)):
        for where in ("tap", "far"):
            metallic_crossings(group(f"skip_sky_{vtag}_{where}", slut_value=value, slut_target=where))
    g = group("skip_normal")
    for ntag, n in (("inf", (np.inf, -1.0, 0.0)), ("minus-inf-y", (0.0, -np.inf, 0.0)), ("nan", (0.0, np.nan, 0.0)), ("all-inf", (np.inf, np.inf, np.inf))):
        for mtag, mv in METALLIC:
            g.add("reflection_skip", f"normal-{ntag}-metallic-{mtag}", ORDINARY, px(n=n, o=(1.0, 0.5, mv)))
    metallic_crossings(group("skip_camera_on_ground", camera=(0.0, 0.0, 0.0)))
    metallic_crossings(group("skip_camera_under_ground", camera=(0.0, 0.5, 0.0)))  # 0.5 m: one float32 step of the radius
    ceil_m = (B.extCeil - B.Rp) * 1e6  # Ra + 0.5 % of the shell: 60.3 km up
    metallic_crossings(group("skip_camera_under_ceiling", camera=(0.0, -(ceil_m - 2.0), 0.0)))
    metallic_crossings(group("skip_camera_over_ceiling", camera=(0.0, -(ceil_m + 2.0), 0.0)))
    g = group("skip_surface_ceiling")
    for mtag, mv in METALLIC:
        g.add("reflection_skip", f"surface-ceiling-metallic-{mtag}", px((0, -(ceil_m - 2.0), 0), o=(1.0, 0.5, mv)),
              px((0, -(ceil_m + 2.0), 0), o=(1.0, 0.5, mv)))

    # --- the classification: sky when depth == 0 or engine y > 0
    g = group("classification")
    for tag, depth in (("plus-zero", 0.0), ("minus-zero", -0.0), ("denormal", 1e-45), ("nan", np.nan)):
        g.add("classification", f"depth-{tag}", ORDINARY, px(depth=depth))
    for tag, y in (("plus-zero", 0.0), ("minus-zero", -0.0), ("denormal", 1e-45), ("nan", np.nan), ("one", 1.0)):
        g.add("classification", f"y-{tag}", ORDINARY, px((1.0, y, 5.0)))
        g.add("classification", f"y-{tag}-metal", METAL, px((1.0, y, 5.0), o=(1.0, 0.25, 1.0)))

    # --- the sun shadow lookup: 25 taps on a 12 x 6 map in rows of 17
    sn = (1.0, -0.5, -1.0)  # projects to (0, 0): taps 1.5 texels apart in both axes
    for kind in ("random", "equal", "zero", "nearer"):
        g = group("shadow_" + kind, shadow=kind)
        centre = px((0.25, -1.0, 2), n=sn)                                                   # s = 0.5625, t = 0.5
        g.add("sun_shadow", "taps-over-s-0-and-t-0", centre, px((-1.75, -0.25, 2), n=sn))    # s W = 0.75, t H = 0.75
        g.add("sun_shadow", "taps-over-s-1-and-t-1", centre, px((1.75, -1.75, 2), n=sn))     # s W = 11.25, t H = 5.25
        g.add("sun_shadow", "centre-on-s-0", centre, px((-dn(2), -1.0, 2), n=sn), px((-2, -1.0, 2), n=sn))
        g.add("sun_shadow", "centre-on-s-1", centre, px((dn(2), -1.0, 2), n=sn), px((2, -1.0, 2), n=sn))
        g.add("sun_shadow", "centre-on-t-0-and-t-1", px((0.25, -0.0, 2), n=sn), px((0.25, -dn(2), 2), n=sn), px((0.25, -2, 2), n=sn))
        g.add("sun_shadow", "clip-w-zero", centre, px((0.25, -1.0, 0.0), n=sn), px((0.25, -1.0, -0.0), n=sn))
        g.add("sun_shadow", "depth-steps", px((0.25, -1.0, up(2)), n=sn), px((0.25, -1.0, dn(2)), n=sn), centre)
        g.add("sun_shadow", "facing-normal", centre, px((0.25, -1.0, 2)))
    G = [part for g in G for part in _split(g)]
    for g in G:
        _finish(g)
    return G


MAX_TILES = 42  # 12 x 5 cells less the cut column and row for the mixed63 tiles: an image of at most 93 x 38 texels


def _split(g):
    """A group with more tiles than one small image holds becomes several calls of the same frame, a crossing never divided."""
    if g.tiles <= MAX_TILES:
        return [g]
    chunks, current, seen = [], [], None
    for sc in g.scenarios:
        crossing = sc.name.split("/")[0]
        if crossing != seen and len(current) + sum(o.name.split("/")[0] == crossing for o in g.scenarios) > MAX_TILES:
            chunks.append(current)
            current = []
        seen = crossing
        current.append(sc)
    chunks.append(current)
    parts = []
    for i, chunk in enumerate(chunks):
        part = copy.copy(g)
        part.name, part.scenarios, part._cells = f"{g.name}_{i}", chunk, None
        for sc in chunk:
            sc.group = part
        parts.append(part)
    return parts


def _zero_at(g, pixel, a, z):
    """inverseProjection rows (a, 0, 0, -a cx0), (0, a, 0, -a cy0), (0, 0, 0, z): a power of two, so a cx - a cx0 is exact."""
    x, y = pixel
    W, H = g.extent
    cx0 = ((f32(x) / f32(W)) - f32(0.5)) * f32(2.0)
    cy0 = ((f32(y) / f32(H)) - f32(0.5)) * f32(2.0)
    return np.array([(a, 0, 0, -f32(a) * cx0), (0, a, 0, -f32(a) * cy0), (0, 0, 0, z), (0, 0, 9.9999008, 9.9999997e-05)], f32)


def _finish(g):
    """Resolve the sky-view poke: under the reflection tap of the first mixed odd lane whose reflection misses the ground and
    whose tap lies well inside a texel, or in the lower half of the LUT, which no ray that misses the ground can reach."""
    if g.slut_target == "far":
        g.slut_poke = (SLUT_EXTENT[1] - 5, 11, 1, g.slut_value)
    elif g.slut_target == "tap":
        for k, sc in enumerate(g.scenarios):
            if sc.odd_lane is None or not g.active(k)[sc.odd_lane]:
                continue
            geo = geometry(g, k)
            tap = geo["reflection_tap"][sc.odd_lane]
            if geo["geometry"][sc.odd_lane] and tap[0] >= 0 and geo["tap_firm"][sc.odd_lane]:
                g.slut_poke = (int(tap[1]), int(tap[0]), 2, g.slut_value)
                return
        raise AssertionError(f"{g.name}: no odd lane reflects into the sky-view LUT")


# ---------------------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------------------
# gate -> (threshold, what it switches). Sides: 1 = value >= threshold (UPPER: value > threshold, the failing side of an upper
# bound; ZERO gates: value > 0), 0 = below, -1 = the value is NaN. FLAG gates are booleans (1 = the factor holds).
GATES = {
    "surface_len_lo": (2.0 ** -60, "samplesLean: |surface - camera|^2 >= 2^-60"),
    "surface_len_hi": (2.0 ** 60, "samplesLean: |surface - camera|^2 <= 2^60"),
    "surface_r_hi": (2.0 ** 60, "samplesLean: surface r^2 <= 2^60"),
    "camera_r_floor": (None, "samplesLean: camera r^2 >= leanFloor2"),
    "camera_r_hi": (2.0 ** 60, "samplesLean: camera r^2 <= 2^60"),
    "sun_lo": (2.0 ** -60, "samplesLean: |sun|^2 >= 2^-60"), "sun_hi": (2.0 ** 60, "samplesLean: |sun|^2 <= 2^60"),
    "view_lo": (2.0 ** -60, "vectorsLean: |direction|^2 >= 2^-60"), "view_hi": (2.0 ** 60, "vectorsLean: |direction|^2 <= 2^60"),
    "half_lo": (2.0 ** -40, "brdfLean: |l + v|^2 >= 2^-40"),
    "planet_hit": (0.5, "raySphere(surface, light, Rp) hits"), "planet_pt0": (0.0, "shadowedByPlanet: pt0 > 0"),
    "ext_moderate": (0.5, "a.extModerate"), "sun_sane": (0.5, "a.sunSane"), "lut_moderate": (0.5, "L.moderate"),
    "sky_finite": (0.5, "S.finite"), "normal_finite": (0.5, "normalFinite"),
    "above_ground": (1.0, "aboveGround: Rp / r <= 1 for the camera and the surface"),
    "camera_ext_ceil": (None, "camera r^2 <= extCeil2"), "surface_ext_ceil": (None, "surface r^2 <= extCeil2"),
    "metallic_zero": (0.0, "metallic != 0: the reflection is evaluated"),
    "depth_zero": (0.0, "sceneDepth == 0: sky"), "underground": (0.0, "engine y > 0: sky"),
}
UPPER = ("surface_len_hi", "surface_r_hi", "camera_r_hi", "sun_hi", "view_hi", "above_ground", "camera_ext_ceil", "surface_ext_ceil")
FLAGS = ("planet_hit", "ext_moderate", "sun_sane", "lut_moderate", "sky_finite", "normal_finite")
EQUALITY = ("metallic_zero", "depth_zero")  # side 1 = the value differs from 0; "exact" = it is a zero of either sign
# gates for which the cases can sit exactly on the threshold in every form
EXACT_REACHABLE = ("surface_len_lo", "surface_len_hi", "surface_r_hi", "camera_r_hi", "sun_lo", "sun_hi", "half_lo", "planet_pt0",
                   "above_ground", "metallic_zero", "depth_zero", "underground")
# gates whose value cannot come within 2^-20 of the threshold from both sides: only the sides are required.
COARSE = {
    "view_lo": "normalize() returns a unit vector, 0, inf or NaN: nothing near 2^-60",
    "view_hi": "normalize() returns a unit vector, 0, inf or NaN: nothing near 2^60",
    "half_lo": "l + v is a difference of two rounded unit vectors: float64 cannot tell the side inside the band",
    "planet_pt0": "the surface radius is quantised to 0.5 m: pt0 moves in steps of about 2^-20 Mm around 0",
    "metallic_zero": "an equality with 0: the nearest other value is the smallest half denormal",
    "depth_zero": "an equality with 0: the nearest other value is the smallest denormal",
    "underground": "a sign test: the nearest other values are the smallest denormals",
}
UNREACHABLE = {
    "surface r^2 >= leanFloor2": "a non-sky pixel has engine y <= 0, hence r >= Rp > sqrt(leanFloor2)",
    "surface r^2 >= extFloor2": "the same: r >= Rp > sqrt(extFloor2)",
    "|l + v|^2 <= 8": "l and v are unit vectors to a few ulps: |l + v|^2 <= 4; where they are not, vectorsLean is already false",
    "camera r^2 >= extFloor2 alone": "a camera under sqrt(extFloor2) is under the ground: aboveGround is false with it "
                                     "(the camera_floor groups are such cameras)",
    "surface r^2 <= 2^60 apart from |surface - camera|^2 <= 2^60": "the camera's radius must stay under 2^30, far less than a "
                                                                    "float32 step of 2^60: the two move together",
}


def _mm(p_engine, Rp):
    """Engine metres -> planet-centred Mm as camera.comp:320-322 / :371-374 do it, float32, returned as float64 [.., 3]."""
    with np.errstate(all="ignore"):
        p = np.asarray(p_engine, f32)
        x = p[..., 0] / f32(1e6)
        y = (-p[..., 1]) / f32(1e6) + f32(Rp)
        z = p[..., 2] / f32(1e6)
        return np.stack([x, y.astype(f32), z], axis=-1).astype(f64)


def _normalize32(v):
    with np.errstate(all="ignore"):
        v = np.asarray(v, f32)
        dot = f32(v[..., 2] * v[..., 2]) + (f32(v[..., 1] * v[..., 1]) + f32(v[..., 0] * v[..., 0]))
        return (v * (f32(1.0) / np.sqrt(dot.astype(f32)))[..., None]).astype(f32)


def _ray_sphere(f, d, R):
    """raySphere of common.glinl in float64 for unit directions: (hit, t0, discriminant)."""
    with np.errstate(all="ignore"):
        b = -(f * d).sum(axis=-1)
        chord = f + b[..., None] * d
        disc = R * R - (chord * chord).sum(axis=-1)
        c = (f * f).sum(axis=-1) - R * R
        s = np.sqrt(np.maximum(disc, 0.0))
        q = np.where(b < 0.0, b - s, b + s)
        a0 = c / q
        t0 = np.minimum(a0, q)
        return disc >= 0.0, t0, disc


def _sky_tap(B, position, direction, size=SLUT_EXTENT):
    """sampleMap_Direction's bilinear footprint (camera.comp:70-121) in float64: (column, row) of its upper-left texel, -1 where
    the coordinates are NaN, and whether the tap lies firmly inside that footprint (0.05 .. 0.95 of the texel)."""
    W, H = size
    with np.errstate(all="ignore"):
        n = direction / np.sqrt((direction * direction).sum(axis=-1, keepdims=True))
        sin_h = B.Rp / np.sqrt((position * position).sum(axis=-1))
        horizon = math.pi - np.arcsin(sin_h)
        cos_h = -np.sqrt(np.maximum(1.0 - sin_h * sin_h, 0.0))
        zen = np.arccos(n[..., 1])
        v = np.where(n[..., 1] > cos_h, (1.0 - np.sqrt(1.0 - zen / horizon)) * 0.5, np.sqrt((zen - horizon) / (math.pi - horizon)) * 0.5 + 0.5)
        pl = np.array([-B.sun[0], -B.sun[2]])
        pl = pl / np.sqrt(pl @ pl)
        pv = direction[..., [0, 2]] / np.sqrt((direction[..., [0, 2]] ** 2).sum(axis=-1, keepdims=True))
        u = np.clip(pv @ pl, -1.0, 1.0) * 0.5 + 0.5
        x, y = u * W - 0.5, v * H - 0.5
        bad = np.isnan(x) | np.isnan(y)
        i, j = np.floor(np.where(bad, 0, x)), np.floor(np.where(bad, 0, y))
        fx, fy = x - i, y - j
        firm = ~bad & (fx > 0.05) & (fx < 0.95) & (fy > 0.05) & (fy < 0.95) & (i >= 0) & (i < W - 1) & (j >= 0) & (j < H - 1)
        tap = np.stack([np.where(bad, -1, i), np.where(bad, -1, j)], axis=-1).astype(np.int64)
        return tap, firm


def geometry(group, k):
    """The float64 quantities of scenario k's 64 lanes, from the float32 / half values the kernel starts from."""
    sc = group.scenarios[k]
    B = group.bounds()
    x0, y0 = group.origin(k)
    with np.errstate(all="ignore"):
        camera = _mm(group.camera, B.Rp)
        direction = group.directions()[y0:y0 + 8, x0:x0 + 8].reshape(LANES, 3)
        depth_zero = sc.depth == 0.0
        underground = sc.planes["p"][:, 1] > 0.0
        geo = ~depth_zero & ~underground
        surface = _mm(sc.planes["p"], B.Rp)
        to_surface = surface - camera
        normal = sc.planes["n"].astype(f64) * np.array([1.0, -1.0, 1.0])
        light = _normalize32(-B.sun.astype(f32))
        view = _normalize32(-direction)
        half = (light + view).astype(f32)  # float32: whether it cancels is a matter of the rounded vectors
        hd = (half.astype(f64) ** 2).sum(axis=-1)
        hit, pt0, disc = _ray_sphere(surface, np.broadcast_to(light.astype(f64), surface.shape), B.Rp)
        neg = -direction.astype(f64)
        refl = 2.0 * (normal * neg).sum(axis=-1, keepdims=True) * normal - neg
        rhit, rt0, rdisc = _ray_sphere(surface, refl / np.sqrt((refl * refl).sum(axis=-1, keepdims=True)), B.Rp)
        reflection_hits_ground = rhit & (rt0 > 0.0)
        rtap, rfirm = _sky_tap(B, surface, refl)
        rfirm &= ~reflection_hits_ground & (np.abs(rdisc) > 1e-6)
        rtap = np.where(reflection_hits_ground[:, None], -1, rtap)
        cam_b = np.broadcast_to(camera, surface.shape)
        vhit, vt0, vdisc = _ray_sphere(cam_b, direction.astype(f64), B.Rp)
        view_hits_ground = vhit & (vt0 > 0.0)
        vtap, vfirm = _sky_tap(B, cam_b, direction.astype(f64))
        vtap = np.where(view_hits_ground[:, None], -1, vtap)
        vfirm &= ~view_hits_ground & (np.abs(vdisc) > 1e-6)
    return {"B": B, "camera": camera, "direction": direction, "direction2": (direction.astype(f64) ** 2).sum(axis=-1), "surface": surface,
            "to_surface": to_surface, "normal": normal, "hd": hd, "hit": hit, "pt0": pt0, "geometry": geo, "depth_zero": depth_zero,
            "underground": underground, "reflection_tap": rtap, "tap_firm": rfirm, "view_tap": vtap, "view_tap_firm": vfirm,
            "metallic": sc.planes["o"][:, 2].astype(f64)}


def census(group, k):
    """Returns {"value": {gate: [64]}, "side": {gate: int8 [64]}, "near": {gate: bool [64]}, "exact": {gate: bool [64]},
    "active": bool [64], "geometry": bool [64] (inside the draw extent and not sky), "poisoned": bool [64], "clean": bool [64],
    "why": [64] str}. A gate of the geometry branch is met only by geometry lanes: `lanes(gate)` selects them."""
    sc = group.scenarios[k]
    q = geometry(group, k)
    B = q["B"]
    active = group.active(k)
    sq = lambda v: (v * v).sum(axis=-1)
    full = lambda x: np.full(LANES, float(x))
    with np.errstate(all="ignore"):
        camera_r2, surface_r2 = float(sq(q["camera"])), sq(q["surface"])
        normal_finite = (np.abs(q["normal"]) <= 2.0 ** 60).all(axis=-1)
        poke = group.slut_poke
        value = {
            "surface_len_lo": sq(q["to_surface"]), "surface_len_hi": sq(q["to_surface"]), "surface_r_hi": surface_r2,
            "camera_r_floor": full(camera_r2), "camera_r_hi": full(camera_r2), "sun_lo": full(B.sun2), "sun_hi": full(B.sun2),
            "view_lo": q["direction2"], "view_hi": q["direction2"], "half_lo": q["hd"],
            "planet_hit": q["hit"].astype(f64), "planet_pt0": np.where(q["hit"], q["pt0"], -np.inf),
            "ext_moderate": full(B.extModerate), "sun_sane": full(B.sunSane), "lut_moderate": full(group.tlut_poke is None),
            "sky_finite": full(poke is None), "normal_finite": normal_finite.astype(f64),
            "above_ground": np.maximum(B.Rp / math.sqrt(camera_r2) if camera_r2 > 0 else np.inf, B.Rp / np.sqrt(surface_r2)),
            "camera_ext_ceil": full(camera_r2), "surface_ext_ceil": surface_r2,
            "metallic_zero": q["metallic"], "depth_zero": sc.depth.astype(f64), "underground": sc.planes["p"][:, 1].astype(f64),
        }
        thresholds = {g: t for g, (t, _) in GATES.items()}
        thresholds["camera_r_floor"] = B.leanFloor ** 2
        thresholds["camera_ext_ceil"] = thresholds["surface_ext_ceil"] = B.extCeil ** 2
        side, near, exact = {}, {}, {}
        for gate, thr in thresholds.items():
            x = value[gate]
            if gate in EQUALITY:
                s, near[gate], exact[gate] = x != 0.0, np.abs(x) <= HALF_MIN, x == 0.0
            elif gate in FLAGS:
                s, near[gate], exact[gate] = x > thr, np.ones(LANES, bool), np.zeros(LANES, bool)
            elif thr == 0.0:
                s, near[gate], exact[gate] = x > 0.0, np.abs(x) <= 2.0 ** -19, x == 0.0
            else:
                s = x > thr if gate in UPPER else x >= thr
                near[gate], exact[gate] = np.abs(x - thr) <= BAND * thr, x == thr
            side[gate] = np.where(np.isnan(x), -1, s.astype(np.int8)).astype(np.int8)
        geo = active & q["geometry"]
        # --- where the reference's arithmetic must give NaN
        why = np.array([""] * LANES, dtype=object)

        def mark(mask, text):
            why[mask & (why == "")] = text

        # (Two NaNs of phase A do NOT reach the pixel. A zero-length segment makes sampleTransmittanceLUT_Segment's direction
        # normalize(0) = NaN, and a cancelled half vector makes h = 0 * inf = NaN; both only enter clamp(), which returns its
        # bound for a NaN in the pinned built-ins: the LUT coordinates and the two pow bases come out finite. Such lanes are
        # claimed CLEAN below: a lean operator that lets the NaN through shows as a NaN.)
        mark(active & np.isnan(q["direction"]).any(axis=-1), "NaN view direction")
        mark(geo & ~np.isfinite(q["normal"]).all(axis=-1), "NaN / inf normal: the reflection direction is NaN")
        mark(geo & np.isnan(q["metallic"]), "NaN metallic")
        unsure = np.zeros(LANES, bool)
        if poke is not None:
            row, col = poke[0], poke[1]
            for tap, firm, lanes in ((q["reflection_tap"], q["tap_firm"], geo), (q["view_tap"], q["view_tap_firm"], active & ~q["geometry"])):
                covers = (tap[:, 0] >= 0) & (np.abs(tap[:, 0] + 0.5 - col) <= 0.5) & (np.abs(tap[:, 1] + 0.5 - row) <= 0.5)
                close = (tap[:, 0] >= 0) & (np.abs(tap[:, 0] + 0.5 - col) <= 1.5) & (np.abs(tap[:, 1] + 0.5 - row) <= 1.5)
                mark(lanes & covers & firm, "the sky-view tap meets the poked texel")
                unsure |= lanes & close & ~(covers & firm)
        poisoned = why != ""
        # --- and where it must not: ordinary texels, or sky, under an ordinary frame
        plain_lane = _is_plain(sc, group.camera)
        plain_frame = group.base_name in CLEAN_GROUPS or group.base_name.startswith(("half_vector_", "view_length_mixed", "view_length_partial"))
        clean = active & ~poisoned & ~unsure & plain_frame & (plain_lane | ~q["geometry"])
        if np.isinf(group.slut_value or 0.0) and group.slut_target == "tap":
            clean &= False  # an inf texel gives inf or NaN by its weight: no claim
    return {"value": value, "side": side, "near": near, "exact": exact, "active": active, "geometry": geo, "poisoned": poisoned,
            "clean": clean, "why": why, "threshold": thresholds, "unsure": unsure}


# groups whose frame-level inputs are ordinary: a lane with an ordinary texel there is finite in the reference
CLEAN_GROUPS = ("surface_length", "surface_radius", "skip_all_true", "skip_normal", "skip_sky_nan_tap", "skip_sky_nan_far",
                "skip_sky_inf_far", "classification", "planet_shadow_day", "shadow_random", "shadow_zero")


def _is_plain(sc, camera):
    """bool [64]: the lane holds the ordinary texel or the ordinary metal (any prior colour), at its own place or AT the camera."""
    out = np.zeros(LANES, bool)
    for ref in (ORDINARY, METAL):
        same = sc.depth == ref["depth"]
        for key in ("n", "d", "s", "o"):
            same &= (sc.planes[key] == ref[key]).all(axis=1)
        out |= same & ((sc.planes["p"] == ref["p"]).all(axis=1) | (sc.planes["p"] == camera).all(axis=1))
    return out


def geometry_gate(gate):
    """Gates evaluated in the geometry branch only: a sky lane does not meet them."""
    return gate not in ("depth_zero", "underground")


def verdict(group, k, lane):
    """One line for a failure message: the side of every gate for one lane, the near ones marked."""
    c = census(group, k)
    parts = []
    for gate in GATES:
        mark = "=" if c["exact"][gate][lane] else ("~" if c["near"][gate][lane] and gate not in FLAGS else "")
        parts.append(f"{gate}:{ {-1: 'nan', 0: 'below', 1: 'above'}[int(c['side'][gate][lane])]}{mark}")
    kind = "geometry" if c["geometry"][lane] else ("sky" if c["active"][lane] else "outside")
    return f"[{kind} | {' '.join(parts)} | {c['why'][lane] or ('clean' if c['clean'][lane] else 'no claim')}]"


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs and the oracle's frame of a group (computed once per process, read-only)
# ---------------------------------------------------------------------------------------------------------------------------
_INPUTS, _ORACLE = {}, {}


class FrameInputs:
    pass


def frame_inputs(group):
    """Everything one recordComposite call of the group reads: rect, blocks, both LUTs (the oracle's, poked), the G-buffer planes,
    depth and prior colour cut to the draw extent, the shadow map view or None."""
    if group.name not in _INPUTS:
        from oracle import binding as ob

        W, H = group.extent
        f = FrameInputs()
        f.width, f.height, f.rect = W, H, abi.Rect(0, 0, W, H)
        f.atm, f.cam = group.atm, group.cam
        f.sun = shadow_sun()
        f.dirs = (abi.DirectionalLightPacked * 2)(f.sun, abi.DirectionalLightPacked())
        planes, depth, prior = group.images()
        f.planes = {k: np.ascontiguousarray(v[:H, :W]) for k, v in planes.items()}
        f.depth, f.prior = np.ascontiguousarray(depth[:H, :W]), np.ascontiguousarray(prior[:H, :W])
        f.tlut = ob.transmittance_lut(f.atm, TLUT_EXTENT[0], TLUT_EXTENT[1], threads=8)
        if group.tlut_poke is not None:
            row, col, channel, value = group.tlut_poke
            f.tlut[row, col, channel] = value
        f.slut = ob.skyview_lut(f.atm, f.cam, f.tlut, SLUT_EXTENT[0], SLUT_EXTENT[1], threads=8)
        if group.slut_poke is not None:
            row, col, channel, value = group.slut_poke
            f.slut[row, col, channel] = value
        f.shadow = shadow_map(group.shadow) if group.shadow is not None else None
        for a in (f.tlut, f.slut, f.depth, f.prior) + tuple(f.planes.values()):
            a.setflags(write=False)
        _INPUTS[group.name] = f
    return _INPUTS[group.name]


def oracle_frame(group, aerial=None):
    """(debug [H, W, 4] float32, colour [H, W, 4] uint16) of oracle.composite over the group; with aerial=(volume, max distance)
    the fast composite on that volume (not cached: the volume is the caller's)."""
    key = group.name
    if aerial is None and key in _ORACLE:
        return _ORACLE[key]
    from oracle import binding as ob

    f = frame_inputs(group)
    frame = ob.HostFrame(f.width, f.height)
    frame.diffuse[:], frame.specular[:], frame.normal[:] = f.planes["diffuse"], f.planes["specular"], f.planes["normal"]
    frame.position[:], frame.orm[:] = f.planes["worldPosition"], f.planes["occlusionRoughnessMetallic"]
    frame.depth[:], frame.color[:] = f.depth, f.prior
    shadow, images = None, (abi.Image * 1)()
    if f.shadow is not None:
        images[0] = ob.host_image(f.shadow, abi.SZG_FORMAT_D32_SFLOAT)
        shadow = abi.ShadowMaps(1, 0, C.cast(images, C.POINTER(abi.Image)))
    ob.composite(frame, f.rect, None, shadow, f.atm, f.cam, f.dirs, 0, f.tlut, f.slut, threads=8, aerial=aerial)
    frame.debug.setflags(write=False)
    frame.color.setflags(write=False)
    if aerial is None:
        _ORACLE[key] = (frame.debug, frame.color)
    return frame.debug, frame.color


def tile_of(group, k, image):
    """[64, c] lanes of scenario k cut from an [H, W, c] image of the draw extent; lanes outside the extent are 0."""
    x0, y0 = group.origin(k)
    out = np.zeros((8, 8) + image.shape[2:], image.dtype)
    part = image[y0:y0 + 8, x0:x0 + 8]
    out[:part.shape[0], :part.shape[1]] = part
    return out.reshape((LANES,) + image.shape[2:])


def counts(G):
    """(groups, scenarios, lanes inside the draw extent, gates) for the record."""
    lanes = sum(int(g.active(k).sum()) for g in G for k in range(g.tiles))
    return len(G), sum(g.tiles for g in G), lanes, len(GATES)
