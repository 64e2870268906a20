"""A float64 numpy restatement of the sky-view LUT's march with BOTH terms of include/szg/multiscatter_sky.h: the reference's
single-scattering sum (atmosphere/common.glinl:364-424) and the multi-scattering sum beside it. An independent model, not a
bit-exact one: every operation is a binary64 one, vectorised over the texels of the LUT, and the only binary32 values in it are
the texels of the two LUTs it is handed as data (the transmittance LUT and the multi-scattering LUT).

What it restates, each from the shader text:
  skyview_rays        skyview_LUT.comp:51-119   texel -> (origin, direction), with the non-linear elevation map
  ray_sphere          common.glinl:220-260      both roots, `false` leaves t0 / t1 at their initial 0
  raycast_atmosphere  common.glinl:284-307
  tap                 common.glinl:40-66        the Bruneton (radius, mu) -> uv map, then `bilinear`
  bilinear            LINEAR / CLAMP_TO_EDGE: u * W - 0.5, floor, weights taken before the indices are clamped
  step_radius_mu      common.glinl:316-334      with its quirk Q2: the "cosine sum" is the square root of a difference
  march               common.glinl:364-424      t < 1e-7 -> transmittanceToBegin = 1 (:338-341); the segment ratio with its
                                                direction flip (:114-136); the multi-scattering term of the header

tests/test_multiscatter_sky_model.py holds the single-scattering part against the oracle's sky-view LUT and the properties of
the multi-scattering part; tests/test_gpu_multiscatter_sky.py holds k_skyview_ms<ONLY> against the multi-scattering part.
"""
import numpy as np

# The model's distance from the oracle (tests/test_multiscatter_sky_model.py, metric() below): the largest value over the
# eight cases of that test (64 x 32 sky-view LUT, 512 x 128 transmittance LUT from the oracle, cameras at 2500 m and
# 30 000 m, suns at 70, 35, 5 and -3 degrees), measured by that test on the CPU against oracle.binding.skyview_lut and
# rounded up to two digits (measured: 6.509e-4 at 2500 m, sun 70 degrees, texel (6, 26); 5.704e-4 at 30 000 m, sun -3 degrees,
# texel (61, 3); that test fails when a figure here is below its measurement or more than a quarter above it). The GPU test's
# tolerance for the multi-scattering part is 2 * D0: it is taken from this comparison with the oracle, never from the kernel.
D0_BY_CAMERA = {2500.0: 6.6e-4, 30000.0: 5.8e-4}
D0 = max(D0_BY_CAMERA.values())

MS_DIM = 32
PI = np.pi


def atmosphere(atm):
    """The fields of an abi.AtmospherePacked as float64 (every one a binary32 value, exactly)."""
    v = lambda a: np.array([float(a[0]), float(a[1]), float(a[2])])  # noqa: E731
    return {"sR": v(atm.scatteringRayleighPerMm), "aR": v(atm.absorptionRayleighPerMm), "sM": v(atm.scatteringMiePerMm),
            "sO": v(atm.scatteringOzonePerMm), "aO": v(atm.absorptionOzonePerMm), "HR": float(atm.densityScaleRayleighMm),
            "HM": float(atm.densityScaleMieMm), "Rp": float(atm.planetRadiusMm), "Ra": float(atm.atmosphereRadiusMm),
            "sun": v(atm.incidentDirectionSun), "sunRadius": float(atm.sunAngularRadius)}


def safe_sqrt(x):
    return np.sqrt(np.maximum(x, 0.0))


def dot(a, b):
    return (a * b).sum(-1)


def length(a):
    return np.sqrt(dot(a, a))


def normalize(a):
    return a / length(a)[..., None]


def skyview_rays(A, cam, W, H):
    """origin [3] and direction [H, W, 3] of every texel (skyview_LUT.comp:100-119)."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    u, v = (x + 0.5) / W, (y + 0.5) / H
    origin = np.array([float(cam.position[0]), float(cam.position[1]), float(cam.position[2])]) / 1000000.0
    origin[1] *= -1.0
    origin[1] += A["Rp"]
    horizon_zenith = PI - np.arcsin(A["Rp"] / length(origin))
    light = np.array([-A["sun"][0], -A["sun"][2]])
    light = light / np.sqrt((light * light).sum())
    azimuth_sun = np.arcsin(light[0])
    if light[1] < 0.0:
        azimuth_sun = PI - azimuth_sun
    azimuth = np.arccos(np.clip((u - 0.5) * 2.0, -1.0, 1.0)) + azimuth_sun
    w = 2.0 * v - 1.0
    zenith = np.where(v < 0.5, (1.0 - w * w) * horizon_zenith, (PI - horizon_zenith) * (w * w) + horizon_zenith)
    elevation = -(zenith - PI / 2.0)
    ce = np.cos(elevation)
    direction = normalize(np.stack([np.sin(azimuth) * ce, np.sin(elevation), np.cos(azimuth) * ce], -1))
    return origin, direction


def ray_sphere(f, d, radius):
    """(hit, t0, t1), t0 <= t1 (common.glinl:220-260); a miss leaves t0 = t1 = 0."""
    b = -dot(f, d)
    chord = f + b[..., None] * d
    disc = radius * radius - dot(chord, chord)
    c = dot(f, f) - radius * radius
    hit = ~(disc < 0.0)
    s = np.sqrt(np.where(hit, disc, 0.0))
    q = np.where(b < 0.0, b - s, b + s)
    with np.errstate(divide="ignore", invalid="ignore"):
        a0, a1 = c / q, q
    t0, t1 = np.where(a0 > a1, a1, a0), np.where(a0 > a1, a0, a1)
    return hit, np.where(hit, t0, 0.0), np.where(hit, t1, 0.0)


def raycast_atmosphere(A, origin, direction):
    hit_a, at0, at1 = ray_sphere(origin, direction, A["Ra"])
    hit_a = hit_a & (at1 > 0.0)
    at0 = np.maximum(0.0, at0)
    hit_p, pt0, _ = ray_sphere(origin, direction, A["Rp"])
    hit_p = hit_p & (pt0 > 0.0)
    at1 = np.where(hit_p, np.minimum(pt0, at1), at1)
    return np.where(hit_a, at1 - at0, 0.0)


def bilinear(texels, s, t):
    """rgb of a LINEAR / CLAMP_TO_EDGE fetch of `texels` [H, W, >= 3] at the normalised coordinates (s, t)."""
    H, W = texels.shape[0], texels.shape[1]
    u, v = s * W - 0.5, t * H - 0.5
    fu, fv = np.floor(u), np.floor(v)
    a, b = (u - fu)[..., None], (v - fv)[..., None]
    i0, i1 = np.clip(fu, 0, W - 1).astype(np.int64), np.clip(fu + 1.0, 0, W - 1).astype(np.int64)
    j0, j1 = np.clip(fv, 0, H - 1).astype(np.int64), np.clip(fv + 1.0, 0, H - 1).astype(np.int64)
    rgb = texels[..., :3].astype(np.float64)
    return a * b * rgb[j1, i1] + ((1.0 - a) * b * rgb[j1, i0] + (a * (1.0 - b) * rgb[j0, i1] + (1.0 - a) * (1.0 - b) * rgb[j0, i0]))


def tap(A, tlut, radius, mu):
    """sampleTransmittanceLUT_RadiusMu: the Bruneton map (common.glinl:40-66) and the bilinear fetch."""
    H, W = tlut.shape[0], tlut.shape[1]
    Ra2, Rp2 = A["Ra"] * A["Ra"], A["Rp"] * A["Rp"]
    Hh = safe_sqrt(Ra2 - Rp2)
    rho = safe_sqrt(radius * radius - Rp2)
    d = np.maximum(-radius * mu + safe_sqrt(radius * radius * (mu * mu - 1.0) + Ra2), 0.0)
    d_min, d_max = A["Ra"] - radius, rho + Hh
    x_mu, x_radius = (d - d_min) / (d_max - d_min), rho / Hh
    return bilinear(tlut, 0.5 / W + x_mu * (1.0 - 1.0 / W), 0.5 / H + x_radius * (1.0 - 1.0 / H))


def tap_ray(A, tlut, position, direction):
    radius = length(position)
    return tap(A, tlut, radius, dot(position, direction) / (radius * length(direction)))


def segment(A, tlut, begin, end):
    """sampleTransmittanceLUT_Segment (common.glinl:114-136): the ratio of two taps, flipped when the segment points down."""
    direction = normalize(end - begin)
    flip = (dot(begin, direction) < 0.0)[..., None]
    up = tap_ray(A, tlut, begin, direction) / tap_ray(A, tlut, end, direction)
    down = tap_ray(A, tlut, end, -direction) / tap_ray(A, tlut, begin, -direction)
    return np.clip(np.where(flip, down, up), 0.0, 1.0)


def step_radius_mu(radius, mu, mu_sun, t):
    # quirk Q2 (common.glinl:325): not cos(a + b) = cos a cos b - sin a sin b, but the square root of that expression
    mu_sun_and_step = safe_sqrt(mu_sun * mu - safe_sqrt((1.0 - mu_sun * mu_sun) * (1.0 - mu * mu)))
    r = safe_sqrt(t * t + 2.0 * radius * mu * t + radius * radius)
    return r, (radius * mu + t) / r, (radius * mu_sun + t * mu_sun_and_step) / r


def extinction(A, altitude):
    dR, dM = np.exp(-altitude / A["HR"])[..., None], np.exp(-altitude / A["HM"])[..., None]
    dO = np.maximum(0.0, 1.0 - np.abs(altitude * 1000.0 - 25.0) / 15.0)[..., None]
    sR, sM = A["sR"] * dR, A["sM"] * dM
    return sR, sM, sR + A["aR"] * dR + sM + A["aR"] * dM + A["sO"] * dO + A["aO"] * dO  # (Mie absorbs with the Rayleigh coefficient, Q1)


def multiscatter_coordinates(A, altitude, mu_sun):
    """(su, sv) of the header's rule."""
    return np.clip(0.5 + 0.5 * mu_sun, 0.0, 1.0), np.clip(altitude / (A["Ra"] - A["Rp"]), 0.0, 1.0)


def march(A, tlut, origin, direction, distance, psi=None):
    """(single, multi): the two sums of the 32-step integral for rays from `origin` [3] along `direction` [..., 3] over
    `distance` [...]. `psi`: the multi-scattering LUT [32, 32, >= 3] or None (multi is then 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = -normalize(direction)
        radius = length(origin)
        mu = dot(origin, direction) / (radius * length(direction))
        mu_sun = dot(origin, -A["sun"]) / (radius * length(A["sun"]))
        cosine = dot(A["sun"], sd)[..., None]
        g = 0.8
        pR = 3.0 / (16.0 * PI) * (1.0 + cosine * cosine)
        pM = 3.0 / (8.0 * PI) * (1.0 - g * g) * (1.0 + cosine * cosine) / ((2.0 + g * g) * (1.0 + g * g - 2.0 * g * cosine) ** 1.5)
        sin_sr, cos_sr = np.sin(A["sunRadius"]), np.cos(A["sunRadius"])
        up = (mu > 0.0)[..., None]
        T_origin = tap(A, tlut, radius, np.where(mu > 0.0, mu, -mu))
        dS = distance / 32.0
        single, multi = np.zeros(direction.shape), np.zeros(direction.shape)
        for i in range(32):
            t = i * dS
            begin = origin - (i * dS)[..., None] * sd
            end = origin - ((i + 1) * dS)[..., None] * sd
            s_r, s_mu, s_musun = step_radius_mu(radius, mu, mu_sun, t)
            altitude = length(begin) - A["Rp"]
            # sampleTransmittanceLUT_Sun (common.glinl:145-172)
            sin_hz = A["Rp"] / s_r
            cos_hz = -safe_sqrt(1.0 - sin_hz * sin_hz)
            e0, e1 = -sin_hz * sin_sr, sin_hz * sin_sr
            ss = np.clip((s_musun - cos_hz * cos_sr - e0) / (e1 - e0), 0.0, 1.0)
            T_sun = tap(A, tlut, s_r, s_musun) * (ss * ss * (3.0 - 2.0 * ss))[..., None]
            sR, sM, ext = extinction(A, altitude)
            # sampleTransmittanceLUT_RayMarchStep (common.glinl:336-361)
            T_end = tap(A, tlut, s_r, np.where(mu > 0.0, s_mu, -s_mu))
            ratio = np.clip(np.where(up, T_origin / T_end, T_end / T_origin), 0.0, 1.0)
            T_begin = np.where((t < 0.0000001)[..., None], 1.0, ratio)
            integral = (1.0 - segment(A, tlut, begin, end)) / ext
            single += (sR * pR + sM * pM) * T_sun * integral * T_begin
            if psi is not None:
                su, sv = multiscatter_coordinates(A, altitude, s_musun)
                multi += (sR + sM) * bilinear(psi, su, sv) * integral * T_begin
    return single, multi


def skyview(atm, cam, tlut, W, H, psi=None):
    """(single, multi) [H, W, 3] each: the sky-view LUT's two terms for an abi.AtmospherePacked and abi.CameraPacked."""
    A = atmosphere(atm)
    origin, direction = skyview_rays(A, cam, W, H)
    return march(A, tlut, origin, direction, raycast_atmosphere(A, origin, direction), psi)


def metric(got, want):
    """|got - want| / max(|want|, 1e-3 * max|want| over the LUT), elementwise."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.maximum(np.abs(want), 1e-3 * np.abs(want).max())
