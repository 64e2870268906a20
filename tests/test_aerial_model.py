"""CPU: the fast composite's aerial-perspective fetch (include/szg/abi.h "THE FETCH of the fast composite").

The oracle's oracle_aerial_sample against an independent numpy model of the header's text (tests/aerial_model.py), bit for
bit; identities that follow from the rule; the proof that the frames of tests/test_gpu_fast_composite.py reach every part of
the fetch; and what "approximate" amounts to. Nothing here needs a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests import aerial_model as am
from tests import util

F = np.float32
W, H, D = DIMS = (32, 32, 32)
# two powers of two (exact slice centres), the bench's setting and one of the GPU tests'
CLOUD_MAX_DISTANCES = (2.0 ** -5, 2.0 ** -13, 0.032, 1.2e-3)
CLOUD_POINTS = 40000  # per max distance: 160 000 in all


def slice_centres(max_distance):
    """d_k as the LUT pass computes it: ((k + .5) / D) * max_distance in binary32."""
    return (np.arange(D, dtype=F) + F(0.5)) / F(D) * F(max_distance)


@functools.lru_cache(maxsize=None)
def volumes():
    """(finite, poisoned): a random positive volume over three decades, and a copy with a few NaN and inf values."""
    rng = np.random.default_rng(0xAE41A1)
    finite = (10.0 ** rng.uniform(-4.0, -1.0, (D * H, W, 4))).astype(F)
    finite[..., 3] = 1.0
    poisoned = finite.copy()
    flat = poisoned.reshape(-1, 4)
    for value, count in ((np.nan, 12), (np.inf, 8)):
        for texel in rng.choice(len(flat), count, replace=False):
            flat[texel, rng.integers(0, 3)] = value
    flat[rng.choice(len(flat), 4, replace=False), :3] = np.nan
    for v in (finite, poisoned):
        v.setflags(write=False)
    return finite, poisoned


@functools.lru_cache(maxsize=None)
def cloud(max_distance):
    """Seeded points (sx, sy, dist): screen coordinates over [0, 1] with 0, 1 and the pixels of 1-, 33- and 64-pixel extents;
    distances from 0 through every slice to 1e3 * max_distance, exact slice centres and their neighbours, +inf, NaN,
    denormals."""
    rng = np.random.default_rng(int(max_distance * 2.0 ** 40) & 0xFFFFFFFF)
    n = CLOUD_POINTS
    m = F(max_distance)

    def screen():
        s = rng.random(n, dtype=F)
        pixels = np.concatenate([np.arange(e, dtype=F) / F(e) for e in (1, 33, 64)])  # x / width, last pixel included
        special = np.concatenate([pixels, np.array([0.0, 1.0, 0.5, 1.0 / 64.0, 63.0 / 64.0], F)])
        s[: n // 4] = special[rng.integers(0, len(special), n // 4)]
        return rng.permutation(s)

    centres = slice_centres(max_distance)
    parts = [
        (rng.random(n // 2) * 1.05 * float(m)).astype(F),                                     # through every slice
        (10.0 ** rng.uniform(-45.0, np.log10(1.0e3 * float(m)), n // 4)).astype(F),         # denormals .. 1e3 max distance
        centres[rng.integers(0, D, n // 16)],                                                # exact slice centres
        np.nextafter(centres[rng.integers(0, D, n // 16)], F(np.inf)),
        np.nextafter(centres[rng.integers(0, D, n // 16)], F(0.0)),
    ]
    special = np.array([0.0, np.inf, np.nan, 1.0e-45, 1.0e-40, 1.1754942e-38, 1.17549435e-38, float(m), 1.0e3 * float(m),
                        float(centres[0]), float(centres[-1]), float(np.nextafter(centres[-1], F(0.0)))], F)
    used = sum(len(p) for p in parts)
    parts.append(special[rng.integers(0, len(special), n - used)])
    dist = rng.permutation(np.concatenate(parts))
    assert dist.size == n
    out = screen(), screen(), dist
    for a in out:
        a.setflags(write=False)
    return out


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == F
    assert (np.isnan(got) == np.isnan(want)).all(), f"{what}: NaN patterns differ"
    ok = ~np.isnan(want)
    bad = got.view(np.uint32)[ok] != want.view(np.uint32)[ok]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(ok.sum())} values differ in bits"


# ---------------------------------------------------------------------------
# oracle == fp32 model, bit for bit
# ---------------------------------------------------------------------------
def test_cloud_is_what_it_claims():
    assert len(CLOUD_MAX_DISTANCES) * CLOUD_POINTS >= 100000
    for m in CLOUD_MAX_DISTANCES:
        sx, sy, dist = cloud(m)
        ramp, k0, k1, wz = am.slice_coordinate(dist, m, D)
        interior = (wz > 0.1) & (wz < 0.9)
        assert all((interior & (k0 == k)).sum() >= 100 for k in range(D - 1)), "every pair of slices"
        with np.errstate(invalid="ignore"):
            assert ((ramp < 1) & (ramp > 0)).sum() >= 1000 and (dist >= 1.0e2 * m).sum() >= 100
        assert np.isnan(dist).any() and np.isinf(dist).any() and (dist == 0).any()
        assert ((dist > 0) & (dist < 1.0e-38)).sum() >= 100, "denormal distances"
        for s in (sx, sy):
            assert (s == 0).any() and (s == F(32.0) / F(33.0)).any() and (s == F(63.0 / 64.0)).any() and s.min() >= 0 and s.max() <= 1
    exact = slice_centres(2.0 ** -5).astype(np.float64) / 2.0 ** -5 * D - 0.5
    assert (exact == np.arange(D)).all(), "with a power-of-two max distance the slice centres are exact"


@pytest.mark.parametrize("max_distance", CLOUD_MAX_DISTANCES)
def test_oracle_sample_equals_the_model_bit_for_bit(max_distance):
    finite, poisoned = volumes()
    sx, sy, dist = cloud(max_distance)
    for name, vol in (("finite", finite), ("poisoned", poisoned)):
        got = ob.aerial_sample(vol, max_distance, sx, sy, dist)
        want = am.sample32(vol, max_distance, sx, sy, dist)
        same_bits(got, want, f"{name} volume, max distance {max_distance}")
        if name == "poisoned":
            assert np.isnan(got).any() and np.isinf(got).any() and np.isfinite(got).any()
        else:
            assert np.isfinite(got).all()


# The largest distance of oracle_aerial_sample from the float64 evaluation of the rule, relative to
# max(|value|, largest froxel * 2^-20), measured on the cloud above (finite volume), per max distance. At the two powers of two
# z = dist / maxDistance * 32 - 0.5 is exact at the slice centres and what remains is a few ulps (the four rounded terms of
# the sums). At 0.032 and 1.2e-3 the worst points sit AT a slice centre (dist = d_17, d_22): z carries the quotient's and the
# product's roundings at the size of z (up to 31: ~2e-6 absolute), so the slice weight wz is off by that much, and beside a
# slice centre the weight of the OTHER slice is about that error itself. The random volume spans three decades: a neighbour
# slice a few hundred times brighter turns 2e-6 of weight into 3e-4 of the value (mean over the cloud: 6e-7). Each bound is
# its measurement times 4, the margin for other seeds.
MEASURED_WORST_VS_FLOAT64 = {2.0 ** -5: 2.73e-7, 2.0 ** -13: 2.52e-7, 0.032: 3.01e-4, 1.2e-3: 2.79e-4}


@pytest.mark.parametrize("max_distance", CLOUD_MAX_DISTANCES)
def test_oracle_sample_against_the_float64_model(max_distance):
    m = max_distance
    finite, _ = volumes()
    floor = float(finite[..., :3].max()) * 2.0 ** -20
    sx, sy, dist = cloud(m)
    got = ob.aerial_sample(finite, m, sx, sy, dist).astype(np.float64)
    want = am.sample64(finite, m, sx, sy, dist)
    assert np.isfinite(want).all()
    err = np.abs(got - want) / np.maximum(np.abs(want), floor)
    i = np.unravel_index(np.argmax(err), err.shape)
    print(f"max distance {m:.6g}: worst relative distance from float64 {err.max():.3e} at dist {dist[i[0]]!r} "
          f"(dist / d_0 = {dist[i[0]] / slice_centres(m)[0]:.4f}), mean {err.mean():.3e}")
    assert err.max() <= 4.0 * MEASURED_WORST_VS_FLOAT64[m]


# ---------------------------------------------------------------------------
# exact identities, for the oracle and for the model
# ---------------------------------------------------------------------------
IMPLEMENTATIONS = {"oracle": ob.aerial_sample, "model": am.sample32}
implementations = pytest.mark.parametrize("sample", list(IMPLEMENTATIONS.values()), ids=list(IMPLEMENTATIONS))


@implementations
def test_pixels_on_froxel_centres_return_the_froxel(sample):
    """Extent 64 x 64: pixel (2i + 1, 2j + 1) has u = i, v = j exactly; at dist = d_k (power-of-two max distance) z = k."""
    finite, _ = volumes()
    m = 2.0 ** -7
    k, j, i = (a.ravel() for a in np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij"))
    sx, sy = (2 * i + 1).astype(F) / F(64), (2 * j + 1).astype(F) / F(64)
    got = sample(finite, m, sx, sy, slice_centres(m)[k])
    want = np.ascontiguousarray(am.volume_view(finite)[k, j, i, :3])
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


@implementations
def test_distance_zero_is_plus_zero(sample):
    finite, _ = volumes()
    rng = np.random.default_rng(5)
    sx, sy = rng.random(512, dtype=F), rng.random(512, dtype=F)
    for m in CLOUD_MAX_DISTANCES:
        got = sample(finite, m, sx, sy, np.zeros(512, F))
        assert (got.view(np.uint32) == 0).all()


@implementations
def test_behind_the_last_slice_is_its_bilinear_tap(sample):
    finite, _ = volumes()
    rng = np.random.default_rng(6)
    sx, sy = rng.random(512, dtype=F), rng.random(512, dtype=F)
    for m in CLOUD_MAX_DISTANCES:
        last = slice_centres(m)[-1]
        want = am.bilinear(am.volume_view(finite)[D - 1], sx, sy)
        # AT the last centre z = D - 1 only where the binary32 quotient is exact: the power-of-two max distances (elsewhere z
        # may round to just below D - 1, and the value is slice D - 2's with a weight of an ulp: the cloud covers that)
        exact_centre = (last,) if np.log2(m) == np.round(np.log2(m)) else ()
        for d in exact_centre + (np.nextafter(F(m), F(0.0)), F(m), F(1.0e3 * m), F(1.0e30), F(np.inf)):
            got = sample(finite, m, sx, sy, np.full(512, d, F))
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), (m, d)


@implementations
def test_the_corner_pixel_reads_only_the_corner_column_and_row(sample):
    """sx = sy = 0: u = v = -0.5, both indices of each axis clamp to 0. Every other froxel is NaN and must not show."""
    finite, _ = volumes()
    vol = np.full((D, H, W, 4), np.nan, F)
    vol[:, 0, 0] = am.volume_view(finite)[:, 0, 0]
    m = 2.0 ** -5
    dist = np.concatenate([cloud(m)[2][:4096], slice_centres(m)])
    dist = dist[~np.isnan(dist)]
    zero = np.zeros(dist.size, F)
    got = sample(vol, m, zero, zero, dist)
    assert np.isfinite(got).all()
    same_bits(got, sample(np.broadcast_to(vol[:, :1, :1], vol.shape).copy(), m, zero, zero, dist), "corner")


def test_index_revealing_volume_stays_inside_the_named_froxels():
    """Froxel (i, j, k) = i + 32 j + 1024 k: the value lies between the smallest and the largest of the eight froxels the
    header names - a swapped axis or a wrong stride in a GATHER would leave that range. The eight indices come from the
    model's own slice and texel coordinates (am.named_froxels), so this checks the gathers of model and oracle, not the index
    arithmetic: that is pinned independently by test_pixels_on_froxel_centres_return_the_froxel."""
    k, j, i = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    vol = np.zeros((D, H, W, 4), F)
    vol[..., :3] = (i + 32 * j + 1024 * k)[..., None]
    for m in CLOUD_MAX_DISTANCES:
        sx, sy, dist = cloud(m)
        keep = dist >= slice_centres(m)[0]  # (below d_0 the ramp scales the value towards 0; NaN distances drop out too)
        sx, sy, dist = sx[keep], sy[keep], dist[keep]
        i0, i1, j0, j1, k0, k1 = am.named_froxels(sx, sy, dist, m)
        corners = np.stack([a + 32 * b + 1024 * c for a in (i0, i1) for b in (j0, j1) for c in (k0, k1)]).astype(np.float64)
        for name, got in (("model", am.sample32(vol, m, sx, sy, dist)), ("float64 model", am.sample64(vol, m, sx, sy, dist)),
                          ("oracle", ob.aerial_sample(vol, m, sx, sy, dist))):
            got = got.astype(np.float64)
            assert (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()
            slack = 4.0 * 2.0 ** -24 * corners.max(0)  # the four roundings of a sum of non-negative terms
            assert (got[:, 0] >= corners.min(0) - slack).all() and (got[:, 0] <= corners.max(0) + slack).all(), name
        assert (corners.max(0) - corners.min(0)).max() == 1 + 32 + 1024 and (corners.max(0) == corners.min(0)).any()


# ---------------------------------------------------------------------------
# the frames of the GPU tests reach the whole fetch
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coverage_inputs(extent):
    return util.Inputs(extent[0], extent[1], elevation_degrees=am.COVERAGE_ELEVATION, spots=am.COVERAGE_SPOTS)


def filled_frame(extent, lights=True):
    inp = coverage_inputs(extent)
    frame = ob.HostFrame(extent[0], extent[1])
    ob.gbuffer_fill(frame, inp.rect, None, inp.cam, inp.synthetic.fill, threads=4)
    if lights:
        ob.lights(frame, inp.rect, None, None, inp.cam, inp.dirs, 2, 1, inp.spots, am.COVERAGE_SPOTS, threads=4)
    return frame


@pytest.mark.parametrize("extent", am.COVERAGE_EXTENTS)
def test_coverage_condition_of_the_gpu_frames(extent):
    """A cap, not a measurement: over the max distances of the GPU tests together, every k0 in 0 .. 30 is hit by at least 32 geometry
    pixels with 0.1 < wz < 0.9, at least 32 lie in the ramp and at least 32 behind the last slice."""
    frame = filled_frame(extent, lights=False)
    geometry, dist = am.geometry_distances(frame, coverage_inputs(extent).cam)
    dist = dist[geometry]
    between = np.zeros(D - 1, np.int64)
    ramp = behind = 0
    for m in am.COVERAGE_MAX_DISTANCES:
        fz = dist / float(F(m)) * D - 0.5
        ramp += int((fz < 0).sum())
        behind += int((fz >= D - 1).sum())
        inside = (fz >= 0) & (fz < D - 1)
        k0 = np.floor(fz[inside]).astype(np.int64)
        wz = fz[inside] - k0
        between += np.bincount(k0[(wz > 0.1) & (wz < 0.9)], minlength=D - 1)
    print(f"{extent}: {geometry.sum()} geometry pixels; fewest between a pair of slices {between.min()} (k0 = {between.argmin()}), "
          f"ramp {ramp}, behind the last slice {behind}")
    assert between.min() >= 32 and ramp >= 32 and behind >= 32


# ---------------------------------------------------------------------------
# what "approximate" means
# ---------------------------------------------------------------------------
APPROXIMATE_MAX_DISTANCES = am.COVERAGE_MAX_DISTANCES + (10.0e-3, 0.032)


def test_what_approximate_means():
    """oracle_composite_fast against oracle_composite on the 70 x 37 frame, and the aerial addend alone against the oracle's
    march, for every max distance of the GPU tests, the 10 km of the closeness test and the bench's 0.032 Mm. Only the
    10 km row is asserted (the 5e-2 / 5e-3 that test_fast_composite_is_close_to_the_exact_one claims); the others document
    the mode."""
    extent = am.COVERAGE_EXTENTS[0]
    width, height = extent
    inp = coverage_inputs(extent)
    (tw, th), (sw, sh) = am.LUT
    tlut = ob.transmittance_lut(inp.atm, tw, th, threads=4)
    slut = ob.skyview_lut(inp.atm, inp.cam, tlut, sw, sh, threads=4)
    exact = filled_frame(extent)
    geometry, dist = am.geometry_distances(exact, inp.cam)
    ob.composite(exact, inp.rect, None, None, inp.atm, inp.cam, inp.dirs, 0, tlut, slut, threads=4)

    # the march of every geometry pixel: camera.comp:320-328 origin and direction, length to the surface
    origin = np.array(inp.cam.position[:3], F) / F(1.0e6)
    origin[1] = -origin[1] + F(inp.atm.planetRadiusMm)
    directions = am.pixel_directions(inp.cam, width, height).astype(F)
    ys, xs = np.nonzero(geometry)
    dist32 = dist[geometry].astype(F)
    march = np.zeros((len(ys), 3), F)
    for n, (y, x) in enumerate(zip(ys, xs)):
        ob.lib().oracle_scattering_integral(C.byref(inp.atm), ob.fptr(tlut), tw, th, ob.fptr(origin), ob.fptr(np.ascontiguousarray(directions[y, x])),
                                            float(dist32[n]), ob.fptr(march[n]))
    assert np.isfinite(march).all() and (march > 0).all()

    # How much of a pixel the addend is: the composite stores pow(10 * transfer * sunIntensitySpectrum + surfaceLuminance, 1.2)
    # (the end of camera.comp's main, as the oracle's composite restates it), so debug ** (1 / 1.2) is the sum before the tone curve and 10 * march * sunIntensity the march's part of it.
    share = (10.0 * march * np.array(inp.atm.sunIntensitySpectrum[:3], np.float64)).mean() / \
        (exact.debug[geometry][:, :3].astype(np.float64) ** (1.0 / 1.2)).mean()
    print(f"the exact march is {share:.3e} of the mean geometry pixel (before the tone curve)")
    print("max distance [Mm] | pixel: max rel, mean rel | aerial addend: max rel, mean rel")
    rows = {}
    for m in APPROXIMATE_MAX_DISTANCES:
        lum, _ = ob.aerial_lut(inp.atm, inp.cam, tlut, m, threads=4)
        fast = filled_frame(extent)
        ob.composite(fast, inp.rect, None, None, inp.atm, inp.cam, inp.dirs, 0, tlut, slut, threads=4, aerial=(lum, m))
        assert (fast.debug[~geometry].view(np.uint32) == exact.debug[~geometry].view(np.uint32)).all(), "sky pixels are the exact composite's"
        rel = util.rel_err(exact.debug[geometry][:, :3], fast.debug[geometry][:, :3], util.ATOL_COLOR)
        addend = ob.aerial_sample(lum, m, xs.astype(F) / F(width), ys.astype(F) / F(height), dist32).astype(np.float64)
        addend_rel = np.abs(addend - march) / march
        rows[m] = (rel.max(), rel.mean(), np.nanmax(addend_rel), np.nanmean(addend_rel))
        print(f"{m:<9.6g} | {rel.max():.3e}, {rel.mean():.3e} | {np.nanmax(addend_rel):.3e}, {np.nanmean(addend_rel):.3e}")
    assert rows[10.0e-3][0] < 5e-2 and rows[10.0e-3][1] < 5e-3
