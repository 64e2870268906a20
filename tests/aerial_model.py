"""The fast composite's aerial-perspective fetch as include/szg/abi.h states it ("THE FETCH of the fast composite"), in numpy.

Written from the header's text, not from the kernel or the oracle: tests/test_aerial_model.py holds the oracle's
oracle_aerial_sample to `sample32` bit for bit, and tests/test_gpu_fast_composite.py holds the kernel to the oracle.

  sample32  binary32, one numpy operation (= one rounding) per operation of the header
  sample64  the same expressions in float64 on the binary32 inputs: what the rule means without rounding

The volume is the luminance image of szg_skyview_aerial_lut as an array [D * H, W, 4] (slice k = rows [k * H, (k + 1) * H)),
or anything that reshapes to [D, H, W, 4]: froxel (i, j, k) is vol[k, j, i].
"""
import numpy as np

F = np.float32

# The frames that carry the fast composite's tests: fill scene, default camera, sun elevation 35 degrees, and the volume's
# max distances (Mm) that - taken together - put geometry pixels into the ramp, between every pair of slices and behind the
# last slice (tests/test_aerial_model.py proves it on the CPU; tests/test_gpu_fast_composite.py runs exactly these).
COVERAGE_ELEVATION = 35.0
COVERAGE_EXTENTS = ((70, 37), (96, 54))
# (With the last five alone, 20, 28 and 18 pixels of the 70 x 37 frame lie between slices 26 / 27, 27 / 28 and 28 / 29 - fewer
# than the 32 the coverage condition asks for; 2.56e-5 puts the dense 20 - 23 m band of the scene there.)
COVERAGE_MAX_DISTANCES = (2.56e-5, 3.2e-5, 6.4e-5, 1.28e-4, 2.56e-4, 1.2e-3)
COVERAGE_SPOTS = 8
LUT = ((128, 32), (128, 64))


def contraction_mask():
    """The classes of include/szg/contraction.h the oracle under test fuses: SZG_CONTRACT_DEFAULT as the header defines it, or
    none for the literal oracle (SZG_ORACLE_LITERAL=1, oracle/binding.py). Read from the header so that a change of the
    product's rule changes the model with it instead of failing the bit-for-bit test for a reason outside the fetch."""
    import os
    import re

    if os.environ.get("SZG_ORACLE_LITERAL") == "1":
        return set()
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "szg", "contraction.h")
    text = open(header).read()
    default = re.search(r"#define SZG_CONTRACT_DEFAULT \(([^)]*)\)", text).group(1)
    return set(re.findall(r"SZG_C_[A-Z]+", default))


def fuses_texcoord():
    mask = contraction_mask()
    # the weighted sum of the tap is modelled with two roundings per term only: an fma of a weight and a texel is not exact in float64
    assert "SZG_C_BILINEAR" not in mask, "the library now fuses the bilinear sum: teach tests/aerial_model.py that rule"
    return "SZG_C_TEXCOORD" in mask


def volume_view(lum, dims=(32, 32, 32)):
    W, H, D = dims
    return np.asarray(lum).reshape(D, H, W, 4)


def _texel_coordinate(s, n, dtype, fused):
    """u = s * n - 0.5. `fused` (SZG_C_TEXCOORD is part of the library's contraction rule): one rounding. In float64 the
    product of a binary32 number and an extent below 2^24 is exact, so the only rounding left is the sum's; the model insists
    that this sum was exact in float64 too, so that narrowing it to binary32 is the single rounding of an fma."""
    if dtype is F and fused:
        p = s.astype(np.float64) * np.float64(n)
        u = p - 0.5
        assert ((u + 0.5) == p).all(), "the float64 sum is not exact here: this model cannot emulate the fma"
        return u.astype(F)
    return s * dtype(n) - dtype(0.5)


def bilinear(slice_, sx, sy, dtype=F, fused_texcoord=None):
    """The LUT sampler's tap of one slice [H, W, 4] at (sx, sy): LINEAR, CLAMP_TO_EDGE, weights taken before the clamp; the
    weighted sum is w11 t11 + (w01 t01 + (w10 t10 + w00 t00)), each product and sum rounded (SZG_C_BILINEAR is not fused)."""
    H, W = slice_.shape[:2]
    one = dtype(1.0)
    fused_texcoord = fuses_texcoord() if fused_texcoord is None else fused_texcoord
    sx, sy = np.asarray(sx, F).astype(dtype), np.asarray(sy, F).astype(dtype)
    u = _texel_coordinate(sx, W, dtype, fused_texcoord)
    v = _texel_coordinate(sy, H, dtype, fused_texcoord)
    fu, fv = np.floor(u), np.floor(v)
    a, b = (u - fu)[:, None], (v - fv)[:, None]
    i0, j0 = fu.astype(np.int64), fv.astype(np.int64)
    i1, j1 = i0 + 1, j0 + 1
    i0, i1 = np.clip(i0, 0, W - 1), np.clip(i1, 0, W - 1)
    j0, j1 = np.clip(j0, 0, H - 1), np.clip(j1, 0, H - 1)
    rgb = slice_[..., :3].astype(dtype)
    t00, t10, t01, t11 = rgb[j0, i0], rgb[j0, i1], rgb[j1, i0], rgb[j1, i1]
    w00 = (one - a) * (one - b)
    w10 = a * (one - b)
    w01 = (one - a) * b
    w11 = a * b
    return w11 * t11 + (w01 * t01 + (w10 * t10 + w00 * t00))


def slice_coordinate(dist, max_distance, D, dtype=F):
    """(ramp, k0, k1, wz) of the header for distances `dist` (binary32 values)."""
    dist = np.asarray(dist, F).astype(dtype)
    m, depth, half, zero, one = dtype(F(max_distance)), dtype(D), dtype(0.5), dtype(0.0), dtype(1.0)
    fz = dist / m * depth - half
    first_centre = half * m / depth
    # fmax / fmin return the other operand when one is NaN, as the header says of max and min
    ramp = np.where(fz < zero, np.fmax(dist / first_centre, zero), one).astype(dtype)
    z = np.fmin(np.fmax(fz, zero), depth - one)
    k0f = np.floor(z)
    k0 = k0f.astype(np.int64)
    k1 = np.minimum(k0 + 1, D - 1)
    wz = z - k0f
    return ramp, k0, k1, wz


def _sample(lum, max_distance, sx, sy, dist, dims, dtype, fused_texcoord):
    W, H, D = dims
    vol = volume_view(lum, dims)
    sx, sy, dist = (np.asarray(a, F).ravel() for a in (sx, sy, dist))
    out = np.empty((dist.size, 3), dtype)
    with np.errstate(all="ignore"):
        ramp, k0, k1, wz = slice_coordinate(dist, max_distance, D, dtype)
        l0 = np.empty((dist.size, 3), dtype)
        l1 = np.empty((dist.size, 3), dtype)
        for k in range(D):
            for index, tap in ((k0, l0), (k1, l1)):
                pick = index == k
                if pick.any():
                    tap[pick] = bilinear(vol[k], sx[pick], sy[pick], dtype, fused_texcoord)
        one = dtype(1.0)
        wz, ramp = wz[:, None], ramp[:, None]
        out[:] = (l0 * (one - wz) + l1 * wz) * ramp
    return out


def sample32(lum, max_distance, sx, sy, dist, dims=(32, 32, 32), fused_texcoord=None):
    """[n, 3] binary32: the header's fetch, one rounding per operation; the two contraction sites as the oracle's rule has
    them (contraction_mask) unless `fused_texcoord` says otherwise."""
    fused_texcoord = fuses_texcoord() if fused_texcoord is None else fused_texcoord
    return _sample(lum, max_distance, sx, sy, dist, dims, F, fused_texcoord)


def sample64(lum, max_distance, sx, sy, dist, dims=(32, 32, 32)):
    """[n, 3] float64: the same expressions without binary32 rounding."""
    return _sample(lum, max_distance, sx, sy, dist, dims, np.float64, False)


def named_froxels(sx, sy, dist, max_distance, dims=(32, 32, 32)):
    """The indices (i0, i1, j0, j1, k0, k1) of the eight froxels the header names for each point, from this model's own
    slice and texel coordinates (so they check gathers, not the index arithmetic)."""
    W, H, D = dims
    sx, sy = np.asarray(sx, F), np.asarray(sy, F)
    _, k0, k1, _ = slice_coordinate(dist, max_distance, D, F)
    out = []
    for s, n in ((sx, W), (sy, H)):
        lo = np.floor(_texel_coordinate(s, n, F, fuses_texcoord())).astype(np.int64)
        out += [np.clip(lo, 0, n - 1), np.clip(lo + 1, 0, n - 1)]
    return (*out, k0, k1)


# ---------------------------------------------------------------------------
# Geometry of a frame: which part of the fetch each geometry pixel reaches
# ---------------------------------------------------------------------------
def geometry_distances(frame, cam_packed):
    """(mask [h, w] of the pixels the composite treats as geometry, float64 distance camera -> surface in Mm).
    camera.comp:354: depth 0 or an underground position (+y is down) is sky; the flips and the planet-radius offset of
    camera.comp:371-374 do not change a length."""
    position = frame.position[..., :3].astype(np.float64)
    camera = np.array(cam_packed.position[:3], np.float64)
    geometry = (frame.depth != 0.0) & ~(frame.position[..., 1] > 0.0)
    return geometry, np.linalg.norm(position - camera, axis=-1) / 1.0e6


def pixel_directions(cam_packed, W, H):
    """camera.comp:324-328 in float64: the view direction of every pixel in the atmosphere's frame (+y up)."""
    inverse_projection = np.array(list(cam_packed.inverseProjection.m), np.float64).reshape(4, 4).T  # column-major
    rotation = np.array(list(cam_packed.rotation.m), np.float64).reshape(4, 4).T
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    clip = np.stack([(x / W - 0.5) * 2.0, (y / H - 0.5) * 2.0, np.ones_like(x, float), np.ones_like(x, float)], axis=-1)
    rot = clip @ inverse_projection.T @ rotation.T
    d = rot[..., :3] / np.linalg.norm(rot[..., :3], axis=-1, keepdims=True)
    d[..., 1] *= -1.0
    return d
