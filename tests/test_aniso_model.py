"""include/szg/anisotropy.h on the CPU: the numpy binary32 model of tests/aniso_model.py against values derived by hand and
against a float64 evaluation of the header's rule written here from scratch, and everything about the new entry point that
needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from syzygy_amd import abi, lib, library_path
from tests import aniso_model as am
from tests import mipmap_model as mm
from tests.test_gpu_mipmaps import _samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SIZES = [(4, 4), (5, 3), (16, 8), (64, 64)]


def _random_chain(w, h, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (hk, wk, 4), dtype=np.uint8) for wk, hk in mm.level_shapes(w, h)]


def _same_bits(a, b):
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


# ---------------------------------------------------------------------------
# off, isotropic and degenerate footprints: today's value bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_anisotropy_1_and_every_single_tap_sample_equal_the_trilinear_model(size, srgb):
    w, h = size
    levels = _random_chain(w, h, w * 31 + h)
    st, ddx, ddy = _samples(w, h, w + h)  # NaN, inf, zero and denormal derivatives in its first rows
    for max_lod in (mm.MAX_LOD_REFERENCE, mm.MAX_LOD_NONE):
        want = mm.sample(levels, srgb, st, ddx, ddy, max_lod)
        assert _same_bits(am.sample(levels, srgb, st, ddx, ddy, max_lod, 1.0), want)
        for A in (2.0, 3.5, 16.0):
            got, detail = am.sample(levels, srgb, st, ddx, ddy, max_lod, A, return_detail=True)
            one = detail["N"] == 1
            assert one.any() and (~one).any()
            assert _same_bits(got[one], want[one])
            assert detail["N"].min() >= 1 and detail["N"].max() == int(np.ceil(A))
            assert (detail["eta"] >= 1).all() and (detail["eta"] <= F(A)).all()


def test_degenerate_footprints_take_one_tap():
    w, h = 16, 8
    nan, inf = np.nan, np.inf
    cases = [((0, 0), (0, 0)), ((nan, 0), (0, 0)), ((nan, nan), (nan, nan)), ((inf, 0), (0, 0)), ((inf, -inf), (inf, inf)),
             ((0.25, 0), (nan, 0)), ((1e30, 1e30), (0, 0)), ((3e38, 0), (0, 3e38)), ((0.125, 0), (0, 0.125)), ((0, 0.5), (0.5, 0))]
    ddx = np.array([c[0] for c in cases], F)
    ddy = np.array([c[1] for c in cases], F)
    N, eta = am.tap_count(w, h, ddx, ddy, 16.0)
    # (0.125, 0) x (0, 0.125) on 16 x 8 is 2 x 1 texels: eta 2; (0, 0.5) x (0.5, 0) is 4 x 8 texels: eta 2
    assert N.tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 2, 2], N
    # a zero minor axis and a denormal one clamp at A instead
    N, eta = am.tap_count(w, h, np.array([[0.5, 0], [0.5, 0]], F), np.array([[0, 0], [0, 1e-42]], F), 16.0)
    assert N.tolist() == [16, 16] and (eta == F(16.0)).all()
    N, _ = am.tap_count(w, h, np.array([[0.5, 0]], F), np.zeros((1, 2), F), 3.5)
    assert N.tolist() == [4]


# ---------------------------------------------------------------------------
# what it is for, by hand
# ---------------------------------------------------------------------------
def test_stripes_under_a_long_footprint_come_back():
    """64 x 64 UNORM, constant along u, rows in stripes of two. Level 1 has stripes of one row (each 2 x 2 block lies in one
    stripe), levels >= 2 are (0 + 0 + 255 + 255 + 2) >> 2 = 128 everywhere. Footprint 8 texels along u, 1 along v: trilinear
    reads level log2(8) = 3, grey. With A = 16: eta = 8, N = 8, lambda = 3 - 3 = 0: level 0 at its row centres, the stripe
    itself. With A = 4: lambda = 3 - 2 = 1, level 1, whose rows are half a row off the level-0 centres: 3/4 of the own stripe
    and 1/4 of the other one. With A = 2: lambda = 2, grey again."""
    rows = np.arange(64)
    code = np.where((rows // 2) % 2 == 1, 255, 0).astype(np.uint8)
    level0 = np.zeros((64, 64, 4), np.uint8)
    level0[...] = code[:, None, None]
    levels = mm.build_chain(level0, False)
    assert (levels[1][:, :, 0] == np.where(np.arange(32) % 2 == 1, 255, 0)[:, None]).all()
    assert all((lv == 128).all() for lv in levels[2:])
    st = np.stack([np.full(64, 0.3), (rows + 0.5) / 64.0], 1).astype(F)
    ddx = np.tile(np.array([8.0 / 64.0, 0.0], F), (64, 1))
    ddy = np.tile(np.array([0.0, 1.0 / 64.0], F), (64, 1))
    stripe = (code / 255.0)[:, None]
    grey = F(128.0) / F(255.0)

    trilinear = mm.sample(levels, False, st, ddx, ddy, mm.MAX_LOD_NONE)
    assert np.abs(trilinear - grey).max() <= 2.0**-22  # (four weights that sum to one up to their roundings)
    got, detail = am.sample(levels, False, st, ddx, ddy, mm.MAX_LOD_NONE, 16.0, return_detail=True)
    assert (detail["N"] == 8).all() and (detail["eta"] == F(8.0)).all()
    # a lambda that misses 0 by an ulp of szg_logf blends at most that much of level 1
    assert np.abs(detail["lam"]).max() <= 1e-6
    assert np.abs(got - stripe).max() <= 1e-5
    got, detail = am.sample(levels, False, st, ddx, ddy, mm.MAX_LOD_NONE, 4.0, return_detail=True)
    assert (detail["N"] == 4).all() and np.abs(detail["lam"] - 1.0).max() <= 1e-6
    assert np.abs(got - (0.25 + 0.5 * stripe)).max() <= 1e-5
    got, detail = am.sample(levels, False, st, ddx, ddy, mm.MAX_LOD_NONE, 2.0, return_detail=True)
    assert (detail["N"] == 2).all() and np.abs(detail["lam"] - 2.0).max() <= 1e-6
    assert np.abs(got - grey).max() <= 1e-5


# ---------------------------------------------------------------------------
# an independent float64 evaluation of the header's rule
# ---------------------------------------------------------------------------
def _decode64(level, srgb):
    c = level[..., :3].astype(np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4) if srgb else c


def _bilinear64(texels, u, v):
    """texels [h, w, 3] float64, (u, v) in [0, 1) REPEAT coordinates, float64."""
    h, w = texels.shape[:2]
    x, y = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    a, b = (x - x0)[:, None], (y - y0)[:, None]
    i0, j0 = x0.astype(np.int64) % w, y0.astype(np.int64) % h
    i1, j1 = (i0 + 1) % w, (j0 + 1) % h
    return (1 - a) * (1 - b) * texels[j0, i0] + a * (1 - b) * texels[j0, i1] + (1 - a) * b * texels[j1, i0] + a * b * texels[j1, i1]


def _rule64(levels, srgb, st, ddx, ddy, max_lod, A):
    """The header's SAMPLER in float64 on finite, non-degenerate footprints. Returns value [n, 3], the unclamped ratio, N and
    which axis is the major one."""
    h, w = levels[0].shape[:2]
    L = len(levels)
    texels = [_decode64(lv, srgb) for lv in levels]
    st, ddx, ddy = st.astype(np.float64), ddx.astype(np.float64), ddy.astype(np.float64)
    px = np.hypot(ddx[:, 0] * w, ddx[:, 1] * h)
    py = np.hypot(ddy[:, 0] * w, ddy[:, 1] * h)
    longer, shorter = np.maximum(px, py), np.minimum(px, py)
    ratio = longer / shorter
    eta = np.minimum(ratio, A)
    N = np.ceil(eta).astype(np.int64)
    lam = np.clip(np.log2(longer) - np.where(N > 1, np.log2(eta), 0.0), 0.0, min(max_lod, L - 1.0))
    d = np.minimum(np.floor(lam).astype(np.int64), L - 1)
    f = lam - d
    x_major = px >= py
    major = np.where(x_major[:, None], ddx, ddy)
    out = np.zeros((len(st), 3))
    for i in range(1, int(N.max()) + 1):
        live = N >= i
        t = np.where(N > 1, i / (N + 1.0) - 0.5, 0.0)[live]
        at = st[live] + t[:, None] * major[live]
        tap = np.zeros((live.sum(), 3))
        for k in range(L):
            lo = d[live] == k
            if lo.any():
                tap[lo] = _bilinear64(texels[k], at[lo, 0], at[lo, 1])
                if k + 1 < L:
                    fk = f[live][lo][:, None]
                    tap[lo] = (1 - fk) * tap[lo] + fk * _bilinear64(texels[k + 1], at[lo, 0], at[lo, 1])
        out[live] += tap
    return out / N[:, None], ratio, N, x_major


def _footprints(w, h, n, seed):
    """Major axis log-uniform over 2^-6 .. 2^4 texels in a random direction, the ratio log-uniform over 1 .. 64, the minor axis
    in a random direction of its own, the two handed to x and y at random."""
    rng = np.random.default_rng(seed)
    st = rng.uniform(-3.0, 3.0, (n, 2)).astype(F)
    longer = 2.0 ** rng.uniform(-6.0, 4.0, n)
    ratio = 2.0 ** rng.uniform(0.0, 6.0, n)
    angle_major, angle_minor = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(0.0, 2.0 * np.pi, n)
    size = np.array([w, h], np.float64)
    major = (longer[:, None] * np.stack([np.cos(angle_major), np.sin(angle_major)], 1) / size).astype(F)
    minor = ((longer / ratio)[:, None] * np.stack([np.cos(angle_minor), np.sin(angle_minor)], 1) / size).astype(F)
    to_x = rng.random(n) < 0.5
    return st, np.where(to_x[:, None], major, minor), np.where(to_x[:, None], minor, major)


@pytest.mark.parametrize("case", [(16.0, mm.MAX_LOD_NONE, False), (16.0, mm.MAX_LOD_NONE, True), (3.5, mm.MAX_LOD_NONE, False),
                                  (16.0, mm.MAX_LOD_REFERENCE, False)], ids=str)
@pytest.mark.parametrize("size", SIZES)
def test_model_agrees_with_a_float64_evaluation_of_the_rule(size, case):
    A, max_lod, srgb = case
    w, h = size
    n = 4096
    levels = _random_chain(w, h, w * 17 + h)
    st, ddx, ddy = _footprints(w, h, n, w * 5 + h + int(A))
    want, ratio, N64, x_major = _rule64(levels, srgb, st, ddx, ddy, max_lod, A)
    got, detail = am.sample(levels, srgb, st, ddx, ddy, max_lod, A, return_detail=True)
    # where the unclamped ratio is within 2^-16 (relative) of an integer <= A the two may count their taps differently
    nearest = np.rint(ratio)
    unsure = (np.abs(ratio - nearest) <= 2.0**-16 * nearest) & (nearest <= A)
    share = unsure.mean()
    assert share <= 0.02, share
    keep = ~unsure
    assert np.array_equal(detail["N"][keep], N64[keep])
    # tolerance, from the numbers of this case (as tests/test_gpu_raster_mipmaps.py derives its own):
    #   a tap's position: st + t * major, times the size, minus 0.5 is four binary32 roundings of values up to
    #   S = (|st| + |major| / 2) * size texels, 2^-24 S each; a bilinear value moves by at most one (the largest difference of
    #   two texels) per texel of displacement along each of the two axes
    reach = np.abs(st).max(axis=1) + 0.5 * np.maximum(np.abs(ddx).max(axis=1), np.abs(ddy).max(axis=1))
    S = float(reach.max()) * max(w, h)
    position = 2.0 * 4.0 * 2.0**-24 * S
    #   lambda: |log2 r2| <= 12 + ..., so every term is below 16, where half an ulp is 2^-21. szg_logf twice (a few ulp each:
    #   take 4), the two products by log2(e), the subtraction, and the relative error 4 * 2^-24 of r2 and of the ratio under
    #   the logarithm: 12 * 2^-20 in all. A value moves by at most one per level of lambda (two levels differ by at most one)
    lam_error = 12.0 * 2.0**-20
    #   the arithmetic: 8 roundings in the bilinear sum, 4 in the blend, 15 in a sum of 16 taps of which each is at most
    #   2^-24 N relative to the mean, 8 for the sRGB decode (szg_powf against pow)
    arithmetic = (8 + 4 + 15 + 1 + 8) * 2.0**-24
    tolerance = position + lam_error + arithmetic
    err = np.abs(got.astype(np.float64) - want)[keep]
    spread = (detail["N"] >= 2) & (ratio < A) & keep
    print(f"{w}x{h} A {A} max_lod {max_lod} srgb {srgb}: left out {unsure.sum()} of {n}; unclamped with N >= 2: {spread.mean():.3f}; "
          f"x-major {x_major.mean():.3f}; S {S:.1f} texels: position {position:.3e} + lambda {lam_error:.3e} + arithmetic {arithmetic:.3e} "
          f"= tolerance {tolerance:.3e}; max error {err.max():.3e}")
    assert err.max() <= tolerance
    assert 0.3 < x_major.mean() < 0.7  # both major axes occur
    if A == 16.0:
        assert spread.mean() >= 1.0 / 3.0
    assert (detail["N"][keep] == int(np.ceil(A))).any()  # and some are clamped


# ---------------------------------------------------------------------------
# the C ABI, without a device
# ---------------------------------------------------------------------------
def header(name):
    return open(os.path.join(ROOT, "include", "szg", name)).read()


def test_the_symbol_of_anisotropy_h_is_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header("anisotropy.h"), flags=re.S)
    names = sorted(set(re.findall(r"\b(szg_[a-z0-9_]+)\s*\(", text)))
    assert names == ["szg_deferred_set_sampler_anisotropy"]
    assert hasattr(C.CDLL(library_path()), names[0])
    assert sorted(abi.ANISOTROPY_FUNCTIONS) == names
    assert abi.ANISOTROPY_FUNCTIONS[names[0]] == (C.c_int, [C.c_void_p, C.c_float])
    fn = lib().szg_deferred_set_sampler_anisotropy
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, C.c_float]
    rows = [row for row in abi.BINDINGS if row[0] == "anisotropy.h"]
    assert rows == [("anisotropy.h", abi.ANISOTROPY_FUNCTIONS, "anisotropic filtering is unavailable with it")]


def test_constants_match_the_header_and_the_abi_version_stays():
    text = header("anisotropy.h")
    assert re.search(r"#define SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE 1\.0f\b", text) and abi.SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE == 1.0
    assert re.search(r"#define SZG_SAMPLER_MAX_ANISOTROPY_LIMIT 16\.0f\b", text) and abi.SZG_SAMPLER_MAX_ANISOTROPY_LIMIT == 16.0
    assert am.MAX_ANISOTROPY_REFERENCE == 1.0 and am.MAX_ANISOTROPY_LIMIT == 16.0
    assert "vulkanstructs.cpp:171-172" in text
    assert "keeps the one-level rule" in text  # a map without a chain, said in the header
    # a new pipeline starts from the reference's value
    common = open(os.path.join(ROOT, "syzygy_amd", "csrc", "api_common.hpp")).read()
    assert re.search(r"float textureMaxAnisotropy = SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE;", common)
    # additive: the version and the structs of raster.h / mipmaps.h stay as they were
    assert abi.SZG_ABI_VERSION == 2 and lib().szg_abi_version() == 2
    assert (C.sizeof(abi.Texture), C.sizeof(abi.Material), C.sizeof(abi.Surface), C.sizeof(abi.MeshInstanced)) == (24, 72, 80, 64)
    assert C.sizeof(abi.TextureMips) == 24
    launch = open(os.path.join(ROOT, "syzygy_amd", "csrc", "szg_launch.hpp")).read()
    assert "static_assert(sizeof(RasterDraw) == 256" in launch


REFUSALS = {"nan": (float("nan"), b"NaN"), "zero": (0.0, b"outside 1..16"), "below one": (0.999, b"outside 1..16"),
            "negative": (-4.0, b"outside 1..16"), "above the limit": (16.5, b"outside 1..16"), "infinite": (float("inf"), b"outside 1..16"),
            "null pipeline": (4.0, b"NULL pipeline"), "null pipeline at 1": (1.0, b"NULL pipeline")}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_set_sampler_anisotropy_refuses(name):
    """No device: the pipeline handle is NULL, and the value is judged before it, each refusal with its own text."""
    value, text = REFUSALS[name]
    assert lib().szg_deferred_set_sampler_anisotropy(None, value) == abi.SZG_ERR_INVALID_ARGUMENT
    message = lib().szg_last_error()
    assert b"szg_deferred_set_sampler_anisotropy" in message and text in message, message


def test_the_examples_anisotropy_switch():
    from syzygy_amd import pipelines

    assert pipelines.parse_anisotropy_option("1") == 1.0 and pipelines.parse_anisotropy_option("16") == 16.0
    assert pipelines.parse_anisotropy_option("3.5") == 3.5
    for bad in ("0", "0.5", "17", "nan", "inf", "many", ""):
        with pytest.raises(ValueError):
            pipelines.parse_anisotropy_option(bad)
    for example in ("render_gltf.py", "frame_loop.py"):
        assert '"--anisotropy"' in open(os.path.join(ROOT, "examples", example)).read()
