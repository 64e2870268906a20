"""The rules of include/szg/texture_display.h on the CPU: the numpy model of tests/texture_display_model.py against exact
arithmetic (fractions.Fraction), hand values, the present pass's NEAREST coordinates and, for MAPPING, against the order the rule
excludes. No GPU needed."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import present_model as pm
from tests import texture_display_model as tm
from tests import ui_layer_model as um

F = np.float32


def rne(x, precision, emin):
    """A non-negative Fraction rounded to nearest, ties to even, in a binary format of `precision` significand bits whose
    smallest normal exponent is emin (below it the quantum stays 2^(emin - precision + 1): denormals)."""
    if x == 0:
        return Fraction(0)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, emin) - (precision - 1))
    n = x / quantum
    f = math.floor(n)
    r = n - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return f * quantum


def exact_unorm_to_half(code, scale):
    """Both roundings of LOAD + STORE: the quotient to binary32 first, that value to binary16."""
    return rne(rne(Fraction(code, scale), 24, -126), 11, -14)


def half_value(bits):
    return Fraction(float(np.array([bits], np.uint16).view(np.float16)[0]))


def copy_1to1(codes, fmt):
    """Every code of `codes` in all four channels through the copy model, 1:1: the stored bits [n, 4]."""
    src = np.repeat(np.asarray(codes)[None, :, None], 4, axis=2).astype(np.uint8 if fmt in (tm.RGBA8_UNORM, tm.RGBA8_SRGB) else np.uint16)
    n = src.shape[1]
    out = tm.copy_image(src, fmt, (0, 0, n, 1), np.zeros((1, n, 4), np.uint16), (0, 0, n, 1))
    return out[0]


def test_every_rgba8_unorm_code_against_exact_arithmetic():
    got = copy_1to1(np.arange(256), tm.RGBA8_UNORM)
    for code in range(256):
        want = exact_unorm_to_half(code, 255)
        assert all(half_value(b) == want for b in got[code]), (code, got[code], want)
    # the two roundings are not one: some code's quotient rounds differently when rounded to binary16 at once
    single = [rne(Fraction(c, 255), 11, -14) for c in range(256)]
    assert single[255] == 1 and got[255].tolist() == [0x3C00] * 4


def test_unorm16_codes_against_exact_arithmetic():
    codes = [0, 1, 32767, 32768, 65534, 65535]
    got = copy_1to1(codes, tm.RGBA16_UNORM)
    for k, code in enumerate(codes):
        want = exact_unorm_to_half(code, 65535)
        assert all(half_value(b) == want for b in got[k]), (code, got[k], want)
    assert got[0].tolist() == [0] * 4 and got[5].tolist() == [0x3C00] * 4
    # 1 / 65535 = 256.004 * 2^-24 lies in binary16's denormal range, whose quantum is 2^-24: it becomes the denormal 2^-16
    assert got[1].tolist() == [0x0100] * 4 and half_value(0x0100) == Fraction(1, 2 ** 16) == exact_unorm_to_half(1, 65535)
    # 32767 / 65535 and 32768 / 65535 lie either side of 0.5 in binary32 and meet at 0.5 in binary16
    assert got[2].tolist() == got[3].tolist() == [0x3800] * 4


def test_srgb_codes_either_side_of_the_threshold_against_hand_values():
    got = copy_1to1([0, 10, 11, 255], tm.RGBA8_SRGB)
    # 10 / 255 = 0.039216 <= 0.04045: linear segment, 0.039216 / 12.92 = 0.00303527 = 0x1.8dd6c2p-9 -> binary16 0x1A37
    # 11 / 255 = 0.043137 >  0.04045: ((0.043137 + 0.055) / 1.055)^2.4 = 0.00334654 = 0x1.b6a31cp-9 -> binary16 0x1ADB
    # alpha is never decoded: 10 / 255 -> 0x2905, 11 / 255 -> 0x2986
    assert got.tolist() == [[0, 0, 0, 0], [0x1A37, 0x1A37, 0x1A37, 0x2905], [0x1ADB, 0x1ADB, 0x1ADB, 0x2986], [0x3C00] * 4]
    for code, bits in ((10, 0x1A37), (11, 0x1ADB)):
        c = code / 255.0
        linear = c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4
        assert abs(float(half_value(bits)) - linear) <= 2.0 ** -20  # half an ulp of binary16 at 2^-9, and the fp32 error
    assert np.float32(10 / 255) <= np.float32(0.04045) < np.float32(11 / 255)


def test_half_to_half_copies_the_bits():
    bits = np.array([[[0x7C01, 0xFE00, 0x8000, 0x0001], [0x7E55, 0xFC00, 0x7BFF, 0x83FF]]], np.uint16)  # signalling and quiet NaNs
    out = tm.copy_image(bits, tm.RGBA16_SFLOAT, (0, 0, 2, 1), np.zeros((2, 4, 4), np.uint16), (0, 0, 4, 2))
    assert np.array_equal(out, bits[[0, 0]][:, [0, 0, 1, 1]])


@pytest.mark.parametrize("n,s0,sw,extent", [(7, 0, 1, 1), (13, 0, 3, 3), (8, 0, 64, 64), (10, 1, 3, 5), (6, 2, 4, 7), (257, 3, 100, 128),
                                            (5, 0, 5, 5), (1, 4, 9, 16), (4096, 0, 64, 64), (1000, 17, 700, 1337)])
def test_coordinates_are_the_nearest_rule_of_the_present_pass(n, s0, sw, extent):
    mine = tm.axis_nearest(n, s0, sw, extent)
    assert np.array_equal(mine, pm.axis_nearest(n, s0, sw, extent))
    assert mine.min() >= s0 and mine.max() < s0 + sw  # it cannot leave the region
    if n == sw:
        assert np.array_equal(mine, s0 + np.arange(n))  # 1:1


def test_copy_honours_offsets_and_leaves_the_rest():
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, (7, 5, 4), dtype=np.uint8)
    dst = rng.integers(0, 65536, (9, 16, 4), dtype=np.uint16)
    out = tm.copy_image(src, tm.RGBA8_UNORM, (1, 2, 3, 4), dst, (3, 1, 10, 6))
    mask = np.ones(dst.shape[:2], bool)
    mask[1:7, 3:13] = False
    assert np.array_equal(out[mask], dst[mask])
    assert np.array_equal(out[1, 3], tm.store_half(tm.load(src[2, 1], tm.RGBA8_UNORM)))
    assert np.array_equal(out[6, 12], tm.store_half(tm.load(src[5, 3], tm.RGBA8_UNORM)))
    assert np.array_equal(tm.copy_image(src, tm.RGBA8_UNORM, (1, 2, 0, 4), dst, (3, 1, 10, 6)), dst)


def test_clear_texels():
    color = (1.0 / 3.0, -1.0, 2.0, float("nan"))
    half = tm.clear_texel(tm.RGBA16_SFLOAT, color)
    assert half[:3].tolist() == [0x3555, 0xBC00, 0x4000] and (half[3] & 0x7C00) == 0x7C00 and (half[3] & 0x03FF) != 0  # kept
    assert tm.clear_texel(tm.RGBA16_UNORM, color).tolist() == [21845, 0, 65535, 0]  # clamped, NaN -> 0


# ---- MAPPING ----
def one_alpha_view(filt):
    rng = np.random.default_rng(9)
    data = rng.random((4, 4, 4)).astype(np.float16)
    return tm.TextureView(data, filt, um.CLAMP_TO_BORDER, (tm.IDENTITY, tm.IDENTITY, tm.IDENTITY, tm.ONE))


def test_one_minus_alpha_plus_alpha_is_one_for_every_finite_weight():
    """Why the order of MAPPING and the filter cannot be told apart with finite weights: for alpha in [0, 1) the binary32
    (1 - alpha) + alpha is 1 (the error of 1 - alpha is at most 2^-25, and 1 +- 2^-25 rounds to 1, the lower tie to even).
    Checked on every power of two and its neighbours, on a dense sweep, and on random values of every exponent."""
    powers = (F(2.0) ** -np.arange(1, 150, dtype=F)).astype(F)
    around = np.concatenate([powers, np.nextafter(powers, F(0)), np.nextafter(powers, F(1))]).astype(F)
    dense = (np.arange(1 << 22, dtype=np.float64) / (1 << 22)).astype(F)
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 0x3F800000, 1 << 22, dtype=np.uint32).view(F)  # every exponent below 1
    for alpha in (around, dense, bits):
        alpha = alpha[(alpha >= 0) & (alpha < 1)]
        assert (((F(1) - alpha).astype(F) + alpha).astype(F) == F(1)).all()


def test_mapping_follows_the_filter():
    """ONE on alpha under LINEAR is exactly 1.0 at every coordinate of the sweep. Mapping the taps first is not: the sweep
    contains u = +inf, -inf and NaN (and 1e38, whose product with the width overflows), where alpha = x - floor(x) is NaN and
    the mapped taps give 1 * NaN + 1 * NaN. By the test above those are the only such alphas: at every finite coordinate
    both orders give 1."""
    tex = one_alpha_view(um.LINEAR)
    finite = np.linspace(-0.5, 1.5, 4001).astype(F)
    nonfinite = np.array([np.inf, -np.inf, np.nan, 1e38], F)
    u = np.concatenate([finite, nonfinite])
    v = np.full(u.shape, 0.37, F)
    for uu, vv in ((u, v), (v, u)):
        after = tm.sample(tex, uu, vv)
        assert (after[:, 3] == F(1)).all()
        before = tm.sample_mapping_the_taps(tex, uu, vv)
        assert (before[:len(finite), 3] == F(1)).all()
        assert np.isnan(before[len(finite):, 3]).all()  # alpha = NaN
        finite_rows = np.isfinite(after[:, :3]).all(axis=1)
        assert np.array_equal(after[finite_rows, :3], before[finite_rows, :3])  # IDENTITY channels do not care
    # ZERO likewise: 0 after the filter, NaN before it
    zero = tex._replace(swizzle=(tm.ZERO,) * 4)
    assert (tm.sample(zero, nonfinite, nonfinite) == 0).all() and np.isnan(tm.sample_mapping_the_taps(zero, nonfinite, nonfinite)).all()


def test_mapping_selects_channels_and_border_taps_are_filtered():
    data = np.array([[[0.25, 0.5, 0.75, 0.125]]], np.float16)
    for slot in range(4):
        for s in range(7):
            sw = [tm.IDENTITY] * 4
            sw[slot] = s
            tex = tm.TextureView(data, um.NEAREST, um.CLAMP_TO_EDGE, tuple(sw))
            got = tm.sample(tex, np.array([0.5], F), np.array([0.5], F))[0]
            want = [0.25, 0.5, 0.75, 0.125]
            want[slot] = [want[slot], 0.0, 1.0, 0.25, 0.5, 0.75, 0.125][s]
            assert got.tolist() == want
    # a LINEAR tap half inside: the border (0, 0, 0, 1) is filtered, then R <- A reads the filtered alpha
    tex = tm.TextureView(data, um.LINEAR, um.CLAMP_TO_BORDER, (tm.A, tm.IDENTITY, tm.IDENTITY, tm.IDENTITY))
    got = tm.sample(tex, np.array([0.0], F), np.array([0.5], F))[0]  # x = -0.5: taps -1 (border) and 0 at weight 0.5
    assert got.tolist() == [0.5 * 1.0 + 0.5 * 0.125, 0.25, 0.375, 0.5625]


def test_half_textures_convert_exactly():
    bits = np.array([0x0000, 0x8000, 0x0001, 0x0400, 0x3800, 0x3C00, 0x7BFF, 0x7C00, 0xFC00, 0x7E00, 0xBC00, 0x83FF], np.uint16)
    data = np.zeros((3, 4, 4), np.uint16)
    data[..., 0] = bits.reshape(3, 4)
    tex = tm.TextureView(data.view(np.float16), um.NEAREST, um.CLAMP_TO_EDGE, tm.IDENTITY_VIEW)
    u = ((np.arange(12) % 4 + 0.5) / 4).astype(F)
    v = ((np.arange(12) // 4 + 0.5) / 3).astype(F)
    got = tm.sample(tex, u, v)[:, 0]
    want = [0.0, -0.0, 2.0 ** -24, 2.0 ** -14, 0.5, 1.0, 65504.0, np.inf, -np.inf, np.nan, -1.0, -(1023 / 1024) * 2.0 ** -14]
    assert np.array_equal(got.view(np.uint32), np.array(want, F).view(np.uint32))


def test_unorm_views_sample_as_plain_textures():
    rng = np.random.default_rng(6)
    u, v = rng.random(500, dtype=F) * F(1.5) - F(0.25), rng.random(500, dtype=F) * F(1.5) - F(0.25)
    for dtype in (np.uint8, np.uint16):
        data = rng.integers(0, np.iinfo(dtype).max + 1, (5, 7, 4)).astype(dtype)
        for filt in (um.NEAREST, um.LINEAR):
            for address in (um.REPEAT, um.CLAMP_TO_EDGE, um.CLAMP_TO_BORDER):
                plain = um.sample(um.Texture(data, filt, address), u, v)
                assert np.array_equal(tm.sample(tm.TextureView(data, filt, address, tm.IDENTITY_VIEW), u, v), plain)
                assert np.array_equal(tm.sample(um.Texture(data, filt, address), u, v), plain)
