"""The present pass's rule (include/szg/present.h) on the CPU: the numpy model of tests/present_model.py against a binary64
evaluation of the same formulas, against exact integer arithmetic on every 16-bit code, and against properties that do not
go through the model's own arithmetic; plus the header / ABI checks that need no device."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import present_model as pm
from tests.texture_display_cases import image as fake_image
from syzygy_amd import abi, lib, library_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source extent, source region as (x0, y0, x1, y1) or None for the whole image, destination extent)
SCALED_CASES = [
    ((640, 360), None, (1280, 720)),
    ((1280, 720), None, (640, 360)),
    ((1000, 700), None, (1337, 911)),
    ((1920, 1080), None, (1280, 720)),
    ((3840, 2160), None, (2560, 1440)),
    ((1280, 720), (17, 9, 1111, 701), (1919, 1079)),
    ((800, 600), (3, 5, 797, 599), (3840, 2160)),
]


def region_of(extent, corners):
    if corners is None:
        return (0, 0, extent[0], extent[1])
    x0, y0, x1, y1 = corners
    return (x0, y0, x1 - x0, y1 - y0)


def noise(width, height, seed=1):
    return np.random.default_rng(seed).integers(0, 65536, (height, width, 4), dtype=np.uint16)


@pytest.mark.parametrize("fmt", [pm.RGBA8, pm.A2B10G10R10], ids=["8bit", "10bit"])
@pytest.mark.parametrize("case", SCALED_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}{'r' if c[1] else ''}-{c[2][0]}x{c[2][1]}")
def test_binary32_rule_against_binary64(case, fmt):
    """On uniform 16-bit noise (seed 1) the binary32 rule is never more than 1 output code from the binary64 evaluation
    with exact rational coordinates, and differs in at most 1e-3 of the channels. The cap is a condition; the worst share
    measured when this test was written was 1.8e-4 (1280x720 -> 640x360, 8 bit)."""
    (W, H), corners, (dw, dh) = case
    src = noise(W, H)
    region = region_of((W, H), corners)
    got = pm.filtered_codes(src, region, dw, dh, fmt)
    want = pm.filtered_codes(src, region, dw, dh, fmt, dtype=np.float64)
    d = np.abs(got - want)
    share = float((d > 0).mean())
    print(f"{W}x{H} {region} -> {dw}x{dh} fmt {fmt}: max {d.max()} code, share {share:.2e}")
    assert d.max() <= 1
    assert share <= 1e-3


def all_codes_image():
    codes = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    return np.repeat(codes[..., None], 4, axis=2)


def exactly_rounded(bits):
    """round(code * (2^b - 1) / 65535) in integers. No ties exist: 2 * code * (2^b - 1) is even, an odd multiple of 65535
    is odd."""
    c = np.arange(65536, dtype=np.int64)
    m = (1 << bits) - 1
    return (2 * c * m + 65535) // (2 * 65535)


def test_one_to_one_8bit_is_exactly_rounded_for_every_code():
    got = pm.filtered_codes(all_codes_image(), (0, 0, 256, 256), 256, 256, pm.RGBA8)
    for c in range(4):
        assert np.array_equal(got[..., c].reshape(-1), exactly_rounded(8))


def test_one_to_one_10bit_is_within_one_code_of_exact_rounding():
    """float(code) / 65535.0f is rounded before the product with 1023, so a quotient just above a half can land on it. With
    the rule as stated exactly ONE code does: 19763 * 1023 / 65535 = 308.50002, stored as 308 (the tie goes to even)."""
    got = pm.filtered_codes(all_codes_image(), (0, 0, 256, 256), 256, 256, pm.A2B10G10R10)
    want = exactly_rounded(10)
    for c in range(3):
        d = got[..., c].reshape(-1) - want
        assert np.abs(d).max() <= 1
        assert np.nonzero(d)[0].tolist() == [19763] and d[19763] == -1
    assert np.array_equal(got[..., 3].reshape(-1), exactly_rounded(2))  # the 2-bit alpha


def test_one_to_one_equals_the_general_rule_with_any_filter_and_offset():
    src = noise(40, 30)
    for fmt in pm.FORMATS:
        a = pm.filtered_codes(src, (5, 3, 20, 10), 20, 10, fmt, pm.LINEAR)
        b = pm.filtered_codes(src, (5, 3, 20, 10), 20, 10, fmt, pm.NEAREST)
        t = src[3:13, 5:25].astype(np.float32) / np.float32(65535.0)
        direct = np.stack([pm.store(t[..., c], pm.channel_bits(fmt)[c]) for c in range(4)], axis=-1)
        assert np.array_equal(a, b) and np.array_equal(a, direct)


def rn32(x):
    """A Fraction correctly rounded to binary32 (ties to even)."""
    f = np.float32(float(x))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(np.float32(c).view(np.uint32)) & 1))


def test_kernel_division_shortcut_is_exact_for_every_code():
    """kernels_present.hip computes float(code) / 65535.0f as q0 = code * y, r = fma(-65535, q0, code), q = fma(r, y, q0) with
    y = RN(1 / 65535) = 0x1.0001p-16. In exact arithmetic, rounded once per operation: equal to the correctly rounded
    quotient (what `/` gives) for all 65 536 codes."""
    y = rn32(Fraction(1, 65535))
    assert float(y) == float.fromhex("0x1.0001p-16")
    fy = Fraction(float(y))
    for code in range(65536):
        q0 = Fraction(float(rn32(code * fy)))
        r = Fraction(float(rn32(code - 65535 * q0)))
        q = rn32(q0 + r * fy)
        assert q == np.float32(code) / np.float32(65535.0), code


# ---- properties that do not go through the model's arithmetic ----------------------------------------------------------
@pytest.mark.parametrize("filter", [pm.LINEAR, pm.NEAREST])
def test_a_constant_image_stays_constant_at_any_scale(filter):
    for code in (0, 1, 257, 12345, 32768, 65534, 65535):
        src = np.full((9, 13, 4), code, np.uint16)
        for dw, dh in ((1, 1), (13, 9), (26, 18), (5, 4), (97, 61), (13, 40)):
            for fmt in (pm.RGBA8, pm.A2B10G10R10):
                got = pm.filtered_codes(src, (0, 0, 13, 9), dw, dh, fmt, filter)
                for c, bits in enumerate(pm.channel_bits(fmt)):
                    t = np.float32(code) / np.float32(65535.0)
                    assert (got[..., c] == int(np.rint(t * np.float32((1 << bits) - 1)))).all(), (code, dw, dh, fmt)


def test_exact_2x_magnification_has_weights_one_and_three_quarters():
    """Source codes 1028 q (= 4 q in 8 bits, exactly): destination column 2m is (q[m-1] + 3 q[m]) / 4 * 4 = q[m-1] + 3 q[m],
    column 2m + 1 is 3 q[m] + q[m+1]; the two border columns replicate the border texel (both taps clamp to it)."""
    rng = np.random.default_rng(7)
    W, H = 31, 5
    q = rng.integers(0, 64, (H, W), dtype=np.int64)
    src = np.repeat((q * 1028).astype(np.uint16)[..., None], 4, axis=2)
    got = pm.filtered_codes(src, (0, 0, W, H), 2 * W, H, pm.RGBA8)[..., 0]  # x only: rows map 1:1
    m = np.arange(1, W)
    assert np.array_equal(got[:, 2 * m], q[:, m - 1] + 3 * q[:, m])
    m = np.arange(0, W - 1)
    assert np.array_equal(got[:, 2 * m + 1], 3 * q[:, m] + q[:, m + 1])
    assert np.array_equal(got[:, 0], 4 * q[:, 0]) and np.array_equal(got[:, 2 * W - 1], 4 * q[:, W - 1])
    i0, i1, alpha = pm.axis_linear(2 * W, 0, W, W)
    assert set(alpha[1:-1].tolist()) == {0.25, 0.75} and i0[0] == 0 and i1[-1] == W - 1


def test_nearest_picks_the_documented_texel_at_integer_ratios():
    src = noise(24, 12, seed=3)
    store8 = lambda a: pm.store(a.astype(np.float32) / np.float32(65535.0), 8)  # noqa: E731
    up = pm.filtered_codes(src, (0, 0, 24, 12), 48, 24, pm.RGBA8, pm.NEAREST)
    assert np.array_equal(up, store8(src[np.arange(24) // 2][:, np.arange(48) // 2]))  # floor((2k + 1) / 4) = k // 2
    down2 = pm.filtered_codes(src, (0, 0, 24, 12), 12, 6, pm.RGBA8, pm.NEAREST)
    assert np.array_equal(down2, store8(src[1::2, 1::2]))  # floor((2k + 1) * 2 / 2) = 2k + 1
    down3 = pm.filtered_codes(src, (3, 0, 18, 12), 6, 4, pm.RGBA8, pm.NEAREST)
    assert np.array_equal(down3, store8(src[1::3][:, 3 + 1:3 + 18:3]))  # s0 + floor((2k + 1) * 3 / 2) = s0 + 3k + 1


def test_subregion_edges_read_the_texel_next_to_the_region_and_nothing_further():
    """Taps clamp to the IMAGE (Vulkan's blit rule), so a magnified subregion's edge texels blend with the texel just outside
    the region; texels two or more away never matter."""
    src = noise(16, 16, seed=5)
    region = (4, 4, 8, 8)
    base = pm.filtered_codes(src, region, 16, 16, pm.A2B10G10R10)
    near = src.copy()
    near[:, 3] ^= 0x8000  # the column just left of the region
    got = pm.filtered_codes(near, region, 16, 16, pm.A2B10G10R10)
    assert (got[:, 0] != base[:, 0]).any() and np.array_equal(got[:, 1:], base[:, 1:])
    near = src.copy()
    near[12] ^= 0x8000  # the row just below the region
    got = pm.filtered_codes(near, region, 16, 16, pm.A2B10G10R10)
    assert (got[15] != base[15]).any() and np.array_equal(got[:15], base[:15])
    far = src.copy()
    far[:, :3] ^= 0x8000
    far[:, 13:] ^= 0x8000
    far[:3] ^= 0x8000
    far[13:] ^= 0x8000
    assert np.array_equal(pm.filtered_codes(far, region, 16, 16, pm.A2B10G10R10), base)
    # a region that touches the image border clamps to the border texel instead
    edge = pm.filtered_codes(src, (0, 0, 8, 8), 16, 16, pm.RGBA8)
    t = src[0, 0].astype(np.float32) / np.float32(65535.0)
    assert np.array_equal(edge[0, 0], pm.store(t, 8))


def test_bgra8_is_rgba8_with_bytes_0_and_2_swapped():
    src = noise(33, 17, seed=9)
    a = pm.present(src, (0, 0, 33, 17), pm.empty_destination(50, 20, pm.RGBA8), (0, 0, 50, 20), pm.RGBA8)
    b = pm.present(src, (0, 0, 33, 17), pm.empty_destination(50, 20, pm.BGRA8), (0, 0, 50, 20), pm.BGRA8)
    assert np.array_equal(a[..., [2, 1, 0, 3]], b) and not np.array_equal(a, b)


def test_a2b10g10r10_bit_layout():
    for channel, word in ((0, 0x3FF), (1, 0x3FF << 10), (2, 0x3FF << 20), (3, 0x3 << 30)):
        src = np.zeros((2, 2, 4), np.uint16)
        src[..., channel] = 65535
        out = pm.present(src, (0, 0, 2, 2), pm.empty_destination(2, 2, pm.A2B10G10R10), (0, 0, 2, 2), pm.A2B10G10R10)
        assert out.dtype == np.uint32 and (out == word).all()


def test_everything_outside_the_destination_region_keeps_its_value():
    src = noise(8, 8)
    dst = pm.empty_destination(20, 10, pm.RGBA8, fill=0xAB)
    out = pm.present(src, (0, 0, 8, 8), dst, (3, 2, 11, 5), pm.RGBA8)
    mask = np.ones((10, 20), bool)
    mask[2:7, 3:14] = False
    assert (out[mask] == 0xAB).all()
    assert np.array_equal(pm.present(src, (0, 0, 0, 8), dst, (3, 2, 11, 5), pm.RGBA8), dst)  # nothing to sample: no-op


# ---- header / ABI --------------------------------------------------------------------------------------------------------
def header(name):
    return open(os.path.join(ROOT, "include", "szg", name)).read()


def test_every_symbol_of_present_h_is_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header("present.h"), flags=re.S)
    names = sorted(set(re.findall(r"\b(szg_[a-z0-9_]+)\s*\(", text)))
    assert names == ["szg_record_present"]
    handle = C.CDLL(library_path())
    for name in names:
        assert hasattr(handle, name), f"{name} declared in present.h but not exported"
        assert name in abi.PRESENT_FUNCTIONS, f"{name} declared in present.h but has no ctypes signature"
    assert sorted(abi.PRESENT_FUNCTIONS) == names
    assert lib().szg_record_present.argtypes is not None


def test_new_formats_do_not_renumber_the_old_ones():
    text = re.sub(r"/\*.*?\*/", "", header("abi.h"), flags=re.S)
    values = {k: int(v) for k, v in re.findall(r"\b(SZG_FORMAT_[A-Z0-9_]+)\s*=\s*(\d+)", text)}
    assert values == {"SZG_FORMAT_UNDEFINED": 0, "SZG_FORMAT_RGBA16_SFLOAT": 1, "SZG_FORMAT_RGBA32_SFLOAT": 2,
                      "SZG_FORMAT_RGBA16_UNORM": 3, "SZG_FORMAT_D32_SFLOAT": 4, "SZG_FORMAT_RGBA8_UNORM": 5,
                      "SZG_FORMAT_BGRA8_UNORM": 6, "SZG_FORMAT_A2B10G10R10_UNORM": 7}
    for name, value in values.items():
        assert getattr(abi, name) == value
    assert (pm.RGBA8, pm.BGRA8, pm.A2B10G10R10) == (5, 6, 7)
    for fmt in pm.FORMATS:
        assert abi.TEXEL_BYTES[fmt] == 4


def test_present_constants_and_struct_match_the_header():
    text = header("present.h")
    defines = dict(re.findall(r"#define\s+(SZG_[A-Z_]+)\s+(0x[0-9A-Fa-f]+|\d+)u", text))
    for name in ("SZG_PRESENT_MAX_EXTENT", "SZG_FILTER_NEAREST", "SZG_FILTER_LINEAR", "SZG_PRESENT_ENCODE_NONE"):
        assert int(defines[name], 0) == getattr(abi, name), name
    assert abi.SZG_PRESENT_ENCODE_NONE not in (abi.SZG_OETF_PURE_GAMMA, abi.SZG_OETF_SRGB)
    assert (pm.NEAREST, pm.LINEAR, pm.MAX_EXTENT) == (abi.SZG_FILTER_NEAREST, abi.SZG_FILTER_LINEAR, abi.SZG_PRESENT_MAX_EXTENT)
    assert C.sizeof(abi.PresentInfo) == 40 and abi.PresentInfo.filter.offset == 32 and abi.PresentInfo.encode.offset == 36
    # the present pass is additive (one new symbol, new format values behind the old ones): the ABI version does not move
    assert lib().szg_abi_version() == abi.SZG_ABI_VERSION


def refusal_cases(S=0x10000000, D=0x20000000):
    """(name, src image, dst image, PresentInfo or None) of every refusal of include/szg/present.h, for a 64x32 source at
    address S and a 48x24 destination at address D (tests/test_gpu_present.py passes real device buffers)."""
    R16, R8 = abi.SZG_FORMAT_RGBA16_UNORM, abi.SZG_FORMAT_RGBA8_UNORM
    src, dst = fake_image(64, 32, R16, S), fake_image(48, 24, R8, D)
    LIN, NONE = abi.SZG_FILTER_LINEAR, abi.SZG_PRESENT_ENCODE_NONE

    def info(sr=(0, 0, 64, 32), dr=(0, 0, 48, 24), filter=LIN, encode=NONE):
        return abi.PresentInfo(abi.Rect(*sr), abi.Rect(*dr), filter, encode)

    big = abi.SZG_PRESENT_MAX_EXTENT + 1
    return [
        ("NULL source", None, dst, info()),
        ("NULL destination", src, None, info()),
        ("NULL info", src, dst, None),
        ("NULL source data", fake_image(64, 32, R16, 0), dst, info()),
        ("NULL destination data", src, fake_image(48, 24, R8, 0), info()),
        ("source format", fake_image(64, 32, abi.SZG_FORMAT_RGBA16_SFLOAT, S), dst, info()),
        ("source is an 8-bit format", fake_image(64, 32, R8, S), dst, info()),
        ("destination format", src, fake_image(48, 24, R16, D), info()),
        ("destination format undefined", src, fake_image(48, 24, abi.SZG_FORMAT_UNDEFINED, D), info()),
        ("source region too wide", src, dst, info(sr=(1, 0, 64, 32))),
        ("source region too high", src, dst, info(sr=(0, 1, 64, 32))),
        ("source region negative x", src, dst, info(sr=(-1, 0, 8, 8))),
        ("source region wraps", src, dst, info(sr=(1, 0, 0xFFFFFFFF, 8))),
        ("destination region too wide", src, dst, info(dr=(40, 0, 9, 24))),
        ("destination region negative y", src, dst, info(dr=(0, -3, 8, 8))),
        ("source pitch below the row", fake_image(64, 32, R16, S, pitch=64 * 8 - 8), dst, info()),
        ("source pitch not a texel multiple", fake_image(64, 32, R16, S, pitch=64 * 8 + 4), dst, info()),
        ("destination pitch below the row", src, fake_image(48, 24, R8, D, pitch=48 * 4 - 4), info()),
        ("destination pitch not a texel multiple", src, fake_image(48, 24, R8, D, pitch=48 * 4 + 2), info()),
        ("source wider than the cap", fake_image(big, 4, R16, S), dst, info(sr=(0, 0, 4, 4))),
        ("destination higher than the cap", src, fake_image(4, big, R8, D), info(dr=(0, 0, 4, 4))),
        ("unknown filter", src, dst, info(filter=2)),
        ("unknown encode", src, dst, info(encode=2)),
        ("overlap", src, fake_image(48, 24, R8, S + 64 * 8 * 16), info()),
        ("overlap, destination first", fake_image(64, 32, R16, D + 48 * 4 * 23), dst, info()),
    ]


@pytest.mark.parametrize("case", refusal_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_refusals_are_decided_on_the_host(case):
    name, src, dst, info = case
    status = lib().szg_record_present(None, C.byref(src) if src is not None else None, C.byref(dst) if dst is not None else None,
                                      C.byref(info) if info is not None else None)
    assert status == abi.SZG_ERR_INVALID_ARGUMENT, name
    assert b"szg_record_present" in lib().szg_last_error(), name


def test_a_region_without_texels_is_a_no_op():
    src = fake_image(64, 32, abi.SZG_FORMAT_RGBA16_UNORM, 0x10000000)
    dst = fake_image(48, 24, abi.SZG_FORMAT_A2B10G10R10_UNORM, 0x20000000)
    for sr, dr in (((0, 0, 0, 32), (0, 0, 48, 24)), ((0, 0, 64, 32), (5, 5, 10, 0)), ((64, 32, 0, 0), (48, 24, 0, 0))):
        info = abi.PresentInfo(abi.Rect(*sr), abi.Rect(*dr), abi.SZG_FILTER_LINEAR, abi.SZG_OETF_SRGB)
        assert lib().szg_record_present(None, C.byref(src), C.byref(dst), C.byref(info)) == abi.SZG_OK
