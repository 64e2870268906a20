"""The refusals of include/szg/texture_display.h as data, shared by tests/test_texture_display_abi.py (addresses of memory that
is never touched: every refusal is decided on the host) and tests/test_gpu_image_copy.py (real device buffers, whose bytes must
not change)."""
from syzygy_amd import abi

R8, SRGB8 = abi.SZG_FORMAT_RGBA8_UNORM, abi.SZG_FORMAT_RGBA8_SRGB
U16, H16 = abi.SZG_FORMAT_RGBA16_UNORM, abi.SZG_FORMAT_RGBA16_SFLOAT
SRC_EXTENT, DST_EXTENT = (64, 32), (48, 24)


def image(width, height, fmt, address, pitch=None):
    """An szg_image at `address`, tightly packed unless `pitch` says otherwise. The refusal lists here and in
    tests/test_present_model.py, tests/test_compute_collection_reflection.py and tests/refusal_texts.py build theirs over
    memory that is never touched: a refusal is decided on the host, before anything is launched."""
    return abi.Image(address, width, height, width * abi.TEXEL_BYTES.get(fmt, 4) if pitch is None else pitch, fmt)


def copy_refusals(S, D):
    """(name, src image, dst image, src region, dst region) of every refusal of szg_record_copy_image, for a 64x32 RGBA8_UNORM
    source at address S and a 48x24 RGBA16_SFLOAT destination at address D."""
    src, dst = image(64, 32, R8, S), image(48, 24, H16, D)
    whole_s, whole_d = (0, 0, 64, 32), (0, 0, 48, 24)
    big = abi.SZG_PRESENT_MAX_EXTENT + 1
    cases = [
        ("NULL source", None, dst, whole_s, whole_d),
        ("NULL destination", src, None, whole_s, whole_d),
        ("NULL source data", image(64, 32, R8, 0), dst, whole_s, whole_d),
        ("NULL destination data", src, image(48, 24, H16, 0), whole_s, whole_d),
        ("source region too wide", src, dst, (1, 0, 64, 32), whole_d),
        ("source region too high", src, dst, (0, 1, 64, 32), whole_d),
        ("source region negative x", src, dst, (-1, 0, 8, 8), whole_d),
        ("source region wraps", src, dst, (1, 0, 0xFFFFFFFF, 8), whole_d),
        ("destination region too wide", src, dst, whole_s, (40, 0, 9, 24)),
        ("destination region negative y", src, dst, whole_s, (0, -3, 8, 8)),
        ("source pitch below the row", image(64, 32, R8, S, pitch=64 * 4 - 4), dst, whole_s, whole_d),
        ("source pitch not a texel multiple", image(64, 32, R8, S, pitch=64 * 4 + 2), dst, whole_s, whole_d),
        ("destination pitch below the row", src, image(48, 24, H16, D, pitch=48 * 8 - 8), whole_s, whole_d),
        ("destination pitch not a texel multiple", src, image(48, 24, H16, D, pitch=48 * 8 + 4), whole_s, whole_d),
        ("source data misaligned", image(16, 8, U16, S + 4), dst, (0, 0, 16, 8), whole_d),
        ("destination data misaligned", src, image(40, 20, H16, D + 4), whole_s, (0, 0, 40, 20)),
        ("source wider than the cap", image(big, 4, R8, S), dst, (0, 0, 4, 4), whole_d),
        ("destination higher than the cap", src, image(4, big, H16, D), whole_s, (0, 0, 4, 4)),
        ("overlap", src, image(48, 8, H16, S + 64 * 4 * 16), whole_s, (0, 0, 48, 8)),
        ("overlap, destination first", image(16, 8, R8, D + 48 * 8 * 23), dst, (0, 0, 16, 8), whole_d),
    ]
    for fmt in (abi.SZG_FORMAT_UNDEFINED, abi.SZG_FORMAT_RGBA32_SFLOAT, abi.SZG_FORMAT_D32_SFLOAT, abi.SZG_FORMAT_BGRA8_UNORM,
                abi.SZG_FORMAT_A2B10G10R10_UNORM, 9):
        cases.append((f"source format {fmt}", image(16, 8, fmt, S), dst, (0, 0, 16, 8), whole_d))
    for fmt in (abi.SZG_FORMAT_UNDEFINED, U16, R8, SRGB8, abi.SZG_FORMAT_RGBA32_SFLOAT, abi.SZG_FORMAT_A2B10G10R10_UNORM):
        cases.append((f"destination format {fmt}", src, image(24, 12, fmt, D), whole_s, (0, 0, 24, 12)))
    return cases


def clear_refusals(D):
    """(name, image, colour or None) of every refusal of szg_record_clear_color_image, for a 48x24 image of 8-byte texels at D."""
    black = (0.0, 0.0, 0.0, 1.0)
    big = abi.SZG_PRESENT_MAX_EXTENT + 1
    cases = [
        ("NULL image", None, black),
        ("NULL data", image(48, 24, H16, 0), black),
        ("NULL colour", image(48, 24, H16, D), None),
        ("pitch below the row", image(48, 24, H16, D, pitch=48 * 8 - 8), black),
        ("pitch not a texel multiple", image(48, 24, U16, D, pitch=48 * 8 + 4), black),
        ("data misaligned", image(40, 20, H16, D + 2), black),
        ("wider than the cap", image(big, 1, H16, D), black),
    ]
    for fmt in (abi.SZG_FORMAT_UNDEFINED, R8, SRGB8, abi.SZG_FORMAT_RGBA32_SFLOAT, abi.SZG_FORMAT_D32_SFLOAT, abi.SZG_FORMAT_BGRA8_UNORM):
        cases.append((f"format {fmt}", image(24, 12, fmt, D), black))
    return cases


EMPTY_REGIONS = (((0, 0, 0, 32), (0, 0, 48, 24)), ((0, 0, 64, 32), (5, 5, 10, 0)), ((64, 32, 0, 0), (48, 24, 0, 0)))
