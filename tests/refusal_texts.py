"""Every refusal of an image argument behind the C-ABI as {case id: [status, last-error text]}, so that the texts (which the
tests of each pass assert only in part) can be compared with a record: tests/golden/refusal_texts.json, written by this
module's __main__ from a build of the commit BEFORE the shared argument checks of api_common.hpp (SZG_HIP_LIBRARY names that
library; the host part needs no device, the GPU part one run on the MI355X), asserted by tests/test_refusal_texts.py.

No message prints a pointer, and no call here launches anything: each is refused on the host. collect_host() uses made-up
addresses; collect_gpu(), whose calls need a pipeline object, takes every address from one zeroed device allocation."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from syzygy_amd import abi, lib  # noqa: E402
from tests import mipmap_model, texture_display_cases as tc  # noqa: E402
from tests.texture_display_cases import image  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "refusal_texts.json")
S, D = 0x10000000, 0x20000000
U16, H16, R8 = abi.SZG_FORMAT_RGBA16_UNORM, abi.SZG_FORMAT_RGBA16_SFLOAT, abi.SZG_FORMAT_RGBA8_UNORM
F32, D32 = abi.SZG_FORMAT_RGBA32_SFLOAT, abi.SZG_FORMAT_D32_SFLOAT
BIG = abi.SZG_PRESENT_MAX_EXTENT + 1


def ref(x):
    return C.byref(x) if x is not None else None


def outcome(status):
    return [status, lib().szg_last_error().decode()]


def put(out, key, status):
    assert key not in out, key
    out[key] = outcome(status)


def jpeg_frame(coefficients=0x3000):
    """an 8x8 grey frame: one plane of one block"""
    frame = abi.JpegFrame(8, 8, 1, abi.SZG_JPEG_GREY, 1, 1, 0)
    frame.planes[0] = abi.JpegPlane(coefficients, 1, 1, 8, 8, 1, 1)
    return frame


def collect_host():
    from tests.test_compute_collection_reflection import record_refusal, record_refusals
    from tests.test_present_model import refusal_cases

    L = lib()
    out = {}
    for name, src, dst, info in refusal_cases(S, D):
        put(out, f"present/{name}", L.szg_record_present(None, ref(src), ref(dst), ref(info)))
    for name, src, dst, sr, dr in tc.copy_refusals(S, D):
        put(out, f"copy_image/{name}", L.szg_record_copy_image(None, ref(src), ref(dst), abi.Rect(*sr), abi.Rect(*dr)))
    for name, im, color in tc.clear_refusals(D):
        cc = (C.c_float * 4)(*color) if color is not None else None
        put(out, f"clear_color_image/{name}", L.szg_record_clear_color_image(None, ref(im), cc))
    for case in record_refusals():
        put(out, f"compute_collection/{case[0]}", record_refusal(case)[0])

    for name, im, w, h in [
        ("NULL image", None, 16, 8),
        ("NULL data", image(16, 8, U16, None), 16, 8),
        ("wrong format", image(16, 8, H16, S), 16, 8),
        ("too narrow", image(16, 8, U16, S), 17, 8),
        ("too low", image(16, 8, U16, S), 16, 9),
        ("pitch below the row", image(16, 8, U16, S, pitch=16 * 8 - 8), 16, 8),
        ("pitch not a texel multiple", image(16, 8, U16, S, pitch=16 * 8 + 4), 16, 8),
        ("data not a texel multiple", image(16, 8, U16, S + 4), 16, 8),
        ("pitch not a 16-byte multiple", image(15, 8, U16, S), 15, 8),
        ("data not 16-byte aligned", image(16, 8, U16, S + 8), 16, 8),
    ]:
        put(out, f"oetf/{name}", L.szg_record_oetf(None, ref(im), w, h, abi.SZG_OETF_SRGB))

    for name, im, w, h in [
        ("NULL data", image(16, 8, U16, None), 16, 8),
        ("wrong format", image(16, 8, R8, D), 16, 8),
        ("too small", image(16, 8, U16, D), 16, 12),
        ("pitch below the row", image(16, 8, U16, D, pitch=16 * 8 - 8), 16, 8),
        ("pitch not a texel multiple", image(16, 8, U16, D, pitch=16 * 8 + 4), 16, 8),
        ("data not a texel multiple", image(16, 8, U16, D + 2), 16, 8),
        ("pitch not a 16-byte multiple", image(16, 8, U16, D, pitch=16 * 8 + 8), 16, 8),
        ("data not 16-byte aligned", image(16, 8, U16, D + 8), 16, 8),
    ]:
        put(out, f"compose_rowtiles/{name}", L.szg_compose_rowtiles(None, C.c_void_p(S), 16 * 8 * 8, 2, 4, ref(im), w, h))

    frame = jpeg_frame()
    for name, im, scratch in [
        ("NULL dst", None, 0x4000),
        ("NULL dst data", image(8, 8, R8, None), 0x4000),
        ("dst data misaligned", image(8, 8, R8, D + 2), 0x4000),
        ("dst format", image(8, 8, abi.SZG_FORMAT_RGBA8_SRGB, D), 0x4000),
        ("dst too narrow", image(7, 8, R8, D), 0x4000),
        ("dst too low", image(8, 7, R8, D), 0x4000),
        ("dst pitch below the row", image(8, 8, R8, D, pitch=8 * 4 - 4), 0x4000),
        ("dst pitch not a texel multiple", image(8, 8, R8, D, pitch=8 * 4 + 2), 0x4000),
        ("wide dst pitch below the row", image(0x40000001, 8, R8, D, pitch=4), 0x4000),
    ]:
        put(out, f"jpeg_reconstruct/{name}", L.szg_record_jpeg_reconstruct(None, C.byref(frame), C.c_void_p(scratch), 64, 0xFFFFFFFF, 0, ref(im)))

    for name, level0, chain, nbytes, _ in mipmap_model.generate_refusals(S, D):
        put(out, f"generate_mipmaps/{name}", L.szg_record_generate_mipmaps(None, ref(level0), chain, nbytes))
    return out


def collect_gpu():
    import torch

    L = lib()
    out = {}
    arena = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")  # every address below lies in it, 4 KiB apart at the least
    A = arena.data_ptr()
    O, T = A + 0x10000, A + 0x20000  # the output image and a texture
    sampler = abi.UISampler(abi.SZG_FILTER_NEAREST, abi.SZG_UI_ADDRESS_REPEAT)

    layer = C.c_void_p()
    assert L.szg_ui_layer_create(C.byref(layer), 1, 1, 0) == abi.SZG_OK, L.szg_last_error()
    try:
        textures = [
            ("NULL image", None),
            ("NULL data", image(4, 4, R8, None)),
            ("zero width", image(0, 4, R8, T)),
            ("zero height", image(4, 0, U16, T)),
            ("wider than the cap", image(BIG, 4, R8, T)),
            ("higher than the cap", image(4, BIG, U16, T)),
            ("pitch below the row", image(16, 16, U16, T, pitch=16 * 8 - 8)),
            ("pitch not a texel multiple", image(16, 16, R8, T, pitch=16 * 4 + 2)),
            ("data misaligned", image(4, 4, U16, T + 4)),
        ]
        formats = (abi.SZG_FORMAT_UNDEFINED, H16, F32, D32, abi.SZG_FORMAT_BGRA8_UNORM, abi.SZG_FORMAT_A2B10G10R10_UNORM,
                   abi.SZG_FORMAT_RGBA8_SRGB, 9)
        handle = C.c_void_p()
        for name, im in textures + [(f"format {fmt}", image(4, 4, fmt, T)) for fmt in formats]:
            put(out, f"ui_add_texture/{name}", L.szg_ui_layer_add_texture(layer, ref(im), sampler, C.byref(handle)))
        view = abi.UITextureView((C.c_uint32 * 4)(0, 0, 0, 0))
        for name, im in textures + [(f"format {fmt}", image(4, 4, fmt, T)) for fmt in formats if fmt != H16]:
            put(out, f"ui_add_texture_view/{name}", L.szg_ui_layer_add_texture_view(layer, ref(im), sampler, C.byref(view), C.byref(handle)))

        # a registered texture whose bytes lie inside the output image's
        output = image(16, 16, U16, O)
        assert L.szg_ui_layer_add_texture(layer, C.byref(image(4, 4, R8, O + 16 * 8 * 4)), sampler, C.byref(handle)) == abi.SZG_OK
        command = abi.UIDrawCmd((C.c_float * 4)(0, 0, 16, 16), handle.value, 0, 0, 3, 0)
        empty = abi.UIDrawData((C.c_float * 2)(0, 0), (C.c_float * 2)(16, 16), (C.c_float * 2)(1, 1), None, 0, None, 0, None, 0)
        draws = abi.UIDrawData((C.c_float * 2)(0, 0), (C.c_float * 2)(16, 16), (C.c_float * 2)(1, 1), A + 0x30000, 3, A + 0x31000, 3,
                               C.pointer(command), 1)
        whole = (0, 0, 16, 16)
        clear = (C.c_float * 4)(0, 0, 0, 1)
        for name, im, area, dd in [
            ("NULL output", None, whole, empty),
            ("NULL output data", image(16, 16, U16, None), whole, empty),
            ("output format", image(16, 16, R8, O), whole, empty),
            ("output format half", image(16, 16, H16, O), whole, empty),
            ("output wider than the cap", image(BIG, 4, U16, O), (0, 0, 4, 4), empty),
            ("output pitch below the row", image(16, 16, U16, O, pitch=16 * 8 - 8), whole, empty),
            ("output pitch not a texel multiple", image(16, 16, U16, O, pitch=16 * 8 + 4), whole, empty),
            ("output data misaligned", image(16, 16, U16, O + 4), whole, empty),
            ("render area too wide", output, (1, 0, 16, 16), empty),
            ("render area too high", output, (0, 1, 16, 16), empty),
            ("render area negative", output, (-1, 0, 8, 8), empty),
            ("render area wraps", output, (1, 0, 0xFFFFFFFF, 8), empty),
            ("texture overlaps the output", output, whole, draws),
        ]:
            put(out, f"ui_record_draw/{name}",
                L.szg_ui_layer_record_draw(layer, None, ref(im), abi.Rect(*area), abi.SZG_UI_LOAD_OP_CLEAR, clear, C.byref(dd)))
    finally:
        L.szg_ui_layer_destroy(layer)

    deferred, sky = C.c_void_p(), C.c_void_p()
    assert L.szg_deferred_create(C.byref(deferred), C.byref(abi.DeferredDesc(16, 16, 1, 1, 0, 0)), 0) == abi.SZG_OK, L.szg_last_error()
    try:
        for name, im in [
            ("wrong format", image(4, 4, R8, T)),
            ("zero extent", image(0, 4, D32, T)),
            ("pitch below the row", image(8, 8, D32, T, pitch=8 * 4 - 4)),
            ("pitch not a texel multiple", image(8, 8, D32, T, pitch=8 * 4 + 2)),
            ("data misaligned", image(8, 8, D32, T + 2)),
        ]:
            put(out, f"set_shadow_map/{name}", L.szg_deferred_set_shadow_map(deferred, 0, C.byref(im)))

        cameras = C.c_void_p(A + 0x40000)
        color, depth = image(16, 16, U16, O), image(16, 16, D32, A + 0x18000)
        fill = abi.FillScene()
        for name, scene, extent in [
            ("scene colour format", abi.SceneTexture(image(16, 16, H16, O), depth, abi.Image()), (16, 16)),
            ("scene colour pitch", abi.SceneTexture(image(16, 16, U16, O, pitch=16 * 8 + 4), depth, abi.Image()), (16, 16)),
            ("scene depth too small", abi.SceneTexture(color, image(16, 8, D32, A + 0x18000), abi.Image()), (16, 16)),
            ("scene debug colour misaligned", abi.SceneTexture(color, depth, image(16, 16, F32, A + 0x50008)), (16, 16)),
            ("draw extent above the G-buffer", abi.SceneTexture(color, depth, abi.Image()), (17, 16)),
        ]:
            put(out, f"gbuffer_fill/{name}", L.szg_deferred_record_gbuffer_fill(deferred, None, abi.Rect(0, 0, *extent), None, C.byref(scene), 0,
                                                                                cameras, C.byref(fill)))

        assert L.szg_skyview_create(C.byref(sky), C.byref(abi.SkyviewDesc(2, 2, 2, 2, 0, 0)), 0) == abi.SZG_OK, L.szg_last_error()
        scene = abi.SceneTexture(color, depth, abi.Image())
        planes = [image(16, 16, F32 if i == 3 else H16, A + 0x60000 + i * 0x2000) for i in range(5)]
        for name, i, bad in [
            ("gbuffer diffuse format", 0, image(16, 16, U16, A + 0x60000)),
            ("gbuffer normal NULL data", 2, image(16, 16, H16, None)),
            ("gbuffer worldPosition pitch", 3, image(16, 16, F32, A + 0x66000, pitch=16 * 16 - 16)),
            ("gbuffer occlusionRoughnessMetallic too small", 4, image(8, 16, H16, A + 0x68000)),
        ]:
            gbuffer = abi.GBuffer(*(planes[:i] + [bad] + planes[i + 1:]))
            put(out, f"composite/{name}", L.szg_skyview_record_composite(sky, None, C.byref(scene), abi.Rect(0, 0, 16, 16), None, C.byref(gbuffer),
                                                                         None, 0, A + 0x41000, 0, cameras, 0, A + 0x42000))
        put(out, "composite/NULL gbuffer", L.szg_skyview_record_composite(sky, None, C.byref(scene), abi.Rect(0, 0, 16, 16), None, None, None, 0,
                                                                          A + 0x41000, 0, cameras, 0, A + 0x42000))
    finally:
        L.szg_skyview_destroy(sky)
        L.szg_deferred_destroy(deferred)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    # python tests/refusal_texts.py host|gpu: (re)write that part of the record from the library SZG_HIP_LIBRARY names
    part = sys.argv[1]
    record = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    record[part] = {"host": collect_host, "gpu": collect_gpu}[part]()
    record[f"{part}_recorded_from"] = lib().szg_build_id().decode()
    with open(GOLDEN, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(record[part])} {part} cases from {os.environ.get('SZG_HIP_LIBRARY', 'the library of this tree')} ({record[f'{part}_recorded_from']})")
