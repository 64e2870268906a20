"""GPU: szg_ui_layer_add_texture_view (include/szg/texture_display.h): RGBA16_SFLOAT textures and the view's component mapping
in the UI layer pass (syzygy_amd/csrc/kernels_ui_layer.hip) against the CPU model (tests/texture_display_model.py on top of
tests/ui_layer_model.py), byte for byte over the whole padded target (tests/ui_layer_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

from syzygy_amd import abi, lib, ui
from tests import texture_display_model as tm
from tests import ui_layer_cases as uc
from tests import ui_layer_gpu as ug
from tests import ui_layer_model as um

pytestmark = pytest.mark.gpu
CLEAR = um.CLEAR
INV = abi.SZG_ERR_INVALID_ARGUMENT
FORMAT = {np.dtype(np.uint8): abi.SZG_FORMAT_RGBA8_UNORM, np.dtype(np.uint16): abi.SZG_FORMAT_RGBA16_UNORM,
          np.dtype(np.float16): abi.SZG_FORMAT_RGBA16_SFLOAT}


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def layer(torch):
    lay = ug.Layer(torch, triangle_capacity=256, command_capacity=16)
    yield lay
    lay.destroy()


def add_view(layer, tex, pitch_pad=0, null_view=False):
    """tm.TextureView -> handle of szg_ui_layer_add_texture_view; the device copy's rows carry `pitch_pad` more texels"""
    data = tex.data
    h, w = data.shape[:2]
    padded = np.zeros((h, w + pitch_pad, 4), data.dtype)
    padded[:, :w] = data
    d = ug.to_device(layer.torch, padded)
    im = abi.Image(d.data_ptr(), w, h, (w + pitch_pad) * data.dtype.itemsize * 4, FORMAT[data.dtype])
    view = abi.UITextureView((C.c_uint32 * 4)(*tex.swizzle))
    out = C.c_void_p()
    rc = lib().szg_ui_layer_add_texture_view(layer.h, C.byref(im), abi.UISampler(tex.filter, tex.address),
                                             None if null_view else C.byref(view), C.byref(out))
    assert rc == abi.SZG_OK, lib().szg_last_error()
    layer.keep.append(d)
    return out.value


def run(layer, target, area, draw, textures, null_view=False):
    """Record `draw` with every TextureView registered as a view and every um.Texture as a plain texture: (bytes, the model's)"""
    handles = {k: add_view(layer, t, i % 3, null_view) if isinstance(t, tm.TextureView) else layer.add_texture(t, i % 3)
               for i, (k, t) in enumerate(textures.items())}
    assert layer.record(target, area, CLEAR, draw, handles) == abi.SZG_OK, lib().szg_last_error()
    got = target.read()
    for h in handles.values():
        assert layer.remove_texture(h) == abi.SZG_OK
    layer.keep.clear()
    return got, target.expect(tm.render(target.image0, area, CLEAR, ug.BLACK, draw, textures))


def check(got, want):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=2))
        y, x = bad[0]
        pytest.fail(f"{len(bad)} texels differ, first at (x={x}, y={y}): got {got[y, x].tolist()}, want {want[y, x].tolist()}")


def quad(size, box, uv0, uv1, cols, key="t"):
    """One textured quad `box` = (x0, y0, x1, y1) on a frame of `size`, uv from uv0 to uv1, one colour per corner"""
    x0, y0, x1, y1 = box
    vertices = [(x0, y0, uv0[0], uv0[1], cols[0]), (x1, y0, uv1[0], uv0[1], cols[1]), (x1, y1, uv1[0], uv1[1], cols[2]),
                (x0, y1, uv0[0], uv1[1], cols[3])]
    return uc.flat(vertices, [0, 1, 2, 0, 2, 3], [(uc.everything(size), key, 0, 0, 6)], size)


TINTS = (ui.col32(255, 255, 255, 255), ui.col32(255, 128, 64, 200), ui.col32(90, 255, 30, 140), ui.col32(10, 20, 255, 255))
SAMPLERS = [(f, a) for f in (um.NEAREST, um.LINEAR) for a in (um.REPEAT, um.CLAMP_TO_EDGE, um.CLAMP_TO_BORDER)]
SAMPLER_IDS = [f"{'linear' if f else 'nearest'}-{ {0: 'repeat', 2: 'edge', 3: 'border'}[a]}" for f, a in SAMPLERS]


# ---- identity views of the two UNORM formats: the bytes of szg_ui_layer_add_texture ----
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["rgba8", "unorm16"])
@pytest.mark.parametrize("null_view", [False, True], ids=["identity", "NULL"])
def test_an_identity_view_of_a_unorm_texture_draws_what_the_plain_handle_draws(torch, layer, dtype, null_view):
    """The sampler case of tests/test_gpu_ui_layer.py (UVs from below 0 to above 1, a tinted, rotated triangle) on a 40x30
    frame, LINEAR / REPEAT and NEAREST / CLAMP_TO_BORDER"""
    for filt, address in ((um.LINEAR, um.REPEAT), (um.NEAREST, um.CLAMP_TO_BORDER)):
        draw, textures = uc.sampler_case(filt, address, dtype)
        draw = draw._replace(display_size=(40.0, 30.0), commands=[draw.commands[0]._replace(clip_rect=uc.everything((40, 30)))])
        plain, want = ug.run_case(layer, ug.Target(torch, 40, 30), (0, 0, 40, 30), CLEAR, draw, textures)
        check(plain, want)
        views = {"t": tm.TextureView(textures["t"].data, filt, address, tm.IDENTITY_VIEW)}
        got, want_view = run(layer, ug.Target(torch, 40, 30), (0, 0, 40, 30), draw, views, null_view)
        check(got, want_view)
        assert np.array_equal(got, plain)
        assert (got[:30, :40] != [0, 0, 0, 65535]).any(axis=2).mean() > 0.15  # under CLAMP_TO_BORDER most of the quad is border


# ---- RGBA16_SFLOAT ----
def special_half_texture():
    """4x4 texels of binary16: both zeros, the smallest denormal, 2^-14, 0.5, 1, 65504, both infinities, NaN, negatives"""
    bits = np.array([0x0000, 0x8000, 0x0001, 0x0400, 0x3800, 0x3C00, 0x7BFF, 0x7C00, 0xFC00, 0x7E00, 0xBC00, 0xB800, 0x83FF, 0x3555,
                     0x2E66, 0x3BFF], np.uint16)
    data = np.stack([np.roll(bits, 3 * k) for k in range(4)], axis=1).reshape(4, 4, 4)
    data[1, 1] = [0x3400, 0x3800, 0x3A00, 0x3C00]  # and ordinary values, so that LINEAR has finite neighbourhoods too
    data[2, 1] = [0x3000, 0x3555, 0x3800, 0x3900]
    data[1, 2] = [0x2E66, 0x3266, 0x34CD, 0x3666]
    return data.view(np.float16)


@pytest.mark.parametrize("filt,address", SAMPLERS, ids=SAMPLER_IDS)
def test_a_half_float_texture_with_every_special_value(torch, layer, filt, address):
    size = (23, 17)
    textures = {"t": tm.TextureView(special_half_texture(), filt, address, tm.IDENTITY_VIEW)}
    draw = quad(size, (0, 0, 23, 17), (-0.25, -0.25), (1.25, 1.25), TINTS)
    got, want = run(layer, ug.Target(torch, 23, 17), (0, 0, 23, 17), draw, textures)
    check(got, want)
    assert len(np.unique(got[:17, :23].reshape(-1, 4), axis=0)) > 20  # not a flat frame


def test_half_float_denormals_reach_the_output(torch, layer):
    """1023 / 1024 * 2^-14 (the largest denormal) times 65535 is 3.99: a flushed denormal would store code 0"""
    data = np.full((2, 2, 4), 0x03FF, np.uint16)
    data[..., 3] = 0x3C00
    textures = {"t": tm.TextureView(data.view(np.float16), um.NEAREST, um.CLAMP_TO_EDGE, tm.IDENTITY_VIEW)}
    draw = quad((8, 8), (0, 0, 8, 8), (0, 0), (1, 1), (uc.OPAQUE,) * 4)
    got, want = run(layer, ug.Target(torch, 8, 8), (0, 0, 8, 8), draw, textures)
    check(got, want)
    assert got[3, 3].tolist() == [4, 4, 4, 65535]


# ---- MAPPING ----
@pytest.mark.parametrize("swizzle", range(7), ids=["identity", "zero", "one", "r", "g", "b", "a"])
def test_every_swizzle_value_in_every_slot(torch, layer, swizzle):
    """Four views of one frame: `swizzle` in slot 0, 1, 2, 3, identity elsewhere; LINEAR / CLAMP_TO_BORDER so that border taps
    go through the filter before the mapping. A half-float and a UNORM16 texture take turns."""
    size = (40, 30)
    rng = np.random.default_rng(12)
    half = rng.random((5, 6, 4)).astype(np.float16)
    codes = rng.integers(0, 65536, (5, 6, 4)).astype(np.uint16)
    vertices, indices, commands, textures = [], [], [], {}
    for slot in range(4):
        sw = [tm.IDENTITY] * 4
        sw[slot] = swizzle
        textures[slot] = tm.TextureView(half if slot % 2 == 0 else codes, um.LINEAR, um.CLAMP_TO_BORDER, tuple(sw))
        x0, y0 = 20 * (slot % 2), 15 * (slot // 2)
        q = quad(size, (x0 + 1, y0 + 1, x0 + 19, y0 + 14), (-0.2, -0.2), (1.2, 1.2), TINTS)
        commands.append((uc.everything(size), slot, len(vertices), len(indices), 6))
        vertices += [(v["pos"][0], v["pos"][1], v["uv"][0], v["uv"][1], v["col"]) for v in q.vertices]
        indices += [0, 1, 2, 0, 2, 3]
    draw = uc.flat(vertices, indices, commands, size)
    got, want = run(layer, ug.Target(torch, 40, 30), (0, 0, 40, 30), draw, textures)
    check(got, want)


def test_one_is_one_where_the_weights_are_nan(torch, layer):
    """MAPPING follows the filter: with u = +inf the LINEAR weights are NaN and the filtered sample is NaN in every channel;
    ONE on alpha still gives 1, ZERO gives 0, and the identity channels become 0 in FRAGMENT. Mapping the taps first would
    make alpha NaN -> 0 and leave the clear colour."""
    size = (12, 9)
    data = np.full((3, 3, 4), 0x3800, np.uint16).view(np.float16)
    textures = {"t": tm.TextureView(data, um.LINEAR, um.CLAMP_TO_EDGE, (tm.ONE, tm.IDENTITY, tm.ZERO, tm.ONE))}
    inf = float("inf")
    draw = quad(size, (2, 2, 10, 7), (inf, 0.0), (inf, 1.0), (uc.OPAQUE,) * 4)
    got, want = run(layer, ug.Target(torch, 12, 9), (0, 0, 12, 9), draw, textures)
    check(got, want)
    assert got[4, 5].tolist() == [65535, 0, 0, 65535] and got[0, 0].tolist() == [0, 0, 0, 65535]


# ---- refusals ----
def test_add_texture_view_refusals(torch, layer):
    t = ug.to_device(torch, np.zeros((4, 4, 8), np.uint8))
    out = C.c_void_p()
    ok = abi.Image(t.data_ptr(), 4, 4, 32, abi.SZG_FORMAT_RGBA16_SFLOAT)
    identity = abi.UITextureView((C.c_uint32 * 4)(0, 0, 0, 0))

    def view(*sw):
        return abi.UITextureView((C.c_uint32 * 4)(*sw))

    cases = [("swizzle", ok, (0, 0), view(0, 7, 0, 0)), ("swizzle", ok, (0, 0), view(0, 0, 0, 0xFFFFFFFF)),
             ("format", abi.Image(t.data_ptr(), 4, 4, 16, abi.SZG_FORMAT_BGRA8_UNORM), (0, 0), identity),
             ("format", abi.Image(t.data_ptr(), 4, 4, 16, abi.SZG_FORMAT_RGBA8_SRGB), (0, 0), identity),
             ("format", abi.Image(t.data_ptr(), 2, 4, 32, abi.SZG_FORMAT_RGBA32_SFLOAT), (0, 0), identity),
             ("format", abi.Image(t.data_ptr(), 4, 4, 32, abi.SZG_FORMAT_UNDEFINED), (0, 0), identity),
             # what szg_ui_layer_add_texture refuses
             ("filter", ok, (2, 0), identity), ("address", ok, (0, 1), identity), ("address", ok, (1, 4), identity),
             ("NULL", abi.Image(None, 4, 4, 32, abi.SZG_FORMAT_RGBA16_SFLOAT), (0, 0), identity),
             ("pitch", abi.Image(t.data_ptr(), 4, 4, 24, abi.SZG_FORMAT_RGBA16_SFLOAT), (0, 0), identity),
             ("alignment", abi.Image(t.data_ptr() + 4, 3, 3, 32, abi.SZG_FORMAT_RGBA16_SFLOAT), (0, 0), identity),
             ("extents", abi.Image(t.data_ptr(), 0, 4, 32, abi.SZG_FORMAT_RGBA16_SFLOAT), (0, 0), identity)]
    for what, im, sampler, v in cases:
        out.value = 1
        assert lib().szg_ui_layer_add_texture_view(layer.h, C.byref(im), abi.UISampler(*sampler), C.byref(v), C.byref(out)) == INV, what
        assert what.encode() in lib().szg_last_error() and b"szg_ui_layer_add_texture_view" in lib().szg_last_error() and not out.value, \
            (what, lib().szg_last_error())
    assert lib().szg_ui_layer_add_texture_view(layer.h, C.byref(ok), abi.UISampler(0, 0), C.byref(identity), None) == INV
    # and szg_ui_layer_add_texture still refuses the half-float format
    assert lib().szg_ui_layer_add_texture(layer.h, C.byref(ok), abi.UISampler(0, 0), C.byref(out)) == INV and not out.value


def test_a_view_that_overlaps_the_output_is_refused_at_record_time(torch, layer):
    draw = quad((40, 30), (2, 2, 30, 20), (0, 0), (1, 1), (uc.OPAQUE,) * 4)
    target = ug.Target(torch, 40, 30)
    inside = abi.Image(target.buffer.data_ptr() + 43 * 8 * 4, 4, 4, 43 * 8, abi.SZG_FORMAT_RGBA16_SFLOAT)
    handle = C.c_void_p()
    view = abi.UITextureView((C.c_uint32 * 4)(0, 0, 0, abi.SZG_SWIZZLE_ONE))
    assert lib().szg_ui_layer_add_texture_view(layer.h, C.byref(inside), abi.UISampler(0, 3), C.byref(view), C.byref(handle)) == abi.SZG_OK
    assert layer.record(target, (0, 0, 40, 30), CLEAR, draw, {"t": handle.value}) == INV
    assert b"overlaps the output" in lib().szg_last_error()
    assert np.array_equal(target.read(), target.buffer0)
    assert layer.remove_texture(handle.value) == abi.SZG_OK and layer.remove_texture(handle.value) == INV
    layer.keep.clear()
