"""GPU: pipelines.TextureDisplay, the Texture Viewer of ui/texturedisplay.cpp through the Python mirror: a 16x16 display image,
textures selected into it and the viewer quad drawn in a 40x30 UI frame. The frame equals the copy model followed by the UI
model (tests/texture_display_model.py), byte for byte."""
import numpy as np
import pytest

from syzygy_amd import abi, ui
from tests import texture_display_model as tm
from tests import ui_layer_model as um

pytestmark = pytest.mark.gpu
SIZE = (40, 30)
DISPLAY = (16, 16)
QUAD = ((12.0, 4.0), (34.0, 26.0))  # the widget: imageSize(22) of a square display image
OPAQUE_BLACK = [0, 0, 0, 0x3C00]


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    return torch


@pytest.fixture()
def viewer(torch):
    from syzygy_amd import pipelines as pl

    layer = pl.UILayer.create(SIZE, triangleCapacity=64, commandCapacity=8)
    white = layer.addTexture(torch.full((1, 1, 4), 255, dtype=torch.uint8, device="cuda"), abi.SZG_FILTER_LINEAR, abi.SZG_UI_ADDRESS_REPEAT)
    display = pl.TextureDisplay(layer, DISPLAY)
    yield layer, display, white
    display.cleanup()
    layer.cleanup()


def frame(display, white):
    """A panel behind the viewer quad, which is wider than the display's texels in uv so that the border shows"""
    dl = ui.DrawList(white)
    dl.add_rect_filled((2, 2), (38, 28), ui.col32(40, 60, 80, 255))
    assert display.imageSize(22.0) == (22.0, 22.0)
    dl.add_image(display.handle, QUAD[0], QUAD[1], (-0.125, 0.0), (1.0, 1.125), ui.col32(255, 230, 200, 255))
    return ui.DrawData((0, 0), SIZE, (1, 1), [dl])


def draw_and_check(torch, layer, display, white, want_display):
    """The display image holds `want_display` (binary16 bits), and the frame is the UI model's with it as the viewer's texture"""
    data = frame(display, white)
    out = layer.recordDraw(None, data)
    torch.cuda.synchronize()
    got_display = display.image.cpu().numpy().view(np.uint16)
    assert np.array_equal(got_display, want_display)
    textures = {white: um.Texture(np.full((1, 1, 4), 255, np.uint8), um.LINEAR, um.REPEAT),
                display.handle: tm.TextureView(want_display.view(np.float16), um.NEAREST, um.CLAMP_TO_BORDER,
                                               (tm.IDENTITY, tm.IDENTITY, tm.IDENTITY, tm.ONE))}
    want = tm.render(np.zeros((SIZE[1], SIZE[0], 4), np.uint16), (0, 0) + SIZE, um.CLEAR, (0.0, 0.0, 0.0, 1.0), data.flatten(), textures)
    got = out.texture.color_numpy()
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} texels differ"
    assert (got[..., 3] == 65535).all()  # alpha ONE: the viewer is opaque whatever the texture's alpha
    return got


def blank():
    return np.zeros((DISPLAY[1], DISPLAY[0], 4), np.uint16)


def test_a_new_display_is_opaque_black(torch, viewer):
    layer, display, white = viewer
    want = blank()
    want[:] = OPAQUE_BLACK
    got = draw_and_check(torch, layer, display, white, want)
    assert got[15, 20].tolist() == [0, 0, 0, 65535]


def test_select_an_srgb_map_whose_alpha_is_zero(torch, viewer):
    layer, display, white = viewer
    rng = np.random.default_rng(21)
    texels = rng.integers(0, 256, (4, 4, 4), dtype=np.uint8)
    texels[..., 3] = 0
    display.select(None, torch.from_numpy(texels).cuda(), srgb=True)
    want = tm.copy_image(texels, tm.RGBA8_SRGB, (0, 0, 4, 4), blank(), (0, 0) + DISPLAY)
    assert (want[..., 3] == 0).all() and np.array_equal(want[0:4, 0:4], np.broadcast_to(want[0, 0], (4, 4, 4)))  # magnified 4x
    got = draw_and_check(torch, layer, display, white, want)
    assert (got[8:24, 18:32, :3] != 0).any()  # and visible, although the texels' alpha is 0
    # the same map as RGBA8_UNORM gives other bytes: the sRGB decode ran
    display.select(None, torch.from_numpy(texels).cuda())
    torch.cuda.synchronize()
    assert not np.array_equal(display.image.cpu().numpy().view(np.uint16), want)


def test_select_a_6x3_unorm_map_stretches_it_to_the_square(torch, viewer):
    layer, display, white = viewer
    texels = np.random.default_rng(22).integers(0, 256, (3, 6, 4), dtype=np.uint8)
    display.select(None, torch.from_numpy(texels).cuda())
    want = tm.copy_image(texels, tm.RGBA8_UNORM, (0, 0, 6, 3), blank(), (0, 0) + DISPLAY)
    assert len(np.unique(want[:, 0, 0])) <= 3 and len(np.unique(want[0].reshape(-1, 4), axis=0)) > 3  # 3 rows, 6 columns, on 16x16
    draw_and_check(torch, layer, display, white, want)


def test_clear_gives_opaque_black_again(torch, viewer):
    layer, display, white = viewer
    display.select(None, torch.full((5, 5, 4), 200, dtype=torch.uint8, device="cuda"))
    display.select(None, None)  # "None"
    want = blank()
    want[:] = OPAQUE_BLACK
    draw_and_check(torch, layer, display, white, want)
    display.select(None, torch.full((5, 5, 4), 200, dtype=torch.uint8, device="cuda"))
    display.clear(None)
    draw_and_check(torch, layer, display, white, want)


def test_select_a_half_float_plane_and_a_unorm16_image(torch, viewer):
    layer, display, white = viewer
    rng = np.random.default_rng(23)
    plane = (rng.random((9, 7, 4)) * 2.0 - 0.5).astype(np.float16)  # a normal plane: values outside [0, 1] too
    plane[0, 0] = [np.inf, -np.inf, np.nan, 2.0]
    display.select(None, torch.from_numpy(plane).cuda())
    want = tm.copy_image(plane.view(np.uint16), tm.RGBA16_SFLOAT, (0, 0, 7, 9), blank(), (0, 0) + DISPLAY)
    draw_and_check(torch, layer, display, white, want)
    codes = rng.integers(0, 65536, (5, 11, 4)).astype(np.uint16)
    display.select(None, torch.from_numpy(codes.view(np.int16)).cuda())
    want = tm.copy_image(codes, tm.RGBA16_UNORM, (0, 0, 11, 5), blank(), (0, 0) + DISPLAY)
    draw_and_check(torch, layer, display, white, want)


def test_two_selects_in_flight_the_last_one_shows(torch, viewer):
    layer, display, white = viewer
    rng = np.random.default_rng(24)
    first = torch.from_numpy(rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)).cuda()
    second_host = rng.integers(0, 256, (2, 3, 4), dtype=np.uint8)
    second = torch.from_numpy(second_host).cuda()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        display.select(stream, first, srgb=True)
        display.select(stream, second)
        data = frame(display, white)
        out = layer.recordDraw(stream, data)
    stream.synchronize()
    want_display = tm.copy_image(second_host, tm.RGBA8_UNORM, (0, 0, 3, 2), blank(), (0, 0) + DISPLAY)
    assert np.array_equal(display.image.cpu().numpy().view(np.uint16), want_display)
    textures = {white: um.Texture(np.full((1, 1, 4), 255, np.uint8), um.LINEAR, um.REPEAT),
                display.handle: tm.TextureView(want_display.view(np.float16), um.NEAREST, um.CLAMP_TO_BORDER, (0, 0, 0, tm.ONE))}
    want = tm.render(np.zeros((SIZE[1], SIZE[0], 4), np.uint16), (0, 0) + SIZE, um.CLEAR, (0.0, 0.0, 0.0, 1.0), data.flatten(), textures)
    assert np.array_equal(out.texture.color_numpy(), want)


@pytest.mark.parametrize("what", ["color", "gbuffer-normal"])
def test_frame_loop_example_with_the_texture_viewer(torch, what):
    """examples/frame_loop.py --ui-layer --texture-viewer: the panel's quad shows the picked image, opaque, over the side panel;
    the rest of the frame is the frame without the switch."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import frame_loop
    finally:
        sys.path.pop(0)
    common = ["--frames", "1", "--width", "260", "--height", "144", "--shadow-map", "256", "--ui-layer"]
    plain = frame_loop.main(common)
    out = frame_loop.main(common + [f"--texture-viewer={what}"])
    quad = (slice(30, 66), slice(8, 44))  # panel 52 px wide: the image is 36 x 36 at (8, 30), framed by 2 px
    frame = np.ones(out.shape[:2], bool)
    frame[28:68, 6:46] = False
    assert np.array_equal(out[frame], plain[frame])
    assert (out[quad] != plain[quad]).any(axis=2).mean() > 0.9 and (out[quad][..., 3] == 65535).all()
    assert len(np.unique(out[quad].reshape(-1, 4), axis=0)) > 1
