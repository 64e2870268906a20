"""GPU: the UI layer pass (include/szg/ui_layer.h, syzygy_amd/csrc/kernels_ui_layer.hip) through the C-ABI against the CPU model
(tests/ui_layer_model.py), bit for bit. Targets are padded and filled with a sentinel (tests/ui_layer_gpu.py: Target) and the
WHOLE buffer is compared: anything written outside the render area, pitch padding included, fails. The cases are those of the
CPU tests (tests/ui_layer_cases.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from syzygy_amd import abi, lib, ui
from tests import gpu_ui_layer_child as child
from tests import ui_layer_cases as uc
from tests import ui_layer_gpu as ug
from tests import ui_layer_model as um

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLEAR, LOAD = um.CLEAR, um.LOAD
STACK_SIZES = (1, 63, 64, 65, 4095, 4096, 4097)  # chunk (64 triangles) and super-chunk (4096) boundaries, in quads and triangles


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def layer(torch):
    lay = ug.Layer(torch)
    yield lay
    lay.destroy()


def check(got, want):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=2))
        y, x = bad[0]
        pytest.fail(f"{len(bad)} texels differ, first at (x={x}, y={y}): got {got[y, x].tolist()}, want {want[y, x].tolist()}")


# ---- the render area: neither extent a multiple of a patch, offset honoured, viewport unchanged ----
@pytest.mark.parametrize("load_op", [CLEAR, LOAD])
@pytest.mark.parametrize("offset", [(0, 0), (3, 2)])
def test_render_area_67x45_in_a_71x53_image(torch, layer, offset, load_op):
    draw, textures = uc.random_sweep(seed=5, n_tris=600, size=(67, 45), n_cmds=10, big_fraction=0.04)
    target = ug.Target(torch, 71, 53)
    got, want = ug.run_case(layer, target, (offset[0], offset[1], 67, 45), load_op, draw, textures, clear=(0.1, 0.2, 0.3, 0.9))
    check(got, want)
    changed = (want != target.buffer0).any(axis=2)
    assert changed[offset[1]:offset[1] + 45, offset[0]:67].mean() > 0.5 and not changed[:, 67 + offset[0]:].any()


@pytest.mark.parametrize("filt,address,dtype", uc.SAMPLER_COMBOS)
def test_the_twelve_samplers(torch, layer, filt, address, dtype):
    draw, textures = uc.sampler_case(filt, address, dtype)
    got, want = ug.run_case(layer, ug.Target(torch, 48, 36), (0, 0, 48, 36), CLEAR, draw, textures)
    check(got, want)


# ---- order ----
@pytest.fixture(scope="module")
def stack_model():
    draw, textures = uc.stack()
    _, snapshots = um.render(np.zeros((64, 64, 4), np.uint16), (0, 0, 64, 64), CLEAR, ug.BLACK, draw, textures,
                             snapshots={2 * n for n in STACK_SIZES})
    return draw, textures, snapshots


@pytest.mark.parametrize("n", STACK_SIZES)
def test_the_stack_blends_in_submission_order(torch, layer, stack_model, n):
    draw, textures, snapshots = stack_model
    target = ug.Target(torch, 64, 64)
    handles = {uc.WHITE: layer.add_texture(textures[uc.WHITE])}
    assert layer.record(target, (0, 0, 64, 64), CLEAR, uc.truncated(draw, n), handles) == abi.SZG_OK, lib().szg_last_error()
    check(target.read(), target.expect(snapshots[2 * n]))
    layer.remove_texture(handles[uc.WHITE])
    layer.keep.clear()


def test_the_reversed_stack_gives_other_bytes(torch, layer, stack_model):
    draw, textures, snapshots = stack_model
    got, want = ug.run_case(layer, ug.Target(torch, 64, 64), (0, 0, 64, 64), CLEAR, uc.reversed_stack(draw), textures)
    check(got, want)
    assert (got[26:38, 26:38] != snapshots[2 * 4097][26:38, 26:38]).any(axis=2).all()


# ---- drops and scissors: the cases of the CPU test ----
DROPS = uc.drop_cases()


@pytest.mark.parametrize("name,draw,textures,kept", DROPS, ids=[d[0] for d in DROPS])
def test_drops(torch, layer, name, draw, textures, kept):
    got, want = ug.run_case(layer, ug.Target(torch, 48, 32), (0, 0, 48, 32), CLEAR, draw, textures)
    check(got, want)
    for x, y in kept:
        assert got[y, x].tolist() != [0, 0, 0, 65535]


def test_a_triangle_at_the_guard_band_itself_still_draws(torch, layer):
    draw, textures = uc.triangles([[(10, 5), (1048576.0, 5), (20, 25)], [(-1048576.0, -1048576.0), (30, 2), (2, 30)]], (48, 32),
                                  col=ui.col32(90, 255, 30, 140))
    got, want = ug.run_case(layer, ug.Target(torch, 48, 32), (0, 0, 48, 32), CLEAR, draw, textures)
    check(got, want)
    assert (got[:32, :48] != [0, 0, 0, 65535]).any(axis=2).sum() > 300


@pytest.mark.parametrize("name,clip,cols,rows", uc.SCISSOR_CASES, ids=[c[0] for c in uc.SCISSOR_CASES])
def test_scissors(torch, layer, name, clip, cols, rows):
    draw, textures = uc.scissor_case(clip)
    got, want = ug.run_case(layer, ug.Target(torch, 40, 30), (0, 0, 40, 30), LOAD, draw, textures)
    check(got, want)


def test_display_pos_scale_and_an_empty_viewport(torch, layer):
    draw, textures = uc.rect(103, 52, 108, 56, (12, 8), col=ui.col32(255, 255, 255, 200))
    draw = draw._replace(display_pos=(100.0, 50.0), framebuffer_scale=(2.0, 2.0),
                         commands=[draw.commands[0]._replace(clip_rect=(100.0, 50.0, 112.0, 58.0))])
    for d in (draw, draw._replace(display_size=(0.0, 8.0)), draw._replace(framebuffer_scale=(1.5, 0.75))):
        got, want = ug.run_case(layer, ug.Target(torch, 30, 20), (3, 2, 15, 9), CLEAR, d, textures, clear=(0.25, 0.5, 0.75, 1.0))
        check(got, want)


# ---- nothing to draw ----
def test_a_command_without_elements_and_no_commands_at_all(torch, layer):
    draw, textures = uc.scissor_case((3.7, 2.2, 20.9, 11.5))
    empty = ui.FlatCmd(uc.everything((40, 30)), None, 0, 0, 0)
    with_empty = draw._replace(commands=[empty, draw.commands[0], empty, draw.commands[1], draw.commands[2], empty])
    got, want = ug.run_case(layer, ug.Target(torch, 40, 30), (0, 0, 40, 30), CLEAR, with_empty, textures)
    check(got, want)
    sentinel = ug.Target(torch, 40, 30)  # the same seed: what the draw gives without the empty commands
    check(got, sentinel.expect(um.render(sentinel.image0, (0, 0, 40, 30), CLEAR, ug.BLACK, draw, textures)))
    none = draw._replace(commands=[])
    for load_op in (CLEAR, LOAD):
        target = ug.Target(torch, 40, 30)
        got, want = ug.run_case(layer, target, (5, 3, 30, 20), load_op, none, textures, clear=(1.0, 0.5, 2.0, float("nan")))
        check(got, want)
        assert np.array_equal(got, target.buffer0) == (load_op == LOAD)
    # only commands without elements, and no vertex or index arrays at all
    nothing = ui.FlatDrawData((0.0, 0.0), (40.0, 30.0), (1.0, 1.0), np.zeros(0, ui.DRAW_VERT), np.zeros(0, np.uint16), [empty])
    got, want = ug.run_case(layer, ug.Target(torch, 40, 30), (0, 0, 40, 30), CLEAR, nothing, {})
    check(got, want)


def test_load_over_a_sentinel_destination_and_every_unorm16_code(torch, layer):
    """LOAD blends over what is there. The destination holds every UNORM16 code and so does the RGBA16 texture of the quad
    drawn over it at alpha 128 / 255: both conversions of the kernel see all 65 536 codes."""
    rng = np.random.default_rng(2)
    codes = np.arange(65536, dtype=np.uint16)
    dst = np.stack([rng.permutation(codes) for _ in range(4)], axis=1).reshape(128, 512, 4)
    tex = np.stack([rng.permutation(codes) for _ in range(4)], axis=1).reshape(128, 512, 4)
    textures = {"t": um.Texture(tex, um.NEAREST, um.CLAMP_TO_EDGE)}
    v = [(0, 0, 0, 0, ui.col32(255, 255, 255, 128)), (512, 0, 1, 0, ui.col32(255, 255, 255, 128)),
         (512, 128, 1, 1, ui.col32(255, 255, 255, 128)), (0, 128, 0, 1, ui.col32(255, 255, 255, 128))]
    draw = uc.flat(v, [0, 1, 2, 0, 2, 3], [((0, 0, 512, 128), "t", 0, 0, 6)], (512, 128))
    target = ug.Target(torch, 512, 128)
    target.reset(dst)
    got, want = ug.run_case(layer, target, (0, 0, 512, 128), LOAD, draw, textures)
    check(got, want)
    assert (got[:128, :512] != dst).any(axis=2).mean() > 0.99


# ---- sweeps ----
def test_random_sweep_of_4000_triangles(torch, layer):
    draw, textures = uc.random_sweep()
    count = np.zeros((256, 512), np.int64)
    target = ug.Target(torch, 512, 256)
    want_image = um.render(target.image0, (0, 0, 512, 256), CLEAR, ug.BLACK, draw, textures, coverage=count)
    assert 0.5 < count.mean() < 20, count.mean()  # not an empty frame
    got, want = ug.run_case(layer, target, (0, 0, 512, 256), CLEAR, draw, textures)
    assert np.array_equal(want[:256, :512], want_image)
    check(got, want)


def test_an_editor_like_frame_through_the_python_mirror(torch):
    """pipelines.UILayer as the editor uses it: the renderer draws into sceneTexture() (here one program of the compute
    collection), the frame is built with syzygy_amd.ui, recordDraw returns the output image and its rendered subregion."""
    from syzygy_amd import pipelines as pl

    capacity, content, size = (1024, 640), (900, 560), (1280, 720)
    layer = pl.UILayer.create((1280, 720), triangleCapacity=4096, commandCapacity=64)
    try:
        scene_texture = pl.SceneTexture(*capacity)
        collection = pl.ComputeCollectionPipeline()
        collection.selectShaderByName("matrix_color")
        collection.writeExampleValues()
        collection.recordDrawCommands(None, scene_texture, pl.rect(*content))
        scene = layer.addTexture(scene_texture.color, abi.SZG_FILTER_NEAREST, abi.SZG_UI_ADDRESS_CLAMP_TO_BORDER)
        white = layer.addTexture(torch.full((1, 1, 4), 255, dtype=torch.uint8, device="cuda"), abi.SZG_FILTER_LINEAR, abi.SZG_UI_ADDRESS_REPEAT)
        frame = uc.editor_frame(scene, white, capacity, content, size)
        out = layer.recordDraw(None, frame)
        assert (out.renderedSubregion.x, out.renderedSubregion.y, out.renderedSubregion.width, out.renderedSubregion.height) == (0, 0, 1280, 720)
        assert out.texture is layer.outputTexture()
        torch.cuda.synchronize()
        got = out.texture.color_numpy()
        textures = {scene: um.Texture(scene_texture.color_numpy(), um.NEAREST, um.CLAMP_TO_BORDER),
                    white: um.Texture(np.full((1, 1, 4), 255, np.uint8), um.LINEAR, um.REPEAT)}
        want = um.render(np.zeros((720, 1280, 4), np.uint16), (0, 0, 1280, 720), CLEAR, ug.BLACK, frame.flatten(), textures)
        check(got, want)
        # the viewport quad is 1:1: away from the overlay, the scene's opaque texels as they are
        texels = scene_texture.color_numpy()[300:560, 400:900]
        opaque = texels[..., 3] == 65535
        assert np.array_equal(got[30 + 300:30 + 560, 308 + 400:308 + 900][opaque], texels[opaque])
        collection.cleanup()
    finally:
        layer.cleanup()


def test_frame_loop_example_with_the_ui_layer_presents_the_output_image(torch):
    """examples/frame_loop.py --ui-layer: the scene is rendered into the layer's scene texture at the viewport window's extent
    and shown by a 1:1 quad, the OETF runs on the OUTPUT image. Inside the viewport the frame is therefore, bit for bit, the
    frame the example renders without the switch at that extent; around it are the title bar and the panel."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import frame_loop
    finally:
        sys.path.pop(0)
    W, H = 260, 144  # both this and the viewport extent, 196 x 110, have rows of a multiple of 16 bytes (szg_record_oetf)
    x0, y0 = max(W // 5, 8) + 6, 22 + 6  # the example's layout: panel, title bar, margins
    cw, ch = W - x0 - 6, H - y0 - 6
    out = frame_loop.main(["--frames", "2", "--width", str(W), "--height", str(H), "--shadow-map", "512", "--ui-layer"])
    plain = frame_loop.main(["--frames", "2", "--width", str(cw), "--height", str(ch), "--shadow-map", "512"])
    assert out.shape == (H, W, 4) and plain.shape == (ch, cw, 4)
    opaque = plain[..., 3] == 65535
    assert opaque.mean() > 0.9
    assert np.array_equal(out[y0:y0 + ch, x0:x0 + cw][opaque], plain[opaque])
    assert (out[..., 3] == 65535).all()  # over the opaque clear every blend keeps alpha at 1
    title, panel, margin = out[5, 128], out[100, 10], out[y0 + ch + 2, x0 + 20]
    assert title[2] > title[1] > title[0] > 0 and 0 < panel[0] < 65535 // 2 and margin.tolist() == [0, 0, 0, 65535]


# ---- the other library ----
def test_the_literal_library_gives_the_same_bytes(torch, layer):
    """The pass belongs to no contraction class: libszg_hip_literal.so, in a process of its own, produces the bytes of
    libszg_hip.so in this one."""
    here = child.digests(torch)
    env = dict(os.environ)
    env["SZG_HIP_LIBRARY"] = os.path.join(ROOT, "syzygy_amd", "csrc", "libszg_hip_literal.so")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_ui_layer_child.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().split("\n")[-1])
    assert out["library"] == "libszg_hip_literal.so"
    assert out["digests"] == here and len(here) == 3


# ---- refusals: nothing launched, nothing written ----
def test_refusals_write_nothing(torch, layer):
    draw, textures = uc.scissor_case((3.7, 2.2, 20.9, 11.5))
    target = ug.Target(torch, 40, 30)
    other = ug.Layer(torch, triangle_capacity=2, command_capacity=2)
    white = layer.add_texture(textures[uc.WHITE])
    foreign = other.add_texture(textures[uc.WHITE])
    handles = {uc.WHITE: white}
    full = (0, 0, 40, 30)
    INV, CAP = abi.SZG_ERR_INVALID_ARGUMENT, abi.SZG_ERR_CAPACITY

    def image(**kw):
        im = target.abi()
        for k, v in kw.items():
            setattr(im, k, v)
        return im

    def attempt(what, code, im=None, area=full, load_op=CLEAR, d=draw, h=handles, lay=layer, clear=ug.BLACK, patch=None):
        dd, keep = lay.draw_data(d, h)
        if patch:
            patch(dd)
        im = target.abi() if im is None else im
        cc = (C.c_float * 4)(*clear) if clear is not None else None
        rc = lib().szg_ui_layer_record_draw(lay.h, None, C.byref(im) if im is not False else None, abi.Rect(*area), load_op, cc, C.byref(dd))
        assert rc == code, (what, rc, lib().szg_last_error())
        assert len(lib().szg_last_error()) > 10, what
        assert np.array_equal(target.read(), target.buffer0), what

    attempt("NULL output", INV, im=False)
    attempt("NULL output data", INV, im=image(data=None))
    attempt("pitch below a row", INV, im=image(pitch_bytes=40 * 8 - 8))
    attempt("pitch not a multiple of 8", INV, im=image(pitch_bytes=43 * 8 + 4))
    attempt("misaligned data", INV, im=image(data=target.buffer.data_ptr() + 4))
    for fmt in (abi.SZG_FORMAT_RGBA16_SFLOAT, abi.SZG_FORMAT_RGBA8_UNORM, abi.SZG_FORMAT_UNDEFINED):
        attempt(f"output format {fmt}", INV, im=image(format=fmt))
    attempt("extent above the cap", INV, im=image(width=abi.SZG_PRESENT_MAX_EXTENT + 1, pitch_bytes=(abi.SZG_PRESENT_MAX_EXTENT + 1) * 8))
    for area in ((0, 0, 41, 30), (0, 0, 40, 31), (-1, 0, 10, 10), (0, -1, 10, 10), (35, 0, 6, 5), (0, 28, 5, 3)):
        attempt(f"render area {area}", INV, area=area)
    attempt("unknown load op", INV, load_op=2)
    attempt("NULL clear colour under CLEAR", INV, clear=None)
    attempt("foreign texture handle", INV, h={uc.WHITE: foreign})
    attempt("stale texture handle", INV, h={uc.WHITE: 0x1000})
    attempt("NULL texture with elements", INV, h={uc.WHITE: None})
    attempt("NULL command array", INV, patch=lambda dd: setattr(dd, "commands", None))
    attempt("NULL vertices", INV, patch=lambda dd: setattr(dd, "d_vertices", None))
    attempt("NULL indices", INV, patch=lambda dd: setattr(dd, "d_indices", None))
    for field in ("display_pos", "display_size", "framebuffer_scale"):
        for value in (float("nan"), float("inf"), -float("inf")):
            def patch(dd, field=field, value=value):
                getattr(dd, field)[1] = value
            attempt(f"{field} {value}", INV, patch=patch)
    # a texture whose memory overlaps the output image
    inside = abi.Image(target.buffer.data_ptr() + 43 * 8 * 4, 4, 4, 43 * 8, abi.SZG_FORMAT_RGBA16_UNORM)
    overlapping = C.c_void_p()
    assert lib().szg_ui_layer_add_texture(layer.h, C.byref(inside), abi.UISampler(0, 0), C.byref(overlapping)) == abi.SZG_OK
    attempt("texture overlapping the output", INV, h={uc.WHITE: overlapping.value})
    assert layer.remove_texture(overlapping.value) == abi.SZG_OK
    # capacities: 4 triangles in 3 commands against a layer of 2 and 2
    attempt("more commands than the capacity", CAP, lay=other, h={uc.WHITE: foreign})
    attempt("more triangles than the capacity", CAP, lay=other, h={uc.WHITE: foreign},
            d=draw._replace(commands=[ui.FlatCmd(uc.everything((40, 30)), uc.WHITE, 0, 0, 12)]))
    # textures: formats, samplers, malformed images, handles of another layer
    t8 = ug.to_device(torch, np.zeros((4, 4, 4), np.uint8))
    out = C.c_void_p()
    ok = abi.Image(t8.data_ptr(), 4, 4, 16, abi.SZG_FORMAT_RGBA8_UNORM)
    for what, im, sampler in (("format", abi.Image(t8.data_ptr(), 4, 2, 32, abi.SZG_FORMAT_RGBA16_SFLOAT), (0, 0)),
                              ("format", abi.Image(t8.data_ptr(), 4, 4, 16, abi.SZG_FORMAT_BGRA8_UNORM), (0, 0)),
                              ("filter", ok, (2, 0)), ("address", ok, (0, 1)), ("address", ok, (1, 4)),
                              ("NULL", abi.Image(None, 4, 4, 16, abi.SZG_FORMAT_RGBA8_UNORM), (0, 0)),
                              ("pitch", abi.Image(t8.data_ptr(), 4, 4, 12, abi.SZG_FORMAT_RGBA8_UNORM), (0, 0)),
                              ("extents", abi.Image(t8.data_ptr(), 0, 4, 16, abi.SZG_FORMAT_RGBA8_UNORM), (0, 0))):
        assert lib().szg_ui_layer_add_texture(layer.h, C.byref(im), abi.UISampler(*sampler), C.byref(out)) == INV, what
        assert what.encode() in lib().szg_last_error() and not out.value, (what, lib().szg_last_error())
    assert layer.remove_texture(foreign) == INV and layer.remove_texture(0x1000) == INV
    assert other.remove_texture(foreign) == abi.SZG_OK and other.remove_texture(foreign) == INV
    # and after all that the same call, unpatched, draws
    got, want = ug.run_case(layer, target, full, CLEAR, draw, textures)
    check(got, want)
    layer.remove_texture(white)
    other.destroy()
