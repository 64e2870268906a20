"""The UI layer pass's rules (include/szg/ui_layer.h) on the CPU: the numpy model of tests/ui_layer_model.py against the
properties the header claims (partition of the fill rule, scissor truncation, blend identities and hand-worked values,
submission order, the twelve samplers, the drops), its vectorised coverage against the brute per-pixel one, the draw-list
builder syzygy_amd/ui.py against ImGui's index patterns, and the C-ABI surface (exported, bound, versioned). No GPU needed."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from syzygy_amd import abi, lib, ui
from syzygy_amd._lib import library_path
from tests import ui_layer_cases as uc
from tests import ui_layer_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLACK = (0.0, 0.0, 0.0, 1.0)


def blank(size, value=0):
    return np.full((size[1], size[0], 4), value, np.uint16)


def draw_on(draw, textures, size=None, load_op=um.CLEAR, dst=None, **kw):
    size = size or (int(draw.display_size[0]), int(draw.display_size[1]))
    dst = blank(size) if dst is None else dst
    return um.render(dst, (0, 0, size[0], size[1]), load_op, BLACK, draw, textures, **kw)


def coverage_of(draw, textures, size=None):
    size = size or (int(draw.display_size[0]), int(draw.display_size[1]))
    count = np.zeros((size[1], size[0]), np.int64)
    draw_on(draw, textures, size, coverage=count)
    return count


# ---- the two coverage paths ----
def test_vectorised_and_brute_coverage_agree_on_a_random_scene():
    draw, textures = uc.random_sweep(seed=23, n_tris=300, size=(96, 64), n_cmds=6, big_fraction=0.04)
    ca, cb = np.zeros((64, 96), np.int64), np.zeros((64, 96), np.int64)
    a = draw_on(draw, textures, coverage=ca)
    b = draw_on(draw, textures, coverage=cb, brute=True)
    assert np.array_equal(ca, cb), np.argwhere(ca != cb)[:5]
    assert np.array_equal(a, b)
    assert ca.sum() > 1000 and ca.max() >= 3  # not an empty frame, and pixels that blend more than once


# ---- partition ----
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("corners", [(3, 2, 17, 11), (3.5, 2.5, 17.5, 11.5), (3, 2.5, 17.5, 11), (0, 0, 24, 16), (-4, -3.5, 5.5, 4)])
def test_a_filled_rect_covers_each_pixel_whose_centre_it_holds_exactly_once(corners, flip):
    x0, y0, x1, y1 = corners
    draw, tex = uc.rect(x0, y0, x1, y1, (24, 16), flip=flip)
    count = coverage_of(draw, tex)
    py, px = np.mgrid[0:16, 0:24]
    want = ((x0 <= px + 0.5) & (px + 0.5 < x1) & (y0 <= py + 0.5) & (py + 0.5 < y1)).astype(np.int64)
    assert np.array_equal(count, want)


@pytest.mark.parametrize("reverse", [False, True])
def test_123_fans_around_a_vertex_on_a_pixel_centre_hit_no_pixel_twice(reverse):
    for n in range(3, 126):
        draw, tex = uc.fan((16.5, 15.5), n, 11.3, (33, 31), reverse=reverse, phase=0.1 + 0.01 * n)
        count = coverage_of(draw, tex)
        assert count.max() == 1, (n, np.argwhere(count > 1)[:3])
        assert count[15, 16] == 1, n
        # the disc of radius 11.3 * cos(pi / n) - 1 around the centre lies inside the fan: no hole either
        py, px = np.mgrid[0:31, 0:33]
        inside = (px - 16) ** 2 + (py - 15) ** 2 <= (11.3 * np.cos(np.pi / n) - 1) ** 2
        assert (count[inside] == 1).all(), n


@pytest.mark.parametrize("flip_a", [False, True])
@pytest.mark.parametrize("flip_b", [False, True])
@pytest.mark.parametrize("edge", [((2.5, 2.5), (20.5, 20.5)), ((2.5, 10.5), (28.5, 10.5)), ((12.5, 1.5), (12.5, 22.5)), ((3.5, 20.5), (27.5, 4.5))])
def test_two_triangles_sharing_an_edge_through_pixel_centres_hit_each_centre_once(edge, flip_a, flip_b):
    p, q = edge
    # apexes on either side of the edge
    d = np.array([q[0] - p[0], q[1] - p[1]], float)
    nrm = np.array([-d[1], d[0]]) / np.hypot(*d)
    mid = (np.array(p) + np.array(q)) / 2
    a, b = tuple(mid + 9.25 * nrm), tuple(mid - 7.75 * nrm)
    ta = (p, q, a) if not flip_a else (q, p, a)
    tb = (q, p, b) if not flip_b else (p, q, b)
    draw, tex = uc.triangles([ta, tb], (32, 24))
    count = coverage_of(draw, tex)
    assert count.max() == 1
    # the pixel centres on the open edge
    n = int(max(abs(q[0] - p[0]), abs(q[1] - p[1])))
    on_edge = [(Fraction(p[0]) + Fraction(k, n) * Fraction(q[0] - p[0]), Fraction(p[1]) + Fraction(k, n) * Fraction(q[1] - p[1])) for k in range(1, n)]
    centres = [(int(x - Fraction(1, 2)), int(y - Fraction(1, 2))) for x, y in on_edge if (x - Fraction(1, 2)).denominator == 1 and (y - Fraction(1, 2)).denominator == 1]
    assert len(centres) >= 5
    for x, y in centres:
        assert count[y, x] == 1, (x, y)


# ---- scissor ----
@pytest.mark.parametrize("name,clip,cols,rows", uc.SCISSOR_CASES, ids=[c[0] for c in uc.SCISSOR_CASES])
def test_scissor_truncates_as_the_backend_does(name, clip, cols, rows):
    draw, tex = uc.scissor_case(clip)
    assert (um.scissor(clip, draw) is None) == (cols is None)
    count = np.zeros((30, 40), np.int64)
    draw_on(draw, tex, coverage=count)
    # without the two small triangles of the neighbouring commands
    only = draw._replace(commands=[draw.commands[1]])
    got = coverage_of(only, tex)
    want = np.zeros((30, 40), np.int64)
    if cols is not None:
        want[rows[0]:rows[1] + 1, cols[0]:cols[1] + 1] = 1
    assert np.array_equal(got, want)
    neighbours = coverage_of(draw._replace(commands=[draw.commands[0], draw.commands[2]]), tex)
    assert neighbours.sum() > 20 and np.array_equal(count, got + neighbours)


# ---- blend ----
def test_alpha_zero_keeps_every_destination_code():
    dst = np.arange(65536, dtype=np.uint16).reshape(64, 256, 4)[:, :, [0, 2, 1, 3]].copy()
    # vertex alpha 0 is culled by ImGui's builder, not by the pass: hand the vertices over directly
    draw, tex = uc.rect(0, 0, 256, 64, (256, 64), col=ui.col32(255, 17, 99, 0))
    count = np.zeros((64, 256), np.int64)
    out = draw_on(draw, tex, load_op=um.LOAD, dst=dst, coverage=count)
    assert (count == 1).all() and np.array_equal(out, dst)


def test_white_times_texel_at_alpha_one_reproduces_every_code_and_the_1_to_1_quad_lands_in_its_texel():
    # capacity 64x48, content 37x29 (statelesswidgets.cpp:868-885: uv_max = content / capacity); every code appears in the
    # content region over the four channels of a few such textures; alpha stays 65535
    codes = np.arange(65536, dtype=np.uint32)
    seen = np.zeros(65536, bool)
    for k in range(0, 65536, 37 * 29 * 3):
        chunk = np.resize(codes[k:k + 37 * 29 * 3], 37 * 29 * 3).reshape(29, 37, 3)
        scene = np.full((48, 64, 4), 12345, np.uint16)
        scene[:29, :37, :3] = chunk
        scene[:29, :37, 3] = 65535
        tex = {"scene": um.Texture(scene, um.NEAREST, um.CLAMP_TO_BORDER)}
        for origin in ((0, 0), (11, 6)):
            ox, oy = origin
            v = [(ox, oy, 0, 0, uc.OPAQUE), (ox + 37, oy, 37 / 64, 0, uc.OPAQUE), (ox + 37, oy + 29, 37 / 64, 29 / 48, uc.OPAQUE),
                 (ox, oy + 29, 0, 29 / 48, uc.OPAQUE)]
            draw = uc.flat(v, [0, 1, 2, 0, 2, 3], [((0, 0, 64, 48), "scene", 0, 0, 6)], (64, 48))
            out = draw_on(draw, tex, dst=blank((64, 48), 777), load_op=um.LOAD)
            assert np.array_equal(out[oy:oy + 29, ox:ox + 37], scene[:29, :37])
            rest = out.copy()
            rest[oy:oy + 29, ox:ox + 37] = 777
            assert (rest == 777).all()
        seen[chunk.reshape(-1)] = True
    assert seen.all()


def test_three_blends_worked_by_hand():
    def blend(dst, col):
        draw, tex = uc.rect(0, 0, 2, 2, (2, 2), col=col)
        return draw_on(draw, tex, load_op=um.LOAD, dst=np.tile(np.array(dst, np.uint16), (2, 2, 1)))[0, 0].tolist()

    # 1. white at alpha 128 / 255 over the cleared (0, 0, 0, 1): alpha = RN(128 / 255) = 8421505 / 2^24. rgb' = 1 * alpha + 0 *
    #    (1 - alpha) = alpha; alpha * 65535 = 32896.0019..., rounds to code 32896 (= 128 * 257). 1 - alpha = 8355711 / 2^24 is
    #    exact, so a' = alpha + 1 * (1 - alpha) = 1 exactly: code 65535.
    assert blend((0, 0, 0, 65535), ui.col32(255, 255, 255, 128)) == [32896, 32896, 32896, 65535]
    # 2. opaque green over opaque red: alpha = 1, 1 - alpha = 0: rgb' = (0 * 1 + 1 * 0, 1 * 1 + 0 * 0, 0), a' = 1 + 1 * 0.
    assert blend((65535, 0, 0, 65535), ui.col32(0, 255, 0, 255)) == [0, 65535, 0, 65535]
    # 3. black at alpha 51 / 255 over opaque white: alpha = RN(0.2) = 13421773 / 2^26 = 0.2000000030; 1 - alpha = 0.7999999970
    #    rounds to RN(0.8) = 13421773 / 2^24 = 0.8000000119 (the neighbour below is 4.5e-8 away, this one 1.5e-8). rgb' = 0 *
    #    alpha + 1 * 0.8000000119; * 65535 = 52428.0008, code 52428. a' = 0.2000000030 + 0.8000000119 = 1.0000000149, which
    #    rounds to 1 (half a step above 1 is 5.96e-8): code 65535.
    assert blend((65535, 65535, 65535, 65535), ui.col32(0, 0, 0, 51)) == [52428, 52428, 52428, 65535]


# ---- order ----
def test_two_overlapping_translucent_triangles_depend_on_their_order():
    a, b = [(2, 2), (28, 4), (6, 22)], [(4, 3), (30, 20), (3, 18)]
    cols = [ui.col32(255, 40, 10, 150), ui.col32(10, 60, 255, 90)]
    d1, tex = uc.triangles([a, b], (32, 24), cols=cols)
    d2, _ = uc.triangles([b, a], (32, 24), cols=cols[::-1])
    o1, o2 = draw_on(d1, tex), draw_on(d2, tex)
    both = (coverage_of(d1, tex) == 2)
    assert both.sum() > 50 and (o1[both] != o2[both]).any(axis=1).all()
    assert np.array_equal(o1[~both], o2[~both])


@pytest.fixture(scope="module")
def stack_images():
    draw, tex = uc.stack()
    sizes = (1, 63, 64, 65, 4095, 4096, 4097)
    _, forward = draw_on(draw, tex, snapshots={2 * n for n in sizes})
    backward = draw_on(uc.reversed_stack(draw), tex)
    return draw, tex, forward, backward


def test_a_stack_of_4097_quads_differs_from_the_reversed_stack(stack_images):
    draw, tex, forward, backward = stack_images
    final = forward[2 * 4097]
    inside = np.zeros((64, 64), bool)
    inside[26:38, 26:38] = True
    assert (final[inside] != backward[inside]).any(axis=1).all()
    assert np.array_equal(final[~inside], backward[~inside]) and (final[~inside] == [0, 0, 0, 65535]).all()
    # every pixel of the stack holds one value: the quads are axis-aligned and the colours constant
    assert len(np.unique(final[inside], axis=0)) == 1
    # and the prefixes the GPU test records one by one are the snapshots, each different from the next
    for n in (1, 63, 64, 65, 4095, 4096, 4097):
        alone = draw_on(uc.truncated(draw, n), tex) if n <= 65 else None
        assert alone is None or np.array_equal(alone, forward[2 * n])
    assert not np.array_equal(forward[2 * 4096], forward[2 * 4097])


# ---- samplers ----
def exact_texel(tex, i, j):
    h, w = tex.data.shape[:2]
    top = 65535 if tex.data.dtype == np.uint16 else 255
    if tex.address == um.REPEAT:
        i, j = i % w, j % h
    elif tex.address == um.CLAMP_TO_EDGE:
        i, j = min(max(i, 0), w - 1), min(max(j, 0), h - 1)
    elif not (0 <= i < w and 0 <= j < h):
        return np.array([0.0, 0.0, 0.0, 1.0])
    return tex.data[j, i].astype(np.float64) / top


@pytest.mark.parametrize("filt,address,dtype", uc.SAMPLER_COMBOS)
def test_the_twelve_samplers_against_binary64(filt, address, dtype):
    tex = um.Texture(uc.sampler_texture(dtype), filt, address)
    rng = np.random.default_rng(1)
    u = rng.uniform(-1.7, 2.6, 400).astype(np.float32)
    v = rng.uniform(-1.4, 2.9, 400).astype(np.float32)
    got = um.sample(tex, u, v)
    for k in range(len(u)):
        x, y = float(u[k]) * 9, float(v[k]) * 7
        if filt == um.NEAREST:
            if min(abs(x - round(x)), abs(y - round(y))) < 1e-4:
                continue  # too close to a texel boundary for binary64 to name the texel of the fp32 product
            want = exact_texel(tex, int(np.floor(x)), int(np.floor(y)))
            assert np.array_equal(got[k], np.float32(want)), k
        else:
            x, y = x - 0.5, y - 0.5
            i, j = int(np.floor(x)), int(np.floor(y))
            a, b = x - i, y - j
            if min(a, 1 - a, b, 1 - b) < 1e-4:
                continue
            want = ((1 - b) * ((1 - a) * exact_texel(tex, i, j) + a * exact_texel(tex, i + 1, j))
                    + b * ((1 - a) * exact_texel(tex, i, j + 1) + a * exact_texel(tex, i + 1, j + 1)))
            assert np.abs(got[k] - want).max() < 4e-6, k


@pytest.mark.parametrize("filt", [um.NEAREST, um.LINEAR])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_the_border_is_opaque_black(filt, dtype):
    tex = um.Texture(uc.sampler_texture(dtype), filt, um.CLAMP_TO_BORDER)
    u = np.array([-0.5, 1.5, 0.5, 0.5, 3.0, np.nan, np.inf], np.float32)
    v = np.array([0.5, 0.5, -0.3, 1.4, -2.0, 0.5, 0.5], np.float32)
    got = um.sample(tex, u, v)
    assert np.array_equal(got[:5], np.tile(np.array([0, 0, 0, 1], np.float32), (5, 1)))
    if filt == um.NEAREST:
        assert np.array_equal(got[5:], np.tile(np.array([0, 0, 0, 1], np.float32), (2, 1)))


@pytest.mark.parametrize("filt,address,dtype", uc.SAMPLER_COMBOS)
def test_sampler_cases_draw_something_everywhere(filt, address, dtype):
    draw, tex = uc.sampler_case(filt, address, dtype)
    count = coverage_of(draw, tex)
    assert count[2:33, 3:44].min() == 1 and count.max() == 2
    out = draw_on(draw, tex)
    assert len(np.unique(out.reshape(-1, 4), axis=0)) > 20


# ---- drops ----
DROPS = uc.drop_cases()


@pytest.mark.parametrize("name,draw,tex,kept", DROPS, ids=[d[0] for d in DROPS])
def test_dropped_triangles_draw_nothing_and_their_neighbours_still_draw(name, draw, tex, kept):
    good, _ = uc.triangles([[(2, 2), (14, 3), (5, 13)], [(30, 15), (45, 18), (34, 30)]], (48, 32), col=ui.col32(255, 200, 100, 200))
    want = draw_on(good, tex)
    got = draw_on(draw, tex)
    assert np.array_equal(got, want)
    for x, y in kept:
        assert got[y, x].tolist() != [0, 0, 0, 65535]


def test_a_triangle_at_the_guard_band_itself_still_draws():
    draw, tex = uc.triangles([[(10, 5), (1048576.0, 5), (20, 25)]], (48, 32))
    assert coverage_of(draw, tex).sum() > 100
    draw, tex = uc.triangles([[(10, 5), (1048576.125, 5), (20, 25)]], (48, 32))
    assert coverage_of(draw, tex).sum() == 0


def test_viewport_render_area_and_display_pos():
    # display_pos (100, 50) at scale 2: the rect (103, 52)-(108, 56) lands on pixels 6..15 x 4..11; the viewport is
    # (0, 0, 24, 16) whatever the render area's offset is, and the render area (3, 2) 15x9 cuts it
    draw, tex = uc.rect(103, 52, 108, 56, (12, 8))
    draw = draw._replace(display_pos=(100.0, 50.0), framebuffer_scale=(2.0, 2.0),
                         commands=[draw.commands[0]._replace(clip_rect=(100.0, 50.0, 112.0, 58.0))])
    assert um.framebuffer_extent(draw) == (24, 16)
    dst = blank((30, 20), 4242)
    out = um.render(dst, (3, 2, 15, 9), um.CLEAR, (0.25, 0.5, 0.75, 1.0), draw, tex)
    want = dst.copy()
    want[2:11, 3:18] = um.unorm16_store(np.array([0.25, 0.5, 0.75, 1.0], np.float32))
    want[4:11, 6:16] = 65535
    assert np.array_equal(out, want)
    # fbw <= 0: the clear still happens and nothing is drawn
    out = um.render(dst, (3, 2, 15, 9), um.CLEAR, (0.25, 0.5, 0.75, 1.0), draw._replace(display_size=(0.0, 8.0)), tex)
    want[4:11, 6:16] = want[2, 3]
    assert np.array_equal(out, want)


# ---- the builder ----
def test_the_builder_emits_imguis_index_pattern_and_command_splits():
    dl = ui.DrawList("font", uv_white=(0.25, 0.75))
    dl.add_rect_filled((1, 2), (5, 7), ui.col32(1, 2, 3, 4))
    dl.add_triangle_filled((0, 0), (4, 0), (0, 4), 0xFF0000FF)
    dl.add_image("scene", (10, 10), (20, 30), (0.0, 0.0), (0.5, 0.25))
    dl.add_rect_filled((0, 0), (1, 1), 0xFFFFFFFF)
    dl.push_clip_rect((2, 3), (9, 8))
    dl.push_clip_rect((0, 0), (4, 20), True)  # intersected: (2, 3, 4, 8)
    dl.add_rect_filled((0, 0), (1, 1), 0xFFFFFFFF)
    dl.pop_clip_rect()
    dl.pop_clip_rect()  # two changes over an empty command: it is rewritten, then merged away
    dl.add_rect_filled((0, 0), (1, 1), 0x00FFFFFF)  # alpha 0: ImGui adds nothing
    assert dl.IdxBuffer.tolist() == [0, 1, 2, 0, 2, 3, 4, 5, 6, 7, 8, 9, 7, 9, 10, 11, 12, 13, 11, 13, 14, 15, 16, 17, 15, 17, 18]
    v = dl.VtxBuffer
    assert v["pos"][:4].tolist() == [[1, 2], [5, 2], [5, 7], [1, 7]] and (v["uv"][:7] == [0.25, 0.75]).all()
    assert v["col"][0] == 0x04030201
    assert v["pos"][7:11].tolist() == [[10, 10], [20, 10], [20, 30], [10, 30]]
    assert v["uv"][7:11].tolist() == [[0, 0], [0.5, 0], [0.5, 0.25], [0, 0.25]]
    full = (-8192.0, -8192.0, 8192.0, 8192.0)
    got = [(c.ClipRect, c.TextureId, c.IdxOffset, c.ElemCount) for c in dl.CmdBuffer]
    assert got == [(full, "font", 0, 9), (full, "scene", 9, 6), (full, "font", 15, 6), ((2.0, 3.0, 4.0, 8.0), "font", 21, 6)] or \
        got == [(full, "font", 0, 9), (full, "scene", 9, 6), (full, "font", 15, 6), ((2.0, 3.0, 4.0, 8.0), "font", 21, 6),
                (full, "font", 27, 0)]
    # two lists: global offsets as ImGui_ImplVulkan_RenderDrawData adds them; a UserCallback is skipped
    other = ui.DrawList("font")
    other.add_rect_filled((0, 0), (2, 2), 0xFFFFFFFF)
    other.CmdBuffer[0].UserCallback = None
    cb = ui.DrawList("font")
    cb.add_rect_filled((0, 0), (2, 2), 0xFFFFFFFF)
    cb.CmdBuffer[0].UserCallback = object()
    flat = ui.DrawData((0, 0), (64, 64), (1, 1), [dl, cb, other]).flatten()
    assert len(flat.vertices) == 19 + 4 + 4 and len(flat.indices) == 27 + 6 + 6
    assert (flat.commands[-1].vtx_offset, flat.commands[-1].idx_offset, flat.commands[-1].elem_count) == (23, 33, 6)
    assert all(c.vtx_offset == 0 for c in flat.commands[:-1]) and len([c for c in flat.commands if c.elem_count]) == 5
    # more than 65535 vertices: a new command with a VtxOffset, indices restart
    big = ui.DrawList("font")
    for _ in range(16384):
        big.add_rect_filled((0, 0), (1, 1), 0xFFFFFFFF)
    assert [(c.VtxOffset, c.IdxOffset, c.ElemCount) for c in big.CmdBuffer] == [(0, 0, 6 * 16383), (65532, 6 * 16383, 6)]
    assert big.IdxBuffer[-6:].tolist() == [0, 1, 2, 0, 2, 3] and big.IdxBuffer.max() == 65531


# ---- the C-ABI surface ----
def test_ui_layer_header_is_exported_bound_and_versioned():
    text = open(os.path.join(ROOT, "include", "szg", "ui_layer.h")).read()
    names = sorted(set(re.findall(r"\b(szg_ui_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert names == sorted(abi.UI_LAYER_FUNCTIONS) and len(names) == 5
    handle = C.CDLL(library_path())
    for name in names:
        assert hasattr(handle, name)
    assert lib().szg_abi_version() == abi.SZG_ABI_VERSION == 2
    for macro in ("SZG_UI_ADDRESS_REPEAT", "SZG_UI_ADDRESS_CLAMP_TO_EDGE", "SZG_UI_ADDRESS_CLAMP_TO_BORDER", "SZG_UI_LOAD_OP_LOAD",
                  "SZG_UI_LOAD_OP_CLEAR", "SZG_UI_GUARD_BAND"):
        m = re.search(rf"#define {macro} ([0-9.]+)", text)
        assert m and float(m.group(1)) == getattr(abi, macro), macro
    assert (C.sizeof(abi.UIDrawVert), C.sizeof(abi.UIDrawCmd), C.sizeof(abi.UIDrawData)) == (20, 40, 72)
    assert ui.DRAW_VERT.itemsize == C.sizeof(abi.UIDrawVert)
    # both libraries carry the pass
    literal = os.path.join(os.path.dirname(library_path()), "libszg_hip_literal.so")
    if os.path.exists(literal):
        assert hasattr(C.CDLL(literal), "szg_ui_layer_record_draw")


def test_refusals_that_need_no_device():
    h = C.c_void_p()
    for tris, cmds in ((0, 8), (abi.SZG_UI_MAX_TRIANGLE_CAPACITY + 1, 8), (8, 0), (8, abi.SZG_UI_MAX_COMMAND_CAPACITY + 1)):
        assert lib().szg_ui_layer_create(C.byref(h), tris, cmds, 0) == abi.SZG_ERR_INVALID_ARGUMENT
        assert b"capacity" in lib().szg_last_error() and not h.value
    assert lib().szg_ui_layer_create(None, 8, 8, 0) == abi.SZG_ERR_INVALID_ARGUMENT
    assert lib().szg_ui_layer_record_draw(None, None, None, abi.Rect(0, 0, 8, 8), abi.SZG_UI_LOAD_OP_CLEAR, None, None) == \
        abi.SZG_ERR_INVALID_ARGUMENT
    assert lib().szg_ui_layer_add_texture(None, None, abi.UISampler(0, 0), None) == abi.SZG_ERR_INVALID_ARGUMENT
    assert lib().szg_ui_layer_remove_texture(None, None) == abi.SZG_ERR_INVALID_ARGUMENT
    lib().szg_ui_layer_destroy(None)
