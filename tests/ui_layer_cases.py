"""Draw data for the UI layer tests, shared by the CPU tests of the model (tests/test_ui_layer_model.py) and the GPU tests of the
kernels against it (tests/test_gpu_ui_layer.py): the same cases run on both sides. Every builder returns (draw, textures):
a ui.FlatDrawData whose commands name keys of `textures` (a dict key -> ui_layer_model.Texture)."""
import numpy as np

from syzygy_amd import ui
from tests import ui_layer_model as um

WHITE = "white"
OPAQUE = 0xFFFFFFFF


def white_texture():
    return um.Texture(np.full((1, 1, 4), 255, np.uint8), um.NEAREST, um.REPEAT)


def flat(vertices, indices, commands, display_size, display_pos=(0.0, 0.0), scale=(1.0, 1.0)):
    """vertices: rows (x, y, u, v, col); commands: (clip_rect, texture, vtx_offset, idx_offset, elem_count)"""
    v = np.zeros(len(vertices), ui.DRAW_VERT)
    for dst, row in zip(v, vertices):
        dst["pos"], dst["uv"], dst["col"] = row[0:2], row[2:4], int(row[4])
    return ui.FlatDrawData(tuple(map(float, display_pos)), tuple(map(float, display_size)), tuple(map(float, scale)), v,
                           np.asarray(indices, np.uint16), [ui.FlatCmd(tuple(map(float, c[0])), *c[1:]) for c in commands])


def everything(display_size):
    return (0.0, 0.0, float(display_size[0]), float(display_size[1]))


def triangles(tris, display_size, col=OPAQUE, clip=None, cols=None):
    """One command of white-textured triangles given as three (x, y) each."""
    vertices, indices = [], []
    for n, t in enumerate(tris):
        c = col if cols is None else cols[n]
        for p in t:
            indices.append(len(vertices))
            vertices.append((p[0], p[1], 0.5, 0.5, c))
    cmd = (clip or everything(display_size), WHITE, 0, 0, len(indices))
    return flat(vertices, indices, [cmd], display_size), {WHITE: white_texture()}


def rect(x0, y0, x1, y1, display_size, flip=False, col=OPAQUE, clip=None):
    """A filled rectangle as ImGui draws it (PrimRect: indices 0 1 2, 0 2 3); `flip` mirrors it: the other winding."""
    corners = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    if flip:
        corners = [(x1, y0), (x0, y0), (x0, y1), (x1, y1)]
    vertices = [(x, y, 0.5, 0.5, col) for x, y in corners]
    cmd = (clip or everything(display_size), WHITE, 0, 0, 6)
    return flat(vertices, [0, 1, 2, 0, 2, 3], [cmd], display_size), {WHITE: white_texture()}


def fan(center, n, radius, display_size, reverse=False, phase=0.1):
    """n consistently wound triangles around `center`"""
    ang = phase + np.arange(n + 1) * (2 * np.pi / n)
    ring = [(center[0] + radius * np.cos(a), center[1] + radius * np.sin(a)) for a in ang]
    tris = [(center, ring[i], ring[i + 1]) for i in range(n)]
    if reverse:
        tris = [(a, c, b) for a, b, c in tris]
    return triangles(tris, display_size, col=ui.col32(255, 255, 255, 128))


# SCISSOR: (name, clip rect, columns admitted, rows admitted) on a 40x30 frame; None: the command is skipped
SCISSOR_CASES = [
    ("truncation", (3.7, 2.2, 20.9, 11.5), (3, 19), (2, 10)),
    ("outside", (50.0, 40.0, 60.0, 50.0), None, None),
    ("max_below_min", (20.0, 5.0, 10.0, 25.0), None, None),
    ("max_equals_min", (5.0, 7.0, 30.0, 7.0), None, None),
    ("negative_min", (-5.5, -2.0, 6.5, 4.25), (0, 5), (0, 3)),
    # cmax is clamped to 40, w = (uint32)(40 - 31.5) = 8: column 39 stays outside, as with the backend
    ("beyond_frame", (31.5, 20.5, 100.0, 100.0), (31, 38), (20, 28)),
    ("nan", (float("nan"), 0.0, 10.0, 10.0), None, None),
]


def scissor_case(clip):
    """A translucent rectangle over the whole 40x30 frame under `clip`, between two small triangles under the full clip."""
    size = (40, 30)
    col = ui.col32(200, 100, 50, 180)
    quad = [(-2, -2), (44, -2), (44, 33), (-2, 33)]
    vertices = [(1, 1, .5, .5, OPAQUE), (4, 1, .5, .5, OPAQUE), (1, 4, .5, .5, OPAQUE)]
    vertices += [(x, y, .5, .5, col) for x, y in quad]
    vertices += [(30, 20, .5, .5, col), (38, 21, .5, .5, col), (33, 28, .5, .5, col)]
    indices = [0, 1, 2, 3, 4, 5, 3, 5, 6, 7, 8, 9]
    cmds = [(everything(size), WHITE, 0, 0, 3), (clip, WHITE, 0, 3, 6), (everything(size), WHITE, 0, 9, 3)]
    return flat(vertices, indices, cmds, size), {WHITE: white_texture()}


def drop_cases():
    """(name, draw, textures, kept): triangle 1 of three must draw nothing; `kept` are pixels inside triangles 0 and 2."""
    size = (48, 32)
    good0 = [(2, 2), (14, 3), (5, 13)]
    good2 = [(30, 15), (45, 18), (34, 30)]
    nan, inf = float("nan"), float("inf")
    bad = {
        "det_zero": [(10, 10), (20, 20), (30, 30)],
        "repeated_vertex": [(10, 10), (10, 10), (30, 12)],
        "nan": [(10, nan), (40, 5), (20, 25)],
        "inf": [(10, 5), (inf, 5), (20, 25)],
        "minus_inf": [(10, 5), (40, 5), (20, -inf)],
        "guard_band": [(10, 5), (1048577.0, 5), (20, 25)],
        "guard_band_negative": [(10, 5), (40, -1048580.0), (20, 25)],
    }
    out = []
    kept = [(6, 5), (36, 20)]
    for name, t in bad.items():
        draw, tex = triangles([good0, t, good2], size, col=ui.col32(255, 200, 100, 200))
        out.append((name, draw, tex, kept))
    # an index >= vertex_count drops its triangle
    draw, tex = triangles([good0, [(10, 5), (40, 5), (20, 25)], good2], size, col=ui.col32(255, 200, 100, 200))
    idx = draw.indices.copy()
    idx[4] = 9
    out.append(("index_past_vertex_count", draw._replace(indices=idx), tex, kept))
    # vtx_offset pushes one index past the end
    draw2 = draw._replace(commands=[ui.FlatCmd(everything(size), WHITE, 0, 0, 3), ui.FlatCmd(everything(size), WHITE, 7, 3, 3),
                                    ui.FlatCmd(everything(size), WHITE, 0, 6, 3)])
    out.append(("vtx_offset_past_vertex_count", draw2, tex, kept))
    # a trailing partial triangle: 8 of the 9 indices
    draw3 = draw._replace(commands=[ui.FlatCmd(everything(size), WHITE, 0, 0, 3), ui.FlatCmd(everything(size), WHITE, 0, 6, 3),
                                    ui.FlatCmd(everything(size), WHITE, 0, 3, 2)])
    out.append(("trailing_partial_triangle", draw3, tex, kept))
    # an index range reaching past index_count is truncated: 9 + 3 asked for, 9 there
    draw4 = draw._replace(commands=[ui.FlatCmd(everything(size), WHITE, 0, 0, 3), ui.FlatCmd(everything(size), WHITE, 0, 6, 6),
                                    ui.FlatCmd(everything(size), WHITE, 0, 9, 3), ui.FlatCmd(everything(size), WHITE, 0, 4000, 3)])
    out.append(("range_past_index_count", draw4, tex, kept))
    return out


def stack(n_quads=4097, seed=7):
    """The blend-order stack: n translucent quads covering pixels 26..37 in x and y of a 64x64 frame, pseudo-random colours,
    alpha in (0.05, 0.95). Returns (draw, textures); the first k quads are the first 2k triangles."""
    rng = np.random.default_rng(seed)
    dl = ui.DrawList(WHITE)
    rgb = rng.integers(0, 256, (n_quads, 3))
    alpha = rng.integers(13, 243, n_quads)  # 13 / 255 > 0.05, 242 / 255 < 0.95
    for c, a in zip(rgb, alpha):
        dl.add_rect_filled((26, 26), (38, 38), ui.col32(c[0], c[1], c[2], a))
    return ui.DrawData((0, 0), (64, 64), (1, 1), [dl]).flatten(), {WHITE: white_texture()}


def truncated(draw, n_quads):
    """The stack's first n quads as a draw of their own (same buffers, a shorter command)."""
    c = draw.commands[0]
    return draw._replace(commands=[c._replace(elem_count=6 * n_quads)])


def reversed_stack(draw):
    idx = draw.indices.reshape(-1, 6)[::-1].reshape(-1).copy()
    return draw._replace(indices=idx)


SAMPLER_COMBOS = [(f, a, d) for f in (um.NEAREST, um.LINEAR) for a in (um.REPEAT, um.CLAMP_TO_EDGE, um.CLAMP_TO_BORDER)
                  for d in (np.uint8, np.uint16)]


def sampler_texture(dtype, seed=3):
    """9x7 texels of random codes (alpha included)"""
    rng = np.random.default_rng(seed)
    top = 256 if dtype == np.uint8 else 65536
    return rng.integers(0, top, (7, 9, 4)).astype(dtype)


def sampler_case(filt, address, dtype):
    """A 41x31 quad on a 48x36 frame whose UVs run from below 0 to above 1 on both axes, and a second one, rotated, with a
    tinted vertex colour; one texture of 9x7 texels under the given sampler."""
    size = (48, 36)
    tex = um.Texture(sampler_texture(dtype), filt, address)
    tint = ui.col32(255, 128, 64, 200)
    vertices = [(3, 2, -0.7, -0.45, OPAQUE), (44, 2, 1.6, -0.45, OPAQUE), (44, 33, 1.6, 1.8, OPAQUE), (3, 33, -0.7, 1.8, OPAQUE),
                (10, 5, 2.5, -1.25, tint), (40, 12, -1.5, 0.25, OPAQUE), (30, 30, 0.5, 3.0, tint)]
    indices = [0, 1, 2, 0, 2, 3, 4, 5, 6]
    return flat(vertices, indices, [(everything(size), "t", 0, 0, 9)], size), {"t": tex}


def random_sweep(seed=11, n_tris=4000, size=(512, 256), n_cmds=40, big_fraction=0.01):
    """4000 triangles in 40 commands with random clip rects, three textures and both windings; 99 % have an extent of at most
    12 px, the rest reach up to twice the frame."""
    rng = np.random.default_rng(seed)
    W, H = size
    textures = {
        "font": um.Texture(rng.integers(0, 256, (16, 16, 4)).astype(np.uint8), um.LINEAR, um.REPEAT),
        "map": um.Texture(rng.integers(0, 256, (13, 10, 4)).astype(np.uint8), um.NEAREST, um.CLAMP_TO_EDGE),
        "scene": um.Texture(rng.integers(0, 65536, (24, 40, 4)).astype(np.uint16), um.NEAREST, um.CLAMP_TO_BORDER),
    }
    keys = list(textures)
    vertices, indices, commands = [], [], []
    per = n_tris // n_cmds
    for c in range(n_cmds):
        base = len(vertices)
        first = len(indices)
        for t in range(per):
            big = rng.random() < big_fraction
            ext = rng.uniform(2.0, 12.0) if not big else rng.uniform(0.3, 2.0) * W
            cx, cy = rng.uniform(-8, W + 8), rng.uniform(-8, H + 8)
            pts = np.stack([cx + rng.uniform(-0.5, 0.5, 3) * ext, cy + rng.uniform(-0.5, 0.5, 3) * ext], axis=1)
            if rng.random() < 0.3:
                pts = np.round(pts * 2) / 2  # vertices on pixel centres and corners: the ties of the fill rule
            if rng.random() < 0.5:
                pts = pts[::-1]
            for p in pts:
                col = int(rng.integers(0, 2 ** 32))
                if big:
                    col = (col & 0x00FFFFFF) | (int(rng.integers(8, 64)) << 24)
                indices.append(len(vertices) - base)
                vertices.append((p[0], p[1], rng.uniform(-0.5, 1.5), rng.uniform(-0.5, 1.5), col))
        if c % 5 == 0:
            clip = everything(size)
        else:
            x0, y0 = rng.uniform(-20, W * 0.7), rng.uniform(-20, H * 0.7)
            clip = (x0, y0, x0 + rng.uniform(20, W), y0 + rng.uniform(20, H))
        commands.append((clip, keys[c % 3], base, first, 3 * per))
    return flat(vertices, indices, commands, size), textures


def editor_frame(scene_handle, white_handle, capacity, content, size=(1280, 720)):
    """An editor-like frame built with syzygy_amd.ui: a translucent side panel, a title bar, the scene viewport quad at the
    editor's UVs (content / capacity), and a frame-time graph of filled rectangles. Returns the ui.DrawData."""
    W, H = size
    dl = ui.DrawList(white_handle)
    dl.add_rect_filled((0, 0), (W, H), ui.col32(30, 30, 34, 255))  # the background window
    dl.add_rect_filled((0, 0), (W, 22), ui.col32(41, 74, 122, 255))  # title bar
    panel_w = 300
    vx0, vy0 = panel_w + 8, 30
    dl.add_image(scene_handle, (vx0, vy0), (vx0 + content[0], vy0 + content[1]), (0.0, 0.0),
                 (content[0] / capacity[0], content[1] / capacity[1]))
    dl.push_clip_rect((0, 22), (panel_w, H), True)
    dl.add_rect_filled((0, 22), (panel_w, H), ui.col32(15, 15, 15, 240))  # the side panel
    rng = np.random.default_rng(5)
    bars = rng.uniform(4.0, 60.0, 120)
    for i, b in enumerate(bars):  # the frame-time graph
        x = 10 + i * 2.25
        dl.add_rect_filled((x, 200 - b), (x + 1.75, 200), ui.col32(230, 180, 60, 200))
    dl.pop_clip_rect()
    overlay = ui.DrawList(white_handle)  # a second list: a translucent window over the viewport
    overlay.push_clip_rect((vx0 + 40, vy0 + 40), (vx0 + 360, vy0 + 200))
    overlay.add_rect_filled((vx0 + 40, vy0 + 40), (vx0 + 360.5, vy0 + 200.5), ui.col32(20, 20, 20, 160))
    overlay.add_triangle_filled((vx0 + 60, vy0 + 60), (vx0 + 120, vy0 + 90), (vx0 + 70, vy0 + 150), ui.col32(255, 80, 80, 220))
    overlay.pop_clip_rect()
    return ui.DrawData((0, 0), (W, H), (1, 1), [dl, overlay])
