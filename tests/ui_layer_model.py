"""CPU model of the UI layer pass (include/szg/ui_layer.h) in numpy. It follows the header's rules literally: vertices snapped
to 8 sub-pixel bits, coverage by exact integer edge functions with the top-left rule, every floating-point operation one
binary32 operation in the order the header writes it, the blend on the destination's UNORM16 codes, fragments in submission
order. The kernels (syzygy_amd/csrc/kernels_ui_layer.hip) must reproduce its bytes.

Two coverage paths share the shading: `render(..., brute=False)` evaluates the edge functions as int64 arrays over each
triangle's pixel box; `brute=True` walks EVERY pixel the scissor admits with Python integers and no box. They must agree
(tests/test_ui_layer_model.py).

The input is what syzygy_amd.ui.DrawData.flatten() returns (or anything with the same fields); a command's `texture` is a key
of `textures`, which maps it to a Texture. A command whose texture is None must have elem_count 0.
"""
from collections import namedtuple

import numpy as np

from syzygy_amd import abi

F = np.float32
I64 = np.int64
NEAREST, LINEAR = abi.SZG_FILTER_NEAREST, abi.SZG_FILTER_LINEAR
REPEAT, CLAMP_TO_EDGE, CLAMP_TO_BORDER = abi.SZG_UI_ADDRESS_REPEAT, abi.SZG_UI_ADDRESS_CLAMP_TO_EDGE, abi.SZG_UI_ADDRESS_CLAMP_TO_BORDER
CLEAR, LOAD = abi.SZG_UI_LOAD_OP_CLEAR, abi.SZG_UI_LOAD_OP_LOAD

# data: uint8 [h, w, 4] (RGBA8_UNORM) or uint16 [h, w, 4] (RGBA16_UNORM)
Texture = namedtuple("Texture", "data filter address")


def int64_to_f32(x):
    """One rounding to nearest even (a C cast of int64; np.float32(python int) would round twice, through binary64)."""
    return np.asarray(x, I64).astype(F)


def unorm16_store(x):
    """The library's UNORM16 store: clamp to [0, 1] (NaN -> 0), * 65535, round to nearest even."""
    x = np.asarray(x, F)
    c = np.where(np.isnan(x), F(0), np.minimum(np.maximum(x, F(0)), F(1))).astype(F)
    return np.rint(c * F(65535)).astype(np.uint16)


def saturate(x):
    return np.where(np.isnan(x), F(0), np.minimum(np.maximum(x, F(0)), F(1))).astype(F)


def trunc_saturated(x):
    """(int)x of VIEWPORT"""
    x = float(x)
    if x >= 2147483648.0:
        return 2 ** 31 - 1
    if x <= -2147483648.0:
        return -2 ** 31
    return int(x)


def framebuffer_extent(draw):
    ds, sc = np.asarray(draw.display_size, F), np.asarray(draw.framebuffer_scale, F)
    return trunc_saturated(ds[0] * sc[0]), trunc_saturated(ds[1] * sc[1])


def scissor(clip_rect, draw):
    """SCISSOR: (x0, y0, x1, y1) with x1 = x0 + w exclusive, or None when the command is skipped."""
    fbw, fbh = framebuffer_extent(draw)
    dp, sc = np.asarray(draw.display_pos, F), np.asarray(draw.framebuffer_scale, F)
    clip = np.asarray(clip_rect, F)
    box = [0, 0, 0, 0]
    for a, fb in ((0, fbw), (1, fbh)):
        cmin = (clip[a] - dp[a]) * sc[a]
        cmax = (clip[a + 2] - dp[a]) * sc[a]
        if cmin < 0:
            cmin = F(0)
        if cmax > F(fb):
            cmax = F(fb)
        if not (np.isfinite(cmin) and np.isfinite(cmax)) or cmax <= cmin:
            return None
        box[a] = int(cmin)
        box[a + 2] = box[a] + int(F(cmax - cmin))
    return tuple(box)


def snap_vertices(draw):
    """VERTEX for the whole buffer: (valid [n], X [n], Y [n]) with X, Y int64 (0 where dropped)."""
    v = draw.vertices
    dp, sc = np.asarray(draw.display_pos, F), np.asarray(draw.framebuffer_scale, F)
    p = ((np.asarray(v["pos"], F).reshape(-1, 2) - dp).astype(F) * sc).astype(F)
    valid = (np.abs(p) <= F(abi.SZG_UI_GUARD_BAND)).all(axis=1)  # NaN and inf fail
    snapped = np.rint(np.where(valid[:, None], p, F(0)) * F(256)).astype(I64)
    return valid, snapped[:, 0], snapped[:, 1]


def command_triangles(cmd, index_count):
    """ASSEMBLY: how many triangles the command has after the truncation."""
    available = index_count - cmd.idx_offset if cmd.idx_offset < index_count else 0
    return min(int(cmd.elem_count), available) // 3


class Tri:
    """One triangle after setup, sign-normalised: s E_i(px, py) = e0[i] + ex[i] px + ey[i] py, Python integers."""

    __slots__ = ("e0", "ex", "ey", "tl", "det", "xs", "ys")

    def __init__(self, X, Y):
        X, Y = [int(v) for v in X], [int(v) for v in Y]
        det = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
        self.det = abs(det)
        self.xs, self.ys = X, Y
        if det == 0:
            return
        s = 1 if det > 0 else -1
        self.e0, self.ex, self.ey, self.tl = [], [], [], []
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            a, b = -(Y[k] - Y[j]) * s, (X[k] - X[j]) * s
            # E_i at C = (256 px + 128, 256 py + 128): b (C_y - Y_j) + a (C_x - X_j)
            self.e0.append(b * (128 - Y[j]) + a * (128 - X[j]))
            self.ex.append(256 * a)
            self.ey.append(256 * b)
            self.tl.append(1 if (a > 0 or (a == 0 and b > 0)) else 0)


def _axis_taps(coord, n, filt, addr):
    """SAMPLING, one axis: (i0, i1, out0, out1, weight of tap 1)"""
    fn = F(n)
    last = F(fn - F(1))
    x = (coord * fn).astype(F)
    if filt == LINEAR:
        x = (x - F(0.5)).astype(F)
    f0 = np.floor(x).astype(F)
    f1 = (f0 + F(1)).astype(F)
    w = (x - f0).astype(F)
    never = np.zeros(coord.shape, bool)
    if addr == REPEAT:
        m = (f0 - (fn * np.floor((f0 / fn).astype(F)).astype(F)).astype(F)).astype(F)
        ok = (m >= 0) & (m < fn)
        i0 = np.where(ok, m, F(0)).astype(I64)
        i1 = np.where(i0 + 1 == n, 0, i0 + 1)
        return i0, i1, never, never, w

    def clamp(f):
        c = np.minimum(np.maximum(f, F(0)), last)
        return np.where(np.isnan(f), F(0), c).astype(I64)

    if addr == CLAMP_TO_BORDER:
        return clamp(f0), clamp(f1), ~((f0 >= 0) & (f0 <= last)), ~((f1 >= 0) & (f1 <= last)), w
    return clamp(f0), clamp(f1), never, never, w


def _fetch(tex, i, j, outside):
    codes = tex.data[j, i].astype(F)
    t = (codes / (F(65535) if tex.data.dtype == np.uint16 else F(255))).astype(F)
    border = np.array([0, 0, 0, 1], F)
    return np.where(outside[:, None], border, t).astype(F)


def sample(tex, u, v):
    """SAMPLING: [n, 4] float32 texels for [n] float32 coordinates."""
    with np.errstate(all="ignore"):
        return _sample(tex, u, v)


def _sample(tex, u, v):
    h, w = tex.data.shape[:2]
    i0, i1, ox0, ox1, a = _axis_taps(u, w, tex.filter, tex.address)
    j0, j1, oy0, oy1, b = _axis_taps(v, h, tex.filter, tex.address)
    t00 = _fetch(tex, i0, j0, ox0 | oy0)
    if tex.filter != LINEAR:
        return t00
    t10 = _fetch(tex, i1, j0, ox1 | oy0)
    t01 = _fetch(tex, i0, j1, ox0 | oy1)
    t11 = _fetch(tex, i1, j1, ox1 | oy1)
    a, b = a[:, None], b[:, None]
    na, nb = (F(1) - a).astype(F), (F(1) - b).astype(F)
    top = ((t00 * na).astype(F) + (t10 * a).astype(F)).astype(F)
    bot = ((t01 * na).astype(F) + (t11 * a).astype(F)).astype(F)
    return ((top * nb).astype(F) + (bot * b).astype(F)).astype(F)


def shade(sE, det, attrs, tex, dst):
    """INTERPOLATION, SAMPLING, FRAGMENT and BLEND for the covered pixels of one triangle.
    sE: three int64 arrays [n]; det: |det|; attrs: float32 [3 vertices, 6] = u, v, r, g, b, a; dst: uint16 [n, 4]."""
    fd = int64_to_f32(det)
    lam = [(int64_to_f32(e) / fd).astype(F) for e in sE]

    def interp(k):
        return (((lam[0] * attrs[0, k]).astype(F) + (lam[1] * attrs[1, k]).astype(F)).astype(F) + (lam[2] * attrs[2, k]).astype(F)).astype(F)

    u, v = interp(0), interp(1)
    colour = np.stack([interp(2), interp(3), interp(4), interp(5)], axis=1)
    texel = sample(tex, u, v)
    out = saturate((colour * texel).astype(F))
    d = (dst.astype(F) / F(65535)).astype(F)
    alpha = out[:, 3:4]
    na = (F(1) - alpha).astype(F)
    rgb = ((out[:, :3] * alpha).astype(F) + (d[:, :3] * na).astype(F)).astype(F)
    a = (out[:, 3:4] + (d[:, 3:4] * na).astype(F)).astype(F)
    return unorm16_store(np.concatenate([rgb, a], axis=1))


def vertex_attributes(vertices, ids):
    """float32 [3, 6]: u, v and the colour channels float(byte) / 255.0f of three vertices"""
    out = np.empty((3, 6), F)
    for r, i in enumerate(ids):
        out[r, 0:2] = vertices["uv"][i]
        col = int(vertices["col"][i])
        out[r, 2:6] = (np.array([col & 0xFF, (col >> 8) & 0xFF, (col >> 16) & 0xFF, col >> 24], F) / F(255)).astype(F)
    return out


def _cover_box(tri, box):
    """Covered pixels of `box` through int64 arrays over the triangle's own pixel box: (px, py, [sE_0, sE_1, sE_2])."""
    x0 = max((min(tri.xs) + 127) >> 8, box[0])
    x1 = min(((max(tri.xs) - 128) >> 8) + 1, box[2])
    y0 = max((min(tri.ys) + 127) >> 8, box[1])
    y1 = min(((max(tri.ys) - 128) >> 8) + 1, box[3])
    if x0 >= x1 or y0 >= y1:
        return None
    px = np.arange(x0, x1, dtype=I64)[None, :]
    py = np.arange(y0, y1, dtype=I64)[:, None]
    cover = np.ones((y1 - y0, x1 - x0), bool)
    e = []
    for i in range(3):
        ei = I64(tri.e0[i]) + I64(tri.ex[i]) * px + I64(tri.ey[i]) * py
        cover &= ei + tri.tl[i] > 0
        e.append(ei)
    jj, ii = np.nonzero(cover)
    if len(jj) == 0:
        return None
    return ii + x0, jj + y0, [ei[jj, ii] for ei in e]


def _cover_brute(tri, box):
    """The same from the header's words alone: every pixel of `box`, Python integers, no pixel box of the triangle."""
    X, Y = tri.xs, tri.ys
    det = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    s = 1 if det > 0 else -1
    xs, ys, es = [], [], ([], [], [])
    for py in range(box[1], box[3]):
        cy = 256 * py + 128
        for px in range(box[0], box[2]):
            cx = 256 * px + 128
            vals = []
            for i in range(3):
                j, k = (i + 1) % 3, (i + 2) % 3
                e = s * ((X[k] - X[j]) * (cy - Y[j]) - (Y[k] - Y[j]) * (cx - X[j]))
                if e < 0:
                    break
                if e == 0:
                    a, b = -(Y[k] - Y[j]), X[k] - X[j]
                    if not (s * a > 0 or (a == 0 and s * b > 0)):
                        break
                vals.append(e)
            else:
                xs.append(px)
                ys.append(py)
                for i in range(3):
                    es[i].append(vals[i])
    if not xs:
        return None
    return np.array(xs, I64), np.array(ys, I64), [np.array(e, I64) for e in es]


def render(dst, render_area, load_op, clear_color, draw, textures, brute=False, snapshots=(), coverage=None):
    """The pass. dst: uint16 [H, W, 4], the allocated output image (not modified); render_area: (x, y, width, height) inside it.
    Returns the new image, or (image, {k: image after k triangles of the drawable commands}) when `snapshots` names
    triangle counts. `coverage` (int array [H, W], optional) counts the fragments blended into each pixel."""
    out = np.array(dst, np.uint16, copy=True)
    H, W = out.shape[:2]
    ax0, ay0 = int(render_area[0]), int(render_area[1])
    ax1, ay1 = ax0 + int(render_area[2]), ay0 + int(render_area[3])
    assert 0 <= ax0 <= ax1 <= W and 0 <= ay0 <= ay1 <= H, "the render area leaves the image"
    taken = {}
    with np.errstate(all="ignore"):
        if load_op == CLEAR:
            out[ay0:ay1, ax0:ax1] = unorm16_store(np.asarray(clear_color, F))
        fbw, fbh = framebuffer_extent(draw)
        limit = (ax0, ay0, min(ax1, fbw), min(ay1, fbh))
        valid, X, Y = snap_vertices(draw)
        nv, ni = len(draw.vertices), len(draw.indices)
        indices = np.asarray(draw.indices, I64)
        done = 0
        if 0 in snapshots:
            taken[0] = out.copy()
        for cmd in draw.commands:
            if cmd.elem_count == 0:
                continue
            ntri = command_triangles(cmd, ni)
            sc = scissor(cmd.clip_rect, draw) if fbw > 0 and fbh > 0 else None
            if ntri == 0 or sc is None:
                continue
            box = (max(sc[0], limit[0]), max(sc[1], limit[1]), min(sc[2], limit[2]), min(sc[3], limit[3]))
            if box[0] >= box[2] or box[1] >= box[3]:
                continue
            tex = textures[cmd.texture]
            for t in range(ntri):
                done += 1
                ids = cmd.vtx_offset + indices[cmd.idx_offset + 3 * t: cmd.idx_offset + 3 * t + 3]
                if (ids < nv).all() and valid[ids].all():
                    tri = Tri(X[ids], Y[ids])
                    hit = None if tri.det == 0 else (_cover_brute if brute else _cover_box)(tri, box)
                    if hit is not None:
                        px, py, sE = hit
                        out[py, px] = shade(sE, tri.det, vertex_attributes(draw.vertices, ids), tex, out[py, px])
                        if coverage is not None:
                            coverage[py, px] += 1
                if done in snapshots:
                    taken[done] = out.copy()
    return (out, taken) if len(snapshots) else out
