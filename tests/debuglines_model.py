"""CPU model of the debug-line pass (include/szg/debuglines.h), binary32 numpy, vectorised per line. It follows the
header's operation order literally; the kernels (syzygy_amd/csrc/kernels_debuglines.hip) must agree with it bit for bit.

Two ways to enumerate candidate pixels, both applying the same exact coverage test:
  band   for every major-axis column (row) a minor-axis interval around the centre line, with a margin twice the kernel's
         plus 4 px: fast enough for 10^5 lines;
  brute  every pixel of the line's bounding box (clamped to the draw rect): no assumption at all about where the covered
         pixels lie. tests/test_debuglines_model.py checks that both give the same set.
"""
import numpy as np

F32 = np.float32
GUARD_BAND = F32(16777216.0)
GREEN_UNORM = np.array([0, 65535, 0, 65535], np.uint16)
GREEN_F32 = np.array([0.0, 1.0, 0.0, 1.0], np.float32)


def mat(m):
    """szg_mat4 (column-major) -> float32 [16]."""
    return np.array(list(m.m), np.float32)


def proj_view(cam):
    """(projection * view): column j = ((P0*Vj0 + P1*Vj1) + P2*Vj2) + P3*Vj3, P_c = column c of P."""
    P, V = mat(cam.projection), mat(cam.view)
    out = np.zeros(16, np.float32)
    for j in range(4):
        for r in range(4):
            acc = P[r] * V[j * 4 + 0]
            acc = acc + P[4 + r] * V[j * 4 + 1]
            acc = acc + P[8 + r] * V[j * 4 + 2]
            acc = acc + P[12 + r] * V[j * 4 + 3]
            out[j * 4 + r] = acc
    return out


def clip_positions(cam, positions):
    """The vertex stage for an [N, 3] float32 array: [N, 4] clip positions."""
    pv = proj_view(cam)
    p = np.asarray(positions, np.float32).reshape(-1, 3)
    out = np.empty((len(p), 4), np.float32)
    with np.errstate(all="ignore"):
        for r in range(4):
            acc = pv[r] * p[:, 0]
            acc = acc + pv[4 + r] * p[:, 1]
            acc = acc + pv[8 + r] * p[:, 2]
            acc = acc + pv[12 + r] * F32(1.0)
            out[:, r] = acc
    return out


def positions_of(vertices):
    """ctypes array of abi.VertexPacked (or a raw uint8 / float32 buffer of them) -> [N, 3] float32."""
    raw = np.frombuffer(bytes(vertices), np.float32) if not isinstance(vertices, np.ndarray) else vertices.view(np.float32)
    return raw.reshape(-1, 12)[:, 0:3].copy()


def setup(cam, positions, W, H):
    """Primitive assembly, depth clipping, viewport. Returns (xa, ya, xb, yb) float32 arrays of the lines that survive."""
    n = len(positions) // 2
    c = clip_positions(cam, positions[: 2 * n])
    a, b = c[0::2].copy(), c[1::2].copy()
    keep = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
    with np.errstate(all="ignore"):
        for far in (False, True):
            da = a[:, 3] - a[:, 2] if far else a[:, 2].copy()
            db = b[:, 3] - b[:, 2] if far else b[:, 2].copy()
            keep &= ~((da < 0) & (db < 0))
            cut = (da < 0) ^ (db < 0)
            t = da / (da - db)
            nxt = a + t[:, None] * (b - a)
            a = np.where((cut & (da < 0))[:, None], nxt, a)
            b = np.where((cut & (db < 0))[:, None], nxt, b)
        hW, hH = F32(W) * F32(0.5), F32(H) * F32(0.5)
        xa = (a[:, 0] / a[:, 3] + F32(1.0)) * hW
        ya = (a[:, 1] / a[:, 3] + F32(1.0)) * hH
        xb = (b[:, 0] / b[:, 3] + F32(1.0)) * hW
        yb = (b[:, 1] / b[:, 3] + F32(1.0)) * hH
        for v in (xa, ya, xb, yb):
            keep &= np.abs(v) <= GUARD_BAND
    return xa[keep], ya[keep], xb[keep], yb[keep]


def covered(px, py, xa, ya, xb, yb, width):
    """The exact test for pixel indices px, py (broadcast against the line arrays)."""
    with np.errstate(all="ignore"):
        cx = px.astype(np.float32) + F32(0.5)
        cy = py.astype(np.float32) + F32(0.5)
        dx = xb - xa
        dy = yb - ya
        L2 = dx * dx + dy * dy
        ex = cx - xa
        ey = cy - ya
        u = ex * dx + ey * dy
        v = dx * ey - dy * ex
        w2 = F32(width) * F32(width)
        return (L2 > 0) & (F32(0) <= u) & (u <= L2) & ((F32(4.0) * v) * v <= w2 * L2)


def _margin(xa, ya, xb, yb):
    m = np.maximum(np.maximum(np.abs(xa), np.abs(ya)), np.maximum(np.abs(xb), np.abs(yb))).astype(np.float64)
    return 2.0 * (2.0 + (m + 32768.0) * 2.0 ** -18) + 4.0


def coverage_brute(lines, W, H, width):
    mask = np.zeros((H, W), bool)
    hw = float(width) * 0.5
    for xa, ya, xb, yb in zip(*lines):
        g = _margin(xa, ya, xb, yb) + hw
        x0, x1 = int(max(0, np.floor(min(xa, xb) - g))), int(min(W - 1, np.floor(max(xa, xb) + g)))
        y0, y1 = int(max(0, np.floor(min(ya, yb) - g))), int(min(H - 1, np.floor(max(ya, yb) + g)))
        if x0 > x1 or y0 > y1:
            continue
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        mask[y0:y1 + 1, x0:x1 + 1] |= covered(px, py, xa, ya, xb, yb, width)
    return mask


def coverage_band(lines, W, H, width, chunk=1 << 22):
    xa, ya, xb, yb = (np.asarray(v, np.float32) for v in lines)
    mask = np.zeros((H, W), bool)
    if len(xa) == 0:
        return mask
    hw = float(width) * 0.5
    g = _margin(xa, ya, xb, yb)
    dx, dy = (xb - xa).astype(np.float64), (yb - ya).astype(np.float64)
    ymajor = np.abs(dy) > np.abs(dx)
    for major in (False, True):
        sel = np.nonzero(ymajor == major)[0]
        if len(sel) == 0:
            continue
        pa, pb = (ya, yb) if major else (xa, xb)
        qa = (xa if major else ya).astype(np.float64)
        dm, dn = (dy, dx) if major else (dx, dy)
        ext = g[sel] + hw
        lo = np.maximum(np.floor(np.minimum(pa[sel], pb[sel]) - ext), 0)
        hi = np.minimum(np.floor(np.maximum(pa[sel], pb[sel]) + ext), (H if major else W) - 1)
        cnt = np.maximum(hi - lo + 1, 0).astype(np.int64)
        with np.errstate(all="ignore"):
            slope = np.where(dm[sel] != 0, dn[sel] / np.where(dm[sel] != 0, dm[sel], 1), 0.0)
        half = hw * 1.5 + g[sel]
        starts = np.concatenate([[0], np.cumsum(cnt)])
        total = int(starts[-1])
        pos = 0
        while pos < total:
            end = min(total, pos + max(1, chunk // int(2 * half.max() + 3)))
            item = np.arange(pos, end)
            li = np.searchsorted(starts, item, side="right") - 1
            m = lo[li] + (item - starts[li])
            centre = qa[sel][li] + (m + 0.5 - pa[sel][li].astype(np.float64)) * slope[li]
            nlo = np.maximum(np.floor(centre - half[li]), 0).astype(np.int64)
            nhi = np.minimum(np.floor(centre + half[li]), (W if major else H) - 1).astype(np.int64)
            k = int((nhi - nlo).max(initial=-1)) + 1
            if k > 0:
                off = np.arange(k)[None, :]
                n = nlo[:, None] + off
                ok = n <= nhi[:, None]
                mm = np.broadcast_to(m.astype(np.int64)[:, None], n.shape)
                px, py = (n, mm) if major else (mm, n)
                L = sel[li][:, None]
                hit = ok & covered(px, py, xa[L], ya[L], xb[L], yb[L], width)
                mask[py[hit], px[hit]] = True
            pos = end
    return mask


def render(mask, color, debug=None):
    """Apply the pass's output to copies of the colour plane (uint16 [H, W, 4]) and the debug plane (float32, optional)
    over the mask's extent (the draw rect, top-left)."""
    color = color.copy()
    H, W = mask.shape
    color[:H, :W][mask] = GREEN_UNORM
    if debug is not None:
        debug = debug.copy()
        debug[:H, :W][mask] = GREEN_F32
    return color, debug


def model(cam, positions, W, H, width, brute=False):
    """The covered-pixel mask of a draw over the W x H draw rect."""
    lines = setup(cam, np.asarray(positions, np.float32), W, H)
    return (coverage_brute if brute else coverage_band)(lines, W, H, width)
