"""numpy model of include/szg/jpeg.h rules 3 (IDCT), 4 (upsampling) and 5 (colour): dequantised coefficient planes -> RGBA8.

Written from the header's text, vectorised over blocks and rows; all arithmetic is uint32 (wraps), looked at as int32 only by
the arithmetic shifts and the clamps. A frame is a dict: width, height, color ("grey" | "ycbcr" | "rgb"), planes = [(h, v,
coefficients int16 [blocks_h, blocks_w, 8, 8])]."""
import numpy as np

GREY, YCBCR, RGB = 0, 1, 2
COLOR_NAMES = {GREY: "grey", YCBCR: "ycbcr", RGB: "rgb"}


def f2f(c):
    """(int)(c * 4096 + 0.5) with c read as binary32 and the arithmetic in double; the cast truncates toward zero"""
    return int(float(np.float32(c)) * 4096 + 0.5)


IDCT_CONSTANTS = {c: f2f(c) for c in (0.5411961, -1.847759065, 0.765366865, 1.175875602, 0.298631336, 2.053119869, 3.072711026,
                                      1.501321110, -0.899976223, -2.562915447, -1.961570560, -0.390180644)}


def color_fixed(x):
    """f(x) = ((int)(x * 4096.0f + 0.5f)) << 8, in binary32"""
    return int(np.float32(np.float32(x) * np.float32(4096.0) + np.float32(0.5))) << 8


def _u(v):
    return np.uint32(v & 0xFFFFFFFF)


def _asr(v, n):
    return (v.view(np.int32) >> n)


def idct_1d(s, bias):
    """s: uint32 [..., 8]; returns the eight outputs before their shift, uint32 [..., 8]"""
    K = {c: _u(v) for c, v in IDCT_CONSTANTS.items()}
    s0, s1, s2, s3, s4, s5, s6, s7 = (s[..., k] for k in range(8))
    with np.errstate(over="ignore"):
        p1 = (s2 + s6) * K[0.5411961]
        t2 = p1 + s6 * K[-1.847759065]
        t3 = p1 + s2 * K[0.765366865]
        t0 = (s0 + s4) * _u(4096)
        t1 = (s0 - s4) * _u(4096)
        b = _u(bias)
        x0, x3, x1, x2 = t0 + t3 + b, t0 - t3 + b, t1 + t2 + b, t1 - t2 + b
        t0, t1, t2, t3 = s7, s5, s3, s1
        p3, p4, p1, p2 = t0 + t2, t1 + t3, t0 + t3, t1 + t2
        p5 = (p3 + p4) * K[1.175875602]
        t0 = t0 * K[0.298631336]
        t1 = t1 * K[2.053119869]
        t2 = t2 * K[3.072711026]
        t3 = t3 * K[1.501321110]
        p1 = p5 + p1 * K[-0.899976223]
        p2 = p5 + p2 * K[-2.562915447]
        p3 = p3 * K[-1.961570560]
        p4 = p4 * K[-0.390180644]
        t3 = t3 + p1 + p4
        t2 = t2 + p2 + p3
        t1 = t1 + p2 + p4
        t0 = t0 + p1 + p3
        return np.stack([x0 + t3, x1 + t2, x2 + t1, x3 + t0, x3 - t0, x2 - t1, x1 - t2, x0 - t3], axis=-1)


def idct_blocks(coefficients):
    """int16 [..., 8, 8] (row, column) -> uint8 [..., 8, 8]"""
    d = np.ascontiguousarray(coefficients, dtype=np.int16).astype(np.int32).view(np.uint32)
    # column pass: the eight inputs of column c are d[..., :, c]
    cols = idct_1d(np.swapaxes(d, -1, -2), 512)          # [..., c, r]
    mid = np.ascontiguousarray(np.swapaxes(_asr(cols, 10), -1, -2)).view(np.uint32)  # [..., r, c]
    rows = idct_1d(mid, 65536 + (128 << 17))
    return np.clip(_asr(rows, 17), 0, 255).astype(np.uint8)


def sample_plane(coefficients):
    """int16 [blocks_h, blocks_w, 8, 8] -> uint8 [blocks_h * 8, blocks_w * 8]"""
    px = idct_blocks(coefficients)
    bh, bw = px.shape[:2]
    return np.ascontiguousarray(px.transpose(0, 2, 1, 3)).reshape(bh * 8, bw * 8)


def _row_h2(n, wl):
    n = n.astype(np.int32)
    out = np.empty(2 * wl, np.int32)
    if wl == 1:
        out[:] = n[0]
        return out
    s = np.arange(wl)
    out[0::2] = (3 * n[s] + n[np.maximum(s - 1, 0)] + 2) >> 2
    out[1::2] = (3 * n[s] + n[np.minimum(s + 1, wl - 1)] + 2) >> 2
    out[0] = n[0]
    out[2 * wl - 1] = n[wl - 1]
    out[2 * wl - 2] = (3 * n[wl - 2] + n[wl - 1] + 2) >> 2  # the quirk: wl - 2 carries the weight 3
    return out


def _row_hv2(n, f, wl):
    t = 3 * n.astype(np.int32) + f.astype(np.int32)
    out = np.empty(2 * wl, np.int32)
    if wl == 1:
        out[:] = (t[0] + 2) >> 2
        return out
    s = np.arange(wl)
    out[0::2] = (3 * t[s] + t[np.maximum(s - 1, 0)] + 8) >> 4
    out[1::2] = (3 * t[s] + t[np.minimum(s + 1, wl - 1)] + 8) >> 4
    out[0] = (t[0] + 2) >> 2
    out[2 * wl - 1] = (t[wl - 1] + 2) >> 2
    return out


def upsample(samples, W, H, h, v, h_max, v_max):
    """rule 4: uint8 sample plane (MCU padded) -> uint8 [H, W]"""
    hs, vs = h_max // h, v_max // v
    ch = -(-H * v // v_max)
    wl = -(-W // hs)
    out = np.empty((H, W), np.uint8)
    for j in range(H):
        near = min(j // vs, ch - 1)
        far = (max(near - 1, 0) if j % 2 == 0 else min(near + 1, ch - 1)) if vs == 2 else near
        n, f = samples[near, :wl], samples[far, :wl]
        if (hs, vs) == (1, 1):
            row = n
        elif (hs, vs) == (1, 2):
            row = (3 * n.astype(np.int32) + f.astype(np.int32) + 2) >> 2
        elif (hs, vs) == (2, 1):
            row = _row_h2(n, wl)
        elif (hs, vs) == (2, 2):
            row = _row_hv2(n, f, wl)
        else:
            row = np.repeat(n, hs)
        out[j] = row[:W]
    return out


def ycbcr_to_rgb(y, cb, cr):
    """rule 5 on uint8 arrays -> three uint8 arrays"""
    with np.errstate(over="ignore"):
        yf = (y.astype(np.uint32) << np.uint32(20)) + _u(1 << 19)
        crs = cr.astype(np.uint32) - _u(128)
        cbs = cb.astype(np.uint32) - _u(128)
        r = yf + crs * _u(color_fixed(1.40200))
        g = yf - crs * _u(color_fixed(0.71414)) + (((_u(0) - cbs) * _u(color_fixed(0.34414))) & _u(0xFFFF0000))
        b = yf + cbs * _u(color_fixed(1.77200))
    return tuple(np.clip(_asr(np.ascontiguousarray(c), 20), 0, 255).astype(np.uint8) for c in (r, g, b))


def reconstruct(frame, rgba_and=0xFFFFFFFF, rgba_or=0):
    """frame dict -> uint8 [H, W, 4]"""
    W, H = frame["width"], frame["height"]
    planes = frame["planes"]
    h_max = max(p[0] for p in planes)
    v_max = max(p[1] for p in planes)
    up = [upsample(sample_plane(c), W, H, h, v, h_max, v_max) for h, v, c in planes]
    color = frame["color"]
    if len(up) == 1:
        r = g = b = up[0]
    elif color == "rgb":
        r, g, b = up
    else:
        r, g, b = ycbcr_to_rgb(*up)
    texel = r.astype(np.uint32) | (g.astype(np.uint32) << 8) | (b.astype(np.uint32) << 16) | np.uint32(0xFF000000)
    texel = (texel & np.uint32(rgba_and)) | np.uint32(rgba_or)
    return np.ascontiguousarray(texel).view(np.uint8).reshape(H, W, 4)


def plane_grid(W, H, h, v, h_max, v_max):
    """(blocks_w, blocks_h, cw, ch) of rule 2 / rule 4"""
    mx, my = -(-W // (8 * h_max)), -(-H // (8 * v_max))
    return mx * h, my * v, -(-W * h // h_max), -(-H * v // v_max)
