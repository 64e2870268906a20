"""CPU model of the present pass (include/szg/present.h) in numpy. It follows the header's rule literally: coordinates in
integers, taps clamped to the image, every binary32 operation rounded on its own (numpy float32 arrays round after each
operation), UNORM store by round-to-nearest-even. The kernels (syzygy_amd/csrc/kernels_present.hip) must agree with it bit
for bit (tests/test_gpu_present.py).

`dtype=np.float64` evaluates the SAME formulas in binary64: the weights are then the exact rationals rounded once to 53
bits, which is the reference the binary32 rule is measured against in tests/test_present_model.py.

Regions are (x, y, width, height), like szg_rect.
"""
import numpy as np

RGBA8, BGRA8, A2B10G10R10 = 5, 6, 7  # szg_format values of the destinations
NEAREST, LINEAR = 0, 1
FORMATS = (RGBA8, BGRA8, A2B10G10R10)
MAX_EXTENT = 16384


def channel_bits(fmt):
    """Bits of (R, G, B, A) in the stored texel."""
    return (10, 10, 10, 2) if fmt == A2B10G10R10 else (8, 8, 8, 8)


def axis_linear(n, s0, sw, extent, dtype=np.float32):
    """COORDINATES of the header for the n destination indices of one axis: (i0, i1, alpha), taps clamped to the image."""
    k = np.arange(n, dtype=np.int64)
    num = (2 * k + 1) * sw + (2 * s0 - 1) * n
    den = 2 * n
    i0 = np.floor_divide(num, den)  # towards minus infinity
    rem = num - i0 * den
    alpha = rem.astype(dtype) / dtype(den)  # both exact, one rounding
    return np.clip(i0, 0, extent - 1), np.clip(i0 + 1, 0, extent - 1), alpha


def axis_nearest(n, s0, sw, extent):
    k = np.arange(n, dtype=np.int64)
    return np.clip(s0 + np.floor_divide((2 * k + 1) * sw, 2 * n), 0, extent - 1)


def oetf_table(function):
    """The 65 536-entry table of szg_record_oetf: the CPU oracle's OETF of every UNORM16 code (uint16[65536])."""
    from oracle import binding as ob

    codes = np.arange(65536, dtype=np.uint16)
    image = np.zeros((64, 1024, 4), np.uint16)
    image[..., 0] = codes.reshape(64, 1024)
    return np.ascontiguousarray(ob.oetf(image, function)[..., 0]).reshape(65536).copy()


def _texels(src, rows, cols, table, dtype):
    """Taps src[rows][:, cols] as normalised channels: ENCODE on R, G, B first, then t = code / 65535."""
    codes = src[rows][:, cols]
    if table is not None:
        codes = codes.copy()
        codes[..., :3] = table[codes[..., :3]]
    return codes.astype(dtype) / dtype(65535.0)


def store(r, bits):
    """STORE: clamp to [0, 1], scale by 2^b - 1, round to nearest even. `r` keeps its dtype through the product."""
    dtype = r.dtype.type
    c = np.minimum(np.maximum(r, dtype(0.0)), dtype(1.0))
    return np.rint(c * dtype((1 << bits) - 1)).astype(np.int64)


def filtered_values(src, src_region, dst_w, dst_h, filter=LINEAR, table=None, dtype=np.float32, chunk_rows=128):
    """The filter's results r before the STORE, in chunks of destination rows: yields (row slice, r [rows, dst_w, 4])."""
    H, W, _ = src.shape
    sx, sy, sw, sh = src_region
    if filter == LINEAR:
        i0, i1, alpha = axis_linear(dst_w, sx, sw, W, dtype)
        j0, j1, beta = axis_linear(dst_h, sy, sh, H, dtype)
        one = dtype(1.0)
        a = alpha[None, :, None]
        na = (one - alpha)[None, :, None]
        for y0 in range(0, dst_h, chunk_rows):
            ys = slice(y0, min(y0 + chunk_rows, dst_h))
            b = beta[ys][:, None, None]
            nb = (one - beta[ys])[:, None, None]
            t00 = _texels(src, j0[ys], i0, table, dtype)
            t10 = _texels(src, j0[ys], i1, table, dtype)
            t01 = _texels(src, j1[ys], i0, table, dtype)
            t11 = _texels(src, j1[ys], i1, table, dtype)
            top = t00 * na + t10 * a  # numpy rounds each product and the sum to the array's dtype
            bot = t01 * na + t11 * a
            yield ys, top * nb + bot * b
    elif filter == NEAREST:
        i = axis_nearest(dst_w, sx, sw, W)
        j = axis_nearest(dst_h, sy, sh, H)
        for y0 in range(0, dst_h, chunk_rows):
            ys = slice(y0, min(y0 + chunk_rows, dst_h))
            yield ys, _texels(src, j[ys], i, table, dtype)
    else:
        raise ValueError(f"unknown filter {filter}")


def filtered_codes(src, src_region, dst_w, dst_h, fmt, filter=LINEAR, table=None, dtype=np.float32, chunk_rows=128):
    """The stored channel codes [dst_h, dst_w, 4] (R, G, B, A order, whatever the format's byte order) of a blit of
    `src_region` of the uint16 image `src` [H, W, 4] onto dst_w x dst_h texels."""
    return filtered_codes_by_bits(src, src_region, dst_w, dst_h, (fmt,), filter, table, dtype, chunk_rows)[channel_bits(fmt)]


def filtered_codes_by_bits(src, src_region, dst_w, dst_h, fmts=FORMATS, filter=LINEAR, table=None, dtype=np.float32,
                           chunk_rows=128):
    """filtered_codes for several formats with the filter evaluated once: {channel_bits(fmt): codes int64 [h, w, 4]}."""
    outs = {channel_bits(f): None for f in fmts}
    for bits in outs:
        outs[bits] = np.empty((dst_h, dst_w, 4), np.int64)
    for ys, r in filtered_values(src, src_region, dst_w, dst_h, filter, table, dtype, chunk_rows):
        for bits, out in outs.items():
            for c in range(4):
                out[ys, :, c] = store(r[..., c], bits[c])
    return outs


def pack(codes, fmt):
    """Channel codes [h, w, 4] -> the destination's texels: uint8 [h, w, 4] for the 8-bit formats (memory order), uint32
    [h, w] for A2B10G10R10 (R bits 0-9, G 10-19, B 20-29, A 30-31)."""
    if fmt == A2B10G10R10:
        c = codes.astype(np.uint32)
        return c[..., 0] | (c[..., 1] << np.uint32(10)) | (c[..., 2] << np.uint32(20)) | (c[..., 3] << np.uint32(30))
    order = [2, 1, 0, 3] if fmt == BGRA8 else [0, 1, 2, 3]
    return codes[..., order].astype(np.uint8)


def empty_destination(width, height, fmt, fill=0):
    if fmt == A2B10G10R10:
        return np.full((height, width), fill, np.uint32)
    return np.full((height, width, 4), fill, np.uint8)


def present(src, src_region, dst, dst_region, fmt, filter=LINEAR, table=None, dtype=np.float32):
    """szg_record_present on host arrays: returns a copy of `dst` (uint8 [h, w, 4] or uint32 [h, w]) whose dst_region holds
    the blit of src_region of `src`; everything else keeps its value."""
    H, W, _ = src.shape
    sx, sy, sw, sh = src_region
    dx, dy, dw, dh = dst_region
    assert max(H, W, dst.shape[0], dst.shape[1]) <= MAX_EXTENT
    assert 0 <= sx and 0 <= sy and sx + sw <= W and sy + sh <= H, "source region leaves the image"
    assert 0 <= dx and 0 <= dy and dx + dw <= dst.shape[1] and dy + dh <= dst.shape[0], "destination region leaves the image"
    out = dst.copy()
    if min(sw, sh, dw, dh) == 0:
        return out
    out[dy:dy + dh, dx:dx + dw] = pack(filtered_codes(src, src_region, dw, dh, fmt, filter, table, dtype), fmt)
    return out
