"""CPU model of include/szg/texture_display.h in numpy: the image copy (szg_record_copy_image), the clear
(szg_record_clear_color_image) and the two additions to the UI layer's rules (RGBA16_SFLOAT textures, the view's component
mapping applied to the filtered sample), on top of tests/ui_layer_model.py. Every floating-point operation is one binary32
operation (numpy float32 arrays round after each); the binary16 store is numpy's astype(float16), round to nearest even
(tests/test_oracle.py holds that equal to the oracle's half conversion). The kernels (kernels_image_copy.hip,
kernels_ui_layer.hip) must reproduce these bytes.

Images are numpy arrays [h, w, 4]: uint8 (RGBA8_UNORM / RGBA8_SRGB), uint16 (RGBA16_UNORM codes, or the BITS of an
RGBA16_SFLOAT image: what the format argument says). Regions are (x, y, width, height), like szg_rect.
"""
import contextlib
from collections import namedtuple

import numpy as np

from syzygy_amd import abi
from tests import mipmap_model as mm
from tests import ui_layer_model as um

F = np.float32
RGBA8_UNORM, RGBA8_SRGB = abi.SZG_FORMAT_RGBA8_UNORM, abi.SZG_FORMAT_RGBA8_SRGB
RGBA16_UNORM, RGBA16_SFLOAT = abi.SZG_FORMAT_RGBA16_UNORM, abi.SZG_FORMAT_RGBA16_SFLOAT
SOURCE_FORMATS = (RGBA8_UNORM, RGBA8_SRGB, RGBA16_UNORM, RGBA16_SFLOAT)
IDENTITY, ZERO, ONE, R, G, B, A = range(7)
ROWS_PER_LANE = 8  # IMAGE_COPY_ROWS_PER_LANE of syzygy_amd/csrc/szg_launch.hpp: the rows a lane of k_image_copy walks


# ---- the copy ----
def axis_nearest(n, s0, sw, extent):
    """COORDINATES: the source texel of each of the n destination indices of one axis, in Python integers."""
    return np.array([min(max(s0 + ((2 * k + 1) * sw) // (2 * n), 0), extent - 1) for k in range(n)], np.int64)


def load(texels, fmt):
    """LOAD: [..., 4] texels of a source of `fmt` as float32 channels."""
    if fmt == RGBA8_UNORM:
        return mm.decode_table(False)[texels]
    if fmt == RGBA8_SRGB:
        return np.concatenate([mm.decode_table(True)[texels[..., :3]], mm.decode_table(False)[texels[..., 3:]]], axis=-1).astype(F)
    if fmt == RGBA16_UNORM:
        return (texels.astype(F) / F(65535.0)).astype(F)
    if fmt == RGBA16_SFLOAT:
        return texels.view(np.float16).astype(F)
    raise ValueError(f"format {fmt} is no source of the copy")


def store_half(values):
    """STORE: float32 -> the bits of binary16, round to nearest even."""
    with np.errstate(all="ignore"):
        return np.asarray(values, F).astype(np.float16).view(np.uint16)


def copy_image(src, src_fmt, src_region, dst, dst_region):
    """szg_record_copy_image on host arrays: a copy of `dst` (uint16 [H, W, 4], binary16 bits) whose dst_region holds the
    NEAREST blit of src_region of `src`; everything else keeps its value."""
    H, W = src.shape[:2]
    sx, sy, sw, sh = src_region
    dx, dy, dw, dh = dst_region
    assert 0 <= sx and 0 <= sy and sx + sw <= W and sy + sh <= H, "source region leaves the image"
    assert 0 <= dx and 0 <= dy and dx + dw <= dst.shape[1] and dy + dh <= dst.shape[0], "destination region leaves the image"
    out = dst.copy()
    if min(sw, sh, dw, dh) == 0:
        return out
    i = axis_nearest(dw, sx, sw, W)
    j = axis_nearest(dh, sy, sh, H)
    texels = src[j][:, i]
    # RGBA16_SFLOAT -> RGBA16_SFLOAT copies the bits (a NaN keeps its payload; a conversion would quieten it)
    out[dy:dy + dh, dx:dx + dw] = texels if src_fmt == RGBA16_SFLOAT else store_half(load(texels, src_fmt))
    return out


def clear_texel(fmt, color):
    """CLEAR: the uint16 [4] every texel becomes."""
    c = np.asarray(color, F)
    if fmt == RGBA16_SFLOAT:
        return store_half(c)
    if fmt == RGBA16_UNORM:
        return um.unorm16_store(c)
    raise ValueError(f"format {fmt} cannot be cleared")


# ---- the UI layer's additions ----
# data: uint8 / uint16 [h, w, 4] as um.Texture, or float16 [h, w, 4] (RGBA16_SFLOAT); swizzle: four values 0..6
TextureView = namedtuple("TextureView", "data filter address swizzle")
IDENTITY_VIEW = (IDENTITY,) * 4


def fetch(tex, i, j, outside):
    """SAMPLING's texel load with the addition: a binary16 channel is its value, converted exactly."""
    if tex.data.dtype == np.float16:
        t = tex.data[j, i].astype(F)
        return np.where(outside[:, None], np.array([0, 0, 0, 1], F), t).astype(F)
    return um._fetch(tex, i, j, outside)


def filtered(tex, u, v, fetch=fetch):
    """SAMPLING of ui_layer.h with `fetch` for the taps: [n, 4] float32."""
    h, w = tex.data.shape[:2]
    i0, i1, ox0, ox1, a = um._axis_taps(u, w, tex.filter, tex.address)
    j0, j1, oy0, oy1, b = um._axis_taps(v, h, tex.filter, tex.address)
    t00 = fetch(tex, i0, j0, ox0 | oy0)
    if tex.filter != um.LINEAR:
        return t00
    t10 = fetch(tex, i1, j0, ox1 | oy0)
    t01 = fetch(tex, i0, j1, ox0 | oy1)
    t11 = fetch(tex, i1, j1, ox1 | oy1)
    a, b = a[:, None], b[:, None]
    na, nb = (F(1) - a).astype(F), (F(1) - b).astype(F)
    top = ((t00 * na).astype(F) + (t10 * a).astype(F)).astype(F)
    bot = ((t01 * na).astype(F) + (t11 * a).astype(F)).astype(F)
    return ((top * nb).astype(F) + (bot * b).astype(F)).astype(F)


def mapped(r, swizzle):
    """MAPPING: the swizzle on [n, 4] float32."""
    out = np.empty_like(r)
    for k, s in enumerate(swizzle):
        out[:, k] = r[:, k] if s == IDENTITY else F(0) if s == ZERO else F(1) if s == ONE else r[:, s - R]
    return out


def sample(tex, u, v):
    """SAMPLING, then MAPPING."""
    with np.errstate(all="ignore"):
        r = filtered(tex, u, v)
        return mapped(r, tex.swizzle) if isinstance(tex, TextureView) else r


def sample_mapping_the_taps(tex, u, v):
    """What MAPPING is NOT: the swizzle applied to every tap, border taps included, before the filter."""
    with np.errstate(all="ignore"):
        return filtered(tex, u, v, fetch=lambda t, i, j, outside: mapped(fetch(t, i, j, outside), t.swizzle))


@contextlib.contextmanager
def _sampling_views():
    # um.shade looks `sample` up in its module when it runs: for the length of a render it is the one above, which gives
    # um.Texture entries exactly what um.sample gives them (the same taps, the same filter expressions)
    saved = um.sample
    um.sample = sample
    try:
        yield
    finally:
        um.sample = saved


def render(dst, render_area, load_op, clear_color, draw, textures, **kw):
    """um.render with textures that may be TextureView entries."""
    with _sampling_views():
        return um.render(dst, render_area, load_op, clear_color, draw, textures, **kw)
