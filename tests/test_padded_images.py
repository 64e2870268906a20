"""tests/padded_images.py itself, without a GPU: the outside mask is exactly capacity minus rect plus padding, one flipped
byte anywhere outside is reported, and the premise of tests/test_gpu_capacity_extent.py - the allocated extent of an image
cannot change which texel a NEAREST sample at (texel + 0.5) / allocatedExtent reads - holds in float32."""
import numpy as np
import pytest

from syzygy_amd import abi
from tests import padded_images as pi

CASES = [  # (format, sentinel, capacity, pad texels, rect)
    (abi.SZG_FORMAT_RGBA16_UNORM, pi.POISON_COLOR, (96, 48), 3, (70, 37)),
    (abi.SZG_FORMAT_D32_SFLOAT, pi.POISON_DEPTH, (64, 16), 5, (33, 9)),
    (abi.SZG_FORMAT_RGBA32_SFLOAT, pi.POISON_FLOAT4, (40, 9), 0, (32, 8)),
    (abi.SZG_FORMAT_RGBA16_SFLOAT, pi.POISON_DIFFUSE, (16, 16), 7, (1, 1)),
    (abi.SZG_FORMAT_RGBA16_SFLOAT, pi.POISON_HALF, (70, 37), 11, (70, 37)),
]


@pytest.mark.parametrize("fmt,sentinel,cap,pad,rect", CASES)
def test_outside_mask_is_capacity_minus_rect_plus_padding(fmt, sentinel, cap, pad, rect):
    im = pi.PaddedImage(fmt, cap[0], cap[1], pad, sentinel)
    texel = abi.TEXEL_BYTES[fmt]
    assert im.pitch_bytes == (cap[0] + pad) * texel and im.host.shape == (cap[1], im.pitch_bytes)
    mask = im.outside_mask(rect)
    # from the definition: a byte is inside when its row is a row of the rect and its texel a column of it
    rows, texels = np.arange(cap[1])[:, None], np.arange(im.pitch_bytes)[None, :] // texel
    assert np.array_equal(mask, ~((rows < rect[1]) & (texels < rect[0])))
    assert mask.sum() == cap[1] * im.pitch_bytes - rect[0] * rect[1] * texel
    assert mask.sum() == (cap[0] * cap[1] - rect[0] * rect[1]) * texel + cap[1] * pad * texel
    assert np.array_equal(im.outside_mask(abi.Rect(0, 0, rect[0], rect[1])), mask)
    # every texel, padding included, holds the sentinel
    assert (im.host.reshape(cap[1], cap[0] + pad, texel) == np.frombuffer(sentinel, np.uint8)).all()


@pytest.mark.parametrize("fmt,sentinel,cap,pad,rect", CASES)
def test_one_flipped_byte_anywhere_outside_is_reported_and_none_inside(fmt, sentinel, cap, pad, rect):
    im = pi.PaddedImage(fmt, cap[0], cap[1], pad, sentinel)
    texel = abi.TEXEL_BYTES[fmt]
    assert len(im.changed_outside(im.host.copy(), rect)) == 0
    outside = np.argwhere(im.outside_mask(rect))
    rng = np.random.default_rng(cap[0] * 131 + pad)
    picks = [outside[0], outside[-1]] + [outside[i] for i in rng.integers(0, len(outside), 8)]
    # the bytes that border the rect: first byte right of it, first row below it, last padding byte of the first row
    if rect[0] * texel < im.pitch_bytes:
        picks += [np.array([0, rect[0] * texel]), np.array([rect[1] - 1, rect[0] * texel])]
    if rect[1] < cap[1]:
        picks += [np.array([rect[1], 0]), np.array([rect[1], rect[0] * texel - 1])]
    if pad:
        picks += [np.array([0, im.pitch_bytes - 1]), np.array([0, cap[0] * texel])]
    for y, b in picks:
        raw = im.host.copy()
        raw[y, b] ^= 0x01
        assert im.changed_outside(raw, rect).tolist() == [[y, b]]
    raw = im.host.copy()
    raw[: rect[1], : rect[0] * texel] ^= 0xFF  # the whole inside rewritten: not the helper's business
    assert len(im.changed_outside(raw, rect)) == 0
    assert len(im.changed_outside(raw, (0, 0))) == rect[0] * rect[1] * texel  # ... unless the image is read-only


def test_typed_view_and_write_inside():
    im = pi.PaddedImage(abi.SZG_FORMAT_RGBA16_SFLOAT, 8, 4, 3, pi.POISON_DIFFUSE)
    view = im.typed(im.host, (8, 4))
    assert view.shape == (4, 8, 4) and view.dtype == np.float16
    assert np.isnan(view[..., :3]).all() and (view[..., 3] == 1.0).all()
    block = np.arange(3 * 5 * 4, dtype=np.float16).reshape(3, 5, 4)
    im.write_inside(block)
    assert np.array_equal(im.typed(im.host, (5, 3)), block)
    assert np.isnan(im.typed(im.host, (8, 4))[:, 5:, :3]).all() and np.isnan(im.typed(im.host, (8, 4))[3:, :, :3]).all()
    depth = pi.PaddedImage(abi.SZG_FORMAT_D32_SFLOAT, 8, 4, 1, pi.POISON_DEPTH)
    assert depth.typed(depth.host, (3, 2)).shape == (2, 3) and np.isnan(depth.typed(depth.host, (8, 4))).all()
    poison = pi.gbuffer_poison(6, 2)
    assert poison["diffuse"].shape == (2, 6, 4) and (poison["diffuse"][..., 3] == 1.0).all()
    assert np.isnan(poison["worldPosition"]).all() and poison["worldPosition"].dtype == np.float32


@pytest.mark.parametrize("n", [70, 96, 4096, 32768])
def test_nearest_sample_at_the_texel_centre_reads_that_texel_whatever_the_allocated_extent(n):
    """The reference samples its attachments NEAREST at (texel + 0.5) / allocatedExtent (lights.comp, camera.comp with
    imageSize / textureSize of the capacity-sized image). The sampler scales back by the extent and floors: for every texel
    below an extent up to 32768 that gives the texel again in float32 (the rounding error of the quotient, scaled by n, stays
    far below the 0.5 margin), so the values inside the draw rect cannot depend on the allocated size."""
    texel = np.arange(n, dtype=np.float32)
    extent = np.float32(n)
    uv = (texel + np.float32(0.5)) / extent
    assert uv.dtype == np.float32
    back = np.floor(uv * extent)
    assert np.array_equal(back, texel)
    # and for every allocated extent from the draw extent up to the capacity, at the draw extents the GPU tests use
    if n <= 96:
        a = np.arange(n, 4097, dtype=np.float32)[:, None]
        assert np.array_equal(np.floor(((texel[None, :] + np.float32(0.5)) / a) * a), np.broadcast_to(texel, (len(a), n)))
