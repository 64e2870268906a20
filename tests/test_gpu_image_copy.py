"""GPU: szg_record_copy_image and szg_record_clear_color_image (include/szg/texture_display.h,
syzygy_amd/csrc/kernels_image_copy.hip) against the CPU model (tests/texture_display_model.py), byte for byte. Every image lies
inside a larger buffer filled with a sentinel, with padded rows, and the WHOLE buffers are compared: a byte written outside the
destination region, pitch padding included, or anywhere in the source, fails."""
import ctypes as C
import types

import numpy as np
import pytest

from syzygy_amd import abi, lib
from tests import stream_order as so
from tests import texture_display_cases as tc
from tests import texture_display_model as tm

pytestmark = pytest.mark.gpu
ROWS = tm.ROWS_PER_LANE  # IMAGE_COPY_ROWS_PER_LANE: a lane walks this many rows with the column setup it made once
DTYPE = {tm.RGBA8_UNORM: np.uint8, tm.RGBA8_SRGB: np.uint8, tm.RGBA16_UNORM: np.uint16, tm.RGBA16_SFLOAT: np.uint16}
FORMAT_IDS = {tm.RGBA8_UNORM: "rgba8", tm.RGBA8_SRGB: "srgb8", tm.RGBA16_UNORM: "unorm16", tm.RGBA16_SFLOAT: "half"}


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    return torch


class Buffer:
    """An image of w x h texels inside a flat device buffer of sentinel texels: `shift` texels in front of it, rows of w + pad
    texels, two more rows behind it. `texels`: the image's content [h, w, 4], or None for sentinels everywhere."""

    def __init__(self, torch, w, h, fmt, texels=None, pad=0, shift=0, seed=1):
        dtype = DTYPE[fmt]
        rng = np.random.default_rng(seed)
        self.torch, self.w, self.h, self.fmt, self.row, self.shift = torch, w, h, fmt, w + pad, shift
        self.flat0 = rng.integers(0, np.iinfo(dtype).max + 1, (shift + (h + 2) * self.row, 4)).astype(dtype)
        if texels is not None:
            self.flat0 = self.put(self.flat0, np.asarray(texels, dtype))
        self.device = torch.from_numpy(self.flat0.view(np.uint8).copy()).cuda()

    def index(self):
        return self.shift + np.arange(self.h)[:, None] * self.row + np.arange(self.w)[None, :]

    def image0(self):
        return self.flat0[self.index()]

    def put(self, flat, texels):
        out = flat.copy()
        out[self.index()] = texels
        return out

    def abi(self):
        tb = self.flat0.dtype.itemsize * 4
        return abi.Image(self.device.data_ptr() + self.shift * tb, self.w, self.h, self.row * tb, self.fmt)

    def read(self):
        self.torch.cuda.synchronize()
        return self.device.cpu().numpy().view(self.flat0.dtype).reshape(self.flat0.shape)


def random_source(fmt, w, h, seed=2):
    return np.random.default_rng(seed).integers(0, np.iinfo(DTYPE[fmt]).max + 1, (h, w, 4)).astype(DTYPE[fmt])


def first_difference(got, want):
    bad = np.argwhere((got != want).any(axis=-1))
    return f"{len(bad)} texels differ, first at flat index {bad[0].tolist()}: got {got[tuple(bad[0])].tolist()}, want {want[tuple(bad[0])].tolist()}"


def run_copy(torch, texels, fmt, src_region, dst_extent, dst_region, src_pad=0, dst_pad=0, dst_shift=0, stream=None):
    """Copy on the GPU and in the model; asserts the whole destination buffer equals the model's and the whole source buffer is
    unchanged. Returns the destination image."""
    h, w = texels.shape[:2]
    src = Buffer(torch, w, h, fmt, texels, pad=src_pad, seed=3)
    dst = Buffer(torch, dst_extent[0], dst_extent[1], tm.RGBA16_SFLOAT, pad=dst_pad, shift=dst_shift, seed=4)
    s_im, d_im = src.abi(), dst.abi()
    rc = lib().szg_record_copy_image(stream, C.byref(s_im), C.byref(d_im), abi.Rect(*src_region), abi.Rect(*dst_region))
    assert rc == abi.SZG_OK, lib().szg_last_error()
    want_image = tm.copy_image(texels, fmt, src_region, dst.image0(), dst_region)
    want, got = dst.put(dst.flat0, want_image), dst.read()
    assert np.array_equal(got, want), first_difference(got, want)
    assert np.array_equal(src.read(), src.flat0), "the source was written"
    return want_image


# ---- 1:1, every code ----
@pytest.mark.parametrize("fmt", [tm.RGBA8_UNORM, tm.RGBA8_SRGB], ids=FORMAT_IDS.get)
def test_every_8_bit_code_in_every_channel(torch, fmt):
    codes = np.arange(256)
    texels = np.stack([(codes + 64 * k) % 256 for k in range(4)], axis=1).astype(np.uint8)[None]  # 256 x 1, R, G, B, A differ
    out = run_copy(torch, texels, fmt, (0, 0, 256, 1), (256, 1), (0, 0, 256, 1))
    assert len(np.unique(out[0, :, 0])) > 200 and not np.array_equal(out[0, :, 0], out[0, :, 3])


def test_every_unorm16_code_in_every_channel(torch):
    codes = np.arange(65536).reshape(256, 256)
    texels = np.stack([(codes + 16384 * k) % 65536 for k in range(4)], axis=2).astype(np.uint16)
    run_copy(torch, texels, tm.RGBA16_UNORM, (0, 0, 256, 256), (256, 256), (0, 0, 256, 256))


def test_every_binary16_bit_pattern_is_copied_as_it_is(torch):
    bits = np.arange(65536).reshape(256, 256)
    texels = np.stack([(bits + 16384 * k) % 65536 for k in range(4)], axis=2).astype(np.uint16)
    out = run_copy(torch, texels, tm.RGBA16_SFLOAT, (0, 0, 256, 256), (256, 256), (0, 0, 256, 256))
    assert np.array_equal(out, texels)  # signalling NaNs, payloads, denormals, both zeros


# ---- scaled ----
@pytest.mark.parametrize("fmt", tm.SOURCE_FORMATS, ids=FORMAT_IDS.get)
@pytest.mark.parametrize("src_extent,dst_extent", [((1, 1), (7, 5)), ((3, 2), (13, 9)), ((64, 64), (8, 8))], ids=["1x1-7x5", "3x2-13x9", "64x64-8x8"])
def test_scaled(torch, fmt, src_extent, dst_extent):
    texels = random_source(fmt, *src_extent)
    run_copy(torch, texels, fmt, (0, 0) + src_extent, dst_extent, (0, 0) + dst_extent)


@pytest.mark.parametrize("fmt", tm.SOURCE_FORMATS, ids=FORMAT_IDS.get)
@pytest.mark.parametrize("dst_shift", [0, 1], ids=["aligned", "base+8B"])
def test_offsets_padded_pitches_and_a_base_that_leaves_no_row_16_byte_aligned(torch, fmt, dst_shift):
    """Region (1, 2, 3, 4) of 5 x 7 onto region (3, 1, 10, 6) of 16 x 9. dst_pad 2 keeps the pitch a multiple of 16 bytes, so
    with the base moved by one texel the first texel of every row sits 8 bytes after a 16-byte boundary; the region's x = 3
    then starts on a boundary and x = 3 of the unmoved image does not."""
    texels = random_source(fmt, 5, 7)
    run_copy(torch, texels, fmt, (1, 2, 3, 4), (16, 9), (3, 1, 10, 6), src_pad=3, dst_pad=2, dst_shift=dst_shift)
    run_copy(torch, texels, fmt, (1, 2, 3, 4), (16, 9), (3, 1, 10, 6), src_pad=1, dst_pad=3, dst_shift=dst_shift)  # pitch % 16 == 8


@pytest.mark.parametrize("width", [1, 2, 3, 4, 5, 257])
def test_destination_widths(torch, width):
    """257 texels are 129 groups of 16 bytes: more than one wave, and with the base moved by 8 bytes a group on each edge"""
    texels = random_source(tm.RGBA8_SRGB, 9, 3)
    for shift in (0, 1):
        run_copy(torch, texels, tm.RGBA8_SRGB, (0, 0, 9, 3), (width, 4), (0, 0, width, 4), dst_shift=shift)


def test_a_destination_wider_than_one_workgroup(torch):
    """A workgroup covers 256 groups = 512 texels: 1027 texels take three, the last one partly"""
    texels = random_source(tm.RGBA8_UNORM, 100, 2)
    run_copy(torch, texels, tm.RGBA8_UNORM, (0, 0, 100, 2), (1027, 3), (0, 0, 1027, 3), dst_pad=1)


@pytest.mark.parametrize("height", [ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1])
def test_heights_around_the_rows_per_lane(torch, height):
    texels = random_source(tm.RGBA16_UNORM, 4, 5)
    run_copy(torch, texels, tm.RGBA16_UNORM, (0, 0, 4, 5), (6, height), (0, 0, 6, height), dst_pad=1)


# ---- clear ----
COLOR = (1.0 / 3.0, -1.0, 2.0, float("nan"))


@pytest.mark.parametrize("fmt", [tm.RGBA16_SFLOAT, tm.RGBA16_UNORM], ids=FORMAT_IDS.get)
@pytest.mark.parametrize("extent,pad,shift", [((5, 3), 2, 0), ((5, 3), 1, 1), ((1, 1), 0, 1), ((515, ROWS + 1), 3, 0)],
                         ids=["5x3", "5x3-base+8B", "1x1", "515x9"])
def test_clear(torch, fmt, extent, pad, shift):
    image = Buffer(torch, extent[0], extent[1], fmt, pad=pad, shift=shift, seed=6)
    im = image.abi()
    assert lib().szg_record_clear_color_image(None, C.byref(im), (C.c_float * 4)(*COLOR)) == abi.SZG_OK, lib().szg_last_error()
    texel = tm.clear_texel(fmt, COLOR)
    want, got = image.put(image.flat0, np.broadcast_to(texel, (extent[1], extent[0], 4))), image.read()
    assert np.array_equal(got, want), first_difference(got, want)  # the padding keeps its sentinels
    if fmt == tm.RGBA16_SFLOAT:
        assert texel[:3].tolist() == [0x3555, 0xBC00, 0x4000] and texel[3] & 0x7C00 == 0x7C00 and texel[3] & 0x3FF  # kept
    else:
        assert texel.tolist() == [21845, 0, 65535, 0]  # clamped, NaN -> 0


# ---- refusals: nothing launched, nothing written ----
def test_refusals_write_nothing_and_empty_regions_are_ok(torch):
    src = Buffer(torch, 64, 32, tm.RGBA8_UNORM, seed=7)
    dst = Buffer(torch, 48, 24, tm.RGBA16_SFLOAT, seed=8)
    S, D = src.device.data_ptr(), dst.device.data_ptr()

    def ref(x):
        return C.byref(x) if x is not None else None

    def untouched(what):
        assert np.array_equal(dst.read(), dst.flat0) and np.array_equal(src.read(), src.flat0), what

    for name, s_im, d_im, sr, dr in tc.copy_refusals(S, D):
        assert lib().szg_record_copy_image(None, ref(s_im), ref(d_im), abi.Rect(*sr), abi.Rect(*dr)) == abi.SZG_ERR_INVALID_ARGUMENT, name
        assert b"szg_record_copy_image" in lib().szg_last_error(), name
    untouched("copy refusals")
    for name, im, color in tc.clear_refusals(D):
        cc = (C.c_float * 4)(*color) if color is not None else None
        assert lib().szg_record_clear_color_image(None, ref(im), cc) == abi.SZG_ERR_INVALID_ARGUMENT, name
    untouched("clear refusals")
    s_im, d_im = src.abi(), dst.abi()
    for sr, dr in tc.EMPTY_REGIONS:
        assert lib().szg_record_copy_image(None, C.byref(s_im), C.byref(d_im), abi.Rect(*sr), abi.Rect(*dr)) == abi.SZG_OK
    untouched("empty regions")
    # and after all that the same images copy
    assert lib().szg_record_copy_image(None, C.byref(s_im), C.byref(d_im), abi.Rect(0, 0, 64, 32), abi.Rect(0, 0, 48, 24)) == abi.SZG_OK
    want = dst.put(dst.flat0, tm.copy_image(src.image0(), tm.RGBA8_UNORM, (0, 0, 64, 32), dst.image0(), (0, 0, 48, 24)))
    assert np.array_equal(dst.read(), want)


# ---- the stream argument ----
class CopyAndClearCase:
    """One copy and one clear through the Python mirror on a non-blocking stream (tests/stream_order.py): inputs and the
    destinations' sentinels reach the device in stream order, behind the blocker."""
    id = "image-copy-and-clear"
    conditions = True

    def setup(self, gpu):
        return types.SimpleNamespace()

    def prepare(self, gpu, state, variant):
        torch = gpu.torch
        rng = np.random.default_rng(40 + variant)
        r = types.SimpleNamespace()
        r.texels = rng.integers(0, 256, (33, 47, 4), dtype=np.uint8)
        r.dst0 = rng.integers(0, 65536, (70, 131 + 3, 4), dtype=np.uint16)
        r.clr0 = rng.integers(0, 65536, (19, 37 + 2, 4), dtype=np.uint16)
        r.color = (0.25 * variant, 1.0 / 3.0, -2.0, 1.0)
        r.staged = [so.staged_tensor(torch, a) for a in (r.texels, r.dst0.view(np.float16), r.clr0.view(np.float16))]
        r.live = [torch.zeros_like(t) for t in r.staged]
        r.want_dst = r.dst0.copy()
        r.want_dst[:, :131] = tm.copy_image(r.texels, tm.RGBA8_SRGB, (2, 1, 40, 30), r.dst0[:, :131], (5, 3, 120, 61))
        r.want_clr = r.clr0.copy()
        r.want_clr[:, :37] = tm.clear_texel(tm.RGBA16_SFLOAT, r.color)
        return r

    def enqueue(self, gpu, state, r, S):
        for live, staged in zip(r.live, r.staged):
            live.copy_(staged)
        gpu.pl.record_copy_image(S, r.live[0], r.live[1][:, :131], srcRegion=(2, 1, 40, 30), dstRegion=(5, 3, 120, 61), srgb=True)
        gpu.pl.record_clear_color_image(S, r.live[2][:, :37], r.color)

    def check(self, gpu, state, r, what):
        got_dst = r.live[1].cpu().numpy().view(np.uint16)
        got_clr = r.live[2].cpu().numpy().view(np.uint16)
        assert np.array_equal(got_dst, r.want_dst), f"{what}: copy: {first_difference(got_dst, r.want_dst)}"
        assert np.array_equal(got_clr, r.want_clr), f"{what}: clear: {first_difference(got_clr, r.want_clr)}"
        assert np.array_equal(r.live[0].cpu().numpy(), r.texels), f"{what}: the source was written"

    def teardown(self, gpu, state):
        pass


def test_copy_and_clear_on_a_non_blocking_stream_behind_and_beside_a_blocker(torch):
    from syzygy_amd import pipelines

    gpu = types.SimpleNamespace(torch=torch, pl=pipelines)
    gpu.blocker = so.Blocker(torch)
    try:
        so.run_case(gpu, CopyAndClearCase())
    finally:
        del gpu.blocker
        torch.cuda.synchronize()
