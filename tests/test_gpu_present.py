"""The present pass on the GPU (include/szg/present.h, syzygy_amd/csrc/kernels_present.hip): the kernels against the CPU
model of tests/present_model.py, bit for bit, over formats x filters x encodes; untouched bytes outside the region; the
encode against the szg_record_oetf chain; the C++ shim; every refusal; both libraries; one example run."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from syzygy_amd import abi, lib
from tests import gpu_present_child as child
from tests import native
from tests import present_model as pm
from tests.test_present_model import SCALED_CASES, refusal_cases, region_of

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

FILTERS = (pm.LINEAR, pm.NEAREST)
ENCODES = (abi.SZG_PRESENT_ENCODE_NONE, abi.SZG_OETF_PURE_GAMMA, abi.SZG_OETF_SRGB)


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def tables():
    """encode -> the model's table (None for no encoding): the CPU oracle's OETF, which szg_record_oetf equals bit for bit
    (tests/test_gpu_parity.py)."""
    return {abi.SZG_PRESENT_ENCODE_NONE: None, abi.SZG_OETF_PURE_GAMMA: pm.oetf_table(abi.SZG_OETF_PURE_GAMMA),
            abi.SZG_OETF_SRGB: pm.oetf_table(abi.SZG_OETF_SRGB)}


def noise(width, height, seed=1):
    return np.random.default_rng(seed).integers(0, 65536, (height, width, 4), dtype=np.uint16)


def pattern(count):
    """`count` bytes that differ from their neighbours and from zero."""
    return np.resize(((np.arange(251, dtype=np.int64) * 37 + 11) % 251 + 1).astype(np.uint8), count)


class DeviceImage:
    """A flat device buffer with a strided image inside it: `offset_texels` before the first texel, `pitch_texels` per row,
    so that tests choose where rows start. Keeps the host copy of the initial bytes."""

    def __init__(self, torch, width, height, texel_bytes, pitch_texels=None, offset_texels=0, fill=None):
        self.torch, self.width, self.height, self.tb = torch, width, height, texel_bytes
        self.pitch = width if pitch_texels is None else pitch_texels
        self.offset = offset_texels
        assert self.pitch >= width
        self.count = (self.offset + self.pitch * height + 3) * texel_bytes  # a few bytes of slack behind the last row
        self.initial = pattern(self.count) if fill is None else fill
        self.flat = None
        self.upload()

    def upload(self):
        self.flat = self.torch.from_numpy(self.initial).cuda()

    def rows(self, host_bytes):
        """[height, width * tb] view of the image's bytes inside a host copy of the buffer."""
        start = self.offset * self.tb
        body = host_bytes[start:start + self.pitch * self.height * self.tb].reshape(self.height, self.pitch * self.tb)
        return body[:, :self.width * self.tb]

    def image(self, fmt):
        return abi.Image(self.flat.data_ptr() + self.offset * self.tb, self.width, self.height, self.pitch * self.tb, fmt)

    def download(self):
        return self.flat.cpu().numpy()


def upload_source(torch, src, pitch_texels=None, offset_texels=0):
    H, W, _ = src.shape
    image = DeviceImage(torch, W, H, 8, pitch_texels, offset_texels, fill=np.zeros(0, np.uint8))
    image.initial = pattern(image.count)
    image.rows(image.initial)[:] = src.reshape(H, W * 4).view(np.uint8)
    image.upload()
    return image


def record(torch, src_image, dst_image, fmt, src_region, dst_region, filter, encode):
    s, d = src_image.image(abi.SZG_FORMAT_RGBA16_UNORM), dst_image.image(fmt)
    info = abi.PresentInfo(abi.Rect(*src_region), abi.Rect(*dst_region), filter, encode)
    status = lib().szg_record_present(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(s), C.byref(d), C.byref(info))
    torch.cuda.synchronize()
    return status


def expected_bytes(dst_image, fmt, codes, dst_region):
    """The destination buffer's initial bytes with the model's texels in dst_region."""
    want = dst_image.initial.copy()
    dx, dy, dw, dh = dst_region
    texels = pm.pack(codes, fmt)
    raw = texels.view(np.uint8).reshape(dh, dw * 4) if fmt == pm.A2B10G10R10 else texels.reshape(dh, dw * 4)
    dst_image.rows(want)[dy:dy + dh, dx * 4:(dx + dw) * 4] = raw
    return want


def check_all_combinations(torch, tables, src, src_region, dst_extent, dst_region=None, src_layout=(None, 0), dst_layout=(None, 0),
                           formats=pm.FORMATS, filters=FILTERS, encodes=ENCODES):
    """Kernel == model for formats x filters x encodes on one geometry; every byte of the destination buffer outside the
    region and every byte of the source buffer must keep its value."""
    dw, dh = dst_extent
    dst_region = (0, 0, dw, dh) if dst_region is None else dst_region
    src_image = upload_source(torch, src, *src_layout)
    for filter in filters:
        for encode in encodes:
            by_bits = pm.filtered_codes_by_bits(src, src_region, dst_region[2], dst_region[3], formats, filter, tables[encode])
            for fmt in formats:
                dst_image = DeviceImage(torch, dw, dh, 4, *dst_layout)
                assert record(torch, src_image, dst_image, fmt, src_region, dst_region, filter, encode) == abi.SZG_OK, \
                    lib().szg_last_error()
                got = dst_image.download()
                want = expected_bytes(dst_image, fmt, by_bits[pm.channel_bits(fmt)], dst_region)
                if not np.array_equal(got, want):
                    bad = np.nonzero(got != want)[0]
                    pytest.fail(f"fmt {fmt} filter {filter} encode {encode}: {len(bad)} of {len(got)} bytes differ, first at "
                                f"{bad[0]} (got {got[bad[0]]}, want {want[bad[0]]})")
    assert np.array_equal(src_image.download(), src_image.initial), "the source was written"


@pytest.mark.parametrize("case", SCALED_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}{'r' if c[1] else ''}-{c[2][0]}x{c[2][1]}")
def test_kernel_equals_model_on_the_scaled_cases(torch, tables, case):
    (W, H), corners, dst_extent = case
    check_all_combinations(torch, tables, noise(W, H), region_of((W, H), corners), dst_extent)


@pytest.mark.parametrize("width", [1, 2, 3, 5, 4097])
def test_kernel_equals_model_on_odd_widths(torch, tables, width):
    src = noise(width, 9, seed=width)
    check_all_combinations(torch, tables, src, (0, 0, width, 9), (width, 9))  # 1:1
    wide = noise(33, 7, seed=width + 100)
    check_all_combinations(torch, tables, wide, (0, 0, 33, 7), (width, 11))  # scaled onto the odd width
    check_all_combinations(torch, tables, src, (0, 0, width, 9), (40, 5))  # scaled from the odd width


def test_kernel_equals_model_at_the_extremes_of_scale(torch, tables):
    one = noise(1, 1, seed=11)
    check_all_combinations(torch, tables, one, (0, 0, 1, 1), (64, 64))
    check_all_combinations(torch, tables, noise(64, 64, seed=12), (0, 0, 64, 64), (1, 1))


def test_kernel_equals_model_on_every_code_one_to_one(torch, tables):
    codes = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    src = np.stack([codes, codes[::-1], codes.T, codes[:, ::-1]], axis=-1).copy()
    check_all_combinations(torch, tables, src, (0, 0, 256, 256), (256, 256))


@pytest.mark.parametrize("extent", [((3840, 2160), (3840, 2160)), ((7680, 4320), (3840, 2160))], ids=["4k-1to1", "8k-to-4k"])
def test_kernel_equals_model_on_large_frames(torch, tables, extent):
    (W, H), dst_extent = extent
    check_all_combinations(torch, tables, noise(W, H), (0, 0, W, H), dst_extent)


@pytest.mark.parametrize("scaled", [False, True], ids=["one_to_one", "scaled"])
def test_every_row_alignment_phase(torch, tables, scaled):
    """Region offsets and pitches that put the first texel of a row at every 8-B phase (source) and every 4-B phase
    (destination) of a 16-B line, with pitches that change the phase from row to row; all bytes outside the region,
    pitch padding included, keep their pattern (check_all_combinations compares the whole buffer)."""
    src = noise(41, 13, seed=21)
    for src_offset in (0, 1):
        for src_pitch in (41, 42):
            for dst_offset in (0, 1, 2, 3):
                for dst_pitch_extra in (0, 1, 2, 4):
                    for width in (1, 2, 4, 7, 8, 9, 19):
                        x = (dst_offset + width) % 5
                        src_region = (2 + src_offset, 1, 23 if scaled else width, 9 if scaled else 11)
                        dst_extent = (x + width + 3, 13)
                        check_all_combinations(
                            torch, tables, src, src_region, dst_extent, (x, 1, width, 11), (src_pitch, src_offset),
                            (dst_extent[0] + dst_pitch_extra, dst_offset), formats=(pm.BGRA8, pm.A2B10G10R10),
                            encodes=(abi.SZG_PRESENT_ENCODE_NONE, abi.SZG_OETF_SRGB))


def test_offset_regions_inside_padded_images(torch, tables):
    """A subregion of a padded source onto a subregion of a padded destination, larger than one block's columns."""
    src = noise(1300, 90, seed=31)
    check_all_combinations(torch, tables, src, (13, 7, 1111, 70), (1400, 100), (5, 3, 1111, 70), (1307, 3), (1411, 2))
    check_all_combinations(torch, tables, src, (13, 7, 1111, 70), (1400, 100), (5, 3, 1290, 91), (1307, 3), (1411, 2))


@pytest.mark.parametrize("function", [abi.SZG_OETF_PURE_GAMMA, abi.SZG_OETF_SRGB], ids=["pure_gamma", "srgb"])
@pytest.mark.parametrize("geometry", [((640, 360), (0, 0, 640, 360), (640, 360)), ((640, 360), (9, 4, 600, 333), (1337, 911))],
                         ids=["one_to_one", "scaled"])
def test_encode_equals_oetf_then_plain_present(torch, function, geometry):
    """szg_record_present with an encode == szg_record_oetf over the whole of a COPY of the source, then a plain present."""
    from syzygy_amd import pipelines as pl

    (W, H), region, (dw, dh) = geometry
    src = torch.from_numpy(noise(W, H, seed=41).view(np.int16)).cuda()
    before = src.clone()
    for fmt in pm.FORMATS:
        for filter in FILTERS:
            fused = pl.swapchain_image(dw, dh, fmt)
            pl.record_copy_image_to_image(None, src, fused, region, None, filter, function, fmt)
            copy = src.clone()
            image = pl.present_images(copy, fused, fmt)[0]
            assert lib().szg_record_oetf(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(image), W, H, function) == 0
            chained = pl.swapchain_image(dw, dh, fmt)
            pl.record_copy_image_to_image(None, copy, chained, region, None, filter, abi.SZG_PRESENT_ENCODE_NONE, fmt)
            torch.cuda.synchronize()
            assert torch.equal(fused, chained), (fmt, filter)
            assert not torch.equal(copy, src)
    assert torch.equal(src, before), "the encode must leave the source linear"


@pytest.mark.parametrize("case", refusal_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_refusals_write_nothing(torch, case):
    name = case[0]
    src_buffer = DeviceImage(torch, 64, 32, 8)
    dst_buffer = DeviceImage(torch, 48, 24, 4)
    # the same case over real device memory (the overlap cases point the other image into the source buffer)
    _, src, dst, info = next(c for c in refusal_cases(src_buffer.flat.data_ptr(), dst_buffer.flat.data_ptr()) if c[0] == name)
    status = lib().szg_record_present(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(src) if src is not None else None,
                                      C.byref(dst) if dst is not None else None, C.byref(info) if info is not None else None)
    torch.cuda.synchronize()
    assert status == abi.SZG_ERR_INVALID_ARGUMENT, name
    message = lib().szg_last_error()
    assert b"szg_record_present" in message and len(message) > len(b"szg_record_present: "), name
    assert np.array_equal(dst_buffer.download(), dst_buffer.initial) and np.array_equal(src_buffer.download(), src_buffer.initial)


def test_python_wrappers_take_strided_tensors(torch, tables):
    """record_copy_image_to_image on a padded uint8 view and an int32 view; record_present = OETF over the top-left
    destination extent + LINEAR blit of the subregion."""
    from syzygy_amd import pipelines as pl

    src_np = noise(320, 200, seed=51)
    src = torch.from_numpy(src_np.view(np.int16)).cuda()
    backing = torch.full((120, 200, 4), 0x5A, dtype=torch.uint8, device="cuda")
    view = backing[:, :160]
    pl.record_copy_image_to_image(None, src, view, (10, 20, 300, 170), (4, 6, 150, 100), abi.SZG_FILTER_LINEAR)
    torch.cuda.synchronize()
    want = pm.present(src_np, (10, 20, 300, 170), np.full((120, 200, 4), 0x5A, np.uint8), (4, 6, 150, 100), pm.RGBA8)
    assert np.array_equal(backing.cpu().numpy(), want)
    words = torch.zeros((100, 150), dtype=torch.int32, device="cuda")
    pl.record_copy_image_to_image(None, src, words, None, None, abi.SZG_FILTER_NEAREST, abi.SZG_OETF_SRGB)
    torch.cuda.synchronize()
    want = pm.present(src_np, (0, 0, 320, 200), pm.empty_destination(150, 100, pm.A2B10G10R10), (0, 0, 150, 100),
                      pm.A2B10G10R10, pm.NEAREST, tables[abi.SZG_OETF_SRGB])
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want)
    # record_present: the scene texture is encoded over the top-left 150 x 100 only (editor.cpp:328-337), then blitted
    scene = pl.SceneTexture(320, 200)
    scene.color.copy_(src)
    swapchain = pl.swapchain_image(150, 100, abi.SZG_FORMAT_BGRA8_UNORM)
    pl.record_present(None, scene, (100, 50, 200, 140), swapchain, abi.SZG_OETF_SRGB, dstFormat=abi.SZG_FORMAT_BGRA8_UNORM)
    torch.cuda.synchronize()
    encoded = src_np.copy()
    encoded[:100, :150, :3] = tables[abi.SZG_OETF_SRGB][src_np[:100, :150, :3]]
    assert np.array_equal(scene.color_numpy(), encoded)
    want = pm.present(encoded, (100, 50, 200, 140), pm.empty_destination(150, 100, pm.BGRA8), (0, 0, 150, 100), pm.BGRA8)
    assert np.array_equal(swapchain.cpu().numpy(), want)
    with pytest.raises(ValueError):
        pl.record_copy_image_to_image(None, src, torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda"))


@pytest.fixture(scope="module")
def record_present_exe(torch):
    lib()  # built and loadable
    return native.build("cpp/record_present")


@pytest.mark.parametrize("fmt", pm.FORMATS)
def test_cpp_record_present_equals_the_python_chain(torch, tables, record_present_exe, tmp_path, fmt):
    """szg::recordPresent / recordPresentEncoded / the NEAREST recordCopyImageToImage from a C++ caller
    (tests/cpp/record_present.cpp) against pipelines.record_present on the same input and against the model."""
    from syzygy_amd import pipelines as pl

    W, H, sub, DW, DH = 400, 240, (37, 21, 301, 199), 333, 222
    src_np = noise(W, H, seed=61)
    src_np.tofile(tmp_path / "scene.bin")
    prefix = str(tmp_path / "out")
    r = subprocess.run([record_present_exe, str(tmp_path / "scene.bin"), str(W), str(H), *map(str, sub), str(DW), str(DH), str(fmt), prefix],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

    def load(name):
        raw = np.fromfile(prefix + name, dtype=np.uint8)
        return raw.view(np.uint32).reshape(DH, DW) if fmt == pm.A2B10G10R10 else raw.reshape(DH, DW, 4)

    scene = pl.SceneTexture(W, H)
    scene.color.copy_(torch.from_numpy(src_np.view(np.int16)))
    swapchain = pl.swapchain_image(DW, DH, fmt)
    pl.record_present(None, scene, sub, swapchain, abi.SZG_OETF_SRGB, dstFormat=fmt)
    torch.cuda.synchronize()
    python_chain = swapchain.cpu().numpy()
    assert np.array_equal(load(".present.bin").view(np.uint8), python_chain.view(np.uint8))
    assert np.array_equal(np.fromfile(prefix + ".scene.bin", dtype=np.uint16).reshape(H, W, 4), scene.color_numpy())
    encoded = src_np.copy()
    encoded[:DH, :DW, :3] = tables[abi.SZG_OETF_SRGB][src_np[:DH, :DW, :3]]  # the top-left DESTINATION extent, not `sub`
    empty = pm.empty_destination(DW, DH, fmt)
    assert np.array_equal(load(".present.bin"), pm.present(encoded, sub, empty, (0, 0, DW, DH), fmt))
    assert np.array_equal(load(".encoded.bin"), pm.present(src_np, sub, empty, (0, 0, DW, DH), fmt, pm.LINEAR, tables[abi.SZG_OETF_SRGB]))
    assert np.array_equal(np.fromfile(prefix + ".linear.bin", dtype=np.uint16).reshape(H, W, 4), src_np)
    assert np.array_equal(load(".nearest.bin"), pm.present(src_np, sub, empty, (0, 0, DW, DH), fmt, pm.NEAREST))


def run_child(literal):
    env = dict(os.environ)
    env.pop("SZG_HIP_LIBRARY", None)
    if literal:
        env["SZG_HIP_LIBRARY"] = os.path.join(ROOT, "syzygy_amd", "csrc", "libszg_hip_literal.so")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_present_child.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().split("\n")[-1])
    assert out["library"] == ("libszg_hip_literal.so" if literal else "libszg_hip.so"), out["library"]
    return out["digests"]


def test_both_libraries_give_the_models_bytes(torch, tables):
    """The present pass belongs to no contraction class: libszg_hip.so and libszg_hip_literal.so, each in a process of its
    own, produce identical bytes, and they are the model's."""
    product = run_child(literal=False)
    literal = run_child(literal=True)
    assert product == literal
    want = {}
    for name, extent, region, (dw, dh) in child.CASES:
        src = child.source(extent)
        for filter in child.FILTERS:
            for encode in child.ENCODES:
                by_bits = pm.filtered_codes_by_bits(src, region, dw, dh, pm.FORMATS, filter, tables[encode])
                for fmt in child.FORMATS:
                    texels = pm.pack(by_bits[pm.channel_bits(fmt)], fmt)
                    want[child.key(name, fmt, filter, encode)] = hashlib.sha256(texels.tobytes()).hexdigest()
    assert product == want


def read_ppm(path):
    with open(path, "rb") as f:
        magic, w, h, maxval = f.readline().split()
        assert magic == b"P6"
        data = np.frombuffer(f.read(), dtype=np.uint8 if int(maxval) < 256 else ">u2")
    return data.reshape(int(h), int(w), 3).astype(np.int64), int(maxval)


@pytest.mark.parametrize("option,fmt", [("200x120", pm.RGBA8), ("333x190:bgra8", pm.BGRA8), ("256x144:a2b10g10r10", pm.A2B10G10R10)])
def test_frame_loop_example_presents_on_the_gpu(torch, tmp_path, option, fmt):
    """examples/frame_loop.py --present writes the model's image of the frame's scene texture; without the switch it writes
    the high bytes of the scene colour, as before."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import frame_loop
    finally:
        sys.path.pop(0)
    common = ["--frames", "2", "--width", "256", "--height", "144", "--shadow-map", "512"]
    out = str(tmp_path / "presented.ppm")
    scene = frame_loop.main(common + ["--out", out, "--present", option])
    got, maxval = read_ppm(out)
    dw, dh = (int(v) for v in option.split(":")[0].split("x"))
    want = pm.filtered_codes(scene, (0, 0, 256, 144), dw, dh, fmt)
    assert maxval == (1023 if fmt == pm.A2B10G10R10 else 255) and np.array_equal(got, want[..., :3])
    plain = str(tmp_path / "plain.ppm")
    scene2 = frame_loop.main(common + ["--out", plain])
    got, maxval = read_ppm(plain)
    assert maxval == 255 and np.array_equal(got, scene2[..., :3].astype(np.int64) >> 8)


def test_render_gltf_example_presents_on_the_gpu(torch, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import render_gltf
    finally:
        sys.path.pop(0)
    out = str(tmp_path / "gltf.ppm")
    scene, covered = render_gltf.main(["--width", "320", "--height", "180", "--out", out, "--present", "480x270"])
    got, maxval = read_ppm(out)
    assert covered > 0 and maxval == 255
    assert np.array_equal(got, pm.filtered_codes(scene, (0, 0, 320, 180), 480, 270, pm.RGBA8)[..., :3])
