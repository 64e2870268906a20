"""include/szg/jpeg.h on the GPU, bit for bit: k_jpeg_idct and k_jpeg_color against tests/jpeg_model.py from random coefficient
planes (no file involved), pipelines.decode_jpeg against the recorded outputs of the reference's decoder, the padding, mask,
refusal and stream-order rules of szg_record_jpeg_reconstruct."""
import ctypes as C

import numpy as np
import pytest

from syzygy_amd import abi, lib
from tests import jpeg_fixtures as jf
from tests import jpeg_model as jm
from tests import mipmap_model as mm

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (33, 31), (65, 8), (130, 70)]  # the last two: more than 8 blocks per row (tail group)
LAYOUTS = {
    "grey": ([(1, 1)], abi.SZG_JPEG_GREY),
    "h1v1": ([(1, 1), (1, 1), (1, 1)], abi.SZG_JPEG_YCBCR),
    "h2v1": ([(2, 1), (1, 1), (1, 1)], abi.SZG_JPEG_YCBCR),
    "h1v2": ([(1, 2), (1, 1), (1, 1)], abi.SZG_JPEG_YCBCR),
    "h2v2": ([(2, 2), (1, 1), (1, 1)], abi.SZG_JPEG_YCBCR),
    "h4v1": ([(4, 1), (1, 1), (1, 1)], abi.SZG_JPEG_YCBCR),
    "rgb": ([(1, 1), (1, 1), (1, 1)], abi.SZG_JPEG_RGB),
}
RANGES = ("realistic", "dense", "full")


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    from syzygy_amd import pipelines

    class Ctx:
        pass

    c = Ctx()
    c.pl, c.torch = pipelines, torch
    return c


def _planes(width, height, factors, kind, seed):
    """random int16 coefficient planes [blocks_h, blocks_w, 8, 8] for every component"""
    rng = np.random.default_rng(seed)
    h_max, v_max = max(f[0] for f in factors), max(f[1] for f in factors)
    out = []
    for h, v in factors:
        bw, bh, _, _ = jm.plane_grid(width, height, h, v, h_max, v_max)
        shape = (bh, bw, 8, 8)
        if kind == "realistic":  # |c| <= 2047, mostly zero, a DC term everywhere
            c = rng.integers(-2047, 2048, shape) * (rng.random(shape) < 0.15)
            c[..., 0, 0] = rng.integers(-1024, 1024, (bh, bw))
        elif kind == "dense":
            c = rng.integers(-300, 301, shape)
        else:  # the whole int16 range: reaches the wrap rule
            c = rng.integers(-32768, 32768, shape)
            c.reshape(-1)[:4] = [32767, -32768, 32767, -32768]
        out.append(np.ascontiguousarray(c, dtype=np.int16))
    return out


def _device_frame(gpu, width, height, factors, color, planes):
    tensors = [gpu.torch.from_numpy(p.reshape(-1)).cuda() for p in planes]
    return jf.make_frame(width, height, factors, color, [t.data_ptr() for t in tensors]), tensors


def _model(width, height, factors, color, planes, rgba_and=0xFFFFFFFF, rgba_or=0):
    frame = {"width": width, "height": height, "color": jm.COLOR_NAMES[color],
             "planes": [(h, v, p) for (h, v), p in zip(factors, planes)]}
    return jm.reconstruct(frame, rgba_and, rgba_or)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("size", SIZES)
def test_kernels_equal_the_model_from_coefficients(gpu, size, layout):
    w, h = size
    factors, color = LAYOUTS[layout]
    for kind in RANGES:
        planes = _planes(w, h, factors, kind, seed=w * 131 + h * 7 + len(layout) + RANGES.index(kind))
        frame, keep = _device_frame(gpu, w, h, factors, color, planes)
        out = gpu.torch.full((h, w, 4), 0xEE, dtype=gpu.torch.uint8, device="cuda")
        gpu.pl.record_jpeg_reconstruct(frame, out)
        gpu.torch.cuda.synchronize()
        got, want = out.cpu().numpy(), _model(w, h, factors, color, planes)
        assert np.array_equal(got, want), f"{kind}: {(got != want).sum()} of {got.size} bytes differ"


def test_host_reconstruction_equals_the_kernels_on_the_full_range(gpu):
    w, h = 33, 31
    factors, color = LAYOUTS["h2v2"]
    planes = _planes(w, h, factors, "full", seed=99)
    host_frame = jf.make_frame(w, h, factors, color, [p.ctypes.data for p in planes])
    host = np.zeros((h, w, 4), np.uint8)
    assert lib().szg_jpeg_reconstruct_host(C.byref(host_frame), 0xFFFFFFFF, 0, host.ctypes.data_as(C.c_void_p), w * 4) == abi.SZG_OK
    frame, keep = _device_frame(gpu, w, h, factors, color, planes)
    out = gpu.torch.zeros((h, w, 4), dtype=gpu.torch.uint8, device="cuda")
    gpu.pl.record_jpeg_reconstruct(frame, out)
    gpu.torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(host, _model(w, h, factors, color, planes))


END_TO_END = [n for n in jf.names() if "_33x31_" in n or n.startswith(("h1v2_33x33", "h4v1_33x16", "h1v4_15x31", "rgbids_", "adobe0_"))]


def test_end_to_end_equals_the_reference(gpu):
    assert len(END_TO_END) == 4 * 3 * 2 + 5
    for name in END_TO_END:
        got = gpu.pl.decode_jpeg(jf.data(name))
        gpu.torch.cuda.synchronize()
        assert got.dtype == gpu.torch.uint8 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), jf.expected(name)), name


def test_padding_scratch_and_coefficients_are_left_alone(gpu):
    w, h = 33, 31
    for layout in ("h2v2", "grey", "h2v1"):
        factors, color = LAYOUTS[layout]
        planes = _planes(w, h, factors, "realistic", seed=5)
        frame, keep = _device_frame(gpu, w, h, factors, color, planes)
        need = lib().szg_jpeg_scratch_bytes(C.byref(frame))
        assert need == sum(p.size for p in planes)
        scratch = gpu.torch.full((need + 512,), 0xEE, dtype=gpu.torch.uint8, device="cuda")
        # allocated 41 x 37 texels with 12 bytes of row padding; the frame is drawn into its top-left 33 x 31
        alloc_w, alloc_h, pitch = 41, 37, 41 * 4 + 12
        raw = gpu.torch.full((alloc_h, pitch), 0xEE, dtype=gpu.torch.uint8, device="cuda")
        im = abi.Image()
        im.data, im.width, im.height, im.pitch_bytes, im.format = raw.data_ptr(), alloc_w, alloc_h, pitch, abi.SZG_FORMAT_RGBA8_UNORM
        status = lib().szg_record_jpeg_reconstruct(C.c_void_p(gpu.torch.cuda.current_stream().cuda_stream), C.byref(frame),
                                                   C.c_void_p(scratch.data_ptr()), need, 0xFFFFFFFF, 0, C.byref(im))
        assert status == abi.SZG_OK, lib().szg_last_error()
        gpu.torch.cuda.synchronize()
        got = raw.cpu().numpy()
        inside = got[:h, :w * 4].reshape(h, w, 4)
        assert np.array_equal(inside, _model(w, h, factors, color, planes)), layout
        outside = got.copy()
        outside[:h, :w * 4] = 0xEE
        assert (outside == 0xEE).all(), layout
        assert (scratch[need:] == 0xEE).all().item(), layout
        # the sample planes are the model's, MCU padding included
        at = 0
        s = scratch.cpu().numpy()
        for p in planes:
            assert np.array_equal(s[at:at + p.size], jm.sample_plane(p).reshape(-1)), layout
            at += p.size
        for t, p in zip(keep, planes):
            assert np.array_equal(t.cpu().numpy(), p.reshape(-1)), layout


def test_masks_equal_the_host_loaders_overrides(gpu):
    name = "420_33x31_base_q92"
    want = jf.expected(name)
    red = gpu.pl.decode_jpeg(jf.data(name), 0xFFFFFF00, 0x000000FF).cpu().numpy()
    override = want.copy()
    override[..., 0] = 255
    assert np.array_equal(red, override)
    occ = gpu.pl.decode_jpeg(jf.data(name), 0xFF0000FF, 0).cpu().numpy()
    override = want.copy()
    override[..., 1:3] = 0
    assert np.array_equal(occ, override)
    with jf.Jpeg(jf.data(name)) as j:
        assert np.array_equal(occ.reshape(31, -1), j.reconstruct_host(0xFF0000FF, 0))


def test_refusals_leave_the_outputs_untouched(gpu):
    w, h = 17, 9
    factors, color = LAYOUTS["h2v2"]
    planes = _planes(w, h, factors, "dense", seed=3)
    frame, keep = _device_frame(gpu, w, h, factors, color, planes)
    need = lib().szg_jpeg_scratch_bytes(C.byref(frame))
    scratch = gpu.torch.full((need + 64,), 0xEE, dtype=gpu.torch.uint8, device="cuda")
    out = gpu.torch.full((h + 1, w + 1, 4), 0xEE, dtype=gpu.torch.uint8, device="cuda")
    stream = C.c_void_p(gpu.torch.cuda.current_stream().cuda_stream)

    def image(**change):
        im = abi.Image()
        im.data, im.width, im.height, im.pitch_bytes, im.format = out.data_ptr(), w + 1, h + 1, (w + 1) * 4, abi.SZG_FORMAT_RGBA8_UNORM
        for k, v in change.items():
            setattr(im, k, v)
        return im

    def changed(**change):
        f = abi.JpegFrame.from_buffer_copy(frame)
        for k, v in change.items():
            target, _, field = k.rpartition("__")
            setattr(f.planes[int(target[-1])] if target else f, field, v)
        return f

    def call(f=frame, s=scratch.data_ptr(), n=need, im=None, fp=True, ip=True):
        im = image() if im is None else im
        return lib().szg_record_jpeg_reconstruct(stream, C.byref(f) if fp else None, C.c_void_p(s), n, 0xFFFFFFFF, 0,
                                                 C.byref(im) if ip else None)

    cases = {
        "NULL frame": lambda: call(fp=False),
        "NULL scratch": lambda: call(s=None),
        "NULL image": lambda: call(ip=False),
        "NULL image data": lambda: call(im=image(data=None)),
        "NULL coefficients": lambda: call(changed(plane1__coefficients=None)),
        "plane_count 2": lambda: call(changed(plane_count=2)),
        "plane_count 4": lambda: call(changed(plane_count=4)),
        "grey with three planes": lambda: call(changed(color=abi.SZG_JPEG_GREY)),
        "width 0": lambda: call(changed(width=0)),
        "height above the limit": lambda: call(changed(height=32769)),
        "wider than its planes": lambda: call(changed(width=w + 16)),
        "taller than its planes": lambda: call(changed(height=h + 16)),
        "h_max": lambda: call(changed(h_max=1)),
        "v_max": lambda: call(changed(v_max=4)),
        "factor 0": lambda: call(changed(plane1__h=0)),
        "factor 5": lambda: call(changed(plane2__v=5)),
        "factor that does not divide": lambda: call(changed(plane0__h=3, h_max=3, plane1__h=2)),
        "blocks_w too large": lambda: call(changed(plane0__blocks_w=frame.planes[0].blocks_w + 1)),
        "blocks_h too small": lambda: call(changed(plane2__blocks_h=frame.planes[2].blocks_h - 1)),
        "plane width": lambda: call(changed(plane1__width=frame.planes[1].width + 1)),
        "plane height": lambda: call(changed(plane1__height=frame.planes[1].height - 1)),
        "small scratch": lambda: call(n=need - 1),
        "misaligned scratch": lambda: call(s=scratch.data_ptr() + 8),
        "misaligned coefficients": lambda: call(changed(plane0__coefficients=frame.planes[0].coefficients + 2)),
        "misaligned image": lambda: call(im=image(data=out.data_ptr() + 2)),
        "wrong format": lambda: call(im=image(format=abi.SZG_FORMAT_BGRA8_UNORM)),
        "narrow image": lambda: call(im=image(width=w - 1)),
        "short image": lambda: call(im=image(height=h - 1)),
        "pitch below a row": lambda: call(im=image(pitch_bytes=w * 4)),
        "pitch no multiple of 4": lambda: call(im=image(pitch_bytes=(w + 1) * 4 + 2)),
    }
    for name, refuse in cases.items():
        assert refuse() == abi.SZG_ERR_INVALID_ARGUMENT, name
        assert lib().szg_last_error().startswith(b"szg_record_jpeg_reconstruct:"), name
    gpu.torch.cuda.synchronize()
    assert (out == 0xEE).all().item() and (scratch == 0xEE).all().item()
    for t, p in zip(keep, planes):
        assert np.array_equal(t.cpu().numpy(), p.reshape(-1))
    # and the unchanged call is accepted
    assert call() == abi.SZG_OK
    gpu.torch.cuda.synchronize()
    assert np.array_equal(out[:h, :w].cpu().numpy(), _model(w, h, factors, color, planes))
    assert (out[h:] == 0xEE).all().item() and (out[:, w:] == 0xEE).all().item()


@pytest.mark.parametrize("srgb", [False, True])
def test_mip_chain_behind_the_reconstruction_on_one_stream(gpu, srgb):
    name = "420_130x70_prog_q92"
    want = jf.expected(name)
    with jf.Jpeg(jf.data(name)) as j:
        frame, keep = gpu.pl.upload_jpeg_frame(j.frame)
    out = gpu.torch.zeros((70, 130, 4), dtype=gpu.torch.uint8, device="cuda")
    stream = gpu.torch.cuda.Stream()
    stream.wait_stream(gpu.torch.cuda.current_stream())
    with gpu.torch.cuda.stream(stream):
        scratch = gpu.pl.record_jpeg_reconstruct(frame, out, cmd=stream)
        chain = gpu.pl.generate_mipmaps(out, srgb, cmd=stream)  # no synchronisation between the two records
    stream.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(chain.cpu().numpy(), mm.pack_chain(mm.build_chain(want, srgb)))
    del scratch, keep
