"""The compute-collection pipeline on the GPU (include/szg/compute_collection.h,
syzygy_amd/csrc/kernels_compute_collection.hip): the kernels against the CPU model of tests/compute_collection_model.py, bit
for bit, all four programs x the three kinds of block of the SPIR-V vectors, in both libraries; every byte outside the written
set unchanged; every row phase of the 16-B store; push-constant semantics of the byte block; every refusal; the Python
class; the examples."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from syzygy_amd import abi, lib
from syzygy_amd._lib import SzgError
from tests import compute_collection_model as model
from tests import gpu_compute_collection_child as child

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def blocks():
    return child.blocks()


def pattern(count):
    """`count` bytes that differ from their neighbours and from zero."""
    return np.resize(((np.arange(251, dtype=np.int64) * 37 + 11) % 251 + 1).astype(np.uint8), count)


def expected_buffer(initial, shader, block, extent, image_extent, pitch, offset):
    """The buffer's initial bytes with the model's texels in the written set."""
    (w, h), (iw, ih) = extent, image_extent
    cols, rows = model.written_extent(w, h, iw, ih)
    codes = model.unorm16(model.values(shader, block, w, h, np.arange(cols), np.arange(rows)))
    want = initial.copy()
    body = want[offset * 8: (offset + pitch * ih) * 8].reshape(ih, pitch * 8)
    body[:rows, : cols * 8] = codes.reshape(rows, cols * 4).view(np.uint8)
    return want


def run(torch, initial, shader, block, extent, image_extent, pitch, offset, after_record=None):
    flat = torch.from_numpy(initial).cuda()
    im = abi.Image(flat.data_ptr() + offset * 8, image_extent[0], image_extent[1], pitch * 8, abi.SZG_FORMAT_RGBA16_UNORM)
    raw = C.create_string_buffer(block, len(block))
    status = lib().szg_record_compute_collection(C.c_void_p(torch.cuda.current_stream().cuda_stream), model.SHADERS.index(shader),
                                                 raw, len(block), C.byref(im), extent[0], extent[1])
    if after_record is not None:
        after_record(raw)
    torch.cuda.synchronize()
    assert status == abi.SZG_OK, lib().szg_last_error()
    return flat.cpu().numpy()


def assert_same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        pytest.fail(f"{what}: {len(bad)} of {len(got)} bytes differ, first at {bad[0]} (got {got[bad[0]]}, want {want[bad[0]]})")


_DIGESTS = {}  # what the product library wrote in test_kernel_equals_model, for the comparison with the literal library


@pytest.mark.parametrize("case", child.CASES, ids=[c[0] for c in child.CASES])
def test_kernel_equals_model(torch, blocks, case):
    """Kernel == model with 0 differing bytes over the whole buffer, pre-filled with a pattern: the written set holds the
    model's codes and every byte outside it, pitch padding included, keeps its value."""
    name, extent, image_extent, pitch, offset = case
    count = child.buffer_bytes(image_extent, pitch, offset)
    initial = pattern(count)
    for (shader, kind), block in blocks.items():
        got = run(torch, initial, shader, block, extent, image_extent, pitch, offset)
        want = expected_buffer(initial, shader, block, extent, image_extent, pitch, offset)
        assert_same(got, want, f"{name} {shader} {kind}")
        # the child fills with one byte value: the digest of the model's image over that fill
        filled = expected_buffer(np.full(count, child.FILL, np.uint8), shader, block, extent, image_extent, pitch, offset)
        _DIGESTS[child.key(name, shader, kind)] = hashlib.sha256(filled.tobytes()).hexdigest()


def run_child(literal):
    env = dict(os.environ)
    env.pop("SZG_HIP_LIBRARY", None)
    if literal:
        env["SZG_HIP_LIBRARY"] = os.path.join(ROOT, "syzygy_amd", "csrc", "libszg_hip_literal.so")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_compute_collection_child.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().split("\n")[-1])
    assert out["library"] == ("libszg_hip_literal.so" if literal else "libszg_hip.so"), out["library"]
    return out["digests"]


def test_both_libraries_give_the_models_bytes(torch, blocks):
    """The pass belongs to no contraction class: libszg_hip.so and libszg_hip_literal.so, each in a process of its own,
    write identical bytes over every geometry, program and block, and they are the model's."""
    want = {}
    for name, extent, image_extent, pitch, offset in child.CASES:
        count = child.buffer_bytes(image_extent, pitch, offset)
        for (shader, kind), block in blocks.items():
            k = child.key(name, shader, kind)
            if k in _DIGESTS:
                want[k] = _DIGESTS[k]
                continue
            filled = expected_buffer(np.full(count, child.FILL, np.uint8), shader, block, extent, image_extent, pitch, offset)
            want[k] = hashlib.sha256(filled.tobytes()).hexdigest()
    literal = run_child(literal=True)
    product = run_child(literal=False)
    differing = sorted(k for k in want if literal.get(k) != want[k] or product.get(k) != want[k])
    assert not differing and set(literal) == set(want) == set(product), differing[:10]


def test_every_row_phase_of_the_store(torch, blocks):
    """Views whose first texel sits at either 8-B phase of a 16-B line, with pitches that keep or flip the phase from row to
    row, widths around the pair size, an extent below the image (spill) and equal to it."""
    for offset in (0, 1, 2, 3):
        for pitch_extra in (0, 1, 2, 3):
            for w in (1, 2, 3, 4, 15, 16, 17, 31, 33):
                for image_w in (w, w + 1, w + 20):
                    extent, image_extent = (w, 7), (image_w, 9 if image_w > w else 7)
                    pitch = image_w + pitch_extra
                    initial = pattern(child.buffer_bytes(image_extent, pitch, offset))
                    for shader, kind in (("booleanpush", "example"), ("gradient_color", "ordinary"), ("matrix_color", "ordinary")):
                        block = blocks[(shader, kind)]
                        got = run(torch, initial, shader, block, extent, image_extent, pitch, offset)
                        want = expected_buffer(initial, shader, block, extent, image_extent, pitch, offset)
                        assert_same(got, want, f"offset {offset} pitch +{pitch_extra} width {w} in {image_w} {shader}")


def test_the_bytes_are_copied_at_record_time(torch, blocks):
    """Push-constant semantics: the caller overwrites its buffer right after the record call, before the kernel has
    necessarily run; the image is the one of the bytes at the call."""
    extent = image_extent = (3840, 2160)
    initial = np.zeros(child.buffer_bytes(image_extent, 3840, 0), np.uint8)
    for shader in model.SHADERS:
        block = blocks[(shader, "example")]

        def scribble(raw):
            C.memset(raw, 0xFF, len(block))

        got = run(torch, initial, shader, block, extent, image_extent, 3840, 0, after_record=scribble)
        assert_same(got, expected_buffer(initial, shader, block, extent, image_extent, 3840, 0), shader)


def test_the_prefix_is_overwritten(torch, blocks):
    """The first 16 bytes of the caller's block never matter (pipelines.cpp:330-344)."""
    initial = pattern(child.buffer_bytes((64, 32), 64, 0))
    for shader in model.SHADERS:
        block = blocks[(shader, "ordinary")]
        a = run(torch, initial, shader, bytes(16) + block[16:], (40, 24), (64, 32), 64, 0)
        b = run(torch, initial, shader, np.array([7.0, -3.0, 1e9, np.nan], np.float32).tobytes() + block[16:], (40, 24), (64, 32), 64, 0)
        assert_same(a, b, shader)
        assert_same(a, expected_buffer(initial, shader, block, (40, 24), (64, 32), 64, 0), shader)


def test_refusals_write_nothing(torch):
    initial = pattern(child.buffer_bytes((64, 32), 66, 1))
    flat = torch.from_numpy(initial).cuda()
    base = flat.data_ptr() + 8
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rgba16 = abi.SZG_FORMAT_RGBA16_UNORM

    def image(width=64, height=32, pitch=66 * 8, fmt=rgba16, data=base):
        return abi.Image(data, width, height, pitch, fmt)

    block = bytes(48)
    cases = [
        ("NULL bytes", 1, None, 48, image(), 40, 24),
        ("NULL image", 1, block, 48, None, 40, 24),
        ("NULL data", 1, block, 48, image(data=None), 40, 24),
        ("index 4", 4, bytes(208), 208, image(), 40, 24),
        ("byte count 80 for gradient_color", 1, bytes(80), 80, image(), 40, 24),
        ("byte count 48 for booleanpush", 0, block, 48, image(), 40, 24),
        ("byte count 80 for matrix_color", 3, bytes(80), 80, image(), 40, 24),
        ("byte count 208 for sparse_push_constant", 2, bytes(208), 208, image(), 40, 24),
        ("RGBA16_SFLOAT", 1, block, 48, image(fmt=abi.SZG_FORMAT_RGBA16_SFLOAT), 40, 24),
        ("RGBA8_UNORM", 1, block, 48, image(fmt=abi.SZG_FORMAT_RGBA8_UNORM), 40, 24),
        ("pitch below a row", 1, block, 48, image(pitch=63 * 8), 40, 24),
        ("pitch not a multiple of 8", 1, block, 48, image(pitch=66 * 8 + 4), 40, 24),
        ("data not 8-B aligned", 1, block, 48, image(data=base + 4), 40, 24),
        ("empty width", 1, block, 48, image(), 0, 24),
        ("empty height", 1, block, 48, image(), 40, 0),
        ("extent wider than the image", 1, block, 48, image(), 65, 24),
        ("extent higher than the image", 1, block, 48, image(), 40, 33),
        ("image wider than the cap", 1, block, 48, image(width=16385, height=1, pitch=16385 * 8), 40, 1),
        ("image higher than the cap", 1, block, 48, image(width=1, height=16385, pitch=8), 1, 24),
    ]
    for name, index, raw, count, im, w, h in cases:
        status = lib().szg_record_compute_collection(stream, index, raw, count, C.byref(im) if im is not None else None, w, h)
        torch.cuda.synchronize()
        message = lib().szg_last_error()
        assert status == abi.SZG_ERR_INVALID_ARGUMENT, name
        assert b"szg_record_compute_collection" in message and len(message) > len(b"szg_record_compute_collection: "), name
        assert np.array_equal(flat.cpu().numpy(), initial), name


def test_python_pipeline_on_tensors(torch, blocks):
    """pipelines.ComputeCollectionPipeline on a SceneTexture larger than the extent and on a padded view of a tensor."""
    from syzygy_amd import pipelines as pl

    p = pl.ComputeCollectionPipeline()
    scene = pl.SceneTexture(128, 96)
    for index, shader in enumerate(model.SHADERS):
        p.selectShader(index)
        assert p.currentShader().name == shader
        zero = np.full((96, 128, 4), 0x1234, np.uint16)
        scene.color.copy_(torch.from_numpy(zero.view(np.int16)))
        p.recordDrawCommands(None, scene, (100, 70))  # the all-zero block of a new pipeline
        torch.cuda.synchronize()
        assert np.array_equal(scene.color_numpy(), model.render(shader, bytes(model.block_size(shader)), zero, 100, 70)[0])
        p.writeExampleValues()
        p.recordDrawCommands(None, scene, pl.rect(100, 70))
        torch.cuda.synchronize()
        assert np.array_equal(scene.color_numpy(), model.render(shader, p.readPushConstantBytes(), zero, 100, 70)[0])
        assert p.readPushConstantBytes() == blocks[(shader, "example")]
    backing = torch.full((40, 50, 4), 0x0101, dtype=torch.int16, device="cuda")
    view = backing[:, 1:34]  # 33 texels wide, one texel in, pitch 50 texels
    p.selectShader(abi.SZG_CC_MATRIX_COLOR)
    pl.record_compute_collection(None, p.shaderIndex(), p.readPushConstantBytes(), view, 20, 30)
    torch.cuda.synchronize()
    want = np.full((40, 50, 4), 0x0101, np.uint16)
    want[:, 1:34] = model.render("matrix_color", p.readPushConstantBytes(), want[:, 1:34], 20, 30)[0]
    assert np.array_equal(backing.cpu().numpy().view(np.uint16), want)
    with pytest.raises(ValueError):
        pl.record_compute_collection(None, 0, bytes(80), torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda"), 4, 4)
    with pytest.raises(SzgError):
        pl.record_compute_collection(None, 1, bytes(80), backing, 4, 4)  # 80 bytes for gradient_color


def read_ppm(path):
    with open(path, "rb") as f:
        magic, w, h, maxval = f.readline().split()
        assert magic == b"P6"
        data = np.frombuffer(f.read(), dtype=np.uint8 if int(maxval) < 256 else ">u2")
    return data.reshape(int(h), int(w), 3).astype(np.int64), int(maxval)


def example_image(shader, W, H, present):
    """What the examples write for --pipeline compute-collection:SHADER --present: the model's image of the example block, the
    editor's sRGB OETF over it (editor.cpp:303-340), then the model of the LINEAR blit onto the swapchain extent."""
    from tests import present_model as pm

    block = model.pack_block(shader, abi.COMPUTE_COLLECTION_EXAMPLE_VALUES[shader])
    scene = model.render(shader, block, np.zeros((H, W, 4), np.uint16), W, H)[0]
    scene[..., :3] = pm.oetf_table(abi.SZG_OETF_SRGB)[scene[..., :3]]
    return scene, pm.filtered_codes(scene, (0, 0, W, H), present[0], present[1], pm.RGBA8)


@pytest.mark.parametrize("shader", ["gradient_color", "booleanpush"])
def test_frame_loop_example_renders_the_collection(torch, tmp_path, shader):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import frame_loop
    finally:
        sys.path.pop(0)
    out = str(tmp_path / "collection.ppm")
    scene = frame_loop.main(["--frames", "2", "--width", "1000", "--height", "600", "--shadow-map", "512", "--out", out,
                             "--pipeline", "compute-collection:" + shader, "--present", "1280x720"])
    want_scene, want = example_image(shader, 1000, 600, (1280, 720))
    assert np.array_equal(scene, want_scene)
    got, maxval = read_ppm(out)
    assert maxval == 255 and np.array_equal(got, want[..., :3])
    assert got.max() > 0, "the example block must render something visible"


def test_render_gltf_example_renders_the_collection(torch, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import render_gltf
    finally:
        sys.path.pop(0)
    out = str(tmp_path / "collection.ppm")
    scene, _ = render_gltf.main(["--width", "640", "--height", "360", "--out", out, "--pipeline", "compute-collection:gradient_color",
                                 "--present", "1280x720"])
    want_scene, want = example_image("gradient_color", 640, 360, (1280, 720))
    assert np.array_equal(scene, want_scene)
    got, maxval = read_ppm(out)
    assert maxval == 255 and np.array_equal(got, want[..., :3]) and got.max() > 0
