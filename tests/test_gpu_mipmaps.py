"""include/szg/mipmaps.h on the GPU, bit for bit against tests/mipmap_model.py: the chain builder (k_mip_downsample) and the
device sampler of syzygy_amd/csrc/szg_texture.hpp in isolation, called by the test-only kernel of tests/mipsample (built by
the DEVICE_LIBS rule of tests/Makefile with the product's HIPFLAGS)."""
import ctypes as C

import numpy as np
import pytest

from syzygy_amd import abi, lib
from tests import mipmap_model as mm
from tests import native

pytestmark = pytest.mark.gpu
F = np.float32


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


# ---------------------------------------------------------------------------
# generation
# ---------------------------------------------------------------------------
def _random_image(w, h, seed):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    img.reshape(-1, 4)[:4] = [[0, 0, 0, 0], [255, 255, 255, 255], [10, 11, 255, 3], [11, 10, 0, 254]]  # both sRGB branches
    return img


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("size", [(2, 2), (3, 5), (8, 1), (64, 64), (257, 129)])
def test_generated_chain_equals_the_model(gpu, size, srgb):
    w, h = size
    img = _random_image(w, h, w * 1000 + h + int(srgb))
    chain = gpu.pl.generate_mipmaps(gpu.torch.from_numpy(img).cuda(), srgb)
    gpu.torch.cuda.synchronize()
    want = mm.pack_chain(mm.build_chain(img, srgb))
    got = chain.cpu().numpy()
    assert got.size == want.size == mm.chain_bytes(w, h)
    assert np.array_equal(got, want), f"{(got != want).sum()} of {got.size} bytes differ"


@pytest.mark.parametrize("srgb", [False, True])
def test_generation_honours_a_pitch_wider_than_a_row(gpu, srgb):
    w, h, pad = 37, 19, 5
    img = _random_image(w, h, 77)
    wide = gpu.torch.full((h, w + pad, 4), 0xEE, dtype=gpu.torch.uint8, device="cuda")
    wide[:, :w] = gpu.torch.from_numpy(img).cuda()
    view = wide[:, :w]
    assert view.stride(0) == (w + pad) * 4
    chain = gpu.pl.generate_mipmaps(view, srgb)
    gpu.torch.cuda.synchronize()
    assert np.array_equal(chain.cpu().numpy(), mm.pack_chain(mm.build_chain(img, srgb)))
    assert (wide[:, w:] == 0xEE).all()  # the source is never written


def test_refusals_leave_the_output_untouched(gpu):
    w, h = 37, 19
    img = gpu.torch.from_numpy(_random_image(w, h, 5)).cuda()
    out = gpu.torch.full((mm.chain_bytes(w, h) + 64,), 0xAB, dtype=gpu.torch.uint8, device="cuda")
    for name, level0, chain, nbytes, text in mm.generate_refusals(img.data_ptr(), out.data_ptr()):
        status = lib().szg_record_generate_mipmaps(None, C.byref(level0) if level0 is not None else None, chain, nbytes)
        assert status == abi.SZG_ERR_INVALID_ARGUMENT and text in lib().szg_last_error(), name
    gpu.torch.cuda.synchronize()
    assert (out == 0xAB).all()
    # and the accepted call writes exactly the chain
    level0 = abi.Texture(img.data_ptr(), w, h, w * 4, 0)
    assert lib().szg_record_generate_mipmaps(None, C.byref(level0), out.data_ptr(), mm.chain_bytes(w, h)) == abi.SZG_OK
    gpu.torch.cuda.synchronize()
    assert (out[mm.chain_bytes(w, h):] == 0xAB).all() and not (out[:mm.chain_bytes(w, h)] == 0xAB).all()


# ---------------------------------------------------------------------------
# the sampler in isolation
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mipsample():
    handle = C.CDLL(native.build("mipsample/libszg_mipsample.so"))
    handle.szg_mipsample.restype = C.c_int
    handle.szg_mipsample.argtypes = [C.POINTER(abi.Texture), C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 4 + [C.c_uint32]
    return handle


N = 4096


def _samples(w, h, seed):
    """uv in [-3, 3]; derivative magnitudes log-uniform over 2^-12 .. 2^4 texels with random signs; the first rows replaced by
    the special values."""
    rng = np.random.default_rng(seed)
    st = rng.uniform(-3.0, 3.0, (N, 2)).astype(F)
    size = np.array([w, h], F)

    def derivative():
        texels = (2.0 ** rng.uniform(-12.0, 4.0, (N, 2))) * rng.choice([-1.0, 1.0], (N, 2))
        return (texels / size).astype(F)

    ddx, ddy = derivative(), derivative()
    nan, inf = np.nan, np.inf
    special = [((0, 0), (0, 0)), ((-0.0, 0.0), (0.0, -0.0)), ((nan, 0), (0, 0)), ((0, nan), (0.5, 0)), ((nan, nan), (nan, nan)),
               ((0.25, 0), (nan, 0)), ((inf, 0), (0, 0)), ((0, -inf), (0, 0)), ((inf, -inf), (inf, inf)), ((inf, 0), (nan, 0)),
               ((1e-40, 0), (0, 1e-40)), ((1e-45, 1e-45), (1e-45, 1e-45)), ((1e-30, 0), (0, 0)), ((1e-19, 0), (0, 1e-20)),
               ((1e19, 0), (0, 0)), ((1e30, 1e30), (0, 0)), ((3e38, 0), (0, 3e38))]
    for k in range(-4, 12):  # exact powers of two of texels per pixel: f == 0, up to footprints beyond the last level
        special.append(((2.0**k / w, 0), (0, 2.0**-3 / h)))
        special.append(((0, 2.0**-2 / h), (0, -(2.0**k) / h)))
        special.append(((2.0**k / w, 0), (0, 2.0**k / h)))
    for i, (a, b) in enumerate(special):
        ddx[i], ddy[i] = a, b
    st[len(special):len(special) + 8] = [[0, 0], [1, 1], [-3, 3], [0.5, 0.5], [-0.0, 2.0], [1.0 / w, 1.0 / h], [-1.0 / w, 0.5 / h], [3, -3]]
    return st, ddx, ddy


_REFERENCE = {}


def _case(w, h, srgb):
    """Random chain and samples of one texture, and the model's answers per max_lod: computed once."""
    key = (w, h, srgb)
    if key not in _REFERENCE:
        rng = np.random.default_rng(w * 131 + h * 7 + int(srgb))
        levels = [rng.integers(0, 256, (hk, wk, 4), dtype=np.uint8) for wk, hk in mm.level_shapes(w, h)]
        _REFERENCE[key] = (levels, _samples(w, h, w + h), {})
    return _REFERENCE[key]


@pytest.mark.parametrize("max_lod", [0.0, 1.0, 2.5, mm.MAX_LOD_NONE])
@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("size", [(4, 4), (5, 3), (16, 8), (64, 64)])
def test_device_sampler_equals_the_model(gpu, mipsample, size, srgb, max_lod):
    w, h = size
    levels, (st, ddx, ddy), answers = _case(w, h, srgb)
    if max_lod not in answers:
        answers[max_lod] = mm.sample(levels, srgb, st, ddx, ddy, max_lod)
    want = answers[max_lod]
    t = gpu.torch
    level0 = t.from_numpy(levels[0]).cuda()
    chain = t.from_numpy(mm.pack_chain(levels)).cuda()
    d_st, d_ddx, d_ddy = (t.from_numpy(a).cuda() for a in (st, ddx, ddy))
    out = t.full((N, 3), -7.0, dtype=t.float32, device="cuda")
    tex = abi.Texture(level0.data_ptr(), w, h, w * 4, int(srgb))
    t.cuda.synchronize()
    status = mipsample.szg_mipsample(C.byref(tex), chain.data_ptr(), len(levels), max_lod, d_st.data_ptr(), d_ddx.data_ptr(),
                                     d_ddy.data_ptr(), out.data_ptr(), N)
    assert status == 0
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    same = (got.view(np.uint32) == want.view(np.uint32)) | np.isnan(want)
    bad = np.argwhere(~same.all(axis=1)).reshape(-1)
    assert same.all(), f"{bad.size} of {N} samples differ; first: sample {bad[0]} st {st[bad[0]]} ddx {ddx[bad[0]]} ddy {ddy[bad[0]]} " \
                       f"got {got[bad[0]]} want {want[bad[0]]}"
    if max_lod == 0.0:  # and that is the one-level rule
        assert np.array_equal(want, mm.bilinear(levels[0], srgb, st))


def test_device_sampler_without_a_chain_is_the_one_level_rule(gpu, mipsample):
    w, h = 5, 3
    levels, (st, ddx, ddy), _ = _case(w, h, True)
    t = gpu.torch
    level0 = t.from_numpy(levels[0]).cuda()
    d_st, d_ddx, d_ddy = (t.from_numpy(a).cuda() for a in (st, ddx, ddy))
    out = t.zeros((N, 3), dtype=t.float32, device="cuda")
    tex = abi.Texture(level0.data_ptr(), w, h, w * 4, 1)
    t.cuda.synchronize()
    assert mipsample.szg_mipsample(C.byref(tex), None, 1, mm.MAX_LOD_NONE, d_st.data_ptr(), d_ddx.data_ptr(), d_ddy.data_ptr(),
                                   out.data_ptr(), N) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint32), mm.bilinear(levels[0], True, st).view(np.uint32))
