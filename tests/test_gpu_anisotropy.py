"""include/szg/anisotropy.h on the GPU: the device sampler of syzygy_amd/csrc/szg_texture.hpp in isolation, called by the
test-only kernel of tests/anisosample (built by the DEVICE_LIBS rule of tests/Makefile with the product's HIPFLAGS), bit for bit against
tests/aniso_model.py; at max_anisotropy 1 also against the trilinear test kernel of tests/mipsample."""
import ctypes as C

import numpy as np
import pytest

from syzygy_amd import abi
from tests import aniso_model as am
from tests import mipmap_model as mm
from tests import native
from tests.test_gpu_mipmaps import N, _samples

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def anisosample():
    handle = C.CDLL(native.build("anisosample/libszg_anisosample.so"))
    handle.szg_anisosample.restype = C.c_int
    handle.szg_anisosample.argtypes = [C.POINTER(abi.Texture), C.c_void_p, C.c_uint32, C.c_float, C.c_float] + [C.c_void_p] * 4 + [C.c_uint32]
    return handle


@pytest.fixture(scope="module")
def mipsample():
    handle = C.CDLL(native.build("mipsample/libszg_mipsample.so"))
    handle.szg_mipsample.restype = C.c_int
    handle.szg_mipsample.argtypes = [C.POINTER(abi.Texture), C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 4 + [C.c_uint32]
    return handle


_CASES = {}


def _case(w, h, srgb):
    """Random chain and samples of one texture (the specials of tests/test_gpu_mipmaps.py in the first rows, and behind them a
    block of long footprints whose ratio is spread over 1 .. 64, which that distribution reaches only by chance)."""
    key = (w, h, srgb)
    if key not in _CASES:
        rng = np.random.default_rng(w * 137 + h * 11 + int(srgb))
        levels = [rng.integers(0, 256, (hk, wk, 4), dtype=np.uint8) for wk, hk in mm.level_shapes(w, h)]
        st, ddx, ddy = _samples(w, h, w + h + 1)
        block = slice(1024, 3072)
        count = block.stop - block.start
        longer = 2.0 ** rng.uniform(-6.0, 4.0, count)
        ratio = 2.0 ** rng.uniform(0.0, 6.0, count)
        a, b = rng.uniform(0.0, 2.0 * np.pi, count), rng.uniform(0.0, 2.0 * np.pi, count)
        size = np.array([w, h], np.float64)
        major = (longer[:, None] * np.stack([np.cos(a), np.sin(a)], 1) / size).astype(F)
        minor = ((longer / ratio)[:, None] * np.stack([np.cos(b), np.sin(b)], 1) / size).astype(F)
        to_x = (rng.random(count) < 0.5)[:, None]
        ddx[block], ddy[block] = np.where(to_x, major, minor), np.where(to_x, minor, major)
        _CASES[key] = (levels, (st, ddx, ddy), {})
    return _CASES[key]


def _run(torch, fn, levels, w, h, srgb, samples, *sampler):
    st, ddx, ddy = samples
    level0 = torch.from_numpy(levels[0]).cuda()
    chain = torch.from_numpy(mm.pack_chain(levels)).cuda()
    d_st, d_ddx, d_ddy = (torch.from_numpy(a).cuda() for a in (st, ddx, ddy))
    out = torch.full((N, 3), -7.0, dtype=torch.float32, device="cuda")
    tex = abi.Texture(level0.data_ptr(), w, h, w * 4, int(srgb))
    torch.cuda.synchronize()
    status = fn(C.byref(tex), chain.data_ptr(), len(levels), *sampler, d_st.data_ptr(), d_ddx.data_ptr(), d_ddy.data_ptr(), out.data_ptr(), N)
    assert status == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("max_lod", [mm.MAX_LOD_REFERENCE, mm.MAX_LOD_NONE])
@pytest.mark.parametrize("A", [1.0, 2.0, 3.5, 16.0])
@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("size", [(4, 4), (5, 3), (16, 8), (64, 64)])
def test_device_sampler_equals_the_model(torch, anisosample, mipsample, size, srgb, A, max_lod):
    w, h = size
    levels, samples, answers = _case(w, h, srgb)
    st, ddx, ddy = samples
    if (A, max_lod) not in answers:
        answers[(A, max_lod)] = am.sample(levels, srgb, st, ddx, ddy, max_lod, A, return_detail=True)
    want, detail = answers[(A, max_lod)]
    got = _run(torch, anisosample.szg_anisosample, levels, w, h, srgb, samples, max_lod, A)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    same = (got.view(np.uint32) == want.view(np.uint32)) | np.isnan(want)
    bad = np.argwhere(~same.all(axis=1)).reshape(-1)
    assert same.all(), f"{bad.size} of {N} samples differ; first: sample {bad[0]} st {st[bad[0]]} ddx {ddx[bad[0]]} ddy {ddy[bad[0]]} " \
                       f"N {detail['N'][bad[0]]} got {got[bad[0]]} want {want[bad[0]]}"
    counts = np.unique(detail["N"])
    print(f"{w}x{h} srgb {srgb} A {A} max_lod {max_lod}: tap counts {counts.tolist()}, single-tap share {(detail['N'] == 1).mean():.3f}")
    if A == 1.0:  # off: the trilinear sampler, from the model and from the kernel that has no anisotropy in it
        assert counts.tolist() == [1]
        assert np.array_equal(want.view(np.uint32), mm.sample(levels, srgb, st, ddx, ddy, max_lod).view(np.uint32))
        trilinear = _run(torch, mipsample.szg_mipsample, levels, w, h, srgb, samples, max_lod)
        assert np.array_equal(got.view(np.uint32), trilinear.view(np.uint32))
    else:
        assert counts.tolist() == list(range(1, int(np.ceil(A)) + 1))  # every tap count the value allows


def test_device_sampler_without_a_chain_is_the_one_level_rule(torch, anisosample):
    w, h = 5, 3
    levels, samples, _ = _case(w, h, True)
    st, ddx, ddy = samples
    level0 = torch.from_numpy(levels[0]).cuda()
    d_st, d_ddx, d_ddy = (torch.from_numpy(a).cuda() for a in (st, ddx, ddy))
    out = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    tex = abi.Texture(level0.data_ptr(), w, h, w * 4, 1)
    torch.cuda.synchronize()
    assert anisosample.szg_anisosample(C.byref(tex), None, 1, mm.MAX_LOD_NONE, 16.0, d_st.data_ptr(), d_ddx.data_ptr(), d_ddy.data_ptr(),
                                       out.data_ptr(), N) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint32), mm.bilinear(levels[0], True, st).view(np.uint32))
