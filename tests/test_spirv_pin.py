"""The oracle pinned against the reference's own shader binaries.

tests/golden/spirv_vectors.npz holds the outputs of the COMMITTED SPIR-V of transmittance_LUT.comp, skyview_LUT.comp,
lights.comp and camera.comp, executed literally (one IEEE binary32 operation per SPIR-V arithmetic instruction, in program
order) by the interpreter of tests/golden/spirv_interp.py on seeded inputs, together with those inputs
(tests/golden/make_spirv_vectors.py wrote it in the build container, where the reference checkout is; the .spv files
themselves are not in this repository).

What is asserted: the oracle with its contraction rule switched off (oracle/libszg_oracle_literal.so: the same source,
-DSZG_ORACLE_LITERAL turns every fused a * b + c of the rule into two roundings) reproduces every vector BIT FOR BIT. So the
restatement performs the shader's operations, with the shader's constants, in the shader's order, on every path these vectors
walk (sky, sun disc, ground hits, lit and unlit geometry, reflections, all three light types, PCF shadow taps, both LUT
kernels). The default oracle - the parity checker of the GPU tests - differs from the literal one only by the product's
contraction rule (include/szg/contraction.h: the site classes measured to stay within 1e-4 relative / one UNORM16 step of
these vectors), a freedom the SPIR-V grants (no NoContraction decoration).

Not pinned, because Vulkan leaves them to the implementation: the values of exp / pow / sin / cos / asin / acos
(both sides use include/szg/fpmath.h), the texture filter and UNORM conversion models, and where a real GPU contracts.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from oracle import binding as ob
from syzygy_amd import abi
from tests.golden import make_spirv_vectors as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vec():
    return np.load(os.path.join(ROOT, "tests", "golden", "spirv_vectors.npz"))


_TLUTS = {}


def _tlut(vec, k):
    """The 512 x 128 transmittance LUT of scenario k: recomputed by the literal oracle (its texels are what
    test_transmittance_lut_shader pins), and required to be the array the vectors were made with."""
    if k not in _TLUTS:
        atm = _block(abi.AtmospherePacked, vec[f"atm_{k}"])
        with ob.use_literal():
            t = ob.transmittance_lut(atm, 512, 128, threads=8)
        assert hashlib.sha256(t.tobytes()).digest() == bytes(vec[f"tlut_sha256_{k}"]), "the transmittance LUT changed"
        _TLUTS[k] = t
    return _TLUTS[k]


def _block(ctype, raw):
    return ctype.from_buffer_copy(bytes(np.ascontiguousarray(raw, np.uint8)))


def _array(ctype, raw):
    raw = bytes(np.ascontiguousarray(raw, np.uint8))
    n = len(raw) // C.sizeof(ctype)
    return (ctype * n).from_buffer_copy(raw), n


def _same(got, want_bits, what):
    got_bits = np.ascontiguousarray(got, np.float32).view(np.uint32)
    bad = np.argwhere(got_bits != want_bits)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), np.asarray(got)[tuple(bad[0][:-1])] if bad.size else None,
                           want_bits.view(np.float32)[tuple(bad[0][:-1])] if bad.size else None)


def test_transmittance_lut_shader(vec):
    W, H = (int(v) for v in vec["transmittance_extent"])
    got = np.zeros((len(vec["transmittance_xy"]), 4), np.float32)
    with ob.use_literal():
        for i, ((x, y), raw) in enumerate(zip(vec["transmittance_xy"], vec["transmittance_atm"])):
            atm = _block(abi.AtmospherePacked, raw)
            ob.lib().oracle_transmittance_texel(C.byref(atm), W, H, int(x), int(y), ob.fptr(got[i]))
    _same(got, vec["transmittance_texel"], "transmittance_LUT.comp")
    assert len(got) >= 60


def test_skyview_lut_shader(vec):
    W, H = (int(v) for v in vec["skyview_extent"])
    got = np.zeros((len(vec["skyview_xy"]), 4), np.float32)
    with ob.use_literal():
        for i, (x, y) in enumerate(vec["skyview_xy"]):
            atm = _block(abi.AtmospherePacked, vec["skyview_atm"][i])
            cam = _block(abi.CameraPacked, vec["skyview_cam"][i])
            tlut = _tlut(vec, int(vec["skyview_tlut"][i]))
            row = ob.skyview_lut(atm, cam, tlut, W, H, row_begin=int(y), row_end=int(y) + 1, threads=8)
            got[i] = row[int(y), int(x)]
    _same(got, vec["skyview_texel"], "skyview_LUT.comp")
    assert len(got) >= 50


def _frame(vec, k):
    atm = _block(abi.AtmospherePacked, vec[f"atm_{k}"])
    cam = _block(abi.CameraPacked, vec[f"cam_{k}"])
    dirs, ndirs = _array(abi.DirectionalLightPacked, vec[f"dirs_{k}"])
    spots, nspots = _array(abi.SpotLightPacked, vec[f"spots_{k}"])
    depth = vec[f"depth_{k}"]
    H, W = depth.shape
    frame = ob.HostFrame(W, H)
    for name, plane in frame.planes().items():
        plane[...] = vec[f"gbuffer_{name}_{k}"]
    frame.depth[...] = depth
    nslots = ndirs + nspots
    keep = [np.ascontiguousarray(vec[f"shadow_{k}_{s}"]) for s in range(nslots)]
    images = (abi.Image * nslots)()
    for s in range(nslots):
        images[s] = ob.host_image(keep[s], abi.SZG_FORMAT_D32_SFLOAT)
    sm = abi.ShadowMaps(nslots, 0, C.cast(images, C.POINTER(abi.Image)))
    return frame, atm, cam, dirs, ndirs, spots, nspots, sm, (keep, images)


@pytest.mark.parametrize("k", range(6))
def test_lights_and_camera_shaders(vec, k):
    assert int(vec["scenarios"]) == 6
    frame, atm, cam, dirs, ndirs, spots, nspots, sm, keep = _frame(vec, k)
    H, W = frame.depth.shape
    rect = abi.Rect(0, 0, W, H)
    with ob.use_literal():
        ob.lights(frame, rect, None, sm, cam, dirs, ndirs, 1, spots, nspots, threads=8)
        xy = vec[f"lights_xy_{k}"]
        _same(frame.debug[xy[:, 1], xy[:, 0]], vec[f"lights_value_{k}"], f"lights.comp scenario {k}")
        assert np.array_equal(frame.color[xy[:, 1], xy[:, 0]], vec[f"lights_unorm_{k}"])
        # geometry and background both occur
        stored = vec[f"lights_stored_{k}"]
        assert (stored.any() and not stored.all()) or k == 3  # (scenario 3 looks down from 2.5 km: sky and ground only)
        assert np.array_equal(frame.color, vec[f"prior_{k}"])  # what camera.comp read back when the vectors were made
        tlut = _tlut(vec, k)
        slut = np.ascontiguousarray(vec[f"slut_{k}"])
        ob.composite(frame, rect, None, sm, atm, cam, dirs, 0, tlut, slut, threads=8)
        xy = vec[f"camera_xy_{k}"]
        _same(frame.debug[xy[:, 1], xy[:, 0]], vec[f"camera_value_{k}"], f"camera.comp scenario {k}")
        assert np.array_equal(frame.color[xy[:, 1], xy[:, 0]], vec[f"camera_unorm_{k}"])


@pytest.mark.parametrize("name,function", [("oetf_pure_gamma", abi.SZG_OETF_PURE_GAMMA), ("oetf_srgb", abi.SZG_OETF_SRGB)])
def test_oetf_shaders_every_code_value(vec, name, function):
    """transfer/oetf_*.comp.spv on every 16-bit code value (red channel; the other channels walk the codes in other orders,
    alpha passes through): the oracle's in-place OETF gives the same UNORM16 codes. (No product of the contraction rule
    occurs in these shaders: the default build is the literal one.)"""
    colour = np.ascontiguousarray(vec["oetf_input"]).copy()
    got = ob.oetf(colour, function)
    assert np.array_equal(got, vec[name])
    assert np.array_equal(got[..., 3], vec["oetf_input"][..., 3])


def test_raster_pass_vertex_shaders(vec):
    """offscreen.vert and depthpass.vert (the programmable stage in front of the fixed-function rasteriser): clip position,
    world position, normalised normal and texture coordinate of 24 vertices x 3 instances against the oracle's vertex stage."""
    lib = ob.lib_literal()
    FP = C.POINTER(C.c_float)
    lib.oracle_vertex_stage.argtypes = [C.POINTER(abi.VertexPacked), C.POINTER(abi.Mat4), C.POINTER(abi.Mat4), C.POINTER(abi.Mat4),
                                        C.POINTER(abi.Mat4), C.c_int, FP]
    vertices, nv = _array(abi.VertexPacked, vec["raster_vertices"])
    models, ni = _array(abi.Mat4, vec["raster_models"])
    mits, _ = _array(abi.Mat4, vec["raster_mits"])
    cam = _block(abi.CameraPacked, vec["raster_camera"])
    light = _block(abi.Mat4, vec["raster_light"])
    got_v = np.zeros((ni * nv, 12), np.float32)
    got_d = np.zeros((ni * nv, 12), np.float32)
    for inst in range(ni):
        for vi in range(nv):
            k = inst * nv + vi
            lib.oracle_vertex_stage(C.byref(vertices[vi]), C.byref(models[inst]), C.byref(mits[inst]), C.byref(cam.projection),
                                    C.byref(cam.view), 0, got_v[k].ctypes.data_as(FP))
            lib.oracle_vertex_stage(C.byref(vertices[vi]), C.byref(models[inst]), None, C.byref(light), None, 1,
                                    got_d[k].ctypes.data_as(FP))
    _same(got_v, vec["offscreen_vert"], "offscreen.vert")
    _same(got_d[:, :4], vec["depthpass_vert"], "depthpass.vert")
    assert len(got_v) == 72


def test_gbuffer_fragment_shader(vec):
    """offscreen.frag on 160 fragments with random interpolants, screen-space differences and 8-bit material maps (sRGB
    colour map, REPEAT addressing): all five G-buffer outputs against the oracle's fragment stage."""
    lib = ob.lib_literal()
    FP = C.POINTER(C.c_float)
    lib.oracle_fragment_stage.argtypes = [C.POINTER(abi.Material)] + [FP] * 8
    keep = {n: np.ascontiguousarray(vec[f"frag_tex_{n}"]) for n in ("color", "normal", "orm")}
    mat = abi.Material()
    for n, field in (("color", mat.color), ("normal", mat.normal), ("orm", mat.orm)):
        a = keep[n]
        field.data, field.height, field.width, field.pitch_bytes, field.srgb = a.ctypes.data, a.shape[0], a.shape[1], a.strides[0], int(n == "color")
    fin = np.ascontiguousarray(vec["frag_in"]).view(np.float32)
    got = np.zeros((len(fin), 20), np.float32)
    for i, row in enumerate(fin):
        parts = [np.ascontiguousarray(row[a:b]) for a, b in ((0, 3), (3, 6), (6, 8), (8, 11), (11, 14), (14, 16), (16, 18))]
        lib.oracle_fragment_stage(C.byref(mat), *[p.ctypes.data_as(FP) for p in parts], got[i].ctypes.data_as(FP))
    _same(got, vec["offscreen_frag"], "offscreen.frag")
    assert len(got) == 160


@pytest.mark.parametrize("k", range(6))
def test_the_product_rule_stays_within_1e4_and_one_step_of_the_spirv_vectors(vec, k):
    """The parity oracle (the product's contraction rule, include/szg/contraction.h: the classes measured to be harmless)
    against the vectors of the literal execution: north_star's 1e-4 relative and one UNORM16 step, on every recorded pixel of
    lights.comp and camera.comp. Round 2's rule (every class fused) was 2.3e-3 / 7 steps away on the same vectors."""
    frame, atm, cam, dirs, ndirs, spots, nspots, sm, keep = _frame(vec, k)
    H, W = frame.depth.shape
    rect = abi.Rect(0, 0, W, H)
    ob.lights(frame, rect, None, sm, cam, dirs, ndirs, 1, spots, nspots, threads=8)
    for shader in ("lights", "camera"):
        if shader == "camera":
            # (the literal LUT: the product's rule fuses nothing inside transmittance_LUT.comp, test below)
            ob.composite(frame, rect, None, sm, atm, cam, dirs, 0, _tlut(vec, k), np.ascontiguousarray(vec[f"slut_{k}"]), threads=8)
        xy = vec[f"{shader}_xy_{k}"]
        want = vec[f"{shader}_value_{k}"].view(np.float32)
        got = frame.debug[xy[:, 1], xy[:, 0]]
        rel = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-3)
        assert rel.max() <= 1e-4, (shader, k, rel.max())
        step = np.abs(frame.color[xy[:, 1], xy[:, 0]].astype(np.int64) - vec[f"{shader}_unorm_{k}"].astype(np.int64))
        assert step.max() <= 1, (shader, k, step.max())


def test_the_product_rule_leaves_the_lut_shaders_at_the_literal_values(vec):
    """transmittance_LUT.comp: no fused class occurs in it, the default oracle IS the literal one there (whole LUT, SHA-256).
    skyview_LUT.comp: within 1e-4 of the literal texels (whole LUTs: tests/test_contraction_whole_images.py)."""
    atm = _block(abi.AtmospherePacked, vec["atm_0"])
    t = ob.transmittance_lut(atm, 512, 128, threads=8)
    assert hashlib.sha256(t.tobytes()).digest() == bytes(vec["tlut_sha256_0"])
    W, H = (int(v) for v in vec["skyview_extent"])
    worst = 0.0
    for i, (x, y) in enumerate(vec["skyview_xy"]):
        atm = _block(abi.AtmospherePacked, vec["skyview_atm"][i])
        cam = _block(abi.CameraPacked, vec["skyview_cam"][i])
        row = ob.skyview_lut(atm, cam, _tlut(vec, int(vec["skyview_tlut"][i])), W, H, row_begin=int(y), row_end=int(y) + 1, threads=8)
        want = vec["skyview_texel"][i].view(np.float32).astype(np.float64)
        worst = max(worst, float((np.abs(row[int(y), int(x)] - want) / np.maximum(np.abs(want), 1e-3)).max()))
    assert worst <= 1e-4, worst


@pytest.mark.skipif(not gen.available(), reason="the reference's committed SPIR-V is only present in the build container")
def test_committed_vectors_are_what_the_reference_binaries_produce(vec):
    """Where the reference checkout exists, run the interpreter again and compare with the committed fixture."""
    live = gen.generate(log=lambda *_: None)
    assert sorted(live) == sorted(vec.files)
    for name in vec.files:
        assert np.array_equal(np.asarray(live[name]), vec[name]), name
