"""The product's contraction rule against the literal evaluation on WHOLE images, on the CPU.

The accuracy claim has two links: the kernels equal the oracle bit for bit under the same rule (the GPU suite), and the
rule (include/szg/contraction.h, SZG_CONTRACT_DEFAULT) stays within north_star's bar of the literal execution of the
reference's SPIR-V: 1e-4 relative (against max(|a|, |b|, 1e-3)) and one UNORM16 step. tests/test_spirv_pin.py checks the
second link on the 5 248 recorded values of tests/golden/spirv_vectors.npz, of which only 84 are sky-view texels, none of
them in the rows next to the horizon. Because the oracle and the kernels read the same header, a rule that drifts outside
the bar there keeps every GPU test green; this file checks the second link where the sample does not reach: the default
oracle (the product's rule) against the literal one (mask 0, libszg_oracle_literal.so, the build pinned to the SPIR-V),
on the whole transmittance LUT, the whole 2048 x 1024 sky-view LUT and whole 640 x 360 frames.

The bounds are the bar itself, not a multiple of a measurement. The cameras include horizontal offsets from the planet's
vertical axis: on the axis (x = z = 0) the near-horizon rows of the sky-view LUT are far better conditioned, and a
rule that fused stepRadiusMu (SZG_C_STEP) stayed inside the bar there while it was up to 1.4e-4 away off the axis.
"""
import contextlib
import functools
import hashlib
import os

import numpy as np
import pytest

from oracle import binding as ob
from syzygy_amd import scene
from tests import util
from tests.test_gpu_parity import _absorbing_and_scattering, _dense_atmosphere, _thin_shell

THREADS = min(16, os.cpu_count() or 1)
BAR_REL = 1e-4  # north_star: relative, against max(|a|, |b|, 1e-3)
BAR_FLOOR = 1e-3
BAR_STEPS = 1  # UNORM16 codes
W, H = 640, 360
SPOTS = 64


def rel_distance(a, b):
    """Largest |a - b| / max(|a|, |b|, 1e-3) over the values that are not NaN; the NaN patterns must be equal."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert (np.isnan(a) == np.isnan(b)).all(), f"NaN patterns differ ({int(np.isnan(a).sum())} vs {int(np.isnan(b).sum())})"
    ok = ~np.isnan(a) & (a != b)  # (equal values are at distance 0, equal infinities included)
    if not ok.any():
        return 0.0
    d = np.abs(a[ok] - b[ok]) / np.maximum(np.maximum(np.abs(a[ok]), np.abs(b[ok])), BAR_FLOOR)
    return float(d.max())


def steps(a, b):
    return np.abs(np.asarray(a, np.int64) - np.asarray(b, np.int64))


def inputs(sun, position=None):
    cam = scene.default_camera()
    if position is not None:
        cam.cameraPosition[:] = [float(v) for v in position]
    return util.Inputs(W, H, elevation_degrees=sun, spots=SPOTS, camera=cam)


@functools.lru_cache(maxsize=None)
def _literal_tlut(atm_bytes):
    from syzygy_amd import abi

    atm = abi.AtmospherePacked.from_buffer_copy(atm_bytes)
    with ob.use_literal():
        t = ob.transmittance_lut(atm, 512, 128, threads=THREADS)
    t.setflags(write=False)
    return t


def literal_tlut(inp):
    return _literal_tlut(bytes(inp.atm))


@functools.lru_cache(maxsize=3)
def skyview_pair(sun, position):
    """(product, literal) 2048 x 1024 sky-view LUTs, both on the same literal 512 x 128 transmittance LUT. Cached for the
    three suns of the frame tests (the default camera), whose chained frames read them."""
    inp = inputs(sun, position)
    tlut = literal_tlut(inp)
    product = ob.skyview_lut(inp.atm, inp.cam, tlut, 2048, 1024, threads=THREADS)
    with ob.use_literal():
        literal = ob.skyview_lut(inp.atm, inp.cam, tlut, 2048, 1024, threads=THREADS)
    return product, literal


# ---------------------------------------------------------------------------
# transmittance LUT: no fused class reaches transmittance_LUT.comp's arithmetic
# ---------------------------------------------------------------------------
def _earth(a):
    pass


@pytest.mark.parametrize("edit", [_earth, _absorbing_and_scattering, _dense_atmosphere, _thin_shell])
def test_transmittance_lut_is_the_literal_lut(edit):
    inp = util.Inputs(W, H, elevation_degrees=35.0, spots=0, atmosphere_edit=edit)
    product = ob.transmittance_lut(inp.atm, 512, 128, threads=THREADS)
    literal = literal_tlut(inp)
    assert hashlib.sha256(product.tobytes()).digest() == hashlib.sha256(literal.tobytes()).digest(), edit.__name__


# ---------------------------------------------------------------------------
# sky-view LUT, all 2048 x 1024 texels
# ---------------------------------------------------------------------------
DEFAULT = (0.0, -10.0, -13.0)  # scene.default_camera(): 10 m up, 13 m off the planet's vertical axis
SKYVIEW_CASES = [
    ((0.0, -2.0, -13.0), 5.0),
    ((0.0, -100.0, -13.0), 35.0),
    ((0.0, -2500.0, -13.0), 5.0),
    ((300.0, -2500.0, -200.0), 5.0),  # off-axis
    (DEFAULT, 35.0),  # the bench's camera and sun
    (DEFAULT, 5.0),
    (DEFAULT, -3.0),  # sun below the horizon
]


@pytest.mark.parametrize("position,sun", SKYVIEW_CASES, ids=[f"x{p[0]:g}_alt{-p[1]:g}_z{p[2]:g}_sun{s:g}" for p, s in SKYVIEW_CASES])
def test_skyview_lut_stays_within_the_bar_of_the_literal_lut(position, sun):
    product, literal = skyview_pair(sun, position)
    rel = rel_distance(product[..., :3], literal[..., :3])
    exact = float((product.view(np.uint32) == literal.view(np.uint32)).mean())
    print(f"sky-view 2048x1024 camera {position} sun {sun}: max rel {rel:.3e}, bit-identical fraction {exact:.4f}")
    assert rel <= BAR_REL, (position, sun, rel)
    assert (product[..., 3] == literal[..., 3]).all()


# ---------------------------------------------------------------------------
# whole frames, 640 x 360, default camera, 64 spot lights
# ---------------------------------------------------------------------------
FRAME_SUNS = [35.0, 5.0, -3.0]


class _Passes:
    pass


@functools.lru_cache(maxsize=None)
def frame(sun):
    """Both builds' passes on one frame. The G-buffer fill contains no fused class; its output is shared."""
    inp = inputs(sun)
    r = _Passes()
    fills = []
    for literal in (False, True):
        f = ob.HostFrame(W, H)
        with ob.use_literal() if literal else contextlib.nullcontext():
            ob.gbuffer_fill(f, inp.rect, None, inp.cam, inp.synthetic.fill, threads=THREADS)
        fills.append(f)
    r.fill_identical = all(np.array_equal(fills[0].planes()[n].view(np.uint8), fills[1].planes()[n].view(np.uint8))
                           for n in fills[0].planes()) and np.array_equal(fills[0].depth.view(np.uint32), fills[1].depth.view(np.uint32))
    r.geometry = float((fills[0].depth > 0).mean())

    def lights(f, literal):
        with ob.use_literal() if literal else contextlib.nullcontext():
            ob.lights(f, inp.rect, None, None, inp.cam, inp.dirs, 2, 1, inp.spots, SPOTS, threads=THREADS)
        return f.debug.copy(), f.color.copy()

    def composite(f, prior, tlut, slut, literal):
        f.color[...] = prior
        with ob.use_literal() if literal else contextlib.nullcontext():
            ob.composite(f, inp.rect, None, None, inp.atm, inp.cam, inp.dirs, 0, tlut, slut, threads=THREADS)
        return f.debug.copy(), f.color.copy()

    shared = fills[1]  # the literal build's G-buffer
    r.lights_p = lights(_copy_gbuffer(shared), False)
    r.lights_l = lights(_copy_gbuffer(shared), True)
    tlut_l = literal_tlut(inp)
    tlut_p = ob.transmittance_lut(inp.atm, 512, 128, threads=THREADS)
    slut_p, slut_l = skyview_pair(sun, DEFAULT)
    # the all-literal chain, and the product composite on the same (literal) inputs
    r.chain_l = composite(_copy_gbuffer(shared), r.lights_l[1], tlut_l, slut_l, True)
    r.composite_p = composite(_copy_gbuffer(shared), r.lights_l[1], tlut_l, slut_l, False)
    # the product chain: product lights -> product LUTs -> product composite (slut_p was marched on the literal transmittance
    # LUT, which test_transmittance_lut_is_the_literal_lut requires to be the product's own)
    assert np.array_equal(tlut_p.view(np.uint32), tlut_l.view(np.uint32))
    r.chain_p = composite(_copy_gbuffer(shared), r.lights_p[1], tlut_p, slut_p, False)
    return r


def _copy_gbuffer(src):
    f = ob.HostFrame(W, H)
    for name, plane in f.planes().items():
        plane[...] = src.planes()[name]
    f.depth[...] = src.depth
    return f


@pytest.mark.parametrize("sun", FRAME_SUNS)
def test_lights_alone_on_a_shared_gbuffer(sun):
    r = frame(sun)
    assert r.fill_identical  # gbuffer_fill contains no fused class: both builds write the same bits
    assert 0.2 < r.geometry < 0.95
    (dbg_p, col_p), (dbg_l, col_l) = r.lights_p, r.lights_l
    rel, step = rel_distance(dbg_p, dbg_l), int(steps(col_p, col_l).max())
    print(f"lights sun {sun}: max rel {rel:.3e}, max step {step}, pixels with a different colour "
          f"{int((col_p != col_l).any(-1).sum())}")
    assert rel <= BAR_REL and step <= BAR_STEPS, (sun, rel, step)


@pytest.mark.parametrize("sun", FRAME_SUNS)
def test_composite_on_literal_inputs(sun):
    """Lights colour, transmittance LUT and sky-view LUT from the literal build feed both composites."""
    r = frame(sun)
    (dbg_p, col_p), (dbg_l, col_l) = r.composite_p, r.chain_l
    rel, step = rel_distance(dbg_p, dbg_l), int(steps(col_p, col_l).max())
    print(f"composite on literal inputs sun {sun}: max rel {rel:.3e}, max step {step}")
    assert rel <= BAR_REL and step <= BAR_STEPS, (sun, rel, step)


@pytest.mark.parametrize("sun", FRAME_SUNS)
def test_chained_frame_differs_only_through_the_requantised_lights_colour(sun):
    """Product lights -> product LUTs -> product composite against the all-literal chain. The lights pass stores UNORM16 and
    the composite reads that code back as its prior colour, so a lights colour one code apart - allowed by the
    bar - is carried into the composite, where it can be a relative 1e-3 of a dark pixel and, added to the composite's own
    one-step freedom, two codes. The test pins that explanation: every pixel whose stored lights colour is the same in both
    chains is within the bar, and every other pixel within two codes."""
    r = frame(sun)
    (dbg_p, col_p), (dbg_l, col_l) = r.chain_p, r.chain_l
    same_prior = (r.lights_p[1] == r.lights_l[1]).all(-1)
    n_same, n_diff = int(same_prior.sum()), int((~same_prior).sum())
    rel_same = rel_distance(dbg_p[same_prior], dbg_l[same_prior])
    step_same = int(steps(col_p[same_prior], col_l[same_prior]).max()) if n_same else 0
    step_diff = int(steps(col_p[~same_prior], col_l[~same_prior]).max()) if n_diff else 0
    rel_all = rel_distance(dbg_p, dbg_l)
    print(f"chained frame sun {sun}: {n_same} pixels with the same lights colour (max rel {rel_same:.3e}, max step {step_same}), "
          f"{n_diff} with a different one (max step {step_diff}); whole frame max rel {rel_all:.3e}")
    assert n_same > 0.9 * W * H
    assert rel_same <= BAR_REL and step_same <= BAR_STEPS, (sun, rel_same, step_same)
    assert step_diff <= 2 * BAR_STEPS, (sun, step_diff)
