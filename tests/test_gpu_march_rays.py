"""scatteringIntegral / marchLoop ray by ray on the GPU (tests/cpp/marchrays.hip), every lane against the oracle's scalar march.

The march takes its fast paths per WAVE. The parity tests compare whole images, where the camera decides which rays share a
wave; here the test does. Every family of tests/march_rays.py - a sweep of one knob across one gate's threshold - is laid out
as whole waves of one ray (both sides of the threshold appear as whole waves, wherever float32 puts it), as windows of
neighbouring rays (mixed waves), with one spoiler lane per wave, with every third lane switched off and as waves with a single
active lane (the divergent call of k_composite's phase B), in both configurations the product has: load_atm(block) /
make_tlut(t, w, h), and the FramePrep forms behind the product's own k_frame_prep and k_lut_range.

Equality rule: every float bit-identical to oracle_scattering_integral of the lane's ray, sign of zero included; NaN for NaN.
No ray is left out. Hole slots and the slots past n keep the sentinel."""
import ctypes as C

import numpy as np
import pytest

from tests import literal_pair as lp
from tests import march_rays as mr
from tests import native

pytestmark = pytest.mark.gpu


class Flags(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("lean", "signClearCoefficients", "zeroAbsorptionRayleigh", "zeroScatteringOzone",
                                          "extModerate", "moderate", "rowsInterior")] + \
               [(n, C.c_float) for n in ("innerCeil2", "leanFloor2", "extFloor2", "extCeil2")]


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        # the harness of the pair this process tests: with -DSZG_LITERAL beside libszg_hip_literal.so (tests/literal_pair.py)
        if lp.pair() == "literal":
            h = C.CDLL(native.build("cpp/libszg_marchrays_literal.so"))
        else:
            h = C.CDLL(native.build("cpp/libszg_marchrays.so"))
        h.szg_mr_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.c_void_p, C.c_uint, C.c_uint32, C.c_void_p,
                                 C.POINTER(Flags)]
        _LIB = h
    return _LIB


def run(atm, lut, prepped, rays8):
    """The harness on `rays8` ([n, 8] uint32): the launch's whole output ([256 ceil(n / 256), 3] float32) and the flags."""
    n = len(rays8)
    rays8 = np.ascontiguousarray(rays8, np.uint32)
    out = np.zeros((256 * ((n + 255) // 256), 3), np.float32)
    flags = Flags()
    lut = np.ascontiguousarray(lut, np.float32)
    st = lib().szg_mr_run(C.addressof(atm), lut.ctypes.data, lut.shape[1], lut.shape[0], 1 if prepped else 0, rays8.ctypes.data, n,
                          mr.SENTINEL, out.ctypes.data, C.byref(flags))
    assert st == 0, "HIP error %d" % st
    return out, flags


class Context:
    """One block-and-LUT variant: its LUT, its bounds, its spoilers, and the oracle's value of every ray asked for - computed
    once and shared by the two configurations."""

    def __init__(self, variant):
        self.v, self.B, self.lut = variant, variant.bounds(), variant.lut()
        self.spoilers = mr.spoilers(self.B)
        self.spoiler_want = {g: mr.oracle_values(variant.atm, self.lut, r[None, :])[0] for g, r in self.spoilers.items()}
        self._want, self._families = {}, {}

    def families(self, group):
        if group not in self._families:
            if group == "variant":
                fams = mr.setup_families(self.B, only=mr.VARIANT_FAMILIES)
            elif group == "step":
                fams = mr.step_families(self.B)
            elif group == "random":
                fams = [mr.random_rays(self.B)]
            else:
                fams = [f for f in mr.setup_families(self.B) if f.name.startswith(group + "/")]
            self._families[group] = fams
        return self._families[group]

    def want(self, fam):
        if fam.name not in self._want:
            self._want[fam.name] = mr.oracle_values(self.v.atm, self.lut, fam.rays)
        return self._want[fam.name]


_CONTEXTS = {}


def context(name):
    if name not in _CONTEXTS:
        _CONTEXTS[name] = Context({v.name: v for v in mr.variants()}[name])
    return _CONTEXTS[name]


def hexes(v):
    return "(" + " ".join("%08x" % int(b) for b in np.asarray(v, np.float32).view(np.uint32)) + ")"


def check_flags(ctx, flags, prepped):
    for name, want in ctx.v.flags.items():
        assert getattr(flags, name) == want, (ctx.v.name, name, getattr(flags, name), want)
    if not prepped:
        assert flags.rowsInterior == 0  # make_tlut(t, w, h) never sets it
    elif ctx.v.rows_interior is not None:
        want = ctx.v.rows_interior[lp.pair()] if isinstance(ctx.v.rows_interior, dict) else ctx.v.rows_interior
        assert flags.rowsInterior == want, (ctx.v.name, lp.pair(), flags.rowsInterior)
    # the bounds the census is written with are the ones the device holds, to float32
    B = ctx.B
    for name, value in (("innerCeil2", B.innerCeil ** 2), ("leanFloor2", B.leanFloor ** 2), ("extFloor2", B.extFloor ** 2),
                        ("extCeil2", B.extCeil ** 2)):
        assert abs(getattr(flags, name) - value) <= 2.0 ** -20 * value, (ctx.v.name, name, getattr(flags, name), value)


def check_family(ctx, fam, prepped):
    lay = mr.random_layout(len(fam), mr.random_shuffles(len(fam))) if fam.kind == "random" else mr.layout(len(fam))
    spoiler = ctx.spoilers[fam.spoiler]
    rays8 = mr.launch_rays(fam.rays, spoiler, lay)
    n = len(rays8)
    assert n % 64 != 0  # the last wave is cut short
    out, flags = run(ctx.v.atm, ctx.lut, prepped, rays8)
    check_flags(ctx, flags, prepped)
    slots, hole = lay.slots(), lay.holes()
    want = np.concatenate([ctx.want(fam), ctx.spoiler_want[fam.spoiler][None, :]])[slots]
    kept = (out.view(np.uint32) == mr.SENTINEL).all(axis=1)
    assert kept[n:].all(), "%s: a slot past n = %d was written" % (fam.name, n)
    assert kept[:n][hole].all(), "%s: hole slot %d was written" % (fam.name, int(np.flatnonzero(~kept[:n] & hole)[0]))
    lp.compared(3 * int((~hole).sum()))
    bad = np.flatnonzero(~(mr.same_bits(out[:n], want).all(axis=1) | hole))
    if len(bad) == 0:
        return
    lines = ["%s [%s, %s, LUT %dx%d]: %d of %d lanes differ from the oracle" % (fam.name, ctx.v.name, "prepped" if prepped else "plain",
                                                                              ctx.lut.shape[1], ctx.lut.shape[0], len(bad), n)]
    first_of_wave = bad[np.unique(bad // 64, return_index=True)[1]]  # one lane of each of the first waves that differ
    for s in first_of_wave[:4]:
        form, wave = lay.form_of(int(s))
        k = int(slots[s])
        ray = spoiler if k == len(fam) else fam.rays[k]
        knob = "spoiler(%s)" % fam.spoiler if k == len(fam) else repr(fam.knobs[k])
        others = sorted(set(int(i) for i in slots[64 * (s // 64): 64 * (s // 64) + 64]))
        lines.append("  knob %s, form %s, wave %d, lane %d (rays of the wave: %d..%d%s): kernel %s %s, oracle %s %s\n    ray %s\n    census: %s"
                     % (knob, form, wave, int(s) % 64, others[0], others[-1], ", spoiled" if len(fam) in others else "", out[s],
                        hexes(out[s]), want[s], hexes(want[s]), hexes(ray), mr.census_line(mr.census(ray, ctx.B))))
    pytest.fail("\n".join(lines), pytrace=False)


EARTH_GROUPS = ("setupLean", "lean", "extLean", "firstStepOnly", "belowOzone", "inner", "sunClear", "step", "random")
VARIANT_NAMES = mr.VARIANT_NAMES[1:]
CONFIGS = ("plain", "prepped")


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("group", EARTH_GROUPS)
def test_earth_families(group, config):
    ctx = context("earth")
    fams = ctx.families(group)
    assert fams
    for fam in fams:
        check_family(ctx, fam, config == "prepped")


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_variant_families(name, config):
    """firstStepOnly, belowOzone, INNER and sunClear again under each block and LUT variant; the flags the device reads from the
    variant are the ones it was built for (check_flags)."""
    ctx = context(name)
    for fam in ctx.families("variant"):
        check_family(ctx, fam, config == "prepped")


def test_rows_interior_differs_between_two_extents():
    """TLut::rowsInterior as the device reads it behind k_frame_prep: set for one LUT extent, clear for another, so that both
    forms of radiusPart's row addressing have run above. (The flag is read, not modelled: Variant.rows_interior was filled in
    from the harness.) With 25 rows the flag depends on the build; with 41 rows it is clear in both."""
    seen = {}
    for name in ("lut-256x64", "lut-33x7", "lut-33x25", "lut-33x41"):
        ctx = context(name)
        _, flags = run(ctx.v.atm, ctx.lut, True, np.zeros((0, 8), np.uint32))
        seen[name] = flags.rowsInterior
    assert set(seen.values()) == {0, 1}, seen
