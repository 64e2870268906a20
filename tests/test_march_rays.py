"""tests/march_rays.py without a GPU: the families sweep what they say, the spoilers fail what they say, the wave forms hold
what they say, and the oracle's values make bit equality mean something."""
import numpy as np
import pytest

from tests import march_rays as mr


@pytest.fixture(scope="module")
def earth():
    v = mr.variants()[0]
    return v, v.bounds()


@pytest.fixture(scope="module")
def families(earth):
    v, B = earth
    return mr.setup_families(B) + mr.step_families(B)


def _others(fam):
    return [g for g in mr.SETUP_GATES if g != fam.gate and g not in fam.coupled]


def test_every_sweep_crosses_its_gate_and_no_other(earth, families):
    v, B = earth
    for fam in families:
        if fam.gate is None or fam.kind not in ("sweep", "range"):
            continue
        assert fam.kind == "range" or len(fam) >= 2 * 64 + 8, (fam.name, len(fam))
        ends = [mr.census(fam.rays[0], B), mr.census(fam.rays[-1], B)]
        assert sorted(c[fam.gate] for c in ends) == ["false", "true"], (fam.name, [mr.census_line(c) for c in ends])
        for x, ray in zip(fam.knobs, fam.rays):
            c = mr.census(ray, B)
            for g in _others(fam):
                assert c[g] != "near", (fam.name, x, g, mr.census_line(c))


def test_the_core_steps_are_single_ulps_of_the_gate_quantity(earth, families):
    """Between neighbouring core rays the float64 gate quantity moves by about one float32 ulp of the threshold: the core
    holds at least 64 such steps on each side of the predicted crossing."""
    v, B = earth
    for fam in families:
        if fam.kind != "sweep" or fam.gate not in ("firstStepOnly", "belowOzone", "inner", "extLean"):
            continue
        key = {"firstStepOnly": "dS", "belowOzone": "maxr2", "inner": "maxr2", "extLean": "maxr2" if "ceiling" in fam.name else "rmin2"}[fam.gate]
        q = np.array([mr.census(r, B)["q"][key] for r in fam.rays])
        mid = len(q) // 2
        thr = q[mid]
        ulp = 2.0 ** (np.floor(np.log2(thr)) - 23)
        core = q[mid - 64: mid + 65]
        steps = np.diff(core) / ulp
        assert np.all(np.abs(steps) <= 4.0), (fam.name, steps.max())
        assert abs(core[-1] - core[0]) >= 100 * ulp, fam.name


def test_every_setup_gate_has_a_family_and_sunclear_has_three_sides(earth, families):
    v, B = earth
    swept = {f.gate for f in families if f.kind == "sweep"}
    assert set(mr.SETUP_GATES) <= swept
    sides = set()
    for fam in families:
        if fam.name.startswith("sunClear/"):
            for ray in (fam.rays[0], fam.rays[-1]):
                c = mr.census(ray, B)
                sides.add((c["sunPositive"], c["sunClear"]))
    assert sides >= {("true", "true"), ("true", "false"), ("false", "false")}, sides


def test_the_sunset_family_sets_the_sun_part_way(earth, families):
    v, B = earth
    fam = [f for f in families if f.name == "step/sunset"][0]
    states = [mr.sun_step_states(r, B) for r in fam.rays]
    assert any(all(s) for s in states) and any(not any(s) for s in states)
    assert sum(1 for s in states if any(s) and not all(s)) >= 16


def test_the_ozone_families_enter_and_leave_the_tent(earth, families):
    v, B = earth
    for fam in families:
        if not fam.name.startswith("step/ozone"):
            continue
        mixed = 0
        for ray in fam.rays:
            o, d, D = ray[:3].astype(np.float64), ray[3:6].astype(np.float64), float(ray[6])
            alt = [np.linalg.norm(o + d * (D * i / 32.0)) - B.Rp for i in range(32)]
            inside = [abs(a * 1000.0 - 25.0) < 15.0 for a in alt]
            mixed += any(inside) and not all(inside)
        assert mixed >= 16, (fam.name, mixed)


def test_every_spoiler_fails_exactly_its_gate(earth):
    v, B = earth
    sp = mr.spoilers(B)
    assert set(sp) == set(mr.SETUP_GATES)
    for gate, ray in sp.items():
        c = mr.census(ray, B)
        assert c[gate] == "false", (gate, mr.census_line(c))
        for g in mr.SETUP_GATES:
            if g != gate and g not in mr.SPOILER_COUPLED[gate]:
                assert c[g] == "true", (gate, g, mr.census_line(c))


def test_the_variant_families_sweep_their_gates_on_every_block():
    assert tuple(v.name for v in mr.variants()) == mr.VARIANT_NAMES
    for v in mr.variants():
        B = v.bounds()
        fams = mr.setup_families(B, only=mr.VARIANT_FAMILIES)
        assert [f.name for f in fams] == list(mr.VARIANT_FAMILIES)
        for fam in fams:
            ends = [mr.census(fam.rays[0], B)[fam.gate], mr.census(fam.rays[-1], B)[fam.gate]]
            assert sorted(ends) == ["false", "true"], (v.name, fam.name, ends)


@pytest.mark.parametrize("K", [8, 64, 70, 209])
def test_the_wave_forms_hold_what_they_say(K):
    lay = mr.layout(K)
    idx, hole = lay.slots(), lay.holes()
    forms = {name: (first, waves) for name, first, waves in lay.forms}
    assert list(forms) == ["uniform", "spoiled", "natural", "single", "holes"]

    def waves_of(name):
        first, waves = forms[name]
        return [(idx[64 * w: 64 * w + 64], hole[64 * w: 64 * w + 64]) for w in range(first, first + waves)]

    for k, (i, h) in enumerate(waves_of("uniform")):
        assert len(i) == 64 and np.all(i == k) and not h.any()
    assert len(waves_of("uniform")) == K
    for k, (i, h) in enumerate(waves_of("spoiled")):
        lane = mr.SPOILER_LANES[k % 3]
        assert i[lane] == K and np.all(np.delete(i, lane) == k) and not h.any()
    assert len(waves_of("spoiled")) == K
    starts = mr.windows(K)
    assert starts[0] == 0 and all(b - a <= 16 for a, b in zip(starts, starts[1:])) and (K <= 64 or starts[-1] == K - 64)
    for s, (i, h) in zip(starts, waves_of("natural")):
        assert np.all(i == (s + np.arange(64)) % K) and not h.any()
    seen = set()
    for k, (i, h) in enumerate(waves_of("single")):
        assert np.all(i == k) and (~h).sum() == 1
        seen.add(int(np.flatnonzero(~h)[0]))
    assert len(seen) == min(K, 64)  # the active lane moves through the wave
    hw = waves_of("holes")
    assert len(hw) == len(starts) and len(hw[-1][0]) == 41 and len(idx) % 64 == 41
    for s, (i, h) in zip(starts, hw):
        n = len(i)
        assert np.all(i == ((s + np.arange(64)) % K)[:n]) and np.all(h == (np.arange(n) % 3 == 2))
    assert K not in idx[hole == False][: 64 * K]  # noqa: E712  (no spoiler among the uniform waves)


def test_random_rays_and_their_shuffles(earth):
    v, B = earth
    fam = mr.random_rays(B)
    n = len(fam)
    assert 7900 <= n <= 8100 and n % 64 != 0
    r = np.linalg.norm(fam.rays[:, :3].astype(np.float64), axis=1)
    assert r.min() < B.Rp - 0.09 and r.max() > B.Ra + 0.09
    d = np.linalg.norm(fam.rays[:, 3:6].astype(np.float64), axis=1)
    assert (d == 0).any() and (d > 100).any() and (d < 0.01).any()
    assert fam.rays[:, 6].min() < 1e-11 and fam.rays[:, 6].max() > 100
    perms = mr.random_shuffles(n)
    assert len(perms) == 3 and all(sorted(p) == list(range(n)) for p in perms)
    assert not any(np.array_equal(a, b) for a, b in zip(perms, perms[1:]))
    lay = mr.random_layout(n, perms)
    assert len(lay.slots()) % 64 == n % 64 and not lay.holes().any()


def test_the_oracle_values_tell_the_rays_apart(earth, families):
    """Every distinct ray of the Earth families through the oracle once: no family is all NaN, and the outermost rays of every
    sweep give finite values that differ - bit equality with the oracle along the sweep would otherwise prove nothing."""
    v, B = earth
    lut = v.lut()
    total = 0
    for fam in families + [mr.random_rays(B)]:
        want = mr.oracle_values(v.atm, lut, fam.rays)
        total += len(fam)
        if fam.name in mr.ALL_NAN:  # (stated there: 0 / 0 at every sample, on both sides of the threshold)
            assert np.isnan(want).all(), fam.name
            continue
        assert not np.isnan(want).all(), fam.name
        if fam.name in mr.ALL_ZERO:
            assert not want.view(np.uint32).any(), fam.name
            continue
        if fam.kind == "sweep":
            a, b = want[0], want[-1]
            assert np.isfinite(a).all() and np.isfinite(b).all(), (fam.name, a, b)
            assert not np.array_equal(a, b), (fam.name, a, b)
    assert total < 20000
