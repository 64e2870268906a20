"""tests/march_origin_rays.py without a GPU: the families lie where they say, and the oracle has a value for every ray."""
import numpy as np
import pytest

from tests import march_origin_rays as mo
from tests import march_rays as mr


@pytest.fixture(scope="module")
def variants():
    return {v.name: v for v in mr.variants() if v.name in mo.VARIANTS}


def test_both_sides_of_the_up_gate(variants):
    B = variants["earth"].bounds()
    fams = {f.name: f for f in mo.families(B, "inner")}
    # (Family keeps one of neighbouring rays that are equal in float32: the smallest components of the general frame)
    assert len(fams["gate/axis"]) == 19 and len(fams["gate/sun-0.8"]) >= 11 and len(fams["grazing"]) >= 20, {n: len(f) for n, f in fams.items()}
    axis = fams["gate/axis"]
    up = np.array([mo.up64(r, B) for r in axis.rays])
    assert up.sum() >= 8 and (~up).sum() >= 8, up
    # on the axis the sign of the vertical component, however small, is the side of the gate (0 is not up)
    assert [bool(u) for u in up] == [v > 0.0 for v in axis.knobs]
    assert (axis.rays[:, 4] == np.array(axis.knobs, np.float32)).all() and np.float32(2.0 ** -149) in axis.rays[:, 4]
    # with the sun cosine 0.8 the vertical is no axis: the components float32 can hold lie on their sides
    general = fams["gate/sun-0.8"]
    for v, ray in zip(general.knobs, general.rays):
        c = mr.census(ray, B)["q"]
        assert abs(c["mu_sun"] - mo.SUN) < 1e-6 and abs(c["radius"] - (B.Rp + mo.ALTITUDE)) < 1e-6 and c["D"] == np.float32(mo.PATH)
        if abs(v) >= 2.0 ** -12:
            assert (c["mu"] > 0.0) == (v > 0.0) and abs(c["mu"] - v) < 1e-6, (v, c["mu"])
    # every ray keeps the lean loops: the gate is met inside them
    for fam in fams.values():
        for ray in fam.rays:
            c = mr.census(ray, B)
            assert c["setupLean"] == "true" and c["lean"] == "true" and c["firstStepOnly"] == "true", (fam.name, mr.census_line(c))


def test_the_grazing_rays_point_down_near_the_ground(variants):
    B = variants["earth"].bounds()
    fam = [f for f in mo.families(B, "inner") if f.name == "grazing"][0]
    hits = 0
    for mu, ray in zip(fam.knobs, fam.rays):
        c = mr.census(ray, B)["q"]
        assert not mo.up64(ray, B) or abs(mu) < 1e-7, (mu, c["mu"])
        assert -0.02 - 1e-6 <= c["mu"] <= 1e-7 and abs(c["radius"] - (B.Rp + 1e-6)) < 1e-6
        o, d, D = ray[:3].astype(np.float64), ray[3:6].astype(np.float64), float(ray[6])
        if D != np.float32(mo.PATH):
            hits += 1
            assert abs(np.linalg.norm(o + D * d) - B.Rp) < 2e-6, (mu, D)  # the far end is the ground, to float32
    assert hits >= 16


def test_a_window_holds_both_sides(variants):
    B = variants["earth"].bounds()
    for fam in mo.families(B, "inner")[:2]:
        lay = mr.layout(len(fam))
        up = np.array([mo.up64(r, B) for r in fam.rays] + [False])
        names = [name for name, first, waves in lay.forms]
        assert names == ["uniform", "spoiled", "natural", "single", "holes"]
        mixed = {}
        for name, first, waves in lay.forms:
            for w in range(first, first + waves):
                lanes = slice(64 * w, 64 * w + 64)
                live = up[lay.slots()[lanes]][~lay.holes()[lanes]]
                mixed[name] = mixed.get(name, 0) + int(live.any() and not live.all())
        assert mixed["natural"] >= 1 and mixed["holes"] >= 1 and mixed["uniform"] == 0, (fam.name, mixed)


def test_the_oracle_has_a_value_for_every_ray(variants):
    want = {}
    for name in mo.VARIANTS:
        v = variants[name]
        B, lut = v.bounds(), v.lut()
        for fam in mo.families(B, "inner"):
            values = mr.oracle_values(v.atm, lut, fam.rays)
            assert values.shape == (len(fam), 3)
            assert np.isfinite(values).all(), (name, fam.name, values)
            want[name, fam.name] = values
        for gate in mo.SPOILERS:
            assert np.isfinite(mr.oracle_values(v.atm, lut, mr.spoilers(B)[gate][None, :])).all(), (name, gate)
    # the values tell the two sides of the gate apart, and the rays with +-0.3 read the texel the second variant overwrites
    B = variants["earth"].bounds()
    for fam in mo.families(B, "inner")[:2]:
        fam_name = fam.name
        e, p = want["earth", fam_name], want["lut-texel-2^-60", fam_name]
        k = {v: i for i, v in enumerate(fam.knobs)}
        assert not np.array_equal(e[k[0.3]], e[k[-0.3]])
        if fam_name == "gate/sun-0.8":
            assert not np.array_equal(e[k[0.3]], p[k[0.3]]) and not np.array_equal(e[k[-0.3]], p[k[-0.3]]), fam_name
