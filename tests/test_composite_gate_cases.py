"""The hand-made composite cases (tests/composite_gate_cases.py) without a GPU: that they do sit where they claim - every gate
of k_composite's phase A met from both sides inside a relative 2^-20, and exactly where that is reachable, in every form of
wave - that each group's frame-level flags are the ones it was built for, and the CPU oracle against the census: NaN exactly
in the lanes the census names as poisoned, finite values in the lanes it calls clean."""
import functools

import numpy as np
import pytest

from tests import composite_gate_cases as cg
from tests import march_rays as mr


@functools.lru_cache(maxsize=None)
def built():
    G = cg.build()
    table = {(g.name, k): cg.census(g, k) for g in G for k in range(g.tiles)}
    return G, table


@pytest.fixture(scope="module")
def cases():
    return built()


def test_every_family_and_form_is_present(cases):
    G, _ = cases
    families = {sc.family for g in G for sc in g.scenarios}
    assert families == set(cg.FAMILIES)
    for fam in cg.FAMILIES:
        forms = {sc.form for g in G for sc in g.scenarios if sc.family == fam}
        assert forms == set(cg.FORMS), (fam, forms)
    names = [(g.name, sc.name) for g in G for sc in g.scenarios]
    assert len(names) == len(set(names))
    assert len({g.name for g in G}) == len(G)
    for g in G:  # small images; the last tile column and row are cut by the draw extent; a partial wave keeps its odd lane
        W, H = g.extent
        assert W % 8 and H % 8 and W <= 128 and H <= 40, (g.name, W, H)
        cut_column = cut_row = False
        for k, sc in enumerate(g.scenarios):
            active = g.active(k)
            assert active.any(), (g.name, sc.name)
            x0, y0 = g.origin(k)
            cut_column |= x0 + 8 > W
            cut_row |= y0 + 8 > H
            if sc.odd_lane is not None:
                assert active[sc.odd_lane], (g.name, sc.name)
            if sc.form == "partial":
                hostile = (np.arange(cg.LANES) % 3 == 0) & (np.arange(cg.LANES) != sc.odd_lane)
                assert hostile[active].any() and (sc.depth[hostile] == 0.0).all()
                assert np.isnan(sc.planes["p"][hostile]).all() and np.isinf(sc.planes["n"][hostile].astype(np.float32)).all()
        assert cut_column and cut_row, g.name
    # the prior colour differs from lane to lane: surfaceLuminance is live
    sc = G[0].scenarios[0]
    assert len({tuple(c) for c in sc.prior}) > 32


def test_metallic_values_and_shadow_maps_are_the_stated_ones(cases):
    G, _ = cases
    values = {float(v) if not np.isnan(v) else "nan" for g in G for sc in g.scenarios if sc.family == "reflection_skip"
              for v in sc.planes["o"][:, 2].astype(np.float32)}
    assert {0.0, cg.HALF_MIN, 1.0, "nan"} <= values
    signed = [sc.planes["o"][:, 2] for g in G for sc in g.scenarios if sc.family == "reflection_skip"]
    assert any((np.signbit(v) & (v == 0)).any() for v in signed)
    kinds = {g.shadow for g in G if g.shadow is not None}
    assert kinds == {"random", "equal", "zero", "nearer"}
    m = cg.shadow_map("equal")
    assert m.shape == (cg.MAP_H, cg.MAP_W) and cg.MAP_W != cg.MAP_H and m.strides[0] == 4 * (cg.MAP_W + cg.MAP_PAD)
    assert (m == np.float32(cg.SHADOW_DEPTH)).all() and (cg.shadow_map("zero") == 0).all()


def lanes_of(sc, c, gate):
    lanes = c["active"] if sc.odd_lane is None else (np.arange(cg.LANES) == sc.odd_lane) & c["active"]
    return lanes & c["geometry"] if cg.geometry_gate(gate) else lanes


@pytest.mark.parametrize("gate", list(cg.GATES))
def test_gate_is_met_from_both_sides_in_every_form(cases, gate):
    """For each form of wave: a lane inside the 2^-20 band on each side of the gate (for a mixed or partial wave, held by the
    odd lane - lane 0, 63, 27 or 34), and a lane exactly on the threshold where the inputs can reach it."""
    G, table = cases
    band_needed = gate not in cg.COARSE and gate not in cg.FLAGS
    for form in cg.FORMS:
        found = {0: False, 1: False, "exact": False}
        for g in G:
            for k, sc in enumerate(g.scenarios):
                if sc.form != form:
                    continue
                c = table[g.name, k]
                lanes = lanes_of(sc, c, gate)
                close = lanes & (c["near"][gate] if band_needed else True)
                for side in (0, 1):
                    found[side] |= bool((close & (c["side"][gate] == side)).any())
                found["exact"] |= bool((lanes & c["exact"][gate]).any())
        assert found[0] and found[1], (gate, form, found)
        if gate in cg.EXACT_REACHABLE:
            assert found["exact"], (gate, form)


def test_what_is_recorded_as_unreachable_is_not_reached(cases):
    """No geometry lane of any scenario lies under the planet's surface, and |l + v|^2 never exceeds 4 by more than rounding."""
    G, table = cases
    assert len(cg.UNREACHABLE) == 5 and set(cg.COARSE) <= set(cg.GATES)
    for g in G:
        B = g.bounds()
        for k in range(g.tiles):
            c = table[g.name, k]
            q = cg.geometry(g, k)
            r2 = (q["surface"] ** 2).sum(axis=-1)[c["geometry"]]
            assert not (r2 < B.Rp ** 2 * (1 - 2.0 ** -22)).any(), (g.name, k)  # (a NaN position has no radius)
            hd = q["hd"][c["geometry"]]
            assert not (hd > 4.0 + 2.0 ** -20).any(), (g.name, k)


def frame_sides(table, g):
    c = table[g.name, 0]
    return {gate: int(c["side"][gate][0]) for gate in ("ext_moderate", "sun_sane", "lut_moderate", "sky_finite", "camera_r_floor", "camera_r_hi",
                                                       "sun_lo", "sun_hi", "camera_ext_ceil")}


def test_groups_have_the_frame_level_flags_they_are_built_for(cases):
    G, table = cases
    by = {}
    for g in G:
        by.setdefault(g.base_name, g)
        with np.errstate(all="ignore"):  # (its sun frame is 0 / 0 for the sun of length 0; the radius bounds are not)
            ours, theirs = g.bounds(), mr.Bounds(g.atm)
        assert (ours.leanFloor, ours.extFloor, ours.extCeil) == (theirs.leanFloor, theirs.extFloor, theirs.extCeil)
    ordinary = dict(ext_moderate=1, sun_sane=1, lut_moderate=1, sky_finite=1, camera_r_floor=1, camera_r_hi=0, sun_lo=1, sun_hi=0, camera_ext_ceil=0)
    expect = {
        "skip_all_true": {}, "surface_length": {}, "classification": {}, "shadow_random": {}, "planet_shadow_day": {},
        "skip_normal": {}, "skip_surface_ceiling": {}, "skip_camera_on_ground": {}, "skip_camera_under_ceiling": {},
        "skip_ext_moderate": dict(ext_moderate=0), "skip_sun_radius_2": dict(sun_sane=0), "skip_sun_vertical": dict(sun_sane=0),
        "skip_tlut_texel_2^-60": dict(lut_moderate=0), "skip_camera_over_ceiling": dict(camera_ext_ceil=1),
        "skip_sky_nan_tap": dict(sky_finite=0), "skip_sky_nan_far": dict(sky_finite=0), "skip_sky_inf_tap": dict(sky_finite=0),
        "skip_sky_inf_far": dict(sky_finite=0),
        "sun_length_zero": dict(sun_lo=0, sun_sane=0), "sun_length_lo-below": dict(sun_lo=0, sun_sane=0), "sun_length_lo-on": dict(sun_sane=0),
        "sun_length_lo-above": dict(sun_sane=0), "sun_length_one": {}, "sun_length_hi-below": dict(sun_sane=0),
        "sun_length_hi-on": dict(sun_sane=0), "sun_length_hi-above": dict(sun_hi=1, sun_sane=0),
        "camera_2^30_below": dict(camera_ext_ceil=1), "camera_2^30_on": dict(camera_ext_ceil=1),
        "camera_2^30_above": dict(camera_r_hi=1, camera_ext_ceil=1), "camera_2^30_far-above": dict(camera_r_hi=1, camera_ext_ceil=1),
        "half_vector_cancelled": {}, "half_vector_on": {}, "half_vector_mixed27": {}, "view_length_mixed0": {}, "planet_shadow_night": {},
    }
    for name, change in expect.items():
        assert frame_sides(table, by[name]) == {**ordinary, **change}, name
    # the camera sweep crosses the lean floor, monotonically, within the band on both sides
    sweep = [by[f"camera_floor_{k:02d}"] for k in range(len(cg.CAMERA_SWEEP))]
    sides = [frame_sides(table, g)["camera_r_floor"] for g in sweep]
    assert sides[0] == 1 and sides[-1] == 0 and sides == sorted(sides, reverse=True), sides
    assert all(table[g.name, 0]["near"]["camera_r_floor"][0] for g in sweep)
    radii = [float(np.sqrt(table[g.name, 0]["value"]["camera_r_floor"][0])) for g in sweep]
    step = float(np.spacing(np.float32(radii[0])))
    assert max(np.diff(radii)) <= 0 and min(np.diff(radii)) >= -1.01 * step  # no float32 radius between the ends is left out
    assert radii[0] - radii[-1] >= 6 * step
    # every sky-view poke under a tap is under the odd lane's reflection tap and that lane is a non-metal or a metal alike
    for name in ("skip_sky_nan_tap", "skip_sky_inf_tap"):
        g = by[name]
        assert g.slut_poke is not None and g.slut_poke[0] < cg.SLUT_EXTENT[1] // 2
        assert by[name.replace("tap", "far")].slut_poke[0] > cg.SLUT_EXTENT[1] // 2 + 1


def test_scenarios_land_on_the_side_they_are_named_for(cases):
    G, table = cases
    by_name = {(g.base_name, sc.name): (g, k) for g in G for k, sc in enumerate(g.scenarios)}

    def lane0(group, name, gate):
        g, k = by_name[group, name]
        c = table[g.name, k]
        return int(c["side"][gate][0]), bool(c["near"][gate][0]), bool(c["exact"][gate][0])

    assert lane0("surface_length", "zero-segment/uniform-far", "surface_len_lo") == (0, False, False)
    assert lane0("surface_length", "x-2^-30-step/uniform-on", "surface_len_lo") == (1, True, True)
    assert lane0("surface_length", "x-2^-30-step/uniform-far", "surface_len_lo") == (0, True, False)
    assert lane0("surface_length", "x-2^-30-step/uniform-near", "surface_len_lo") == (1, True, False)
    assert lane0("surface_length", "z-2^-31-among-ordinary/uniform-far", "surface_len_lo")[0] == 0
    assert lane0("surface_length", "x-2^30-step/uniform-on", "surface_len_hi") == (0, True, True)
    assert lane0("surface_length", "x-2^30-step/uniform-far", "surface_len_hi") == (1, True, False)
    assert lane0("surface_radius", "y-2^30-step/uniform-on", "surface_r_hi") == (0, True, True)
    assert lane0("surface_radius", "y-2^30-step/uniform-far", "surface_r_hi") == (1, True, False)
    assert lane0("half_vector_cancelled", cg.STANDARD + "/uniform-near", "half_lo") == (0, False, False)
    assert lane0("half_vector_on", cg.STANDARD + "/uniform-near", "half_lo") == (1, True, True)
    assert lane0("half_vector_below", cg.STANDARD + "/uniform-near", "half_lo") == (0, True, False)
    assert lane0("planet_shadow_night", "ground-against-above/uniform-on", "planet_pt0") == (0, True, True)
    assert lane0("planet_shadow_night", "ground-against-above/uniform-near", "planet_pt0")[0] == 1
    assert lane0("planet_shadow_day", "miss-among-ordinary/uniform-far", "planet_hit")[0] == 0
    assert lane0("skip_camera_under_ground", "metallic-one/uniform-near", "above_ground") == (1, True, False)
    assert lane0("skip_camera_on_ground", "metallic-one/uniform-near", "above_ground") == (0, True, True)
    assert lane0("skip_surface_ceiling", "surface-ceiling-metallic-plus-zero/uniform-far", "surface_ext_ceil") == (1, True, False)
    assert lane0("skip_surface_ceiling", "surface-ceiling-metallic-plus-zero/uniform-near", "surface_ext_ceil") == (0, True, False)
    assert lane0("skip_all_true", "metallic-half-denormal/uniform-far", "metallic_zero") == (1, True, False)
    assert lane0("skip_all_true", "metallic-minus-zero/uniform-far", "metallic_zero") == (0, True, True)
    # in the mixed half-vector and view-length groups ONE lane of ONE wave fails, the odd lane of the form's first scenario
    for g in G:
        for prefix, gate in (("half_vector_", "half_lo"), ("view_length_", "view_lo")):
            form = g.base_name[len(prefix):]
            if not g.base_name.startswith(prefix) or form not in cg.FORMS:
                continue
            x, y, k0 = g.odd_pixel(form)
            failing = [(k, int(lane)) for k in range(g.tiles) for lane in np.flatnonzero(table[g.name, k]["active"] & (table[g.name, k]["side"][gate] != 1))]
            assert failing == [(k0, g.scenarios[k0].odd_lane)], (g.name, failing)


def test_the_cases_bite(cases):
    """The CPU oracle gives NaN exactly where the census says the reference's arithmetic must: a NaN sky-view texel under a
    lane's tap (a non-metal's reflection tap included: 0 * NaN), NaN or inf normals, a NaN metallic, a NaN view direction. A
    reflection that is wrongly skipped there leaves the pixel finite and shows. And it gives finite values in the lanes the
    census calls clean - among them the zero-length segments and the cancelled half vectors, whose NaN ends in a clamp."""
    G, table = cases
    poisoned, clean, kinds = 0, 0, set()
    skipped_nonmetal_under_nan = 0
    for g in G:
        debug, _ = cg.oracle_frame(g)
        assert debug.shape[:2] == (g.extent[1], g.extent[0])
        for k, sc in enumerate(g.scenarios):
            c = table[g.name, k]
            got = cg.tile_of(g, k, debug)[:, :3]
            bad = c["poisoned"] & ~np.isnan(got).any(axis=1)
            assert not bad.any(), f"{g.name}/{sc.name} lane {np.argmax(bad)}: {got[np.argmax(bad)]} {cg.verdict(g, k, int(np.argmax(bad)))}"
            bad = c["clean"] & ~np.isfinite(got).all(axis=1)
            assert not bad.any(), f"{g.name}/{sc.name} lane {np.argmax(bad)}: {got[np.argmax(bad)]} {cg.verdict(g, k, int(np.argmax(bad)))}"
            poisoned, clean = poisoned + int(c["poisoned"].sum()), clean + int(c["clean"].sum())
            kinds |= set(c["why"][c["poisoned"]])
            if g.base_name == "skip_sky_nan_tap":
                skipped_nonmetal_under_nan += int((c["poisoned"] & (c["value"]["metallic_zero"] == 0.0) & c["geometry"]).sum())
    assert kinds == {"NaN / inf normal: the reflection direction is NaN", "NaN metallic", "the sky-view tap meets the poked texel",
                     "NaN view direction"}, kinds
    assert poisoned > 5000 and clean > 20000 and skipped_nonmetal_under_nan >= 5, (poisoned, clean, skipped_nonmetal_under_nan)
    by_name = {(g.base_name, sc.name): (g, k) for g in G for k, sc in enumerate(g.scenarios)}
    for key in (("surface_length", "zero-segment/uniform-far"), ("surface_length", "zero-segment-metal/uniform-far"),
                ("half_vector_cancelled", cg.STANDARD + "/uniform-near"), ("half_vector_cancelled", cg.STANDARD + "/uniform-far")):
        g, k = by_name[key]
        c = table[g.name, k]
        assert c["clean"][c["active"]].all(), key
        gate = "surface_len_lo" if key[0] == "surface_length" else "half_lo"
        assert (c["value"][gate][c["active"]] == 0.0).all(), key


def test_counts_for_the_record(cases):
    G, _ = cases
    groups, scenarios, lanes, gates = cg.counts(G)
    print(f"composite gate cases: {groups} groups, {scenarios} scenarios, {lanes} lanes, {gates} gates")
    assert groups >= 80 and scenarios >= 1500 and gates == len(cg.GATES)
