"""The hand-made lights cases (tests/lights_gate_cases.py) without a GPU: that they do sit where they claim - every gate of
k_lights / k_light_prep met from both sides inside a relative 2^-20, and exactly where that is reachable, in every form of
wave - and the CPU oracle against the census and against a float64 evaluation of the pair's term."""
import numpy as np
import pytest

from tests import lights_gate_cases as lg
from tests.util import RTOL


@pytest.fixture(scope="module")
def cases():
    L, G = lg.build()
    table = {}  # (group name, k, light name) -> census
    for g in G:
        for k in range(g.tiles):
            for name in g.light_names:
                table[g.name, k, name] = lg.census(g, k, L[name])
    return L, G, table


def test_light_records_have_the_flags_they_are_built_for(cases):
    L, G, _ = cases
    assert set(L) == set(lg.LIGHT_FLAGS)
    for name, (lean, tight) in lg.LIGHT_FLAGS.items():
        assert (int(L[name].lean), int(L[name].tight)) == (lean, tight), (name, L[name].fb_raw)
    used = {n for g in G for n in g.light_names}
    assert used == set(L), set(L) - used
    # each criterion of k_light_prep from both sides, the failing record differing from the passing one in that value alone
    assert L["lean_pos_above"].position[0] == lg.up(4096.0) and L["tight_pos_on"].position[0] == 4096.0
    assert np.abs(L["lean_row_above"].rows).max() == lg.up(2.0 ** 14) and np.abs(L["tight_row_on"].rows).max() == 2.0 ** 14
    assert L["lean_fb_hi_above"].fb_raw == lg.up(2.0 ** 20) and L["tight_fb_hi_on"].fb_raw == 2.0 ** 20
    assert L["lean_fb_lo_below"].fb_raw == lg.dn(2.0 ** -20) and L["tight_fb_lo_on"].fb_raw == 2.0 ** -20
    assert L["generic_cs_below"].cs[0] == lg.dn(2.0 ** -30) and L["lean_cs_on"].cs[0] == 2.0 ** -30 and L["lean_cs_zero"].cs[0] == 0.0
    assert np.abs(L["generic_row_above"].rows).max() == lg.up(2.0 ** 28) and np.abs(L["lean_row_on"].rows).max() == 2.0 ** 28
    for name, bound in (("generic_fb30_hi_above", 2.0 ** 30), ("generic_fb30_lo_below", 2.0 ** -30)):
        l = L[name]  # factor and distance are inside their own ranges: only the combined bound fails
        assert 2.0 ** -30 <= l.factor <= 2.0 ** 30 and 2.0 ** -30 <= l.distance <= 2.0 ** 30
        assert abs(float(l.fb_raw) / bound - 1.0) <= lg.BAND and (l.fb_raw > bound if bound > 1 else l.fb_raw < bound)
    assert L["lean_fb30_hi_on"].fb_raw == 2.0 ** 30 and L["lean_fb30_lo_on"].fb_raw == 2.0 ** -30
    assert any(L[n].shadow for n in L) and any(not L[n].shadow for n in L)
    assert any(g.skip < 2 for g in G) and {g.skip for g in G} == {0, 1, 2, 3}


def test_every_family_and_form_is_present(cases):
    _, G, _ = cases
    families = {sc.family for g in G for sc in g.scenarios}
    assert families == set(lg.FAMILIES)
    for fam in lg.FAMILIES:
        forms = {sc.form for g in G for sc in g.scenarios if sc.family == fam}
        assert forms == set(lg.FORMS), (fam, forms)
    names = [(g.name, sc.name) for g in G for sc in g.scenarios]
    assert len(names) == len(set(names))
    for g in G:  # the last tile column and row are cut by the draw extent, and a partial wave keeps its odd lane
        W, H = g.extent
        assert W % 8 and H % 8
        for k, sc in enumerate(g.scenarios):
            active = g.active(k)
            assert active.any(), (g.name, sc.name)
            if sc.form == "partial":
                assert active[sc.odd_lane] and not active.all()


@pytest.mark.parametrize("gate", list(lg.GATES))
def test_gate_is_met_from_both_sides_in_every_form(cases, gate):
    """For each form of wave: a pair inside the 2^-20 band on each side of the gate (for a mixed or partial wave, held by the
    odd lane - lane 0, 63, 27 or 34 - with the rest of the wave on the other side or far away), and a pair exactly on the
    threshold where the inputs can reach it."""
    L, G, table = cases
    band_needed = gate not in lg.COARSE
    for form in lg.FORMS:
        found = {0: False, 1: False, "exact": False}
        for g in G:
            for k, sc in enumerate(g.scenarios):
                if sc.form != form:
                    continue
                for name in g.light_names:
                    c = table[g.name, k, name]
                    lanes = c["active"] if sc.odd_lane is None else (np.arange(lg.LANES) == sc.odd_lane) & c["active"]
                    close = lanes & (c["near"][gate] if band_needed else True)
                    for side in (0, 1):
                        found[side] |= bool((close & (c["side"][gate] == side)).any())
                    found["exact"] |= bool((lanes & c["exact"][gate]).any())
        assert found[0] and found[1], (gate, form, found)
        if gate in lg.EXACT_REACHABLE:
            assert found["exact"], (gate, form)


@pytest.mark.parametrize("flag", ["pixel_finite", "pixel_moderate", "tight_pixel"])
def test_pixel_flag_is_false_in_one_lane_of_every_form(cases, flag):
    L, G, table = cases
    for form in lg.FORMS:
        lone, all_true = False, False
        for g in G:
            for k, sc in enumerate(g.scenarios):
                if sc.form != form:
                    continue
                c = table[g.name, k, g.light_names[0]]
                f, a = c["flags"][flag], c["active"]
                all_true |= bool(f[a].all())
                lone |= (sc.odd_lane is not None and not f[sc.odd_lane] and bool(f[a & (np.arange(lg.LANES) != sc.odd_lane)].all())) or \
                    (sc.odd_lane is None and not f[a].any())
        assert lone and all_true, (flag, form)


def test_scenarios_land_on_the_side_they_are_named_for(cases):
    """A scenario whose census lands on the unintended side is an error of the case builder: spot checks of the designed
    positions (the parametrised coverage test above holds every gate; this one holds individual names)."""
    L, G, table = cases
    by_name = {(g.name, sc.name): (g, k) for g in G for k, sc in enumerate(g.scenarios)}

    def lane0(group, name, gate, light=None):
        g, k = by_name[group, name]
        c = table[g.name, k, light or g.light_names[0]]
        return int(c["side"][gate][0]), bool(c["near"][gate][0]), bool(c["exact"][gate][0])

    assert lane0("cone_exact", "rim-x-step/uniform-on", "cone_exact") == (1, True, True)
    assert lane0("cone_exact", "rim-x-step/uniform-near", "cone_exact") == (0, True, False)
    assert lane0("cone_exact", "rim-345-step/uniform-on", "cone_exact")[:2] == (1, True)
    assert lane0("cone_exact", "rim-345-band/uniform-far", "cone_exact") == (1, True, False)
    assert lane0("cone_reject", "x-step/uniform-on", "cone_reject") == (0, True, True)
    assert lane0("cone_reject", "x-step/uniform-far", "cone_reject") == (1, True, False)
    assert lane0("cone_reject", "between-rim-and-reject/uniform-far", "cone_reject")[0] == 0
    assert lane0("cone_reject", "between-rim-and-reject/uniform-far", "cone_exact")[0] == 1
    assert lane0("clip_w_sign", "behind-inside-mirrored-cone/uniform-far", "cw_sign")[0] == 0
    assert lane0("clip_w_sign", "behind-inside-mirrored-cone/uniform-far", "cone_exact")[0] == 0
    assert lane0("clip_w_sign", "behind-outside-mirrored-cone/uniform-far", "cone_exact")[0] == 1
    assert lane0("clip_w_small", "w-2^-30-step/uniform-on", "cw_lo") == (1, True, True)
    assert lane0("clip_w_small", "w-2^-30-step/uniform-on", "d2_lo")[:2] == (1, False)  # one gate at a time
    assert lane0("clip_w_large", "w-2^30-step/uniform-far", "cw_hi") == (1, True, False)
    assert lane0("clip_w_large", "w-2^30-step/uniform-far", "d2_hi")[:2] == (0, False)
    assert lane0("guard", "guard-step-backface/uniform-on", "guard") == (1, True, True)
    assert lane0("guard", "guard-band-outside/uniform-far", "guard")[:2] == (0, True)
    assert lane0("guard", "guard-band-outside/uniform-far", "cone_reject")[0] == 1
    assert lane0("back_face", "ndl-denormal-guarded-moderate/uniform-near", "back_face") == (1, True, False)
    assert lane0("back_face", "ndl-denormal-unguarded-metallic16/uniform-far", "back_face") == (0, True, False)
    assert lane0("back_face", "ndl-denormal-unguarded-metallic16/uniform-far", "guard")[0] == 0
    assert lane0("half_vector", "hd-2^-40-step/uniform-on", "hd_lo") == (1, True, True)
    assert lane0("half_vector", "hd-2^-40-band/uniform-near", "hd_lo") == (1, True, False)
    assert lane0("half_vector", "hd-zero/uniform-far", "hd_lo")[0] == 0
    assert lane0("half_vector_max", "hd-4-fresnel-base-0/uniform-far", "track_pow") == (0, False, False)
    assert lane0("track_cxy", "cx-2^-60-step/uniform-on", "track_cx") == (1, True, True)
    assert lane0("track_cxy", "cx-2^-60-step/uniform-far", "track_cy")[:2] == (1, False)
    assert lane0("track_cz", "cz-2^-60-step/uniform-far", "track_cz") == (0, True, False)
    assert lane0("track_pow", "specular-base-smallest-normal-band/uniform-far", "track_pow")[:2] == (0, True)
    assert lane0("track_pow", "specular-base-smallest-normal-band/uniform-near", "track_pow")[:2] == (1, True)
    for rough in (2.0, 1.0, 0.5):  # a pow base of exactly 0 on a pair that faces the light and lies inside the cone
        name = f"specular-base-zero-lit-roughness-{rough}/uniform-far"
        assert lane0("half_vector", name, "track_pow") == (0, False, False) and lane0("half_vector", name, "back_face")[0] == 1
        assert lane0("half_vector", name, "cone_exact")[0] == 0 and lane0("half_vector", name, "hd_lo")[0] == 1
        g, k = by_name["half_vector", name]
        assert (table[g.name, k, "tight"]["value"]["track_pow"] == 0.0).all()
    # the pixels of the track scenarios are ones the optimistic pass is entered for: tight pixels under a tight light
    for group in ("track_cxy", "track_cz", "track_cz_denormal", "track_pow", "track_fresnel"):
        for (gn, _), (g, k) in by_name.items():
            if gn == group:
                c = table[g.name, k, g.light_names[0]]
                assert c["flags"]["tight_pixel"][c["active"]].all() and c["flags"]["light_tight"].all(), (group, g.scenarios[k].name)


def _single_light_groups(G):
    return [g for g in G if g.skip >= 2 and len(g.light_names) == 1]


def test_oracle_gives_the_exact_zero_and_the_nan_the_census_predicts(cases):
    """(colour * strength / falloff) * 0 is an exact zero while the quotient is finite and inf * 0 = NaN where it is not:
    what the culls of k_lights rely on, held against the reference's arithmetic."""
    L, G, table = cases
    zeros = nans = 0
    for g in _single_light_groups(G):
        debug, _ = lg.oracle_frame(g, L)
        light = L[g.light_names[0]]
        for k, sc in enumerate(g.scenarios):
            c = table[g.name, k, light.name]
            got = lg.tile_of(g, k, debug)[:, :3]
            z, n = c["zero"] & c["active"], c["nan"] & c["active"]
            bad = z & ~(got == 0.0).all(axis=1)
            assert not bad.any(), f"{g.name}/{sc.name} lane {np.argmax(bad)}: {got[np.argmax(bad)]} {lg.verdict(g, k, int(np.argmax(bad)), light)}"
            bad = n & ~np.isnan(got).all(axis=1)
            assert not bad.any(), f"{g.name}/{sc.name} lane {np.argmax(bad)}: {got[np.argmax(bad)]} {lg.verdict(g, k, int(np.argmax(bad)), light)}"
            zeros, nans = zeros + int(z.sum()), nans + int(n.sum())
            inactive = ~c["active"]
            assert (got[inactive] == 0.0).all()
    assert zeros > 10000 and nans > 100, (zeros, nans)


def test_oracle_matches_a_float64_evaluation_on_interior_pairs(cases):
    """Catches a restatement error that the oracle and the kernel would share. Interior: no gate within 2^-20, q <= 0.2, every
    operand finite and of ordinary size, no shadow map. Bound: the project's RTOL."""
    L, G, table = cases
    pairs = 0
    for g in _single_light_groups(G):
        debug, _ = lg.oracle_frame(g, L)
        light = L[g.light_names[0]]
        for k, sc in enumerate(g.scenarios):
            c = table[g.name, k, light.name]
            sel = c["interior"] & c["active"]
            if not sel.any():
                continue
            want = lg.term64(g, k, light)[sel]
            got = lg.tile_of(g, k, debug)[sel, :3].astype(np.float64)
            err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
            err[want == 0.0] = np.abs(got[want == 0.0])
            assert (err <= RTOL).all(), f"{g.name}/{sc.name}: relative error {err.max():.3e} {lg.verdict(g, k, int(np.flatnonzero(sel)[0]), light)}"
            pairs += int(sel.sum())
    assert pairs > 10000, pairs


def test_slot_numbering_follows_the_skip_count(cases):
    """lights.comp:138-161: the shadow-map index starts at the skip count. With two directional lights, skip counts of 2 and of
    3 (beyond the directional lights, which the C ABI accepts like the shader does) both evaluate the spot lights alone; the
    cases attach each spot light's map at the slot that rule gives, so the oracle's two frames are the same image - and a
    different one from the frame without the maps' shade."""
    L, G, _ = cases
    by = {g.name: g for g in G}
    g2, g3 = by["slots_skip2"], by["slots_skip3"]
    assert [g2.slot(j) for j in range(4)] == [2, 3, 4, 5] and [g3.slot(j) for j in range(4)] == [3, 4, 5, 6]
    assert [by["slots_skip0"].slot(j) for j in range(4)] == [2, 3, 4, 5] and [by["slots_skip1"].slot(j) for j in range(4)] == [2, 3, 4, 5]
    assert sorted(g3.shadow_maps(L)) == [0, 1, 4, 6] and sorted(g2.shadow_maps(L)) == [0, 1, 3, 5]
    a, b = lg.oracle_frame(g2, L)[0], lg.oracle_frame(g3, L)[0]
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    shaded = lg.oracle_frame(by["pcf_nearer"], L)[0]
    assert (shaded[..., :3] == 0).all(axis=-1).any() and (shaded[..., :3] > 0).any()
    # the moon (skip = 1) and the sun as well (skip = 0) add light to the same pixels
    moon, sun = lg.oracle_frame(by["slots_skip1"], L)[0][..., :3], lg.oracle_frame(by["slots_skip0"], L)[0][..., :3]
    assert (moon >= a[..., :3]).all() and (moon > a[..., :3]).any() and (sun >= moon).all() and (sun > moon).any()
    with_moon = lg.oracle_frame(by["light_all_with_moon"], L)[0]
    assert np.isfinite(with_moon).all() and (with_moon[..., :3] > 0).any()
