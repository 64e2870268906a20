"""tests/literal_pair.py and the group tables of tests/gpu_literal_gates_child.py, without a GPU: which pair an environment
names, that half a pair is refused with a text that says what to set, and that the tables hold every parametrized case of the
nine gate suites except the ones tests/test_gpu_literal_gates.py says it leaves out."""
import pytest

from tests import gpu_literal_gates_child as child
from tests import literal_pair as lp

LITERAL = "/somewhere/syzygy_amd/csrc/libszg_hip_literal.so"


def test_pair_from_the_environment():
    assert lp.pair({}) == "product"
    assert lp.pair({"SZG_ORACLE_LITERAL": ""}) == "product"
    assert lp.pair({"SZG_HIP_LIBRARY": "/elsewhere/libszg_hip.so"}) == "product"  # another build of the product, named explicitly
    assert lp.pair({"SZG_ORACLE_LITERAL": "1", "SZG_HIP_LIBRARY": LITERAL}) == "literal"
    env = lp.literal_environment({"PATH": "/bin"})
    assert env["PATH"] == "/bin" and lp.pair(env) == "literal"


@pytest.mark.parametrize("env,says", [
    ({"SZG_ORACLE_LITERAL": "1"}, "does not name libszg_hip_literal.so"),
    ({"SZG_ORACLE_LITERAL": "1", "SZG_HIP_LIBRARY": "/elsewhere/libszg_hip.so"}, "does not name libszg_hip_literal.so"),
    ({"SZG_HIP_LIBRARY": LITERAL}, "SZG_ORACLE_LITERAL is not 1"),
    ({"SZG_ORACLE_LITERAL": "0", "SZG_HIP_LIBRARY": LITERAL}, "set it to 1 or unset it"),
    ({"SZG_ORACLE_LITERAL": "true"}, "set it to 1 or unset it"),
])
def test_half_a_pair_is_an_error(env, says):
    with pytest.raises(ValueError, match=says):
        lp.pair(env)


def test_tally_counts_only_while_it_is_open():
    lp.compared(5)
    with lp.tally() as outer:
        lp.compared(3)
        with lp.tally() as inner:
            lp.compared(4)
        lp.compared(1)
    lp.compared(7)
    assert (outer.compared, inner.compared) == (8, 4)


def test_parametrizations_are_the_product_of_the_marks():
    @pytest.mark.parametrize("a", [1, 2])
    @pytest.mark.parametrize("b,c", [(3, 4), (5, 6), (7, 8)])
    def toy(a, b, c):
        return a, b, c

    got = child.parametrizations(toy)
    assert len(got) == 6 and {toy(**kw) for kw in got} == {(a, b, c) for a in (1, 2) for b, c in ((3, 4), (5, 6), (7, 8))}
    assert child.parametrizations(lambda: None) == [{}]


# what the literal run leaves out of each suite's parametrized tests, by design (tests/test_gpu_literal_gates.py): the padded
# images of the lights gates and the larger sizes of the tile-mask image test. Everything else is a case of some group.
def _parametrized_cases(suite):
    m = child.module(suite)
    total = 0
    for name in dir(m):
        fn = getattr(m, name)
        if name.startswith("test_") and callable(fn) and getattr(fn, "__module__", None) == m.__name__ and \
                any(mark.name == "parametrize" for mark in getattr(fn, "pytestmark", [])):
            total += len(child.parametrizations(fn))
    return total


def test_the_group_tables_hold_every_parametrized_case():
    for suite in child.SUITES:
        table = child.groups(suite)
        assert table and len(set(table)) == len(table), suite
    count = {s: len(child.groups(s)) for s in child.SUITES}
    cases = {s: sum(len(cases()) for cases in child.groups(s).values()) for s in ("lights_tile_masks", "composite_pixel_path", "composite_march_queue",
                                                                                   "composite_slots", "frame_prep_constants")}
    # suites whose groups ARE their parametrized tests (march_rays has one test without parameters beside them)
    assert count["march_rays"] == _parametrized_cases("march_rays") + 1
    assert count["march_origin_reciprocal"] == _parametrized_cases("march_origin_reciprocal")
    assert count["composite_gates"] == _parametrized_cases("composite_gates")
    assert 2 * count["lights_gates"] == _parametrized_cases("lights_gates")  # tight and padded: the tight half
    # suites whose cases are their parametrized tests
    tm = child.module("lights_tile_masks")
    assert cases["lights_tile_masks"] == len(tm.SPOTS) and len(tm.SIZES) * len(tm.SPOTS) == _parametrized_cases("lights_tile_masks")
    assert cases["composite_pixel_path"] == _parametrized_cases("composite_pixel_path")
    assert cases["composite_march_queue"] == _parametrized_cases("composite_march_queue") + 2  # two tests without parameters
    assert cases["composite_slots"] == _parametrized_cases("composite_slots")
    assert cases["frame_prep_constants"] == _parametrized_cases("frame_prep_constants")
