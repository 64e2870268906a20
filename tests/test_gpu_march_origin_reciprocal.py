"""The march's quotient by T_origin, whose divisor is the same at every step of a ray, against the oracle's scalar march.

tests/march_origin_rays.py: rays on both sides of mu = 0, where a lane chooses between T_end / T_origin and
T_origin / T_end, and down rays grazing the ground, where T_origin is small. Laid out as whole waves of one
ray, windows that hold up and down lanes together, waves with one spoiler lane, waves with every third lane off and waves with
a single active lane (march_rays.layout), under the block "earth" and under "lut-texel-2^-60", whose LUT is not moderate and
sends every wave through the generic quotient, in both configurations of the harness (tests/cpp/marchrays.hip).

Equality rule (check_family of tests/test_gpu_march_rays.py): every float bit-identical to oracle_scattering_integral of the
lane's ray, sign of zero included, NaN for NaN; no ray is left out; hole slots and the slots past n keep the sentinel."""
import pytest

from tests import march_origin_rays as mo
from tests.test_gpu_march_rays import CONFIGS, check_family, context, run  # noqa: F401  (run: the harness check_family drives)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("spoiler", mo.SPOILERS)
@pytest.mark.parametrize("name", mo.VARIANTS)
def test_origin_reciprocal_families(name, spoiler, config):
    ctx = context(name)
    fams = mo.families(ctx.B, spoiler)
    assert [f.name for f in fams] == ["gate/sun-0.8", "gate/axis", "grazing"]
    for fam in fams:
        check_family(ctx, fam, config == "prepped")
