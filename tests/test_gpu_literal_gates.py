"""The gate suites on the literal pair: libszg_hip_literal.so against libszg_oracle_literal.so, bit for bit, at every
fast-path gate.

The project ships two builds of the same kernels. The literal one (-DSZG_LITERAL, nothing fused) and the literal oracle are what
is pinned to the reference's SPIR-V (tests/test_gpu_spirv_pin.py); the product is held to stay near that evaluation. Both builds
compile the same fast paths - the lean operators behind wave-uniform gates in the march, k_lights and k_composite, the light-tile
masks, the k_frame_prep constants, the composite's march queue - and "results never depend on the flag" has to hold in each
build separately. Ordinary images keep nearly every wave on the near side of nearly every gate; the nine gate suites do not, and
they load the product pair. Here each of them runs once more in a child process (tests/gpu_literal_gates_child.py) with the two
variables of tests/literal_pair.py set: the suite's own cases, run and comparison.

One module-scoped fixture per suite runs that suite's child once; the children run one after the other. One test per group
reads its entry and requires

  - the three literal libraries: libszg_hip_literal.so, libszg_oracle_literal.so and, for the two march suites,
    tests/cpp/libszg_marchrays_literal.so,
  - no case whose comparison failed,
  - as many cases and as many values compared as the same function (run_group of the child module) reports for the product
    pair in THIS process: no case may be left out for the literal pair.

A child that ends by a signal, with status 134 or 139, with any other status than 0 or at its timeout fails its suite's tests
with the tail of its output, and the suites not yet started are skipped with that reason instead of starting another process
on the GPU. Nothing is retried."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests import gpu_literal_gates_child as child
from tests import literal_pair as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# Seconds a child may take: ten times the suite's product-pair time on an MI355X, and not below 60. The figure beside each
# constant is that time: the sum of pytest --durations=0 over the suite's file, the nine files run in one process (212 tests in
# 9.3 s). Ten times any of them stays below 60. A child is that suite plus one process
# start (import of torch, loading the libraries, the first use of the GPU): 2.1 to 4.5 s each, 27 s together
# (profiles/literal_gates.md). On a fresh checkout the first march child also compiles its harness, a few seconds.
TIMEOUTS = {
    "march_rays": 60,               # 2.2 s
    "march_origin_reciprocal": 60,  # below 0.1 s beside march_rays, whose contexts it shares
    "lights_gates": 60,             # 0.8 s (tight and padded)
    "lights_tile_masks": 60,        # 0.3 s
    "composite_gates": 60,          # 2.2 s
    "composite_pixel_path": 60,     # 0.9 s
    "composite_march_queue": 60,    # 0.5 s
    "composite_slots": 60,          # 0.1 s
    "frame_prep_constants": 60,     # below 0.1 s
}
assert tuple(TIMEOUTS) == child.SUITES

_TROUBLE = []  # the reason why no further child is started, once there is one


def trouble(reason, tail):
    """Fails the suite's fixture - pytest keeps a module fixture's failure, so each of the suite's tests fails with this text."""
    _TROUBLE.append(reason)
    pytest.fail(f"{reason}; its output ended:\n{tail[-5000:]}", pytrace=False)


def run_child(suite):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    if _TROUBLE:
        pytest.skip("not started: " + _TROUBLE[0])
    cmd = [sys.executable, os.path.join(ROOT, "tests", "gpu_literal_gates_child.py"), suite]
    began = time.monotonic()
    try:
        r = subprocess.run(cmd, env=lp.literal_environment(), cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUTS[suite])
    except subprocess.TimeoutExpired as e:
        tail = "\n".join(t.decode("utf-8", "replace") if isinstance(t, bytes) else t for t in (e.stdout, e.stderr) if t)
        trouble(f"the literal child of {suite} did not finish within {TIMEOUTS[suite]} s", tail)
    seconds = time.monotonic() - began
    lines = r.stdout.strip().split("\n")
    if r.returncode != 0:
        how = f"signal {-r.returncode}" if r.returncode < 0 else f"status {r.returncode}"
        trouble(f"the literal child of {suite} ended with {how}", r.stdout[-2500:] + "\n" + r.stderr[-2500:])
    out = json.loads(lines[-1])
    out["seconds"] = seconds
    print(f"literal child of {suite}: {seconds:.1f} s, {sum(g['compared'] for g in out['groups'].values())} values compared "
          f"in {len(out['groups'])} groups")
    return out


def _fixture(suite):
    @pytest.fixture(scope="module", name=suite)
    def literal_run():
        return run_child(suite)

    return literal_run


for _suite in child.SUITES:
    globals()["_fixture_" + _suite] = _fixture(_suite)


@pytest.fixture(scope="module")
def gpu():
    return child.gpu_context()


GROUPS = [(s, g) for s in child.SUITES for g in child.group_names(s)]


@pytest.mark.parametrize("suite,group", GROUPS, ids=[f"{s}:{g}" for s, g in GROUPS])
def test_group_on_the_literal_pair(request, gpu, suite, group):
    out = request.getfixturevalue(suite)
    assert out["pair"] == "literal"
    assert out["library"] == lp.LITERAL_HIP and out["oracle"] == lp.LITERAL_ORACLE, out
    assert out["harness"] == (os.path.join("tests", "cpp", "libszg_marchrays_literal.so") if suite in child.MARCH_SUITES else None)
    assert group in out["groups"], f"the child of {suite} did not run {group}: it ran {sorted(out['groups'])}"
    literal = out["groups"][group]
    assert literal["mismatches"] == 0, f"{literal['mismatches']} of {literal['cases']} cases differ on the literal pair; first:\n{literal['first']}"
    product = child.run_group(suite, group, gpu)
    assert product["mismatches"] == 0, f"product pair: {product['first']}"
    assert literal["cases"] == product["cases"] > 0, (literal, product)
    assert literal["compared"] == product["compared"], (literal, product)


@pytest.mark.parametrize("suite", child.SUITES)
def test_child_ran_exactly_the_groups_of_its_suite(request, suite):
    out = request.getfixturevalue(suite)
    assert list(out["groups"]) == child.group_names(suite)
    assert "error" not in out
