"""The per-unit variables of syzygy_amd/csrc/Makefile (SCHED_<unit>: machine-scheduler options chosen by measurement,
DEFS_<unit>: defines) apply by NAME, through $(SCHED_$*) and $(DEFS_$*): after a unit is renamed or split, a variable that
keeps the old name applies to nothing, the build succeeds, and the only symptom is a slower pass (the lights pass: 8 %).
Here every such variable has its source file, the options reach the command lines of the default and the literal build, and
the resource-usage targets name files that exist. Nothing is built (make -n)."""
import os
import re

from tests import native

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "syzygy_amd", "csrc")
ASSIGNMENTS = native.assignments(os.path.join(CSRC, "Makefile"))


def _per_unit(prefix):
    return {name[len(prefix):]: value for name, (_, value) in ASSIGNMENTS.items() if name.startswith(prefix)}


def _expanded(value):
    """`value` with its references to other variables of the Makefile replaced, as words."""
    return re.sub(r"\$\((\w+)\)", lambda m: ASSIGNMENTS[m.group(1)][1], value).split()


def _contains(words, run):
    return any(words[i:i + len(run)] == run for i in range(len(words) - len(run) + 1))


def test_every_per_unit_variable_has_its_source_file():
    sched, defs = _per_unit("SCHED_"), _per_unit("DEFS_")
    assert {"kernels_lights", "kernels_composite", "kernels_lut"} <= set(sched) and "api_core" in defs
    for unit in sched:
        assert os.path.exists(os.path.join(CSRC, unit + ".hip")), unit
    for unit in defs:
        assert os.path.exists(os.path.join(CSRC, unit + ".cpp")) or os.path.exists(os.path.join(CSRC, unit + ".hip")), unit


def test_scheduler_options_reach_the_command_lines():
    for unit, value in _per_unit("SCHED_").items():
        options = _expanded(value)
        assert options, unit
        for target in (unit + ".o", "literal/" + unit + ".o"):
            compiles = [c.split() for c in native.commands(target, CSRC) if unit + ".hip" in c.split()]
            assert len(compiles) == 1 and _contains(compiles[0], options), (target, compiles)
    # what was measured, by name: the iterative ILP scheduler for the lights pass, and the options of the two march units
    for target in ("kernels_lights.o", "literal/kernels_lights.o"):
        assert "-amdgpu-sched-strategy=iterative-ilp" in " ".join(native.commands(target, CSRC)).split()
    for target in ("kernels_lut.o", "literal/kernels_lut.o"):
        words = " ".join(native.commands(target, CSRC)).split()
        assert "-amdgpu-sched-strategy=max-ilp" in words and "-misched-postra-direction=bottomup" in words
    for target in ("kernels_composite.o", "literal/kernels_composite.o"):
        assert "-misched-postra-direction=bottomup" in " ".join(native.commands(target, CSRC)).split()


def test_resource_usage_targets_name_existing_files():
    for target in ("resource-usage", "march-resource-usage", "ms-resource-usage"):
        compiles = [c.split() for c in native.commands(target, CSRC) if " -c " in c]
        assert compiles, target
        for words in compiles:
            source = words[words.index("-c") + 1]
            assert os.path.exists(os.path.join(CSRC, source)), (target, source)
            # ... compiled with the options the library gives that unit
            assert _contains(words, _expanded(_per_unit("SCHED_").get(os.path.splitext(source)[0], ""))), (target, source)
