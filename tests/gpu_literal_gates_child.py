"""The gate suites as tables of groups, and the child process of tests/test_gpu_literal_gates.py that runs one of them.

Only the gate suites put waves on the far side of a fast-path gate, in mixed waves and in waves with a single lane outside, and
they load the product pair. A library cannot be swapped inside a process that has loaded the other one, so

    python tests/gpu_literal_gates_child.py <suite>

started with the two variables of tests/literal_pair.py set, imports the suite's own test module and calls what its tests call:
the same case tables, the same run, the same bit-for-bit comparison, now of libszg_hip_literal.so against
libszg_oracle_literal.so (and of tests/cpp/libszg_marchrays_literal.so, where the suite drives the march harness). Nothing of
a suite is copied here; where a test's body is the run, the test function itself is called, with the parameters its own
parametrize marks list.

A group is what one parametrized test of the suite runs; its cases are the families, case-table groups, frames or parameter
sets inside it. Per group the child reports the number of cases, the number of values the suite's comparison held to the
oracle (tests/literal_pair.py: compared()), the number of cases whose comparison failed and the suite's own description of
the first failure. A failed comparison does not end the child: every group runs, so one run shows the whole picture.
Anything else - a HIP error, an exception that is no comparison - ends it at once with status 3: nothing more is started on
the GPU after trouble. The last line of the output is one JSON object.

tests/test_gpu_literal_gates.py calls run_group() itself, in its own process, for the product pair: nothing may be dropped in
literal mode, so both must have compared the same number of values."""
import importlib
import inspect
import itertools
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest  # noqa: E402

from tests import literal_pair as lp  # noqa: E402

SUITES = ("march_rays", "march_origin_reciprocal", "lights_gates", "lights_tile_masks", "composite_gates", "composite_pixel_path",
          "composite_march_queue", "composite_slots", "frame_prep_constants")
MARCH_SUITES = ("march_rays", "march_origin_reciprocal")  # the two that load the harness of tests/cpp/marchrays.hip


def module(suite):
    return importlib.import_module("tests.test_gpu_" + suite)


def parametrizations(fn):
    """The keyword sets of a test function's parametrize marks, in pytest's order of ids, each with its id."""
    axes = []
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [n.strip() for n in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
        axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in mark.args[1]])
    out = []
    for combo in itertools.product(*axes):
        kw = {}
        for part in combo:
            kw.update(part)
        out.append(kw)
    return out


def label(value):
    if isinstance(value, (tuple, list)):
        return "x".join(label(v) for v in value)
    return getattr(value, "__name__", str(value))


def call(fn, gpu, **kw):
    """A test function as pytest would call it; `gpu` stands in for the module's fixture of that name."""
    if "gpu" in inspect.signature(fn).parameters:
        kw["gpu"] = gpu
    return fn(**kw)


def whole_tests(gpu, fn, name, keep=lambda kw: True, by=()):
    """Groups of a test function whose body is the run: one group per value of the parameters `by`, one case per remaining
    parameter set."""
    groups = {}
    for kw in parametrizations(fn):
        if not keep(kw):
            continue
        group = "/".join([name] + [label(kw[k]) for k in by])
        case = "-".join(label(v) for k, v in kw.items() if k not in by) or name
        groups.setdefault(group, []).append((case, lambda kw=kw: call(fn, gpu, **kw)))
    return groups


def groups(suite, gpu=None):
    """group name -> function that returns the group's cases as (name, thunk) pairs. Building the table starts nothing; the
    case tables themselves are built when a group's function is called."""
    m = module(suite)
    out = {}
    if suite == "march_rays":
        for kw in parametrizations(m.test_earth_families):
            def cases(kw=kw):
                ctx = m.context("earth")
                return [(f.name, lambda f=f: m.check_family(ctx, f, kw["config"] == "prepped")) for f in ctx.families(kw["group"])]
            out["earth/%s/%s" % (kw["group"], kw["config"])] = cases
        for kw in parametrizations(m.test_variant_families):
            def cases(kw=kw):
                ctx = m.context(kw["name"])
                return [(f.name, lambda f=f: m.check_family(ctx, f, kw["config"] == "prepped")) for f in ctx.families("variant")]
            out["%s/%s" % (kw["name"], kw["config"])] = cases
        out["rows_interior"] = lambda: [("rows_interior", m.test_rows_interior_differs_between_two_extents)]
    elif suite == "march_origin_reciprocal":
        from tests import march_origin_rays as mo

        for kw in parametrizations(m.test_origin_reciprocal_families):
            def cases(kw=kw):
                ctx = m.context(kw["name"])
                return [(f.name, lambda f=f: m.check_family(ctx, f, kw["config"] == "prepped")) for f in mo.families(ctx.B, kw["spoiler"])]
            out["%s/%s/%s" % (kw["name"], label(kw["spoiler"]), kw["config"])] = cases
    elif suite == "lights_gates":
        # the tight images only: the padded run exercises addressing, which does not depend on the build
        for kw in parametrizations(m.test_gate_family_is_bit_identical_to_the_oracle):
            if kw["padded"]:
                continue

            def cases(kw=kw):
                L, _ = m.built()
                return [(g.name, lambda g=g: m.run_group(gpu, g, L, False)) for g in m.groups_of(kw["family"])]
            out[kw["family"]] = cases
    elif suite == "composite_gates":
        for kw in parametrizations(m.test_gate_family_is_bit_identical_to_the_oracle):
            def cases(kw=kw):
                return [(g.name, lambda g=g: m.run_group(gpu, g, kw["fast"])) for g in m.groups_of(kw["family"])]
            out["%s/%s" % (kw["family"], "fast" if kw["fast"] else "exact")] = cases
    elif suite == "lights_tile_masks":
        smallest = min(m.SIZES, key=lambda s: s[0] * s[1])
        table = whole_tests(gpu, m.test_image_is_bit_identical_to_the_oracle, "image", keep=lambda kw: kw["size"] == smallest, by=("size",))
        out.update({k: (lambda v=v: v) for k, v in table.items()})
    elif suite == "composite_pixel_path":
        table = whole_tests(gpu, m.test_composite_frame_is_bit_identical_to_the_oracle, "composite")
        table.update(whole_tests(gpu, m.test_lights_pass_on_the_material_frames_is_bit_identical_to_the_oracle, "lights", by=("spots",)))
        out.update({k: (lambda v=v: v) for k, v in table.items()})
    elif suite == "composite_march_queue":
        table = whole_tests(gpu, m.test_extents_that_are_not_multiples_of_the_workgroup, "extents")
        table.update(whole_tests(gpu, m.test_every_pixel_needs_both_marches, "both_marches"))
        table.update(whole_tests(gpu, m.test_no_pixel_needs_a_march, "no_march"))
        table.update(whole_tests(gpu, m.test_row_tiled_frame, "row_tiled"))
        out.update({k: (lambda v=v: v) for k, v in table.items()})
    elif suite == "composite_slots":
        table = whole_tests(gpu, m.test_four_kinds_of_pixel_in_every_wave, "four_kinds")
        out.update({k: (lambda v=v: v) for k, v in table.items()})
    elif suite == "frame_prep_constants":
        table = whole_tests(gpu, m.test_constants_follow_the_blocks_of_every_record_call, "prep", by=("kind",))
        out.update({k: (lambda v=v: v) for k, v in table.items()})
    else:
        raise KeyError(suite)
    return out


def group_names(suite):
    return list(groups(suite))


def gpu_context():
    """What the suites' `gpu` fixtures hold, all of it: the fixtures differ only in how much of this they carry."""
    import torch

    assert torch.cuda.is_available(), "the gate suites need a GPU; the product path has no CPU fallback"
    from oracle import binding as ob
    from syzygy_amd import abi, pipelines, scene

    class Ctx:
        pass

    c = Ctx()
    c.torch, c.pl, c.ob, c.abi, c.scene = torch, pipelines, ob, abi, scene
    return c


def run_group(suite, name, gpu):
    """One group on whichever pair this process has loaded. A comparison that fails (AssertionError, pytest.fail) is counted
    and described; any other exception passes through."""
    entry = {"cases": 0, "compared": 0, "mismatches": 0, "first": None}
    with lp.tally() as t:
        for case, thunk in groups(suite, gpu)[name]():
            entry["cases"] += 1
            try:
                thunk()
            except (AssertionError, pytest.fail.Exception) as e:
                entry["mismatches"] += 1
                if entry["first"] is None:
                    entry["first"] = "%s: %s" % (case, str(e) or repr(e))
    entry["compared"] = t.compared
    return entry


def libraries(suite):
    """The basenames of what this process loaded: C-ABI library, oracle, and the march harness where the suite drives one."""
    import syzygy_amd
    from oracle import binding as ob
    from syzygy_amd._lib import library_path

    loaded = syzygy_amd.lib()._name
    assert os.path.realpath(loaded) == os.path.realpath(library_path()), (loaded, library_path())
    out = {"library": os.path.basename(loaded), "oracle": os.path.basename(ob.lib()._name), "harness": None}
    if suite in MARCH_SUITES:
        out["harness"] = os.path.relpath(importlib.import_module("tests.test_gpu_march_rays").lib()._name, ROOT)
    return out


def main(suite):
    out = {"suite": suite, "pair": lp.pair(), "groups": {}}  # a half-set environment ends here, with its text
    try:
        gpu = gpu_context()
        out.update(libraries(suite))
        for name in groups(suite):
            out["groups"][name] = run_group(suite, name, gpu)
    except BaseException:
        out["error"] = traceback.format_exc()[-4000:]
        print(json.dumps(out))
        return 3
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
