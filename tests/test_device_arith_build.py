"""tests/cpp/libszg_devarith.so, the library behind tests/test_gpu_device_arith.py: it cross-compiles for gfx950 without a GPU,
and it is compiled with the product's HIPFLAGS (a sweep of code built with other flags says nothing about the kernels)."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _assignments(path):
    """name -> (operator, value) of the variable assignments of a Makefile (no continuation lines in these files)."""
    out = {}
    for line in open(path):
        m = re.match(r"^([A-Za-z_][A-Za-z0-9_]*)\s*(\?=|:=|=)\s*(.*?)\s*$", line)
        if m:
            out[m.group(1)] = (m.group(2), m.group(3))
    return out


def test_devarith_flags_are_the_product_hipflags():
    product = _assignments(os.path.join(ROOT, "syzygy_amd", "csrc", "Makefile"))
    tests = _assignments(os.path.join(HERE, "cpp", "Makefile"))
    op, hipflags = product["HIPFLAGS"]
    assert op == "?="
    want = hipflags.replace("$(ARCH)", product["ARCH"][1]).split()
    assert "--offload-arch=gfx950" in want and "-ffp-contract=off" in want
    assert tests["DEVARITH_FLAGS"][1].split() == want
    rule = open(os.path.join(HERE, "cpp", "Makefile")).read()
    for target in ("libszg_devarith", "libszg_marchrays"):
        recipe = re.search(r"^%s\.so:.*\n\t(.*)$" % target, rule, re.M).group(1)
        assert "$(DEVARITH_FLAGS)" in recipe and not re.search(r"\s-(O\d|f|m|std|-offload)", recipe.replace("$(DEVARITH_FLAGS)", ""))


def test_devarith_library_builds_for_gfx950():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "cpp"), "libszg_devarith.so"], check=True)
    path = os.path.join(HERE, "cpp", "libszg_devarith.so")
    data = open(path, "rb").read()
    assert b"gfx950" in data
    for name in (b"szg_da_sweep", b"szg_da_eval", b"szg_da_unpack_half4", b"szg_da_pack_half4_mul", b"szg_da_pack_half_range"):
        assert name in data, name


def test_marchrays_library_builds_for_gfx950():
    """tests/cpp/libszg_marchrays.so (tests/test_gpu_march_rays.py): the product's kernels_lut.hip compiles inside the harness's
    translation unit, and the march kernels of both configurations are in the code object."""
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "cpp"), "libszg_marchrays.so"], check=True)
    data = open(os.path.join(HERE, "cpp", "libszg_marchrays.so"), "rb").read()
    assert b"gfx950" in data
    for name in (b"szg_mr_run", b"k_march_rays", b"k_march_flags", b"k_frame_prep", b"k_lut_range"):
        assert name in data, name
