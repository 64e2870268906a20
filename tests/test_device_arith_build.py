"""The test libraries around the product's device code - tests/cpp/libszg_devarith.so (tests/test_gpu_device_arith.py),
tests/cpp/libszg_marchrays.so (tests/test_gpu_march_rays.py), tests/mipsample/libszg_mipsample.so (tests/test_gpu_mipmaps.py),
tests/anisosample/libszg_anisosample.so (tests/test_gpu_anisotropy.py): they cross-compile for gfx950 without a GPU, and they are compiled with the product's HIPFLAGS (a sweep of code built with
other flags says nothing about the kernels). tests/cpp/libszg_marchrays_literal.so is the march harness once more with
-DSZG_LITERAL, for the literal pair (tests/literal_pair.py): the plain rule's command line plus that one define."""
import os
import re

from tests import native

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBRARIES = ("cpp/libszg_devarith.so", "cpp/libszg_marchrays.so", "mipsample/libszg_mipsample.so", "anisosample/libszg_anisosample.so")
LITERAL_LIBRARIES = {"cpp/libszg_marchrays_literal.so": "cpp/libszg_marchrays.so"}  # literal target -> the plain one of the same source


def test_devarith_flags_are_the_product_hipflags():
    product = native.assignments(os.path.join(ROOT, "syzygy_amd", "csrc", "Makefile"))
    tests = native.assignments(os.path.join(HERE, "Makefile"))
    op, hipflags = product["HIPFLAGS"]
    assert op == "?="
    want = hipflags.replace("$(ARCH)", product["ARCH"][1]).split()
    assert "--offload-arch=gfx950" in want and "-ffp-contract=off" in want
    assert tests["DEVICE_FLAGS"][1].split() == want
    assert tests["DEVICE_LIBS"][1].split() == list(LIBRARIES) + list(LITERAL_LIBRARIES)
    rule = open(os.path.join(HERE, "Makefile")).read()
    # the four are built by the one pattern rule, which adds no flag of its own
    assert not re.search(r"^[^#\n]*libszg_(devarith|marchrays|mipsample|anisosample)\.so.*:", rule, re.M)
    recipe = re.search(r"^libszg_%\.so:.*\n\t(.*)$", rule, re.M).group(1)
    assert "$(DEVICE_FLAGS)" in recipe and not re.search(r"\s-(O\d|f|m|std|-offload)", recipe.replace("$(DEVICE_FLAGS)", ""))
    for target in LIBRARIES:  # and what make then runs: the compiler, the product's flags, and no such flag after them
        (command,) = native.commands(target)
        words = command.split()
        assert words[1:1 + len(want)] == want and not [w for w in words[1 + len(want):] if re.match(r"-(O\d|f|m|std|-offload)", w)]


def test_literal_rule_is_the_plain_rule_plus_one_define():
    """The literal harness differs from the plain one by -DSZG_LITERAL, placed right behind the product's flags, and by the
    name of its output: same compiler, same flags, same source, same include paths."""
    for literal, plain in LITERAL_LIBRARIES.items():
        (plain_command,) = native.commands(plain)
        (literal_command,) = native.commands(literal)
        words = literal_command.split()
        assert words.count("-DSZG_LITERAL") == 1 and "-DSZG_LITERAL" not in plain_command.split()
        words.remove("-DSZG_LITERAL")
        assert words[-2:] == ["-o", literal] and plain_command.split()[-2:] == ["-o", plain]
        assert words[:-1] == plain_command.split()[:-1]


def test_devarith_library_builds_for_gfx950():
    data = open(native.build("cpp/libszg_devarith.so"), "rb").read()
    assert b"gfx950" in data
    for name in (b"szg_da_sweep", b"szg_da_eval", b"szg_da_unpack_half4", b"szg_da_pack_half4_mul", b"szg_da_pack_half_range"):
        assert name in data, name


def test_marchrays_library_builds_for_gfx950():
    """tests/cpp/libszg_marchrays.so (tests/test_gpu_march_rays.py): the product's kernels_lut.hip compiles inside the harness's
    translation unit, and the march kernels of both configurations are in the code object."""
    data = open(native.build("cpp/libszg_marchrays.so"), "rb").read()
    assert b"gfx950" in data
    for name in (b"szg_mr_run", b"k_march_rays", b"k_march_flags", b"k_frame_prep", b"k_lut_range"):
        assert name in data, name


def test_marchrays_literal_library_builds_for_gfx950():
    data = open(native.build("cpp/libszg_marchrays_literal.so"), "rb").read()
    assert b"gfx950" in data
    for name in (b"szg_mr_run", b"k_march_rays", b"k_march_flags", b"k_frame_prep", b"k_lut_range"):
        assert name in data, name


def test_mipsample_library_builds_for_gfx950():
    """tests/mipsample/libszg_mipsample.so (tests/test_gpu_mipmaps.py): the product's szg_texture.hpp inside a test-only kernel."""
    data = open(native.build("mipsample/libszg_mipsample.so"), "rb").read()
    assert b"gfx950" in data and b"szg_mipsample" in data
