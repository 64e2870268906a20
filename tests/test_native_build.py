"""tests/native.py: a native test program is rebuilt exactly when the hash of its sources differs from its stamp, whatever
file times say (on a toy tree), and every target the tests ask for is one tests/Makefile defines."""
import ast
import glob
import os
import re
import subprocess
import time

import pytest

from tests import native

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture
def toy(tmp_path):
    (tmp_path / "value.h").write_text("#define VALUE 1\n")
    (tmp_path / "prog.cpp").write_text('#include "value.h"\n#include <cstdio>\nint main() { std::printf("%d\\n", VALUE); }\n')
    (tmp_path / "Makefile").write_text("prog: prog.cpp value.h\n\tg++ -O0 prog.cpp -o prog\n")
    hashed = [str(tmp_path / "prog.cpp"), str(tmp_path / "value.h")]
    return tmp_path, lambda: native.build("prog", directory=str(tmp_path), hashed=hashed)


def _output(exe):
    return subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.strip()


def test_second_build_runs_no_compiler(toy):
    tree, build = toy
    exe = build()
    assert exe == str(tree / "prog") and _output(exe) == "1" and (tree / "prog.build_stamp").exists()
    before = os.stat(exe)
    assert build() == exe
    after = os.stat(exe)
    assert (after.st_mtime_ns, after.st_ino) == (before.st_mtime_ns, before.st_ino)


def test_an_edited_header_rebuilds_an_artefact_that_looks_newer(toy):
    """The travelled artefact: its file time is later than every source's, so make alone would do nothing."""
    tree, build = toy
    exe = build()
    (tree / "value.h").write_text("#define VALUE 2\n")
    tomorrow = time.time() + 86400
    os.utime(exe, (tomorrow, tomorrow))
    assert _output(build()) == "2"


def test_a_missing_artefact_is_rebuilt_under_a_matching_stamp(toy):
    tree, build = toy
    exe = build()
    os.remove(exe)
    assert (tree / "prog.build_stamp").exists()
    assert _output(build()) == "1"


def test_a_failed_build_raises_and_leaves_no_fresh_stamp(toy):
    tree, build = toy
    build()
    built_from = (tree / "prog.build_stamp").read_text()
    (tree / "value.h").write_text("#define VALUE (\n")
    with pytest.raises(subprocess.CalledProcessError):
        build()
    assert (tree / "prog.build_stamp").read_text() == built_from
    with pytest.raises(subprocess.CalledProcessError):  # and the next call tries again
        build()
    (tree / "value.h").write_text("#define VALUE 3\n")
    assert _output(build()) == "3"
    assert (tree / "prog.build_stamp").read_text() != built_from


def test_the_tests_ask_for_exactly_the_targets_of_the_makefile():
    """... and in one way: the module is imported and called as native.build with one literal target, so that the search below sees
    every call; `directory` and `hashed` are for the toy tree above; and tests/Makefile is the only Makefile there is to ask."""
    asked = set()
    for path in glob.glob(os.path.join(HERE, "**", "*.py"), recursive=True):
        text = open(path).read()
        calls = re.findall(r'native\.build\("([^"]+)"\)', text)
        nodes = list(ast.walk(ast.parse(text, path)))
        imported = [n for n in nodes if isinstance(n, ast.ImportFrom) and (n.module or "").split(".")[-1] == "native"]
        assert not imported, (path, [n.lineno for n in imported])
        if path != os.path.abspath(__file__):  # the toy's call names a directory too; every other call is a literal target
            assert len(calls) == text.count("native.build("), path
            keyworded = [n for n in nodes if isinstance(n, ast.Call) and {k.arg for k in n.keywords} & {"directory", "hashed"}]
            assert not keyworded, (path, [n.lineno for n in keyworded])
        asked |= set(calls)
    makefiles = glob.glob(os.path.join(HERE, "**", "Makefile"), recursive=True)
    assert makefiles == [os.path.join(HERE, "Makefile")], makefiles
    variables = native.assignments(os.path.join(HERE, "Makefile"))
    defined = variables["TARGETS"][1]
    while "$(" in defined:
        defined = re.sub(r"\$\((\w+)\)", lambda m: variables[m.group(1)][1], defined)
    assert asked == set(defined.split())
    for target in sorted(asked):
        assert native.commands(target), target  # make -n succeeds and has something to run
