"""The one way the tests build their native programs (tests/Makefile): build("cpp/record_draw") returns the artefact's path,
compiled from the sources on disk."""
import fcntl
import glob
import hashlib
import os
import re
import subprocess

from __graft_entry__ import source_hash

TESTS = os.path.dirname(os.path.abspath(__file__))
# the slowest target, cpp/fuzz_assets (g++ with two sanitizers over the asset loaders), builds in 13 s; the slowest hipcc one,
# cpp/record_draw_compute_collection, in 8 s. Ten times the former. Building starts nothing on the GPU: the limit only bounds
# a stuck compiler.
MAKE_TIMEOUT = 130


def sources(directory=TESTS):
    """Every source file of the native test programs: the C++ and HIP files of every directory directly under tests/."""
    return sorted(f for ext in ("*.cpp", "*.hip", "*.hpp", "*.h") for f in glob.glob(os.path.join(directory, "*", ext)))


def wanted_stamp(directory, hashed):
    h = hashlib.sha256(source_hash("hip").encode())  # include/szg and syzygy_amd/csrc, the product's Makefile included
    for f in list(hashed) + [os.path.join(directory, "Makefile")]:
        h.update(os.path.relpath(f, directory).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build(target, directory=TESTS, hashed=None):
    """The absolute path of `target` of `directory`/Makefile, up to date with the product's sources, the files `hashed`
    (default: every test program's sources) and the Makefile. As __graft_entry__._make: the artefacts travel to the GPU box
    untracked, where file times say nothing, so a target is fresh only if it exists and the stamp written after its last build
    equals the hash of the current sources; then nothing runs. Otherwise `make -B <target>`, whatever file times say. The
    hash is deliberately the same for every target: any change of the product or of a test program rebuilds each target the
    next time it is asked for. The mirror programs link against libszg_hip.so, which has to be built first. The tests call
    build("<dir>/<target>") and nothing else; `directory` and `hashed` are for the toy tree of tests/test_native_build.py."""
    artefact = os.path.join(directory, target)
    stamp = artefact + ".build_stamp"
    want = wanted_stamp(directory, sources(directory) if hashed is None else hashed)

    def fresh():
        return os.path.exists(artefact) and os.path.exists(stamp) and open(stamp).read().strip() == want

    if fresh():
        return artefact
    # several processes may arrive here together (pytest-xdist workers, a test and a tool): one builds, the others wait for
    # the lock and then find the stamp fresh
    with open(os.path.join(directory, ".build_lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not fresh():
            subprocess.run(["make", "-s", "-B", "-C", directory, target], check=True, timeout=MAKE_TIMEOUT)
            with open(stamp, "w") as f:
                f.write(want + "\n")
    return artefact


def assignments(path):
    """name -> (operator, value) of the variable assignments of a Makefile (no continuation lines in these files)."""
    out = {}
    for line in open(path):
        m = re.match(r"^([A-Za-z_][A-Za-z0-9_]*)\s*(\?=|:=|=)\s*(.*?)\s*$", line)
        if m:
            out[m.group(1)] = (m.group(2), m.group(3))
    return out


def commands(target, directory=TESTS):
    """The command lines `make` would run for `target` (make -n -B: nothing is built)."""
    return subprocess.run(["make", "-n", "-B", "-C", directory, "--no-print-directory", target], check=True, capture_output=True,
                          text=True, timeout=MAKE_TIMEOUT).stdout.splitlines()


def resource_remarks(target, fields):
    """kernel name -> {field: figure} of what the compiler reports for the kernels of `make <target>` in syzygy_amd/csrc
    (-Rpass-analysis=kernel-resource-usage; the library's flags and per-unit scheduler options). `fields` maps a field to the
    pattern of its figure; only the remark lines are read."""
    csrc = os.path.join(os.path.dirname(TESTS), "syzygy_amd", "csrc")
    done = subprocess.run(["make", "-C", csrc, target], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                          timeout=MAKE_TIMEOUT)
    assert done.returncode == 0, done.stdout[-4000:]
    kernels, current = {}, None
    for line in done.stdout.splitlines():
        if "remark:" not in line:
            continue
        name = re.search(r"Function Name: (\S+)", line)
        if name:
            current = kernels.setdefault(name.group(1), {})
            continue
        for field, pattern in fields.items():
            m = re.search(pattern, line)
            if m and current is not None:
                current[field] = int(m.group(1))
    return kernels
