"""Writes tests/golden/compute_collection_reflection.json: what the reference's four committed compute-collection binaries
declare (push-constant block, members, local size, the storage image), as reported by the reference's own vendored reflection
library through oracle/_ref/reflect_spv, in the order of renderer.cpp:238-243. The file is data, not reference text;
tests/test_compute_collection_reflection.py checks the library's szg_compute_collection_reflect tables against it. Run where
the reference checkout exists:

    python tests/golden/make_compute_collection_reflection.py
"""
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("SZG_REFERENCE", "/root/reference")
TOOL = os.path.join(ROOT, "oracle", "_ref", "reflect_spv")
SHADERS = ["booleanpush", "gradient_color", "sparse_push_constant", "matrix_color"]


def reflect():
    paths = [os.path.join(REFERENCE, "shaders", s + ".comp.spv") for s in SHADERS]
    if not os.path.exists(TOOL) or not all(os.path.exists(p) for p in paths):
        return None
    data = json.loads(subprocess.run([TOOL] + paths, check=True, capture_output=True, text=True).stdout)
    out = []
    for name, path in zip(SHADERS, paths):
        entry = data[os.path.basename(path)]
        blob = open(path, "rb").read()
        words = struct.unpack("<%dI" % (len(blob) // 4), blob)
        assert words[0] == 0x07230203
        i, no_contraction = 5, 0
        while i < len(words):  # OpDecorate = 71, OpMemberDecorate = 72, Decoration NoContraction = 42
            op, n = words[i] & 0xFFFF, words[i] >> 16
            if (op == 71 and words[i + 2] == 42) or (op == 72 and words[i + 3] == 42):
                no_contraction += 1
            i += n
        entry["no_contraction"] = no_contraction
        entry["name"] = name
        out.append(entry)
    return out


if __name__ == "__main__":
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    data = reflect()
    if data is None:
        sys.exit("the reference checkout or oracle/_ref/reflect_spv is missing")
    target = os.path.join(ROOT, "tests", "golden", "compute_collection_reflection.json")
    with open(target, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {target}: {len(data)} shaders")
