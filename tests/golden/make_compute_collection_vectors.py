"""Writes tests/golden/compute_collection_vectors.npz: what the reference's four committed compute-collection binaries
(shaders/booleanpush, gradient_color, sparse_push_constant, matrix_color .comp.spv) store, invocation by invocation, executed
literally by tests/golden/spirv_interp.py. The file is data: blocks, invocation ids, the fp32 value handed to imageStore and the
UNORM16 code; no SPIR-V bytes. tests/test_compute_collection_model.py checks tests/compute_collection_model.py against it.
Run where the reference checkout exists:

    python tests/golden/make_compute_collection_vectors.py

The host side follows ComputeCollectionPipeline::recordDrawCommands (pipelines.cpp:319-344): the first 16 bytes of the block
are overwritten with offset (0, 0) and the draw extent before the push. matrix_color indexes its matrices with the cell
coordinate, which leaves 0..3 beyond the draw extent (undefined in Vulkan): its vectors hold the invocations inside the
extent only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from syzygy_amd import abi  # noqa: E402
from tests import compute_collection_model as model  # noqa: E402
from tests.golden import spirv_interp as si  # noqa: E402
from tests.golden.make_spirv_vectors import Builtins, _images  # noqa: E402

REFERENCE = os.environ.get("SZG_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "compute_collection_vectors.npz")
KINDS = ("ordinary", "special", "example")
# (name, width, height, image width, image height, every invocation of the dispatch?)
CASES = (("full", 40, 24, 64, 32, True), ("subregion", 1000, 700, 1024, 768, False), ("uhd", 3840, 2160, 3840, 2160, False))
# booleanpush needs three opcodes spirv_interp.py does not execute: they are rewritten into OpExtInst with private numbers
PRIVATE = {170: 0x7000AA, 171: 0x7000AB, 139: 0x70008B}  # OpIEqual, OpINotEqual, OpSMod


class Module(si.Module):
    def __init__(self, path):
        super().__init__(path)
        for fn in self.functions.values():
            for block in fn.blocks.values():
                for k, (op, a) in enumerate(block):
                    if op in PRIVATE:
                        block[k] = (12, (a[0], a[1], 0, PRIVATE[op]) + tuple(a[2:]))


class Interpreter(si.Interpreter):
    def _ext(self, inst, x):
        sg = self._signed_scalar
        if inst == PRIVATE[170]:
            return self._map(lambda p, q: bool(p == q), x[0], x[1])
        if inst == PRIVATE[171]:
            return self._map(lambda p, q: bool(p != q), x[0], x[1])
        if inst == PRIVATE[139]:  # the sign of the result follows operand 2, as Python's %
            return self._map(lambda p, q: (sg(p) % sg(q)) & 0xFFFFFFFF, x[0], x[1])
        return super()._ext(inst, x)


def blocks(shader):
    """The three blocks of a shader, as the CALLER hands them over (prefix bytes included: they must not matter)."""
    size, members = model.BLOCKS[shader]
    rng = np.random.default_rng(abs(hash_name(shader)))
    ordinary = {n: (rng.integers(0, 2, c) if d == np.uint32 else rng.random(c, np.float32)) for n, _, c, d in members}
    floats = np.array([-0.5, 1.5, 1e-40, np.inf, 0.25, -np.inf, np.nan, -0.0, 0.75, 3.0, -1e-42, 1.0, 0.5, np.nan, 2.0 ** -127, 0.125],
                      np.float32)
    words = np.array([0, 1, 5, 0x80000000], np.uint32)
    special = {n: (np.roll(words, k)[:c] if d == np.uint32 else np.roll(floats, -3 * k)[:c]) for k, (n, _, c, d) in enumerate(members)}
    return {"ordinary": model.pack_block(shader, ordinary), "special": model.pack_block(shader, special, fill=0xAB),
            "example": model.pack_block(shader, abi.COMPUTE_COLLECTION_EXAMPLE_VALUES[shader])}


def hash_name(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name))


def axis_samples(n, image_n):
    """Corners, both sides of every quarter boundary, the last texel of the extent, the first and last spill texel."""
    picks = {0, 1, n - 1, n, model.ceil16(n) - 1}
    for q in (1, 2, 3):
        k = q * n // 4
        picks |= {k - 1, k, k + 1}
    return sorted(p for p in picks if 0 <= p < min(model.ceil16(n), image_n))


def invocations(shader, case):
    _, w, h, iw, ih, every = case
    cols, rows = model.written_extent(w, h, iw, ih)
    if shader == "matrix_color":
        cols, rows = w, h  # inside the extent only
    if every:
        return [(x, y) for y in range(rows) for x in range(cols)]
    xs = [x for x in axis_samples(w, iw) if x < cols]
    ys = [y for y in axis_samples(h, ih) if y < rows]
    ids = [(x, y) for y in ys for x in xs]
    if shader != "matrix_color":
        ids += [(iw, 0), (0, ih), (iw, ih - 1)]  # outside the image: must store nothing
    return ids


def generate(log=print):
    _, Unorm16, _, _, _ = _images()
    out = {"shaders": np.array(model.SHADERS), "kinds": np.array(KINDS), "cases": np.array([c[0] for c in CASES]),
           "case_extents": np.array([c[1:5] for c in CASES], np.int32)}
    for shader in model.SHADERS:
        module = Module(os.path.join(REFERENCE, "shaders", shader + ".comp.spv"))
        assert module.local_size == (16, 16, 1) and module.no_contraction == 0
        for kind, block in blocks(shader).items():
            out[f"{shader}.{kind}.block"] = np.frombuffer(block, np.uint8)
            for case in CASES:
                name, w, h, iw, ih, _ = case
                image = Unorm16(np.zeros((ih, iw, 4), np.uint16))
                run = Interpreter(module, si.Memory(), Builtins(), model.recorded_block(shader, block, w, h), {(0, 0): image})
                ids = invocations(shader, case)
                stored = np.zeros(len(ids), np.uint8)
                bits = np.zeros((len(ids), 4), np.uint32)
                codes = np.zeros((len(ids), 4), np.uint16)
                for k, (x, y) in enumerate(ids):
                    image.written.clear()
                    image.written_f.clear()
                    run.run(global_id=(x, y, 0))
                    assert set(image.written) <= {(x, y)}, "an invocation stores to its own texel only"
                    if (x, y) in image.written:
                        stored[k] = 1
                        bits[k] = np.array(image.written_f[(x, y)], np.float32).view(np.uint32)
                        codes[k] = image.written[(x, y)]
                key = f"{shader}.{kind}.{name}"
                out[key + ".xy"] = np.array(ids, np.int32)
                out[key + ".stored"] = stored
                out[key + ".f32"] = bits
                out[key + ".code"] = codes
                log(f"{key}: {len(ids)} invocations, {int(stored.sum())} stores")
    np.savez_compressed(OUT, **out)
    log(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    generate()
