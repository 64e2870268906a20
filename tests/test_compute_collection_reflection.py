"""The reflection tables of the compute-collection pipeline (szg_compute_collection_reflect, include/szg/compute_collection.h)
against what the reference's own reflection library reports for the four committed binaries
(tests/golden/compute_collection_reflection.json, written by tests/golden/make_compute_collection_reflection.py), through the
C-ABI, the ctypes mirrors and the Python class; and every refusal of szg_record_compute_collection. No device is needed: the
tables are host data and the refusals come before anything is launched."""
import ctypes as C
import json
import os
import re
import warnings

import numpy as np
import pytest

from syzygy_amd import abi, lib, library_path, pipelines
from tests import compute_collection_model as model
from tests import native
from tests.texture_display_cases import image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "compute_collection_reflection.json")
# spirv-reflect type flags (SpvReflectTypeFlagBits)
FLAG_BOOL, FLAG_INT, FLAG_FLOAT, FLAG_VECTOR, FLAG_MATRIX = 0x2, 0x4, 0x8, 0x100, 0x200
SPV_IMAGE_FORMAT_RGBA16, DESCRIPTOR_TYPE_STORAGE_IMAGE = 10, 3


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_header_declares_what_the_table_binds():
    text = open(os.path.join(ROOT, "include", "szg", "compute_collection.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(szg_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(abi.COMPUTE_COLLECTION_FUNCTIONS)
    handle = C.CDLL(library_path())
    for name in names:
        assert hasattr(handle, name), f"{name} declared but not exported"
    for macro in ("SHADER_COUNT", "MAX_EXTENT", "MAX_BLOCK_BYTES", "PREFIX_BYTES", "MAX_MEMBERS", "WORKGROUP"):
        value = int(re.search(rf"#define SZG_COMPUTE_COLLECTION_{macro} (\d+)u", text).group(1))
        assert value == getattr(abi, "SZG_COMPUTE_COLLECTION_" + macro)
    assert lib().szg_abi_version() == 2  # additive: the version does not move


def test_the_golden_file_is_the_collection(golden):
    assert [g["name"] for g in golden] == list(model.SHADERS)  # renderer.cpp:238-243
    assert [g["push_constants"][0]["size"] for g in golden] == [80, 48, 80, 208]
    for g in golden:
        assert g["local_size"] == [16, 16, 1] and g["no_contraction"] == 0 and g["entry_point"] == "main"
        assert len(g["push_constants"]) == 1 and g["push_constants"][0]["padded_size"] == g["push_constants"][0]["size"]
        (binding,) = g["bindings"]
        assert (binding["set"], binding["binding"], binding["image_format"], binding["descriptor_type"]) == \
            (0, 0, SPV_IMAGE_FORMAT_RGBA16, DESCRIPTOR_TYPE_STORAGE_IMAGE)
        first, second = g["push_constants"][0]["members"][:2]
        assert (first["name"], first["offset"], first["size"], second["name"], second["offset"], second["size"]) == \
            ("drawOffset", 0, 8, "drawExtent", 8, 8)


def test_library_tables_equal_the_reflection_of_the_binaries(golden):
    assert lib().szg_compute_collection_shader_count() == len(golden) == abi.SZG_COMPUTE_COLLECTION_SHADER_COUNT
    for index, g in enumerate(golden):
        r = abi.CCReflection()
        assert lib().szg_compute_collection_reflect(index, C.byref(r)) == abi.SZG_OK
        block = g["push_constants"][0]
        assert r.name.decode() == g["name"]
        assert (r.size_bytes, r.padded_size_bytes, r.layout_offset_bytes) == (block["size"], block["padded_size"], block["offset"])
        assert list(r.local_size) == g["local_size"]
        assert r.member_count == len(block["members"]) <= abi.SZG_COMPUTE_COLLECTION_MAX_MEMBERS
        assert r.padded_size_bytes <= abi.SZG_COMPUTE_COLLECTION_MAX_BLOCK_BYTES
        for got, want in zip(r.members[: r.member_count], block["members"]):
            flags = want["type_flags"]
            assert got.name.decode() == want["name"]
            assert (got.offset_bytes, got.size_bytes, got.padded_size_bytes) == (want["offset"], want["size"], want["padded_size"])
            assert want["scalar_width"] == 32 and flags & FLAG_VECTOR
            # a bvec4 of a push-constant block is declared as 32-bit unsigned words in the binary
            assert got.component_type == (abi.SZG_CC_COMPONENT_FLOAT if flags & FLAG_FLOAT else abi.SZG_CC_COMPONENT_BOOL)
            assert bool(flags & FLAG_FLOAT) != bool(flags & (FLAG_INT | FLAG_BOOL))
            if flags & FLAG_MATRIX:
                assert (got.vector_width, got.column_count) == (want["rows"], want["columns"]) and want["matrix_stride"] == 16
            else:
                assert (got.vector_width, got.column_count) == (want["vector"], 1)
            assert got.size_bytes == 4 * got.vector_width * got.column_count


def test_python_mirror_and_model_agree_with_the_tables(golden):
    reflection = pipelines.compute_collection_reflection()
    assert [r.name for r in reflection] == [g["name"] for g in golden]
    for r, g in zip(reflection, golden):
        block = g["push_constants"][0]
        assert (r.sizeBytes, r.paddedSizeBytes, r.layoutOffsetBytes, list(r.localSize)) == \
            (block["size"], block["padded_size"], 0, g["local_size"])
        assert [(m.name, m.offsetBytes, m.sizeBytes, m.paddedSizeBytes) for m in r.members] == \
            [(m["name"], m["offset"], m["size"], m["padded_size"]) for m in block["members"]]
        # the model's own table (what the vectors were generated with)
        size, members = model.BLOCKS[r.name]
        assert size == r.paddedSizeBytes
        assert [(n, o, 4 * c) for n, o, c, _ in members] == [(m.name, m.offsetBytes, m.sizeBytes) for m in r.members[2:]]
        assert set(abi.COMPUTE_COLLECTION_EXAMPLE_VALUES[r.name]) == {m.name for m in r.members[2:]}


def test_pipeline_object_keeps_one_block_per_shader():
    p = pipelines.ComputeCollectionPipeline()
    assert p.shaderCount() == 4 and p.shaderIndex() == 0
    for i, size in enumerate((80, 48, 80, 208)):
        p.selectShader(i)
        assert p.readPushConstantBytes() == bytes(size)  # zeros at first, pipelines.cpp:255-257
    p.selectShader(1)
    p.writePushConstant("bottomColor", [1.0, 0.5, 0.25, 1.0])
    assert np.frombuffer(p.readPushConstantBytes(), np.float32)[8:12].tolist() == [1.0, 0.5, 0.25, 1.0]
    p.selectShader(0)
    p.writePushConstant("row2", [1, 0, 1, 1])
    assert np.frombuffer(p.readPushConstantBytes(), np.uint32)[8:12].tolist() == [1, 0, 1, 1]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        p.selectShader(7)  # outside the table: a warning and no change
    assert p.shaderIndex() == 0 and len(caught) == 1
    p.selectShader(1)  # the block survived the switches
    assert np.frombuffer(p.readPushConstantBytes(), np.float32)[8:12].tolist() == [1.0, 0.5, 0.25, 1.0]
    p.mapPushConstantBytes()[16:20] = np.float32(0.75).tobytes()
    assert np.frombuffer(p.readPushConstantBytes(), np.float32)[4] == 0.75
    with pytest.raises(KeyError):
        p.writePushConstant("row1", [0, 0, 0, 0])
    with pytest.raises(ValueError):
        p.writePushConstant("topColor", [0, 0])
    fresh = pipelines.ComputeCollectionPipeline()
    for i in range(4):
        fresh.selectShader(i)
        fresh.writeExampleValues()
        name = fresh.currentShader().name
        assert fresh.readPushConstantBytes() == model.pack_block(name, abi.COMPUTE_COLLECTION_EXAMPLE_VALUES[name])
    assert pipelines.parse_pipeline_option("deferred") == ("deferred", None)
    assert pipelines.parse_pipeline_option("compute-collection") == ("compute-collection", "gradient_color")
    assert pipelines.parse_pipeline_option("compute-collection:matrix_color") == ("compute-collection", "matrix_color")
    with pytest.raises(ValueError):
        pipelines.parse_pipeline_option("compute-collection:nothing")


def test_cpp_accessors_agree_with_the_reflection_of_the_binaries(golden, tmp_path):
    """szg::ComputeCollectionPipeline (include/szg/pipelines.hpp) from a host-only C++ caller: shaders(), currentShader(), the
    blocks and the selection, against the golden reflection. The constructor touches no device."""
    import subprocess

    lib()  # built and loadable
    r = subprocess.run([native.build("cpp/compute_collection_reflection")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout)
    assert (got["valid"], got["count"], got["index"]) == (1, len(golden), 0)
    assert (got["wrote"], got["index_after_7"], got["kept"]) == (1, 3, 1) and "selectShader(7)" in r.stderr
    for have, g in zip(got["shaders"], golden):
        block = g["push_constants"][0]
        assert (have["name"], have["size"], have["padded_size"], have["layout_offset"], have["local_size"]) == \
            (g["name"], block["size"], block["padded_size"], block["offset"], g["local_size"])
        assert (have["block_bytes"], have["zeros"], have["current_is_selected"]) == (block["padded_size"], 1, 1)
        assert [(m["name"], m["offset"], m["size"], m["padded_size"]) for m in have["members"]] == \
            [(m["name"], m["offset"], m["size"], m["padded_size"]) for m in block["members"]]
        for m, want in zip(have["members"], block["members"]):
            floating = bool(want["type_flags"] & FLAG_FLOAT)
            assert m["component_type"] == (abi.SZG_CC_COMPONENT_FLOAT if floating else abi.SZG_CC_COMPONENT_BOOL)
            if want["type_flags"] & FLAG_MATRIX:
                assert (m["vector_width"], m["column_count"]) == (want["rows"], want["columns"])
            else:
                assert (m["vector_width"], m["column_count"]) == (want["vector"], 1)


def record_refusals(data=0x1000):
    """(name, arguments of szg_record_compute_collection after the stream, text the message must hold or None) of every
    refusal, for a 64x32 RGBA16_UNORM image at address `data`, which is never dereferenced: every call is refused on the host,
    before anything is launched."""
    U16 = abi.SZG_FORMAT_RGBA16_UNORM
    blocks = [bytes(n) for n in (80, 48, 80, 208)]
    ok = image(64, 32, U16, data)
    cases = [
        ("NULL bytes", (1, None, 48, ok, 40, 24), None),
        ("NULL image", (1, blocks[1], 48, None, 40, 24), None),
        ("NULL data", (1, blocks[1], 48, image(64, 32, U16, None), 40, 24), None),
        ("index 4", (4, blocks[3], 208, ok, 40, 24), b"the collection has 4 programs"),
        ("index 0xFFFFFFFF", (0xFFFFFFFF, blocks[3], 208, ok, 40, 24), None),
    ]
    for index, size in enumerate((80, 48, 80, 208)):  # a byte count other than the padded block size
        for wrong in (0, 16, size - 4, size + 4, 256):
            cases.append((f"program {index} with {wrong} bytes", (index, bytes(256), wrong, ok, 40, 24), None))
    for fmt in (abi.SZG_FORMAT_RGBA16_SFLOAT, abi.SZG_FORMAT_RGBA32_SFLOAT, abi.SZG_FORMAT_RGBA8_UNORM, abi.SZG_FORMAT_UNDEFINED):
        cases.append((f"format {fmt}", (1, blocks[1], 48, image(64, 32, fmt, data, pitch=64 * 8), 40, 24), b"RGBA16_UNORM"))
    cases += [
        ("pitch below the row", (1, blocks[1], 48, image(64, 32, U16, data, pitch=64 * 8 - 8), 40, 24), None),
        ("pitch not a texel multiple", (1, blocks[1], 48, image(64, 32, U16, data, pitch=64 * 8 + 4), 40, 24), None),
        ("data misaligned", (1, blocks[1], 48, image(64, 32, U16, data + 4), 40, 24), None),
    ]
    for w, h in ((0, 24), (40, 0), (0, 0), (65, 24), (40, 33), (0xFFFFFFFF, 24)):  # empty, or leaves the image
        cases.append((f"extent {w}x{h}", (1, blocks[1], 48, ok, w, h), None))
    big = abi.SZG_COMPUTE_COLLECTION_MAX_EXTENT + 1
    cases.append(("wider than the cap", (1, blocks[1], 48, image(big, 8, U16, data), 40, 8), b"exceeds"))
    cases.append(("higher than the cap", (1, blocks[1], 48, image(8, big, U16, data), 8, 8), b"exceeds"))
    return cases


def record_refusal(case):
    """Make the call of one of record_refusals(): (status, last-error text)."""
    index, block, count, im, w, h = case[1]
    status = lib().szg_record_compute_collection(None, index, block, count, C.byref(im) if im is not None else None, w, h)
    return status, lib().szg_last_error()


def test_every_refusal_returns_invalid_argument_without_a_device():
    L = lib()
    bad = abi.SZG_ERR_INVALID_ARGUMENT
    for case in record_refusals():
        status, text = record_refusal(case)
        assert status == bad and b"szg_record_compute_collection" in text, (case[0], status, text)
        assert case[2] is None or case[2] in text, (case[0], text)
    # the reflection entry point
    r = abi.CCReflection()
    assert L.szg_compute_collection_reflect(4, C.byref(r)) == bad and L.szg_compute_collection_reflect(0, None) == bad
