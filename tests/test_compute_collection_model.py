"""tests/compute_collection_model.py (the numpy statement of include/szg/compute_collection.h) against the reference's four
committed compute-collection binaries, through tests/golden/compute_collection_vectors.npz (written by
tests/golden/make_compute_collection_vectors.py with the SPIR-V interpreter), and the properties the header states. CPU only.

Pinned: booleanpush, gradient_color and sparse_push_constant for every recorded invocation, the spill beyond the draw extent
included; matrix_color inside the draw extent (beyond it the shader indexes outside its matrices, undefined in Vulkan; the
clamp to 3 is this library's convention and is tested as such)."""
import os

import numpy as np
import pytest

from tests import compute_collection_model as model

HERE = os.path.dirname(os.path.abspath(__file__))
VECTORS = os.path.join(HERE, "golden", "compute_collection_vectors.npz")
KINDS = ("ordinary", "special", "example")
CASES = ("full", "subregion", "uhd")


@pytest.fixture(scope="module")
def vectors():
    return np.load(VECTORS)


def test_the_fixture_holds_what_the_issue_lists(vectors):
    assert tuple(vectors["shaders"]) == model.SHADERS and tuple(vectors["kinds"]) == KINDS and tuple(vectors["cases"]) == CASES
    assert vectors["case_extents"].tolist() == [[40, 24, 64, 32], [1000, 700, 1024, 768], [3840, 2160, 3840, 2160]]
    for shader in model.SHADERS:
        # every invocation of the 48 x 32 dispatch of 40 x 24 in 64 x 32 (matrix_color: the 40 x 24 inside the extent)
        want = 40 * 24 if shader == "matrix_color" else 48 * 32
        for kind in KINDS:
            assert len(vectors[f"{shader}.{kind}.full.xy"]) == want
            assert len(vectors[f"{shader}.{kind}.block"]) == model.block_size(shader)
        special = vectors[f"{shader}.special.block"][model.PREFIX_BYTES:]
        if shader == "booleanpush":
            assert {0, 1, 5, 0x80000000} <= set(special.view(np.uint32).tolist())
        else:
            f = special.view(np.float32)
            tiny = np.abs(f[np.isfinite(f) & (f != 0)]).min()
            assert np.isnan(f).any() and np.isinf(f).any() and (f < 0).any() and (f[np.isfinite(f)] > 1).any() and tiny < 2.0 ** -126


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shader", model.SHADERS)
def test_model_equals_the_spirv_bit_for_bit(vectors, shader, kind, case):
    w, h, iw, ih = vectors["case_extents"][CASES.index(case)].tolist()
    block = vectors[f"{shader}.{kind}.block"].tobytes()
    key = f"{shader}.{kind}.{case}"
    xy, stored = vectors[key + ".xy"], vectors[key + ".stored"].astype(bool)
    cols, rows = model.written_extent(w, h, iw, ih)
    inside_image = (xy[:, 0] < iw) & (xy[:, 1] < ih)
    # the store is guarded by the image size: exactly the invocations inside the image store
    assert (stored == inside_image).all()
    assert ((xy[stored, 0] < cols) & (xy[stored, 1] < rows)).all()  # and the dispatch is ceil16(extent)
    if shader != "matrix_color" and case != "full":
        assert (~stored).sum() == 3
    for (x, y), bits, code in zip(xy[stored], vectors[key + ".f32"][stored], vectors[key + ".code"][stored]):
        got = model.values(shader, block, w, h, [x], [y])[0, 0]
        want = bits.view(np.float32)
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all(), (x, y, got, want)
        assert (got.view(np.uint32)[~nan] == bits[~nan]).all(), (x, y, got, want)
        assert (model.unorm16(got) == code).all(), (x, y, got, code)


@pytest.mark.parametrize("shader", ["booleanpush", "gradient_color", "sparse_push_constant"])
def test_the_written_set_is_the_rounded_extent_cut_by_the_image(vectors, shader):
    """In the `full` case every invocation of the dispatch was run: the stores are exactly ceil16(extent) within the image, and
    render() writes those texels and no others."""
    xy = vectors[f"{shader}.ordinary.full.xy"]
    stored = vectors[f"{shader}.ordinary.full.stored"].astype(bool)
    assert stored.all() and {tuple(p) for p in xy.tolist()} == {(x, y) for y in range(32) for x in range(48)}
    block = vectors[f"{shader}.ordinary.block"].tobytes()
    image = np.full((32, 64, 4), 0x5A5A, np.uint16)
    out, texels = model.render(shader, block, image, 40, 24)
    assert texels.shape == (32, 48, 4)
    assert (out[:, 48:] == 0x5A5A).all()
    codes = vectors[f"{shader}.ordinary.full.code"]
    assert (out[xy[:, 1], xy[:, 0]] == codes).all()


@pytest.mark.parametrize("extent,image", [((1000, 700), (4096, 4096)), ((1001, 701), (1001, 701)), ((17, 5), (32, 16)),
                                          ((1, 1), (1, 1)), ((1, 1), (16, 16)), ((3840, 2160), (3840, 2160))])
def test_written_extent(extent, image):
    cols, rows = model.written_extent(*extent, *image)
    assert cols == min(-(-extent[0] // 16) * 16, image[0]) and rows == min(-(-extent[1] // 16) * 16, image[1])
    assert extent[0] <= cols < extent[0] + 16 and extent[1] <= rows < extent[1] + 16


@pytest.mark.parametrize("shader", ["gradient_color", "sparse_push_constant", "matrix_color"])
def test_the_zero_block_renders_black(shader):
    """Transparent black for the gradient programs; matrix_color's alpha is the constant 1, so its black is opaque."""
    image = np.full((48, 80, 4), 0xFFFF, np.uint16)
    out, _ = model.render(shader, bytes(model.block_size(shader)), image, 70, 40)
    assert (out[:48, :80] == (0, 0, 0, 0 if shader != "matrix_color" else 0xFFFF)).all()


def test_gradient_equals_sparse_for_equal_colours():
    top, bottom = [0.1, 0.9, 0.3, 1.0], [0.8, 0.2, 1.7, -0.5]
    a = model.pack_block("gradient_color", {"topColor": top, "bottomColor": bottom})
    b = model.pack_block("sparse_push_constant", {"topRG": top[:2], "topBA": top[2:], "bottomRG": bottom[:2], "bottomBA": bottom[2:]},
                         fill=0xEE)  # the padding is never read
    image = np.zeros((64, 64, 4), np.uint16)
    out_a, tex_a = model.render("gradient_color", a, image, 50, 50)
    out_b, tex_b = model.render("sparse_push_constant", b, image, 50, 50)
    assert (out_a == out_b).all() and (tex_a.view(np.uint32) == tex_b.view(np.uint32)).all()


def test_matrix_spill_follows_the_clamp_convention():
    rng = np.random.default_rng(7)
    block = model.pack_block("matrix_color", {n: rng.random(16, np.float32) for n in ("red", "green", "blue")})
    image = np.zeros((32, 64, 4), np.uint16)
    out, _ = model.render("matrix_color", block, image, 40, 24)
    f = np.frombuffer(block, np.float32)
    # beyond the extent both cell indices stay at 3: the last column / row of cells continues
    for y in range(32):
        for x in range(48):
            u = (np.float32(x) + np.float32(0.5)) / np.float32(40)
            v = (np.float32(y) + np.float32(0.5)) / np.float32(24)
            cx, cy = min(int(u * np.float32(4)), 3), min(int(v * np.float32(4)), 3)
            want = model.unorm16(np.array([f[4 + 4 * cy + cx], f[20 + 4 * cy + cx], f[36 + 4 * cy + cx], 1.0], np.float32))
            assert (out[y, x] == want).all(), (x, y)
    assert (out[23, 40:48] == out[23, 39]).all() and (out[24:32, 10] == out[23, 10]).all()


def test_boolean_spill_rows_are_red_and_columns_wrap():
    block = model.pack_block("booleanpush", {"row1": [1, 0, 0, 0], "row2": [0, 0, 0, 0], "row3": [0, 0, 0, 0], "row4": [5, 5, 5, 5]})
    image = np.zeros((16, 16, 4), np.uint16)
    out, texels = model.render("booleanpush", block, image, 1, 1)
    # extent 1 x 1 in 16 x 16: u = x + 0.5, so cx = 4x + 2 and cx % 4 = 2 everywhere; cy = 4y + 2 is outside 0..3 from row 1 on
    assert (texels[0, :, 0] == 0).all() and (texels[0, :, 3] == 1).all()
    assert (texels[1:, :, 0] == (np.arange(16, dtype=np.float32) + np.float32(0.5))[None, :]).all()
    # red * u: 0.5 in column 0 (32767.5 rounds to the even code 32768), clamped to 1 from column 1 on
    assert (out[1:, 0, 0] == 32768).all() and (out[1:, 1:, 0] == 0xFFFF).all()
    assert (out[1:, :, 1:3] == 0).all() and (out[..., 3] == 0xFFFF).all()


def test_in_extent_cells_are_0_to_3_for_every_extent_up_to_the_cap():
    """The header's claim behind SZG_COMPUTE_COLLECTION_MAX_EXTENT: (k + 0.5) / n < 1 and u * 4 < 4 in binary32 for every texel
    inside an extent n <= 16384. The largest k decides (the quotient grows with k)."""
    n = np.arange(1, model.MAX_EXTENT + 1, dtype=np.float32)
    u = ((n - np.float32(1)) + np.float32(0.5)) / n
    assert (u < np.float32(1)).all() and (u * np.float32(4) < np.float32(4)).all()
    assert ((u * np.float32(4)).astype(np.int32) <= 3).all()
    # and exhaustively for every k of a few extents, the cap included
    for extent in (1, 2, 3, 5, 17, 1000, 4095, 16383, 16384):
        k = np.arange(extent, dtype=np.float32)
        c = (((k + np.float32(0.5)) / np.float32(extent)) * np.float32(4)).astype(np.int32)
        assert c.min() >= 0 and c.max() <= 3 and (np.diff(c) >= 0).all()
        assert extent < 4 or (c.min() == 0 and c.max() == 3)


def test_the_prefix_of_the_callers_block_is_ignored():
    rng = np.random.default_rng(3)
    body = rng.random(8, np.float32).tobytes()
    image = np.zeros((32, 32, 4), np.uint16)
    a, _ = model.render("gradient_color", bytes(16) + body, image, 20, 20)
    b, _ = model.render("gradient_color", b"\xff" * 16 + body, image, 20, 20)
    assert (a == b).all()
