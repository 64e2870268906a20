"""CPU model of the compute-collection pipeline: include/szg/compute_collection.h followed literally in numpy binary32.
Every operation below is one float32 operation (numpy rounds each to nearest even; nothing is fused). The kernels
(syzygy_amd/csrc/kernels_compute_collection.hip) must equal render() bit for bit; tests/golden/compute_collection_vectors.npz
pins render() to the reference's committed SPIR-V."""
import numpy as np

F32 = np.float32
SHADERS = ("booleanpush", "gradient_color", "sparse_push_constant", "matrix_color")  # renderer.cpp:238-243
PREFIX_BYTES = 16
WORKGROUP = 16
MAX_EXTENT = 16384
# header, BLOCKS: block size and (member, byte offset, component count, dtype)
BLOCKS = {
    "booleanpush": (80, [("row1", 16, 4, np.uint32), ("row2", 32, 4, np.uint32), ("row3", 48, 4, np.uint32),
                         ("row4", 64, 4, np.uint32)]),
    "gradient_color": (48, [("topColor", 16, 4, np.float32), ("bottomColor", 32, 4, np.float32)]),
    "sparse_push_constant": (80, [("topRG", 16, 2, np.float32), ("topBA", 32, 2, np.float32), ("bottomRG", 48, 2, np.float32),
                                  ("bottomBA", 64, 2, np.float32)]),
    "matrix_color": (208, [("red", 16, 16, np.float32), ("green", 80, 16, np.float32), ("blue", 144, 16, np.float32)]),
}


def block_size(shader):
    return BLOCKS[shader][0]


def pack_block(shader, values, fill=0):
    """A block of `shader` with the members of `values` (name -> components) written and every other byte = `fill`."""
    size, members = BLOCKS[shader]
    raw = bytearray([fill]) * size
    for name, offset, count, dtype in members:
        if name in values:
            data = np.asarray(values[name], dtype=dtype)
            assert data.size == count, (shader, name)
            raw[offset: offset + 4 * count] = data.tobytes()
    return bytes(raw)


def ceil16(n):
    return (n + WORKGROUP - 1) // WORKGROUP * WORKGROUP


def written_extent(width, height, image_width, image_height):
    """DISPATCH: (columns, rows) of the written set, the extent rounded up to the workgroup and cut by the image."""
    return min(ceil16(width), image_width), min(ceil16(height), image_height)


def recorded_block(shader, block, width, height):
    """RECORD: the caller's bytes with the first 16 overwritten by drawOffset = 0 and drawExtent = (width, height)."""
    assert len(block) == block_size(shader)
    return np.array([0, 0, width, height], F32).tobytes() + bytes(block[PREFIX_BYTES:])


def unorm16(x):
    """STORE: clamp (NaN -> 0), x 65535, round to nearest even."""
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(x.astype(F32), F32(0)), F32(1))
        return np.rint(c * F32(65535.0)).astype(np.uint16)


def values(shader, block, width, height, xs, ys):
    """The fp32 texel [len(ys), len(xs), 4] handed to the store by the invocations (x, y) of xs x ys."""
    pc = recorded_block(shader, block, width, height)
    f = np.frombuffer(pc, F32)
    w = np.frombuffer(pc, np.uint32)
    xs = np.asarray(xs, np.int64)
    ys = np.asarray(ys, np.int64)
    half, one, four = F32(0.5), F32(1), F32(4)
    with np.errstate(all="ignore"):
        u = (xs.astype(F32) + half) / f[2]  # UV
        v = (ys.astype(F32) + half) / f[3]
        cx = (u * four).astype(np.int32)  # CELL (truncation; the values are non-negative and small)
        cy = (v * four).astype(np.int32)
        out = np.empty((len(ys), len(xs), 4), F32)
        if shader in ("gradient_color", "sparse_push_constant"):
            top, bottom = (f[4:8], f[8:12]) if shader == "gradient_color" else (f[[4, 5, 8, 9]], f[[12, 13, 16, 17]])
            a = v[:, None]
            out[:] = (top[None, :] * (one - a) + bottom[None, :] * a)[:, None, :]  # MIX: (1 - a), two products, one sum
        elif shader == "matrix_color":
            e = 4 + 4 * np.minimum(cy, 3)[:, None] + np.minimum(cx, 3)[None, :]  # MATRIX: column cy, row cx, clamped to 3
            out[..., 0], out[..., 1], out[..., 2], out[..., 3] = f[e], f[e + 16], f[e + 32], one
        else:
            inside = (cy >= 0) & (cy <= 3)
            word = w[4 + 4 * np.clip(cy, 0, 3)[:, None] + (cx % 4)[None, :]]
            lit = np.where(word != 0, one, F32(0)).astype(F32)
            red = np.where(inside[:, None], lit, one).astype(F32)  # BOOLEAN: red (1, 0, 0, 1) outside rows 0..3
            green_blue = np.where(inside[:, None], lit, F32(0)).astype(F32)
            out[..., 0] = red * u[None, :]
            out[..., 1] = green_blue * v[:, None]
            out[..., 2] = green_blue * F32(0)
            out[..., 3] = one * one
    return out


def render(shader, block, image, width, height):
    """The whole pass on a [H, W, 4] uint16 image: returns the image after it (a copy; bytes outside the written set keep
    their values) and the fp32 texels of the written set."""
    image_height, image_width = image.shape[:2]
    assert 0 < width <= image_width <= MAX_EXTENT and 0 < height <= image_height <= MAX_EXTENT
    cols, rows = written_extent(width, height, image_width, image_height)
    texels = values(shader, block, width, height, np.arange(cols), np.arange(rows))
    out = image.copy()
    out[:rows, :cols] = unorm16(texels)
    return out, texels
