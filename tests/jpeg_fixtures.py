"""The JPEG fixtures of tests/golden/jpeg (written by tests/golden/make_jpeg_fixtures.py): file bytes, the RGBA the
reference's decoder returns for them, and ctypes helpers over include/szg/jpeg.h that the JPEG tests share."""
import ctypes as C
import functools
import glob
import os

import numpy as np

from syzygy_amd import abi, lib

HERE = os.path.dirname(os.path.abspath(__file__))
FOLDER = os.path.join(HERE, "golden", "jpeg")


@functools.lru_cache(maxsize=None)
def _expected_file():
    with np.load(os.path.join(FOLDER, "expected_rgba.npz")) as z:
        return {k: z[k] for k in z.files}


def names():
    """every fixture the reference decodes (the refused ones are listed by refused_names())"""
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(FOLDER, "*.jpg"))
                  if not os.path.basename(f).startswith("refused_"))


def refused_names():
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(FOLDER, "refused_*.jpg")))


def data(name):
    with open(os.path.join(FOLDER, name + ".jpg"), "rb") as f:
        return f.read()


def expected(name):
    """uint8 [h, w, 4], read-only. The file stores [4, h, w]; a progressive or restart-marker file that decodes like its baseline
    sibling is stored under the sibling's name."""
    table = _expected_file()
    key = name if name in table else name.replace("_prog_", "_base_").replace("_rst_", "_base_")
    out = np.ascontiguousarray(table[key].transpose(1, 2, 0))
    out.setflags(write=False)
    return out


class Jpeg:
    """szg_jpeg_open / szg_jpeg_get_frame / szg_jpeg_destroy"""

    def __init__(self, stream):
        self.handle = C.c_void_p()
        self._bytes = (C.c_uint8 * max(len(stream), 1)).from_buffer_copy(bytes(stream) or b"\0")
        self.status = lib().szg_jpeg_open(C.cast(self._bytes, C.c_void_p), len(stream), C.byref(self.handle))
        self.error = lib().szg_last_error().decode(errors="replace") if self.status != abi.SZG_OK else ""
        self.frame = abi.JpegFrame()
        if self.status == abi.SZG_OK:
            assert lib().szg_jpeg_get_frame(self.handle, C.byref(self.frame)) == abi.SZG_OK

    def close(self):
        if self.handle:
            lib().szg_jpeg_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def coefficients(self, plane):
        """int16 [blocks_h, blocks_w, 8, 8], a copy"""
        p = self.frame.planes[plane]
        n = p.blocks_w * p.blocks_h * 64
        flat = np.ctypeslib.as_array(C.cast(p.coefficients, C.POINTER(C.c_int16)), shape=(n,)).copy()
        return flat.reshape(p.blocks_h, p.blocks_w, 8, 8)

    def model_frame(self):
        """the frame as tests/jpeg_model.py wants it"""
        from tests.jpeg_model import COLOR_NAMES

        f = self.frame
        return {"width": f.width, "height": f.height, "color": COLOR_NAMES[f.color],
                "planes": [(f.planes[k].h, f.planes[k].v, self.coefficients(k)) for k in range(f.plane_count)]}

    def reconstruct_host(self, rgba_and=0xFFFFFFFF, rgba_or=0, pitch=None, fill=None):
        f = self.frame
        pitch = f.width * 4 if pitch is None else pitch
        out = np.zeros((f.height, pitch), np.uint8) if fill is None else np.full((f.height, pitch), fill, np.uint8)
        status = lib().szg_jpeg_reconstruct_host(C.byref(f), rgba_and, rgba_or, out.ctypes.data_as(C.c_void_p), pitch)
        assert status == abi.SZG_OK, lib().szg_last_error()
        return out


def make_frame(width, height, factors, color, pointers=None):
    """An abi.JpegFrame whose geometry follows from width, height and [(h, v)] (jpeg.h rules 2 and 4)."""
    from tests.jpeg_model import plane_grid

    f = abi.JpegFrame()
    f.width, f.height, f.plane_count, f.color = width, height, len(factors), color
    f.h_max = max(h for h, _ in factors)
    f.v_max = max(v for _, v in factors)
    for k, (h, v) in enumerate(factors):
        bw, bh, cw, ch = plane_grid(width, height, h, v, f.h_max, f.v_max)
        p = f.planes[k]
        p.h, p.v, p.width, p.height, p.blocks_w, p.blocks_h = h, v, cw, ch, bw, bh
        if pointers is not None:
            p.coefficients = pointers[k]
    return f
