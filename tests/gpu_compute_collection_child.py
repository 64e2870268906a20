"""Child process of tests/test_gpu_compute_collection.py: every program of the compute collection x every kind of block over a
fixed set of geometries, through the C-ABI of whichever library SZG_HIP_LIBRARY names. Prints one JSON line
{"library": name, "digests": {case: sha256 of the whole colour buffer}}. The parent runs it once per library and compares the
digests with each other and with the CPU model's."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from syzygy_amd import abi, lib  # noqa: E402
from syzygy_amd._lib import library_path  # noqa: E402

SHADERS = ("booleanpush", "gradient_color", "sparse_push_constant", "matrix_color")
KINDS = ("ordinary", "special", "example")
# (name, extent, image extent, pitch in texels, texels in front of the image)
CASES = [
    ("hd", (1280, 720), (1280, 720), 1280, 0),
    ("spill_on_both_axes", (1000, 700), (4096, 4096), 4096, 0),
    ("image_cuts_the_spill", (1001, 701), (1001, 701), 1001, 0),  # a pitch of 8008 B: odd rows leave the 16-B grid
    ("uhd", (3840, 2160), (3840, 2160), 3840, 0),
    ("one_texel", (1, 1), (1, 1), 1, 0),
    ("one_texel_in_16", (1, 1), (16, 16), 16, 0),
    ("padded_pitch", (17, 5), (32, 16), 37, 1),
]
FILL = 0x5A


def blocks():
    v = np.load(os.path.join(ROOT, "tests", "golden", "compute_collection_vectors.npz"))
    return {(s, k): v[f"{s}.{k}.block"].tobytes() for s in SHADERS for k in KINDS}


def key(name, shader, kind):
    return f"{name}/{shader}/{kind}"


def buffer_bytes(image_extent, pitch, offset):
    return (offset + pitch * image_extent[1]) * 8


def main():
    digests = {}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (shader, kind), block in blocks().items():
        for name, (w, h), (iw, ih), pitch, offset in CASES:
            flat = torch.full((buffer_bytes((iw, ih), pitch, offset),), FILL, dtype=torch.uint8, device="cuda")
            im = abi.Image(flat.data_ptr() + offset * 8, iw, ih, pitch * 8, abi.SZG_FORMAT_RGBA16_UNORM)
            status = lib().szg_record_compute_collection(stream, SHADERS.index(shader), block, len(block), C.byref(im), w, h)
            assert status == abi.SZG_OK, lib().szg_last_error()
            torch.cuda.synchronize()
            digests[key(name, shader, kind)] = hashlib.sha256(flat.cpu().numpy().tobytes()).hexdigest()
    print(json.dumps({"library": os.path.basename(library_path()), "digests": digests}))


if __name__ == "__main__":
    main()
