"""Child process of tests/test_gpu_present.py: a fixed set of present-pass cases through the C-ABI of whichever library
SZG_HIP_LIBRARY names. Prints one JSON line {"library": name, "digests": {case: sha256 of the destination bytes}}.
The parent runs it once per library and compares the digests with each other and with the CPU model's."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from syzygy_amd import abi, pipelines as pl  # noqa: E402
from syzygy_amd._lib import library_path  # noqa: E402

# (name, source extent, source region, destination extent): one scaled blit of an offset subregion, one 1:1
CASES = [
    ("scaled", (1000, 700), (17, 9, 960, 680), (1337, 911)),
    ("one_to_one", (640, 360), (3, 5, 597, 301), (597, 301)),
]
FORMATS = (abi.SZG_FORMAT_RGBA8_UNORM, abi.SZG_FORMAT_BGRA8_UNORM, abi.SZG_FORMAT_A2B10G10R10_UNORM)
FILTERS = (abi.SZG_FILTER_LINEAR, abi.SZG_FILTER_NEAREST)
ENCODES = (abi.SZG_PRESENT_ENCODE_NONE, abi.SZG_OETF_PURE_GAMMA, abi.SZG_OETF_SRGB)


def source(extent):
    return np.random.default_rng(1).integers(0, 65536, (extent[1], extent[0], 4), dtype=np.uint16)


def key(name, fmt, filter, encode):
    return f"{name}/fmt{fmt}/filter{filter}/encode{encode & 0xFF}"


def main():
    digests = {}
    for name, extent, region, (dw, dh) in CASES:
        src = torch.from_numpy(source(extent).view(np.int16)).cuda()
        for fmt in FORMATS:
            for filter in FILTERS:
                for encode in ENCODES:
                    dst = pl.swapchain_image(dw, dh, fmt)
                    pl.record_copy_image_to_image(None, src, dst, region, None, filter, encode, fmt)
                    torch.cuda.synchronize()
                    digests[key(name, fmt, filter, encode)] = hashlib.sha256(dst.cpu().numpy().tobytes()).hexdigest()
    print(json.dumps({"library": os.path.basename(library_path()), "digests": digests}))


if __name__ == "__main__":
    main()
