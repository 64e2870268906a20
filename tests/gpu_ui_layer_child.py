"""Child process of tests/test_gpu_ui_layer.py: three UI layer cases through whichever library SZG_HIP_LIBRARY names, as
SHA-256 digests of the whole target buffers on the last line of stdout. The parent compares them with its own."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def digests(torch):
    from syzygy_amd import abi, lib
    from tests import ui_layer_cases as uc
    from tests import ui_layer_gpu as ug
    from tests import ui_layer_model as um

    layer = ug.Layer(torch)
    out = {}
    cases = {"sweep": (uc.random_sweep(seed=5, n_tris=600, size=(67, 45), n_cmds=10, big_fraction=0.04), (71, 53), (3, 2, 67, 45), um.LOAD),
             "linear16": (uc.sampler_case(um.LINEAR, um.REPEAT, np.uint16), (48, 36), (0, 0, 48, 36), um.CLEAR),
             "stack65": ((uc.truncated(uc.stack(65)[0], 65), uc.stack(65)[1]), (64, 64), (0, 0, 64, 64), um.CLEAR)}
    for name, ((draw, textures), extent, area, load_op) in cases.items():
        target = ug.Target(torch, *extent)
        handles = {k: layer.add_texture(t) for k, t in textures.items()}
        assert layer.record(target, area, load_op, draw, handles) == abi.SZG_OK, lib().szg_last_error()
        out[name] = hashlib.sha256(target.read().tobytes()).hexdigest()
        for h in handles.values():
            layer.remove_texture(h)
    layer.destroy()
    return out


if __name__ == "__main__":
    import torch

    from syzygy_amd._lib import library_path

    print(json.dumps({"library": os.path.basename(library_path()), "digests": digests(torch)}))
