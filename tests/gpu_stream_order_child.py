"""Child process of tests/test_gpu_stream_order.py: the process-global OETF tables across two streams.

szg_record_oetf builds a 65536-entry table per transfer function on the FIRST caller's stream and orders every later stream
behind a `ready` event (syzygy_amd/csrc/api_image_passes.cpp oetf_table). Here, for each function, the first call of the process
goes on non-blocking stream A behind a blocker, and immediately, with no host sync, a second call with another image goes on
non-blocking stream B, which has nothing in front of it: B's image is right only if its kernel waited for the table that A has
not built yet. Both images must equal the oracle's evaluation of every code (tests/test_gpu_parity.py
test_oetf_every_code_value). Prints one JSON line; exits non-zero on a mismatch or when the blocker had ended too early."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import binding as ob  # noqa: E402
from syzygy_amd import abi, lib  # noqa: E402
from tests import stream_order as so  # noqa: E402

BLOCKER_MS = 60.0  # the two calls take well under a millisecond of host time (profiles/stream_order_mutants.md)


def every_code(arrangement):
    """All 65536 UNORM16 codes in every colour channel, in two different arrangements."""
    codes = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    if arrangement == 0:
        return np.stack([codes, codes[::-1, ::-1], codes.T, codes], -1).copy()
    return np.stack([codes.T, codes, codes[::-1], codes[:, ::-1]], -1).copy()


def record(stream, tensor, function):
    im = abi.Image(tensor.data_ptr(), 256, 256, 256 * 8, abi.SZG_FORMAT_RGBA16_UNORM)
    rc = lib().szg_record_oetf(C.c_void_p(stream.cuda_stream), C.byref(im), 256, 256, function)
    assert rc == abi.SZG_OK, lib().szg_last_error()


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    blocker = so.Blocker(torch)
    out = {"functions": {}}
    ok = True
    with so.side_streams(torch, 2) as (A, B):
        for function in (0, 1):
            images = [every_code(0), every_code(1)]
            tensors = [torch.from_numpy(img.view(np.int16)).cuda() for img in images]
            torch.cuda.synchronize()
            done = blocker.enqueue(A, BLOCKER_MS)
            record(A, tensors[0], function)  # the first use of this function's table in the process: builds it, behind the blocker
            record(B, tensors[1], function)  # another stream, nothing in front of it
            pending = not done.query()
            A.synchronize()
            B.synchronize()
            got = [t.cpu().numpy().view(np.uint16) for t in tensors]
            want = [ob.oetf(img.copy(), function) for img in images]
            result = {
                "blocker_pending_when_both_calls_had_returned": bool(pending),
                "first_stream_equals_model": bool(np.array_equal(got[0], want[0])),
                "second_stream_equals_model": bool(np.array_equal(got[1], want[1])),
                "second_stream_differing_values": int((got[1] != want[1]).sum()),
            }
            out["functions"][str(function)] = result
            ok = ok and all(v for k, v in result.items() if k != "second_stream_differing_values")
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
