"""Device time of the compute-collection pipeline (include/szg/compute_collection.h) next to a plain device fill of the same
bytes, in one process.

Per program at 1920x1080 and 3840x2160 (extent = image: 8 B written per texel, nothing read): ms per record, bytes written
per second, and in the SAME run the yardstick: hipMemsetAsync (through the C runtime torch is linked to) and tensor.fill_ over
the same bytes. The ratio program / fill is reported per case; the expectation from the byte count alone is that a program takes
what the fill takes plus a launch. Nothing is asserted.

How a case is timed (the method of tools/bench_present.py). Every case works on a ring of images larger than the 256 MiB
Infinity Cache, so that the figures are HBM figures and not those of a frame that stays in cache; device events surround one
pass over the ring ("window"), and windows are repeated until about --seconds of device time have been timed.
ms = timed device time / calls. The blocks are the examples' (abi.COMPUTE_COLLECTION_EXAMPLE_VALUES).

    python tools/bench_compute_collection.py [--seconds 0.3] [--json profiles/compute_collection_bench.json]

Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_compute_collection.py --seconds 0.05`."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from syzygy_amd import abi, lib, pipelines as pl  # noqa: E402

RING_BYTES = 600 << 20  # > 2 x the Infinity Cache


def timed(calls, ring, seconds):
    """ms per call: windows of one pass over the ring between device events, repeated for ~`seconds` of device time."""
    def window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(ring):
            calls(i)
        e1.record()
        return e0, e1

    for _ in range(3):  # warm-up: code objects, every buffer touched
        window()
    torch.cuda.synchronize()
    pilot = [window() for _ in range(5)]
    torch.cuda.synchronize()
    per_window = sum(a.elapsed_time(b) for a, b in pilot) / len(pilot) / 1e3
    windows = int(min(max(seconds / max(per_window, 1e-6), 10), 5000))
    events = [window() for _ in range(windows)]
    torch.cuda.synchronize()
    total_ms = sum(a.elapsed_time(b) for a, b in events)
    return total_ms / (windows * ring), windows * ring


def result(name, extent, ring, ms, calls):
    traffic = extent[0] * extent[1] * 8
    r = {"case": name, "extent": list(extent), "ring_buffers": ring, "calls": calls, "ms": round(ms, 5), "bytes": traffic,
         "tb_per_s": round(traffic / ms / 1e9, 3)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="device time to fill per case")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    entry.build(only_if_missing=True)
    assert torch.cuda.is_available(), "bench_compute_collection.py needs a GPU"
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))  # the runtime torch and the library share
    hip.hipMemsetAsync.restype = C.c_int
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pipeline = pl.ComputeCollectionPipeline()
    results, ratios = [], []
    for extent in ((1920, 1080), (3840, 2160)):
        w, h = extent
        tag = f"{w}x{h}"
        nbytes = w * h * 8
        ring = max(2, -(-RING_BYTES // nbytes))
        tensors = [torch.zeros((h, w, 4), dtype=torch.int16, device="cuda") for _ in range(ring)]
        images = [abi.Image(t.data_ptr(), w, h, w * 8, abi.SZG_FORMAT_RGBA16_UNORM) for t in tensors]

        def memset(i):
            assert hip.hipMemsetAsync(tensors[i].data_ptr(), 0x3C, nbytes, stream) == 0

        def fill(i):
            tensors[i].fill_(0x3C3C)

        ms, calls = timed(memset, ring, args.seconds)
        yard_memset = result(f"hipMemsetAsync {tag}", extent, ring, ms, calls)
        ms, calls = timed(fill, ring, args.seconds)
        yard_fill = result(f"tensor.fill_ {tag}", extent, ring, ms, calls)
        results += [yard_memset, yard_fill]
        yard = min(yard_memset["ms"], yard_fill["ms"])
        for index, reflection in enumerate(pipeline.shaders()):
            pipeline.selectShader(index)
            pipeline.writeExampleValues()
            block = pipeline.readPushConstantBytes()

            def record(i):
                rc = lib().szg_record_compute_collection(stream, index, block, len(block), C.byref(images[i]), w, h)
                assert rc == abi.SZG_OK, lib().szg_last_error()

            ms, calls = timed(record, ring, args.seconds)
            r = result(f"{reflection.name} {tag}", extent, ring, ms, calls)
            results.append(r)
            ratios.append({"extent": list(extent), "program": reflection.name, "ms": r["ms"], "fill_ms": yard,
                           "hipMemsetAsync_ms": yard_memset["ms"], "tensor_fill_ms": yard_fill["ms"], "ratio_to_fill": round(r["ms"] / yard, 3)})
        del tensors, images
        torch.cuda.empty_cache()
    out = {"seconds_per_case": args.seconds, "ring_bytes": RING_BYTES, "build_id": entry.build_id(), "source_hash": entry.source_hash("hip"),
           "device": torch.cuda.get_device_name(0), "results": results, "ratios": ratios}
    for r in ratios:
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", args.json)


if __name__ == "__main__":
    main()
