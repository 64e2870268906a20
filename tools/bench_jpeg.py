"""Measures the JPEG reconstruction (include/szg/jpeg.h) and writes profiles/jpeg_reconstruct.json:

  * k_jpeg_idct and k_jpeg_color per map (1024^2 and 4096^2, 4:2:0 and 4:4:4): the pair timed with stream events (warm-up,
    ROUNDS rounds, median, min, max), and split per kernel with torch.profiler when it reports device kernels;
  * the bytes the two kernels must move (coefficients read, planes written and read again, RGBA written) and the time those
    bytes take at the HBM figure DESIGN.md uses;
  * single-thread host times on the same machine for the same inputs: szg_jpeg_open (entropy decode) and
    szg_jpeg_reconstruct_host, and the coefficient upload, which the device path pays and the host path does not.

The pictures are written by Pillow (half gradient, half noise, quality 90). Usage: python tools/bench_jpeg.py [--out FILE]
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12  # the spec figure DESIGN.md §4 uses
ROUNDS, WARMUP = 9, 3


def picture(size, subsampling):
    from PIL import Image

    rng = np.random.default_rng(size)
    y, x = np.mgrid[0:size, 0:size]
    img = np.empty((size, size, 3), np.uint8)
    for c in range(3):
        grad = ((x * (3 + c) + y * (5 - c)) * 255 // ((size - 1) * 8)).astype(np.uint8)
        img[..., c] = np.where(x < size // 2, grad, rng.integers(0, 256, (size, size), dtype=np.uint8))
    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, "JPEG", quality=90, subsampling=subsampling)
    return buf.getvalue()


def spread(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "rounds": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_reconstruct.json"))
    ap.add_argument("--sizes", default="1024,4096")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as entry
    from syzygy_amd import abi, lib, pipelines as pl

    entry.build(only_if_missing=True)
    assert torch.cuda.is_available(), "bench_jpeg needs a GPU"
    L = lib()
    result = {"device": torch.cuda.get_device_name(0), "build_id": entry.build_id(), "hbm_bytes_per_s": HBM_BYTES_PER_S,
              "method": f"{WARMUP} warm-up + {ROUNDS} rounds, stream events around the two launches; host: time.perf_counter, one thread",
              "maps": []}
    for size in (int(s) for s in args.sizes.split(",")):
        for layout, subsampling in (("4:2:0", 2), ("4:4:4", 0)):
            data = picture(size, subsampling)
            buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
            handle = C.c_void_p()
            open_ms = []
            for k in range(5):
                if handle:
                    L.szg_jpeg_destroy(handle)
                    handle = C.c_void_p()
                t0 = time.perf_counter()
                status = L.szg_jpeg_open(C.cast(buf, C.c_void_p), len(data), C.byref(handle))
                open_ms.append((time.perf_counter() - t0) * 1e3)
                assert status == abi.SZG_OK, L.szg_last_error()
            frame = abi.JpegFrame()
            L.szg_jpeg_get_frame(handle, C.byref(frame))
            host = np.empty((size, size, 4), np.uint8)
            host_ms = []
            for k in range(3):
                t0 = time.perf_counter()
                L.szg_jpeg_reconstruct_host(C.byref(frame), 0xFFFFFFFF, 0, host.ctypes.data_as(C.c_void_p), size * 4)
                host_ms.append((time.perf_counter() - t0) * 1e3)
            upload_ms = []
            for k in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d_frame, keep = pl.upload_jpeg_frame(frame)
                torch.cuda.synchronize()
                upload_ms.append((time.perf_counter() - t0) * 1e3)
            coefficient_bytes = sum(t.numel() * 2 for t in keep)
            plane_bytes = L.szg_jpeg_scratch_bytes(C.byref(d_frame))
            out = torch.empty((size, size, 4), dtype=torch.uint8, device="cuda")
            scratch = torch.empty(plane_bytes, dtype=torch.uint8, device="cuda")
            pair_ms = []
            for k in range(WARMUP + ROUNDS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                pl.record_jpeg_reconstruct(d_frame, out, scratch=scratch)
                b.record()
                b.synchronize()
                if k >= WARMUP:
                    pair_ms.append(a.elapsed_time(b))
            assert np.array_equal(out.cpu().numpy(), host), "device and host reconstructions differ"
            kernels = {"k_jpeg_idct": None, "k_jpeg_color": None}
            try:
                from torch.profiler import ProfilerActivity, profile

                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    for k in range(ROUNDS):
                        pl.record_jpeg_reconstruct(d_frame, out, scratch=scratch)
                    torch.cuda.synchronize()
                per = {}
                for ev in prof.events():
                    for name in kernels:
                        if name in ev.name:
                            per.setdefault(name, []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
                for name, us in per.items():
                    kernels[name] = spread([u / 1e3 for u in us])
            except Exception as e:  # the profiler is optional: the pair time above stands on its own
                kernels["error"] = repr(e)
            # planes are written by k_jpeg_idct and read again by k_jpeg_color
            must_move = coefficient_bytes + 2 * plane_bytes + size * size * 4
            result["maps"].append({
                "size": size, "layout": layout, "file_bytes": len(data),
                "both_kernels": spread(pair_ms), "kernels": kernels,
                "bytes": {"coefficients_read": coefficient_bytes, "planes_written": plane_bytes, "planes_read": plane_bytes,
                          "rgba_written": size * size * 4, "total": must_move},
                "hbm_floor_ms": must_move / HBM_BYTES_PER_S * 1e3,
                "host_single_thread": {"szg_jpeg_open": spread(open_ms), "szg_jpeg_reconstruct_host": spread(host_ms)},
                "coefficient_upload_pageable": spread(upload_ms),
            })
            print(json.dumps(result["maps"][-1]), flush=True)
            L.szg_jpeg_destroy(handle)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
