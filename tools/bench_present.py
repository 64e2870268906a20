"""Device time of the present pass (include/szg/present.h) next to szg_record_oetf, in one process.

At 3840x2160 and 1920x1080: the 1:1 present to each destination format, plain and with the sRGB encode, and the untouched
in-place szg_record_oetf of the same extent; then the LINEAR blits 4K -> 1080p, 1080p -> 4K and 8K -> 4K.

How a case is timed. The inputs are uniform 16-bit noise (the worst case for the OETF table's gathers). Every case works
on a ring of buffers larger than the 256 MiB Infinity Cache, so that the figures are HBM figures and not those of a frame
that stays in cache; device events surround one pass over the ring ("window"), the in-place OETF gets its ring refreshed
from pristine copies outside the events (a second application would see encoded, clustered codes), and windows are
repeated until about --seconds of device time have been timed. ms = timed device time / calls.

Two expectations follow from the byte counts alone (12 B/px for the 1:1 present, 16 B/px for the OETF) and are evaluated
in the output: the encoding 1:1 present takes no longer than szg_record_oetf alone, and the plain 1:1 present reaches at
least half of the bandwidth szg_record_oetf reaches in the same run.

    python tools/bench_present.py [--seconds 0.3] [--json profiles/present_bench.json]

Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_present.py --seconds 0.05`."""
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
FORMATS = {"rgba8": abi.SZG_FORMAT_RGBA8_UNORM, "bgra8": abi.SZG_FORMAT_BGRA8_UNORM, "a2b10g10r10": abi.SZG_FORMAT_A2B10G10R10_UNORM}


def noise(width, height, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-32768, 32767, (height, width, 4), dtype=torch.int16, device="cuda", generator=g)


def timed(calls, ring, seconds, refresh=None):
    """ms per call: windows of one pass over the ring between device events, repeated for ~`seconds` of device time."""
    def window():
        if refresh is not None:
            refresh()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(ring):
            calls(i)
        e1.record()
        return e0, e1

    for _ in range(3):  # warm-up: code objects, the OETF table, every buffer touched
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


def present_case(name, src_extent, dst_extent, fmt_name, encode, seconds):
    (sw, sh), (dw, dh) = src_extent, dst_extent
    fmt = FORMATS[fmt_name]
    ring = max(2, -(-RING_BYTES // (sw * sh * 8)))
    sources = [noise(sw, sh, 100 + i) for i in range(ring)]
    dests = [pl.swapchain_image(dw, dh, fmt) for _ in range(ring)]
    images = [pl.present_images(s, d, fmt) for s, d in zip(sources, dests)]
    info = abi.PresentInfo(abi.Rect(0, 0, sw, sh), abi.Rect(0, 0, dw, dh), abi.SZG_FILTER_LINEAR, encode)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(i):
        rc = lib().szg_record_present(stream, C.byref(images[i][0]), C.byref(images[i][1]), C.byref(info))
        assert rc == abi.SZG_OK, lib().szg_last_error()

    ms, calls = timed(call, ring, seconds)
    traffic = sw * sh * 8 + dw * dh * 4 if (sw, sh) == (dw, dh) else None  # scaled: the taps' reuse is the cache's business
    r = {"case": name, "source": [sw, sh], "destination": [dw, dh], "format": fmt_name,
         "encode": "none" if encode == abi.SZG_PRESENT_ENCODE_NONE else "srgb", "ring_buffers": ring, "calls": calls,
         "ms": round(ms, 5), "bytes": traffic, "tb_per_s": round(traffic / ms / 1e9, 3) if traffic else None,
         "ns_per_destination_pixel": round(ms * 1e6 / (dw * dh), 5)}
    print(json.dumps(r), flush=True)
    return r


def oetf_case(extent, seconds):
    w, h = extent
    ring = max(2, -(-RING_BYTES // (w * h * 8)))
    pristine = [noise(w, h, 100 + i) for i in range(ring)]
    work = [p.clone() for p in pristine]
    images = [pl.present_images(t, pl.swapchain_image(1, 1))[0] for t in work]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refresh():
        for a, b in zip(work, pristine):
            a.copy_(b)

    def call(i):
        rc = lib().szg_record_oetf(stream, C.byref(images[i]), w, h, abi.SZG_OETF_SRGB)
        assert rc == abi.SZG_OK, lib().szg_last_error()

    ms, calls = timed(call, ring, seconds, refresh)
    traffic = w * h * 16
    r = {"case": f"szg_record_oetf {w}x{h} (in place, sRGB)", "source": [w, h], "ring_buffers": ring, "calls": calls,
         "ms": round(ms, 5), "bytes": traffic, "tb_per_s": round(traffic / ms / 1e9, 3)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="device time to fill per case")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    entry.build(only_if_missing=True)
    assert torch.cuda.is_available(), "bench_present.py needs a GPU"
    results, expectations = [], []
    for extent in ((3840, 2160), (1920, 1080)):
        tag = f"{extent[0]}x{extent[1]}"
        oetf = oetf_case(extent, args.seconds)
        results.append(oetf)
        plain, encoded = [], []
        for fmt_name in FORMATS:
            plain.append(present_case(f"present 1:1 {tag} -> {fmt_name}", extent, extent, fmt_name, abi.SZG_PRESENT_ENCODE_NONE, args.seconds))
            encoded.append(present_case(f"present 1:1 {tag} -> {fmt_name}, sRGB encode", extent, extent, fmt_name, abi.SZG_OETF_SRGB,
                                        args.seconds))
        results += plain + encoded
        slowest_encoded = max(r["ms"] for r in encoded)
        lowest_plain = min(r["tb_per_s"] for r in plain)
        expectations.append({"extent": list(extent), "expectation": "encoding 1:1 present takes no longer than szg_record_oetf alone",
                             "present_ms_slowest_format": slowest_encoded, "oetf_ms": oetf["ms"], "met": slowest_encoded <= oetf["ms"]})
        expectations.append({"extent": list(extent), "expectation": "plain 1:1 present reaches at least half of szg_record_oetf's bandwidth",
                             "present_tb_per_s_lowest_format": lowest_plain, "oetf_tb_per_s": oetf["tb_per_s"],
                             "met": lowest_plain >= 0.5 * oetf["tb_per_s"]})
    for name, s, d in (("present 4K -> 1080p LINEAR", (3840, 2160), (1920, 1080)), ("present 1080p -> 4K LINEAR", (1920, 1080), (3840, 2160)),
                       ("present 8K -> 4K LINEAR", (7680, 4320), (3840, 2160))):
        results.append(present_case(name, s, d, "rgba8", abi.SZG_PRESENT_ENCODE_NONE, args.seconds))
    out = {"seconds_per_case": args.seconds, "ring_bytes": RING_BYTES, "build_id": entry.build_id(), "source_hash": entry.source_hash("hip"),
           "device": torch.cuda.get_device_name(0), "results": results, "expectations": expectations}
    for e in expectations:
        print(json.dumps(e), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", args.json)


if __name__ == "__main__":
    main()
