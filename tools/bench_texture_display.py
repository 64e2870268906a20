"""Device time of the texture viewer's copy and clear (include/szg/texture_display.h), and the check that the UI layer pass does
not pay for the formats the viewer added to it. Method of tools/bench_ui_layer.py: rings of buffers larger than the Infinity
Cache, device events around one pass over the ring, windows repeated for about --seconds of device time; every case is run
--runs times and reported as the median with min and max.

    python tools/bench_texture_display.py --json copy.json
        copies of 64^2, 1024^2 and 4096^2 RGBA8_SRGB and RGBA8_UNORM maps onto 4096^2 RGBA16_SFLOAT, the clear of that image,
        and the UI pass's clear-only case at 4096^2 (8 B/texel written, nothing read): the ceiling a store-bound kernel of this
        library has reached on the device. Each with the bytes that must move and what they would take at 8 TB/s.
    python tools/bench_texture_display.py --ui-cases --json branch.json
    SZG_HIP_LIBRARY=<parent build>/libszg_hip.so python tools/bench_texture_display.py --ui-cases --json parent.json
        cases (b), (c), (d) of tools/bench_ui_layer.py at 3840x2160, through szg_ui_layer_add_texture only: runs with a library
        built from the parent commit too.
    python tools/bench_texture_display.py --assemble copy.json parent.json branch.json --json profiles/texture_display.json
        one record, with the verdict per UI case: the branch median inside the parent's min-max widened by the parent's spread."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DISPLAY = 4096
HBM_TB_PER_S = 8.0


def summary(name, samples, traffic=None, **more):
    ms = statistics.median(samples)
    r = {"case": name, "ms_median": round(ms, 5), "ms_min": round(min(samples), 5), "ms_max": round(max(samples), 5), "runs": len(samples)}
    if traffic:
        r.update(bytes=traffic, tb_per_s=round(traffic / ms / 1e9, 3), ms_at_8_tb_per_s=round(traffic / HBM_TB_PER_S / 1e9, 5))
    r.update(more)
    print(json.dumps(r), flush=True)
    return r


def copy_cases(seconds, runs):
    import torch

    from bench_present import RING_BYTES, timed
    from bench_ui_layer import Bench
    from syzygy_amd import abi, lib, pipelines as pl, ui

    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ring = max(2, -(-RING_BYTES // (DISPLAY * DISPLAY * 8)))
    displays = [torch.empty((DISPLAY, DISPLAY, 4), dtype=torch.float16, device="cuda") for _ in range(ring)]
    d_images = [pl._strided_image(t, abi.SZG_FORMAT_RGBA16_SFLOAT, 4) for t in displays]
    whole = abi.Rect(0, 0, DISPLAY, DISPLAY)
    results = []
    g = torch.Generator(device="cuda").manual_seed(5)
    for n in (64, 1024, 4096):
        maps = [torch.randint(0, 256, (n, n, 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(ring)]
        for name, fmt in (("RGBA8_SRGB", abi.SZG_FORMAT_RGBA8_SRGB), ("RGBA8_UNORM", abi.SZG_FORMAT_RGBA8_UNORM)):
            s_images = [pl._strided_image(t, fmt, 4) for t in maps]
            region = abi.Rect(0, 0, n, n)

            def call(i):
                rc = lib().szg_record_copy_image(stream, C.byref(s_images[i]), C.byref(d_images[i]), region, whole)
                assert rc == abi.SZG_OK, lib().szg_last_error()

            samples = [timed(call, ring, seconds)[0] for _ in range(runs)]
            results.append(summary(f"copy {n}x{n} {name} -> {DISPLAY}x{DISPLAY} RGBA16_SFLOAT", samples, n * n * 4 + DISPLAY * DISPLAY * 8,
                                   ring_buffers=ring))
        del maps
    black = (C.c_float * 4)(0.0, 0.0, 0.0, 1.0)

    def clear(i):
        assert lib().szg_record_clear_color_image(stream, C.byref(d_images[i]), black) == abi.SZG_OK, lib().szg_last_error()

    results.append(summary(f"clear {DISPLAY}x{DISPLAY} RGBA16_SFLOAT", [timed(clear, ring, seconds)[0] for _ in range(runs)],
                           DISPLAY * DISPLAY * 8, ring_buffers=ring))
    del displays, d_images
    torch.cuda.empty_cache()
    # the ceiling: the UI pass's clear-only case, in this session, at the display's extent and at the extent of
    # profiles/ui_layer_bench.json
    bench = Bench(seconds)
    for w, h in ((DISPLAY, DISPLAY), (3840, 2160)):
        empty = ui.DrawData((0, 0), (w, h), (1, 1), []).flatten()
        samples = [bench.case(f"(a) clear only {w}x{h}", (w, h), empty, w * h * 8)["ms"] for _ in range(runs)]
        results.append(summary(f"szg_ui_layer_record_draw, clear only {w}x{h}", samples, w * h * 8))
    lib().szg_ui_layer_destroy(bench.h)
    return results


def ui_cases(seconds, runs):
    from bench_ui_layer import SCENE, WHITE, Bench, editor_frame, glyph_frame
    from syzygy_amd import lib, ui

    w, h = 3840, 2160
    bench = Bench(seconds)
    quad = ui.DrawList(WHITE)
    quad.add_image(SCENE, (0, 0), (w, h))
    cases = [("(b) scene viewport quad 1:1", ui.DrawData((0, 0), (w, h), (1, 1), [quad]).flatten()),
             ("(c) editor-like frame", editor_frame(w, h)), ("(d) 50000 glyph quads", glyph_frame(w, h))]
    samples = {name: [] for name, _ in cases}
    for _ in range(runs):  # the runs of a case are spread over the session, not back to back
        for name, flat in cases:
            samples[name].append(bench.case(f"{name} {w}x{h}", (w, h), flat)["ms"])
    lib().szg_ui_layer_destroy(bench.h)
    return [summary(f"{name} {w}x{h}", s) for name, s in samples.items()]


def assemble(copy_path, parent_path, branch_path):
    copy, parent, branch = (json.load(open(p)) for p in (copy_path, parent_path, branch_path))
    verdicts = []
    for p, b in zip(parent["results"], branch["results"]):
        assert p["case"] == b["case"]
        spread = p["ms_max"] - p["ms_min"]
        lo, hi = p["ms_min"] - spread, p["ms_max"] + spread
        verdicts.append({"case": p["case"], "parent_ms": [p["ms_min"], p["ms_median"], p["ms_max"]],
                         "branch_ms": [b["ms_min"], b["ms_median"], b["ms_max"]], "allowed_ms": [round(lo, 5), round(hi, 5)],
                         "inside": lo <= b["ms_median"] <= hi})
    return {"copy_and_clear": copy, "ui_layer_parent": parent, "ui_layer_branch": branch, "ui_layer_verdict": verdicts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="device time to fill per run of a case")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ui-cases", action="store_true")
    ap.add_argument("--assemble", nargs=3, metavar=("COPY", "PARENT", "BRANCH"))
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.assemble:
        out = assemble(*args.assemble)
    else:
        import torch

        import __graft_entry__ as entry

        if "SZG_HIP_LIBRARY" not in os.environ:
            entry.build(only_if_missing=True)
        assert torch.cuda.is_available(), "bench_texture_display.py needs a GPU"
        results = ui_cases(args.seconds, args.runs) if args.ui_cases else copy_cases(args.seconds, args.runs)
        out = {"seconds_per_run": args.seconds, "runs": args.runs, "build_id": entry.build_id(), "library_named_explicitly": "SZG_HIP_LIBRARY" in os.environ,
               "device": torch.cuda.get_device_name(0), "results": results}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", args.json)


if __name__ == "__main__":
    main()
