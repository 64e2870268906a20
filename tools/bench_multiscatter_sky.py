"""Device time of the LUT passes of the sky-view pipeline with and without multiple scattering
(include/szg/multiscatter_sky.h), in one session.

Per library, a child process times each record call between device events: the sky-view LUT at 2048 x 1024 in mode OFF
(k_skyview) and in mode ADD (k_skyview_ms<ADD>), the aerial LUT in both modes (k_aerial_lut, k_aerial_lut_ms<ADD>), and the
multi-scattering LUT (k_multiscatter). A run is --launches timed calls, its figure their median; there are --runs runs, and the
figure reported is the median of the runs' medians. A record call is what is timed: the sky-view figures include the one-lane
k_frame_prep and the 4-byte memset in front of the kernel, alike in both modes.

Two libraries are measured: libszg_hip.so, and libszg_hip_msalt.so, which takes the multi-scattering texels of k_skyview_ms from
the other place (kernels_lut_ms.hip SZG_MS_STAGE_LDS: LDS staging against global loads); `make -C syzygy_amd/csrc
libszg_hip_msalt.so` builds it. Which of the two is "lds" and which "global" is read from the default in kernels_lut_ms.hip.

    python tools/bench_multiscatter_sky.py [--runs 3] [--launches 15] [--json profiles/multiscatter_sky.json]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "syzygy_amd", "csrc")


def child(args):
    import torch

    from syzygy_amd import abi, pipelines as pl, scene

    assert torch.cuda.is_available(), "bench_multiscatter_sky.py needs a GPU"
    syn = scene.SyntheticScene()
    atm, sun, moon = scene.atmosphere_baked(scene.default_atmosphere(scene.sun_euler_for_elevation(35.0)), syn.bounds)
    cam = scene.camera_packed(scene.default_camera(), 16.0 / 9.0)
    cameras, atmospheres = pl.TStagedBuffer(abi.CameraPacked, 1), pl.TStagedBuffer(abi.AtmospherePacked, 1)
    cameras.push(cam)
    atmospheres.push(atm)
    cameras.recordCopyToDevice()
    atmospheres.recordCopyToDevice()
    sky = pl.SkyViewComputePipeline.create()  # 512 x 128, 2048 x 1024
    sky.recordTransmittance(None, 0, atmospheres)
    sky.recordMultiScatterLUT(None, 0, atmospheres)

    def mode(m):
        def go():
            sky.setMultiScattering(m)
        return go

    cases = [
        ("skyview_off", mode(abi.SZG_MULTISCATTER_OFF), lambda: sky.recordSkyViewLUT(None, 0, atmospheres, 0, cameras)),
        ("skyview_add", mode(abi.SZG_MULTISCATTER_ADD), lambda: sky.recordSkyViewLUT(None, 0, atmospheres, 0, cameras)),
        ("aerial_off", mode(abi.SZG_MULTISCATTER_OFF), lambda: sky.recordAerialLUT(None, 0, atmospheres, 0, cameras, 0.032)),
        ("aerial_add", mode(abi.SZG_MULTISCATTER_ADD), lambda: sky.recordAerialLUT(None, 0, atmospheres, 0, cameras, 0.032)),
        ("multiscatter_lut", mode(abi.SZG_MULTISCATTER_OFF), lambda: sky.recordMultiScatterLUT(None, 0, atmospheres)),
    ]
    out = {}
    for name, prepare, call in cases:
        prepare()
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        medians = []
        for _ in range(args.runs):
            events = []
            for _ in range(args.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                events.append((e0, e1))
            torch.cuda.synchronize()
            medians.append(statistics.median(a.elapsed_time(b) for a, b in events))
        out[name] = {"ms": round(statistics.median(medians), 5), "run_medians_ms": [round(m, 5) for m in medians]}
    import __graft_entry__ as entry

    print("RESULT " + json.dumps({"build_id": entry.build_id(), "device": torch.cuda.get_device_name(0), "cases": out}), flush=True)
    sky.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--json", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import __graft_entry__ as entry

    entry.build(only_if_missing=True)
    alt = os.path.join(CSRC, "libszg_hip_msalt.so")
    if not os.path.exists(alt):
        subprocess.run(["make", "-C", CSRC, "-j", "4", "libszg_hip_msalt.so"], check=True)
    default_is_lds = int(re.search(r"#define SZG_MS_STAGE_LDS (\d)", open(os.path.join(CSRC, "kernels_lut_ms.hip")).read()).group(1)) != 0
    libraries = {"lds" if default_is_lds else "global": None, "global" if default_is_lds else "lds": alt}
    results = {}
    for variant, path in libraries.items():
        env = dict(os.environ)
        if path is not None:
            env["SZG_HIP_LIBRARY"] = path
        # a fresh child per library: a process binds one library
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs), "--launches", str(args.launches)],
                              env=env, capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            return 1
        line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")][-1]
        results[variant] = dict(json.loads(line[len("RESULT "):]), library=os.path.basename(path or "libszg_hip.so"))
        print(variant, json.dumps(results[variant]), flush=True)
    g, l = results["global"]["cases"], results["lds"]["cases"]
    out = {"runs": args.runs, "launches_per_run": args.launches, "skyview_extent": [2048, 1024], "default_variant": "lds" if default_is_lds else "global",
           "source_hash": entry.source_hash("hip"), "variants": results,
           "skyview_add_ms": {"global": g["skyview_add"]["ms"], "lds": l["skyview_add"]["ms"]},
           "skyview_add_over_off": {"global": round(g["skyview_add"]["ms"] / g["skyview_off"]["ms"], 4),
                                    "lds": round(l["skyview_add"]["ms"] / l["skyview_off"]["ms"], 4)}}
    print(json.dumps({k: out[k] for k in ("default_variant", "skyview_add_ms", "skyview_add_over_off")}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", args.json)
    return 0


if __name__ == "__main__":
    sys.exit(main())
