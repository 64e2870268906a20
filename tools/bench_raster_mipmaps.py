"""G-buffer raster record times with and without mip chains (include/szg/mipmaps.h) and under anisotropic filtering
(include/szg/anisotropy.h), and the chain builder's throughput.
The configurations are alternated within one call, a fresh process per configuration and round; HIP events around 20 records
after 3 warm-up records; medians over the rounds, each configuration's own max - min spread beside them.
usage: python tools/bench_raster_mipmaps.py [--rounds 5] [--baseline PATH/libszg_hip.so] [--out profiles/raster_mipmaps.json]
Scenes at 3840x2160, every material map 2048^2 random bytes (colour sRGB, normal and ORM UNORM): a ground plane of 800 x 800
units receding from the default camera with uv repeating 32 times, and the reference's default scene. Configurations: no table
(k_raster_tile<false>), full chains (k_raster_tile<true>, max_lod NONE), full chains with the reference's max_lod = 1.0, and
full chains with max_lod NONE under max_anisotropy 2, 4 and 16 (k_raster_tile_aniso). With --baseline the first two are also
run against that build of the library (a parent commit's, which need not know anisotropy.h), alternated with the rest.
Generation: szg_record_generate_mipmaps of 1024^2 and 4096^2, sRGB and UNORM, in GB/s of bytes read plus bytes written."""
import argparse, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANISO = {"aniso_2": 2.0, "aniso_4": 4.0, "aniso_16": 16.0}
CONFIGS = ("none", "full", "full_max_lod_1") + tuple(ANISO)
BASELINE_CONFIGS = ("baseline_none", "baseline_full")  # the same two configurations through the --baseline library
MAP = 2048


def time_it(torch, fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def child(config):
    import numpy as np
    import torch
    from tests import util
    from tests import raster_scenes as rs
    from syzygy_amd import meshes, abi, pipelines as pl

    out = {}
    if config == "generate":
        for size in (1024, 4096):
            for srgb in (False, True):
                level0 = torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device="cuda")
                ms = time_it(torch, lambda: pl.generate_mipmaps(level0, srgb), reps=10)
                # every level but the last is read once, every level but the first written once
                chain = lib_chain_bytes(size)
                moved = (size * size * 4 + chain - 4) + chain
                out[f"generate_{size}x{size}_{'srgb' if srgb else 'unorm'}"] = {"ms": ms, "GB_per_s": moved / ms / 1e6}
        print("RESULT " + json.dumps(out), flush=True)
        return
    config = config[len("baseline_"):] if config.startswith("baseline_") else config  # the library is chosen by the parent process
    W, H = 3840, 2160
    inp = util.Inputs(W, H, elevation_degrees=40.0, spots=1)
    cams = pl.TStagedBuffer(abi.CameraPacked, 1); cams.push(inp.cam); cams.recordCopyToDevice()
    target = pl.SceneTexture(W, H)
    d = pl.DeferredShadingPipeline((W, H), max_spot_lights=1, max_shadow_maps=0)
    rng = np.random.default_rng(1)
    material = {"color": (rng.integers(0, 256, (MAP, MAP, 4), dtype=np.uint8), True),
                "normal": (rng.integers(96, 160, (MAP, MAP, 4), dtype=np.uint8), False),
                "orm": (rng.integers(0, 256, (MAP, MAP, 4), dtype=np.uint8), False)}
    corners = np.array([(-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1)], np.float32) * (400.0, 1.0, 400.0) + (0.0, -1.0, 0.0)
    plane = rs.mesh_of(corners, [0, 1, 3, 1, 2, 3], material=material, uv=corners[:, [0, 2]] * 0.04, normal=(0.0, -1.0, 0.0))
    default = meshes.reference_default_scene()
    for m in default:
        m.surfaces = [(first, count, material) for first, count, _ in m.surfaces]
    scenes = {"receding_plane": [plane], "default_scene": default}
    for name, ms in scenes.items():
        for m in ms:
            m.mipmaps = config != "none"
        if config == "none":
            d.setTextureMips([])
        else:
            meshes.register_texture_mips(d, ms, abi.SZG_SAMPLER_MAX_LOD_REFERENCE if config == "full_max_lod_1" else abi.SZG_SAMPLER_MAX_LOD_NONE,
                                         max_anisotropy=ANISO.get(config, 1.0))
        out[f"gbuffer_3840x2160/{name}"] = time_it(torch, lambda: d.recordGBufferRaster(None, inp.rect, target, 0, cams, ms))
        out[f"coverage/{name}"] = float((target.depth > 0).float().mean())
    d.cleanup()
    print("RESULT " + json.dumps(out), flush=True)


def lib_chain_bytes(size):
    from syzygy_amd import lib

    return lib().szg_mip_chain_bytes(size, size)


def run_child(config, baseline=None):
    env = dict(os.environ, SZG_HIP_LIBRARY=baseline) if config.startswith("baseline_") else None
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config], env=env, capture_output=True, text=True, timeout=150)
    if p.returncode != 0:  # nothing more is started on the GPU after a failure
        print(p.stdout[-2000:], p.stderr[-3000:])
        sys.exit(f"child failed with {p.returncode} ({config})")
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline", help="another build of libszg_hip.so: 'none' and 'full' are also timed through it")
    ap.add_argument("--out")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    configs = CONFIGS + (BASELINE_CONFIGS if a.baseline else ())
    baseline = os.path.abspath(a.baseline) if a.baseline else None
    runs = {c: [] for c in configs}
    for r in range(a.rounds):
        for config in (configs if r % 2 == 0 else configs[::-1]):
            runs[config].append(run_child(config, baseline))
            print(r, config, json.dumps(runs[config][-1]), flush=True)
    generation = run_child("generate")
    print("generate", json.dumps(generation), flush=True)
    results, same_kernels = {}, {}
    for key in runs["none"][0]:
        if key.startswith("coverage/"):
            results[key] = runs["none"][0][key]
            continue
        results[key] = {}
        base = statistics.median(x[key] for x in runs["none"])
        full = statistics.median(x[key] for x in runs["full"])
        for config in configs:
            t = [x[key] for x in runs[config]]
            results[key][config] = {"ms_median": statistics.median(t), "spread_ms": max(t) - min(t), "ms": t,
                                    "delta_percent_vs_none": 100.0 * (statistics.median(t) / base - 1.0),
                                    "delta_percent_vs_full": 100.0 * (statistics.median(t) / full - 1.0)}
            print(f"{key} [{config}]: {statistics.median(t):.4f} ms (spread {max(t) - min(t):.4f}), {100.0 * (statistics.median(t) / base - 1.0):+.2f} % vs none, "
                  f"{100.0 * (statistics.median(t) / full - 1.0):+.2f} % vs full")
        # "the same kernels": with anisotropy at 1.0 the tree's median lies within the baseline's own max - min of its median
        for config in (BASELINE_CONFIGS if a.baseline else ()):
            tree, other = results[key][config[len("baseline_"):]], results[key][config]
            delta = tree["ms_median"] - other["ms_median"]
            same_kernels[f"{key} [{config[len('baseline_'):]}]"] = {"tree_ms_median": tree["ms_median"], "baseline_ms_median": other["ms_median"],
                                                                   "delta_ms": delta, "baseline_spread_ms": other["spread_ms"],
                                                                   "inside_baseline_spread": abs(delta) <= other["spread_ms"]}
            print(f"{key} [{config[len('baseline_'):]}] tree - baseline {delta:+.4f} ms, baseline spread {other['spread_ms']:.4f}")
    if a.out:
        record = {"rounds": a.rounds, "method": __doc__.split("usage:")[0].strip(), "raster": results, "generation": generation}
        if a.baseline:
            record["tree_against_baseline_at_anisotropy_1"] = same_kernels
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
