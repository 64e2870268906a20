"""Raster record times of two builds of libszg_hip.so against each other (e.g. a parent commit's library and the tree's):
the libraries are alternated within one call, a fresh process per library and round (SZG_HIP_LIBRARY), HIP events around 20
records after 3 warm-up records; medians over the rounds, each library's own max - min spread beside them.
usage: python tools/bench_raster_libraries.py --baseline PATH/libszg_hip.so [--rounds 5] [--out profiles/NAME.json]
Scenes at 3840x2160 (G-buffer) and two 2048^2 shadow maps: the reference's default scene, the analytic scene as meshes, a soup
of 4000 triangles, and a pixel-aligned lattice (every 16th pixel centre a vertex: the worst case for exact edge signs)."""
import argparse, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child():
    import torch
    from tests import util
    from tests.test_raster import _soup
    from tests import raster_scenes as rs
    from syzygy_amd import meshes, abi, pipelines as pl

    def time_it(fn, reps=20):
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

    out = {}
    W, H = 3840, 2160
    inp = util.Inputs(W, H, elevation_degrees=40.0, spots=1)
    cams = pl.TStagedBuffer(abi.CameraPacked, 1); cams.push(inp.cam); cams.recordCopyToDevice()
    icam = pl.TStagedBuffer(abi.CameraPacked, 1); icam.push(rs.identity_camera()); icam.recordCopyToDevice()
    target = pl.SceneTexture(W, H)
    d = pl.DeferredShadingPipeline((W, H), max_spot_lights=1, max_shadow_maps=2, shadow_map_dim=2048)
    lights = pl.TStagedBuffer(abi.DirectionalLightPacked, 2); lights.push([inp.sun, inp.moon]); lights.recordCopyToDevice()
    pos, idx = rs.lattice(W, H, 16, "w1")
    scenes = {"default_scene_26": meshes.reference_default_scene(), "fill_scene_290": meshes.meshes_of_fill_scene(inp.synthetic.fill),
              "soup_4000": _soup(1, 1000), "aligned_lattice_%d" % (len(idx) // 3): [rs.mesh_of(pos, idx)]}
    for name, ms in scenes.items():
        c = icam if name.startswith("aligned") else cams
        out["gbuffer_3840x2160/" + name] = time_it(lambda: d.recordGBufferRaster(None, inp.rect, target, 0, c, ms))
        if not name.startswith("aligned"):
            out["shadow_2x2048/" + name] = time_it(lambda: d.recordShadowRaster(None, lights, None, ms))
    d.cleanup()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    libs = {"baseline": os.path.abspath(a.baseline), "tree": os.path.join(ROOT, "syzygy_amd", "csrc", "libszg_hip.so")}
    runs = {k: [] for k in libs}
    for r in range(a.rounds):
        for name in (("baseline", "tree") if r % 2 == 0 else ("tree", "baseline")):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, SZG_HIP_LIBRARY=libs[name]),
                               capture_output=True, text=True, timeout=150)
            if p.returncode != 0:  # nothing more is started on the GPU after a failure
                print(p.stdout[-2000:], p.stderr[-3000:])
                sys.exit(f"child failed with {p.returncode} ({name})")
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[7:]))
            print(r, name, line[7:], flush=True)
    results = {}
    for key in runs["baseline"][0]:
        b, t = [x[key] for x in runs["baseline"]], [x[key] for x in runs["tree"]]
        mb, mt = statistics.median(b), statistics.median(t)
        results[key] = {"baseline_ms_median": mb, "tree_ms_median": mt, "baseline_spread_ms": max(b) - min(b), "tree_spread_ms": max(t) - min(t),
                        "delta_ms": mt - mb, "delta_percent": 100.0 * (mt / mb - 1.0), "baseline_ms": b, "tree_ms": t}
        print(f"{key}: baseline {mb:.4f} ms (spread {max(b) - min(b):.4f}), tree {mt:.4f} ms (spread {max(t) - min(t):.4f}), delta {100.0 * (mt / mb - 1.0):+.2f} %")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"rounds": a.rounds, "method": __doc__.split("usage:")[0].strip(), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
