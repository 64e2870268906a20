"""The light records of k_light_prep as the tile cull sees them, and the per-pixel early-out of the light loop, in numpy float32
(syzygy_amd/csrc/szg_light_tiles.hpp: LightCull, pairCull). For tests/test_lights_tile_bounds.py, which hands the records to
the native program, and tests/test_gpu_lights_tile_masks.py, which holds the mask words of a frame against the early-out."""
import numpy as np

from syzygy_amd import abi, scene

F = np.float32
# shadowmap.glinl:2-7, indexed [row, col]
TO_TEX = np.array([[0.5, 0, 0, 0.5], [0, 0.5, 0, 0.5], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=F)
# tests/lights_tiles/light_tile_bounds.cpp struct Rec: rx[4] ry[4] rw[4] position[3] falloffBound isSpot flags
REC = np.dtype([("rx", F, 4), ("ry", F, 4), ("rw", F, 4), ("position", F, 3), ("falloffBound", F), ("isSpot", np.uint32),
                ("flags", np.uint32)])
assert REC.itemsize == 72


def matmul32(a, b):
    """4x4 product with every product and sum rounded to float32 (last-bit differences from k_light_prep's order of sums do
    not matter to either test: a cleared bit leaves 1 % between the thresholds 0.51 and 0.505)."""
    out = np.zeros((4, 4), dtype=F)
    for k in range(4):
        out = (out + np.outer(a[:, k], b[k, :]).astype(F)).astype(F)
    return out


def spot_records(spots, count, flags=1):
    """One REC per spot light: rows x, y, w of TO_TEX * projection * view, position, falloffFactor / falloffDistance^2."""
    recs = np.zeros(count, dtype=REC)
    for i in range(count):
        s = spots[i]
        m = matmul32(TO_TEX, matmul32(s.projection.to_numpy(), s.view.to_numpy()))
        recs[i]["rx"], recs[i]["ry"], recs[i]["rw"] = m[0], m[1], m[3]
        recs[i]["position"] = np.array(s.position[:3], dtype=F)
        recs[i]["falloffBound"] = F(s.falloffFactor) * (F(1.0) / F(s.falloffDistance)) * (F(1.0) / F(s.falloffDistance))
        recs[i]["isSpot"] = 1
        recs[i]["flags"] = flags
    return recs


def perturbed_ring(count, seed):
    """scene.spot_ring's lights with their positions moved by up to 6 units and their axes turned by up to ~20 degrees."""
    rng = np.random.default_rng(seed)
    ring = scene.spot_ring(count)
    out = (abi.SpotLightPacked * count)()
    for i in range(count):
        position = np.array(ring[i].position[:3]) + rng.uniform(-6.0, 6.0, 3)
        forward = np.array(ring[i].forward[:3]) + rng.uniform(-0.35, 0.35, 3)
        forward /= np.linalg.norm(forward)
        out[i] = scene.make_spot(tuple(ring[i].color[:3]), tuple(position), scene.eulers_from_forward(tuple(forward)))
    return out


def pair_skip(rec, positions):
    """pairCull(...).skip of one record for an array [..., 3] of float32 positions, operation by operation in float32 (d^2 in
    float64: its fused sums only matter within an ulp of the 2^-28 guard)."""
    p = positions.astype(F)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]

    def row(r):
        return ((r[0] * x + r[1] * y).astype(F) + r[2] * z).astype(F) + r[3]

    with np.errstate(all="ignore"):
        cx, cy, cw = row(rec["rx"]), row(rec["ry"]), row(rec["rw"])
        t = rec["position"].astype(F) - p
        d2 = (t.astype(np.float64) ** 2).sum(axis=-1).astype(F)
        away = rec["falloffBound"] * d2 >= F(2.0 ** -28)
        acw = np.abs(cw)
        ax, ay = np.abs(cx - F(0.5) * cw), np.abs(cy - F(0.5) * cw)
        outside = (acw > 0) & ((ax > F(0.505) * acw) | (ay > F(0.505) * acw))
    return bool(rec["isSpot"]) & bool(rec["flags"] & 1) & away & outside
