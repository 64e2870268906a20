"""Device time of the UI layer pass (include/szg/ui_layer.h) next to szg_record_oetf, in one process.

At 3840x2160 and 1920x1080, all under SZG_UI_LOAD_OP_CLEAR:
  (a) clear      no commands: the clear alone (8 B/px written)
  (b) viewport   the scene viewport quad alone, 1:1 over the whole frame (NEAREST / CLAMP_TO_BORDER; 8 B/px read + 8 written)
  (c) editor     an editor-like frame of about 5 000 triangles: background, title bar, the viewport quad, a translucent side
                 panel with rows of small widget rectangles, a frame-time graph
  (d) glyphs     50 000 small glyph-like quads (100 000 triangles) from a synthetic 512x512 atlas, LINEAR / REPEAT, laid out
                 in lines of text over the frame
and the in-place szg_record_oetf of the same extent, which also moves 16 B/px: every case is reported in ms and as a
multiple of that OETF time.

How a case is timed: as tools/bench_present.py does it (its `timed`): every case works on a ring of output images (and, where
it samples one, scene textures) larger than the 256 MiB Infinity Cache; device events surround one pass over the ring, and
windows are repeated until about --seconds of device time have been timed. ms = timed device time / calls. A call here is
one szg_ui_layer_record_draw: set-up kernel, box hierarchy and tile kernel, behind the copy of its command array.

    python tools/bench_ui_layer.py [--seconds 0.3] [--json profiles/ui_layer_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
from bench_present import RING_BYTES, noise, timed  # noqa: E402
from syzygy_amd import abi, lib, pipelines as pl, ui  # noqa: E402

WHITE, SCENE, ATLAS = "white", "scene", "atlas"


def editor_frame(w, h):
    """About 5 000 triangles in submission order: a window, then its widgets."""
    rng = np.random.default_rng(1)
    dl = ui.DrawList(WHITE)
    dl.add_rect_filled((0, 0), (w, h), ui.col32(30, 30, 34))
    dl.add_rect_filled((0, 0), (w, 24), ui.col32(41, 74, 122))
    panel = int(w * 0.22)
    dl.add_image(SCENE, (panel + 8, 32), (w - 8, h - 8), (0, 0), ((w - 16 - panel) / w, (h - 40) / h))
    dl.push_clip_rect((0, 24), (panel, h), True)
    dl.add_rect_filled((0, 24), (panel, h), ui.col32(15, 15, 15, 240))
    rows = (h - 260) // 22
    per_row = max(1, 2300 // max(rows, 1))
    for r in range(rows):  # labels and sliders: runs of small rectangles
        y = 40 + 22 * r
        x = 10.0
        for _ in range(per_row):
            ww = float(rng.integers(3, 9))
            if x + ww > panel - 8:
                break
            dl.add_rect_filled((x, y), (x + ww, y + 14), ui.col32(220, 220, 220, int(rng.integers(120, 256))))
            x += ww + 1
    for i in range(120):  # the frame-time graph
        b = float(rng.uniform(4, 90))
        dl.add_rect_filled((10 + i * 2.5, h - 20 - b), (12 + i * 2.5, h - 20), ui.col32(230, 180, 60, 200))
    dl.pop_clip_rect()
    return ui.DrawData((0, 0), (w, h), (1, 1), [dl]).flatten()


def glyph_frame(w, h, count=50000):
    """Lines of glyph-like quads, 7 x 13 px, each sampling its own cell of the atlas."""
    rng = np.random.default_rng(2)
    dl = ui.DrawList(ATLAS)
    per_line = (w - 20) // 8
    for k in range(count):
        line, col = divmod(k, per_line)
        x, y = 10 + 8 * col, 10 + 15 * (line % ((h - 20) // 15))
        cu, cv = int(rng.integers(0, 32)) / 32, int(rng.integers(0, 32)) / 32
        dl._prim_rect_uv((x, y), (x + 7, y + 13), (cu, cv), (cu + 7 / 512, cv + 13 / 512), ui.col32(235, 235, 235, 255))
    return ui.DrawData((0, 0), (w, h), (1, 1), [dl]).flatten()


class Bench:
    def __init__(self, seconds):
        self.seconds = seconds
        self.h = C.c_void_p()
        assert lib().szg_ui_layer_create(C.byref(self.h), 110000, 64, 0) == abi.SZG_OK, lib().szg_last_error()
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.white = torch.full((1, 1, 4), 255, dtype=torch.uint8, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(7)
        self.atlas = torch.randint(0, 256, (512, 512, 4), dtype=torch.uint8, device="cuda", generator=g)
        self.fixed = {WHITE: self.add(self.white, abi.SZG_FORMAT_RGBA8_UNORM, abi.SZG_FILTER_LINEAR, abi.SZG_UI_ADDRESS_REPEAT),
                      ATLAS: self.add(self.atlas, abi.SZG_FORMAT_RGBA8_UNORM, abi.SZG_FILTER_LINEAR, abi.SZG_UI_ADDRESS_REPEAT)}

    def add(self, tensor, fmt, filt, address):
        im = pl._strided_image(tensor, fmt, 4)
        out = C.c_void_p()
        assert lib().szg_ui_layer_add_texture(self.h, C.byref(im), abi.UISampler(filt, address), C.byref(out)) == abi.SZG_OK, lib().szg_last_error()
        return out.value

    def case(self, name, extent, flat, traffic=None):
        w, h = extent
        ring = max(2, -(-RING_BYTES // (w * h * 8)))
        outputs = [noise(w, h, 300 + i) for i in range(ring)]
        images = [pl._strided_image(t, abi.SZG_FORMAT_RGBA16_UNORM, 4) for t in outputs]
        uses_scene = any(c.texture == SCENE for c in flat.commands)
        scenes = [noise(w, h, 400 + i) for i in range(ring)] if uses_scene else []
        scene_handles = [self.add(t, abi.SZG_FORMAT_RGBA16_UNORM, abi.SZG_FILTER_NEAREST, abi.SZG_UI_ADDRESS_CLAMP_TO_BORDER) for t in scenes]
        d_v = torch.from_numpy(np.frombuffer(flat.vertices.tobytes() or b"\0", np.uint8).copy()).cuda()
        d_i = torch.from_numpy(np.frombuffer(np.asarray(flat.indices, np.uint16).tobytes() or b"\0", np.uint8).copy()).cuda()
        datas, keep = [], []
        for slot in range(ring):
            n = len(flat.commands)
            commands = (abi.UIDrawCmd * max(n, 1))()
            for dst, c in zip(commands, flat.commands):
                dst.clip_rect[:] = c.clip_rect
                dst.texture = scene_handles[slot] if c.texture == SCENE else self.fixed[c.texture]
                dst.vtx_offset, dst.idx_offset, dst.elem_count = c.vtx_offset, c.idx_offset, c.elem_count
            dd = abi.UIDrawData()
            dd.display_pos[:], dd.display_size[:], dd.framebuffer_scale[:] = flat.display_pos, flat.display_size, flat.framebuffer_scale
            dd.d_vertices, dd.vertex_count = d_v.data_ptr(), len(flat.vertices)
            dd.d_indices, dd.index_count = d_i.data_ptr(), len(flat.indices)
            dd.commands, dd.command_count = commands, n
            datas.append(dd)
            keep.append(commands)
        clear = (C.c_float * 4)(0.0, 0.0, 0.0, 1.0)
        area = abi.Rect(0, 0, w, h)

        def call(i):
            rc = lib().szg_ui_layer_record_draw(self.h, self.stream, C.byref(images[i]), area, abi.SZG_UI_LOAD_OP_CLEAR, clear, C.byref(datas[i]))
            assert rc == abi.SZG_OK, lib().szg_last_error()

        ms, calls = timed(call, ring, self.seconds)
        for hnd in scene_handles:
            lib().szg_ui_layer_remove_texture(self.h, C.c_void_p(hnd))
        tris = sum(min(c.elem_count, len(flat.indices) - c.idx_offset) // 3 for c in flat.commands)
        r = {"case": name, "extent": [w, h], "triangles": tris, "commands": len(flat.commands), "ring_buffers": ring, "calls": calls,
             "ms": round(ms, 5), "bytes": traffic, "tb_per_s": round(traffic / ms / 1e9, 3) if traffic else None}
        print(json.dumps(r), flush=True)
        return r

    def oetf(self, extent):
        w, h = extent
        ring = max(2, -(-RING_BYTES // (w * h * 8)))
        pristine = [noise(w, h, 100 + i) for i in range(ring)]
        work = [p.clone() for p in pristine]
        images = [pl._strided_image(t, abi.SZG_FORMAT_RGBA16_UNORM, 4) for t in work]

        def refresh():
            for a, b in zip(work, pristine):
                a.copy_(b)

        def call(i):
            assert lib().szg_record_oetf(self.stream, C.byref(images[i]), w, h, abi.SZG_OETF_SRGB) == abi.SZG_OK, lib().szg_last_error()

        ms, calls = timed(call, ring, self.seconds, refresh)
        r = {"case": f"szg_record_oetf {w}x{h} (in place, sRGB)", "extent": [w, h], "ring_buffers": ring, "calls": calls, "ms": round(ms, 5),
             "bytes": w * h * 16, "tb_per_s": round(w * h * 16 / ms / 1e9, 3)}
        print(json.dumps(r), flush=True)
        return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="device time to fill per case")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    entry.build(only_if_missing=True)
    assert torch.cuda.is_available(), "bench_ui_layer.py needs a GPU"
    bench = Bench(args.seconds)
    results = []
    for extent in ((3840, 2160), (1920, 1080)):
        w, h = extent
        tag = f"{w}x{h}"
        oetf = bench.oetf(extent)
        results.append(oetf)
        empty = ui.DrawData((0, 0), (w, h), (1, 1), []).flatten()
        quad = ui.DrawList(WHITE)
        quad.add_image(SCENE, (0, 0), (w, h))
        cases = [(f"(a) clear only {tag}", empty, w * h * 8),
                 (f"(b) scene viewport quad 1:1 {tag}", ui.DrawData((0, 0), (w, h), (1, 1), [quad]).flatten(), w * h * 16),
                 (f"(c) editor-like frame {tag}", editor_frame(w, h), None),
                 (f"(d) 50000 glyph quads {tag}", glyph_frame(w, h), None)]
        for name, flat, traffic in cases:
            r = bench.case(name, extent, flat, traffic)
            r["times_oetf"] = round(r["ms"] / oetf["ms"], 3)
            results.append(r)
    lib().szg_ui_layer_destroy(bench.h)
    out = {"seconds_per_case": args.seconds, "ring_bytes": RING_BYTES, "build_id": entry.build_id(), "source_hash": entry.source_hash("hip"),
           "device": torch.cuda.get_device_name(0), "results": results}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", args.json)


if __name__ == "__main__":
    main()
