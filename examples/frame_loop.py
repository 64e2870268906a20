#!/usr/bin/env python3
"""An engine-style frame loop over the MI355X path, in the shape of Renderer::recordDraw (renderer.cpp:278-443):

    scene tick (sun animation, mesh-instance animation)            scene.cpp:461-574
    shadow bounds -> baked atmosphere + sun / moon lights           scene.cpp:95-148, :718-737
    staged buffers (cameras, atmospheres, directional lights)       renderer.cpp:302-342
    DeferredShadingPipeline::recordDrawCommands(meshes)             shadow raster, G-buffer raster, lights
    SkyViewComputePipeline::recordDrawCommands                      transmittance LUT, sky-view LUT, composite
    --debug-lines: a box per instance + the shadow bounds, in green renderer.cpp:355-365, :417-427, :445-476
    OETF on the presented image                                     editor.cpp:303-340
    --present WxH[:format]: the blit onto a swapchain-sized image   editor.cpp:355-361 (szg/present.h), on the GPU
    --pipeline compute-collection[:NAME]: the editor's other        renderer.cpp:431-438 (szg/compute_collection.h)
      rendering pipeline instead of the deferred one
    --ui-layer: the UI draw between the scene and the OETF          editor.cpp:720-748, uilayer.cpp:513-572 (szg/ui_layer.h)
    --texture-viewer: the Texture Viewer window in that UI          editor.cpp:485-505, :684-692 (szg/texture_display.h)

    python examples/frame_loop.py --frames 60 --width 1920 --height 1080 --out /tmp/frame.ppm [--debug-lines [--line-width 2]]
                                  [--present 1280x720[:rgba8|bgra8|a2b10g10r10]]
                                  [--pipeline compute-collection[:booleanpush|gradient_color|sparse_push_constant|matrix_color]]
                                  [--ui-layer [--texture-viewer[=color|normal|orm|gbuffer-normal]]]

--pipeline mirrors the editor's "Deferred" / "Compute Collection" switch (ui/engineui.cpp:19-22). With compute-collection
the frame uploads and fills the debug-line list as before, then records ONE program of the collection over the scene colour
(default gradient_color) with a visible block (abi.COMPUTE_COLLECTION_EXAMPLE_VALUES): no shadow, G-buffer, light, atmosphere
or debug-line launches. The OETF and --present follow as in the editor.

--ui-layer builds the frame the way the editor does: the renderer draws into UILayer::sceneTexture() at the extent of the scene
viewport window, a draw list made with syzygy_amd.ui (a title bar, the scene viewport quad at the editor's UVs, a translucent
side panel, a frame-time graph of filled rectangles) is drawn by UILayer::recordDraw into the output texture, and the OETF,
--present and --out work on that OUTPUT image, as Editor::endFrame does.

--texture-viewer (with --ui-layer) adds a "Texture Viewer" panel: a small RGBA16_SFLOAT display image (the editor's is 4096^2),
into which every frame the picked texture is blitted (pipelines.TextureDisplay.select: a material map of the scene, or the
G-buffer's normal plane after the frame's raster pass) and which ui.DrawList.add_image draws in the side panel.

Without --present the 16-bit scene colour is copied to the host and the PPM holds its high bytes; with it every frame ends
with the reference's LINEAR blit onto a WxH image of the given swapchain format (default rgba8) and the PPM is that image
(maxval 255, or 1023 for a2b10g10r10).

Needs an MI355X (no CPU fallback). Everything on the GPU is enqueued on one stream; the host only ticks the scene.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--shadow-map", type=int, default=2048)
    ap.add_argument("--out", default="", help="write the last frame as a binary PPM (8 bit)")
    ap.add_argument("--debug-lines", action="store_true", help="the editor's Debug Lines switch (engineui.cpp:95-109)")
    ap.add_argument("--line-width", type=float, default=1.0)
    ap.add_argument("--present", default="", metavar="WxH[:format]",
                    help="end every frame with the blit onto a WxH swapchain image (rgba8, bgra8 or a2b10g10r10) and write --out from it")
    ap.add_argument("--pipeline", default="deferred", metavar="deferred|compute-collection[:NAME]",
                    help="the rendering pipeline of Renderer::recordDraw (renderer.cpp:379-439)")
    ap.add_argument("--mipmaps", nargs="?", const="none", default=None, metavar="MAXLOD",
                    help="build mip chains for the material textures and sample them trilinearly (szg/mipmaps.h); MAXLOD: none "
                         "(default), reference (the reference sampler's 1.0) or a number")
    ap.add_argument("--anisotropy", default=None, metavar="A",
                    help="with --mipmaps: the sampler's maxAnisotropy, 1 to 16 (szg/anisotropy.h); default off (1, the reference's)")
    ap.add_argument("--multiscatter", nargs="?", const="add", default=None, choices=("add", "only"), metavar="add|only",
                    help="multiple scattering in the sky-view LUT (szg/multiscatter_sky.h): the higher orders added to the sky, or "
                         "alone; the frame then records the multi-scattering LUT as well. Default off (the reference's single scattering)")
    ap.add_argument("--ui-layer", action="store_true",
                    help="draw an editor-like UI frame over the scene (szg/ui_layer.h) and present the UI output texture")
    ap.add_argument("--texture-viewer", nargs="?", const="color", default=None, choices=["color", "normal", "orm", "gbuffer-normal"],
                    help="with --ui-layer: a Texture Viewer panel showing a material map or the G-buffer's normal plane (szg/texture_display.h)")
    args = ap.parse_args(argv)
    if args.texture_viewer and not args.ui_layer:
        ap.error("--texture-viewer needs --ui-layer")

    import torch

    from syzygy_amd import abi, lib, meshes, pipelines as pl, scene, ui

    W, H = args.width, args.height
    try:
        pipeline, shader = pl.parse_pipeline_option(args.pipeline)
    except ValueError as e:
        ap.error(f"--pipeline {e}")
    try:
        max_lod = pl.parse_mipmaps_option(args.mipmaps) if args.mipmaps is not None else None
    except ValueError as e:
        ap.error(f"--mipmaps {e}")
    try:
        max_anisotropy = pl.parse_anisotropy_option(args.anisotropy) if args.anisotropy is not None else 1.0
    except ValueError as e:
        ap.error(f"--anisotropy {e}")
    if args.anisotropy is not None and max_lod is None:
        ap.error("--anisotropy needs --mipmaps: only maps with a mip chain are filtered anisotropically")
    # ---- scene: the editor's start-up scene, its cubes animated (editor.cpp:500-545) -----------------------------
    material = meshes.default_material()
    cv, ci = meshes.cube_mesh()
    pv, pi = meshes.plane_mesh()
    cube_bounds, plane_bounds = abi.AABB(), abi.AABB()
    lib().szg_aabb_create(abi.f3(*cv["position"].min(0)), abi.f3(*cv["position"].max(0)), C.byref(cube_bounds))
    lib().szg_aabb_create(abi.f3(*pv["position"].min(0)), abi.f3(*pv["position"].max(0)), C.byref(plane_bounds))

    def instance(vertices, indices, bounds, animation, items):
        n = len(items)
        originals = (abi.Transform * n)()
        for t, (tr, sc) in zip(originals, items):
            t.translation[:], t.eulerAnglesRadians[:], t.scale[:] = list(tr), [0.0, 0.0, 0.0], list(sc)
        return {"vertices": vertices, "indices": indices, "bounds": bounds, "animation": animation, "originals": originals,
                "transforms": (abi.Transform * n)(*originals), "models": (abi.Mat4 * n)(), "mits": (abi.Mat4 * n)(), "n": n}

    instances = [
        instance(cv, ci, cube_bounds, abi.SZG_INSTANCE_ANIMATION_SPIN_ALONG_WORLD_UP, [((0, -8, 6), (5, 5, 5))]),
        instance(cv, ci, cube_bounds, abi.SZG_INSTANCE_ANIMATION_DIAGONAL_WAVE, [((0, -8, -6), (5, 5, 5)), ((14, -6, -2), (2, 2, 2))]),
        instance(pv, pi, plane_bounds, abi.SZG_INSTANCE_ANIMATION_NONE, [((0, -1, 0), (20, 1, 20))]),
    ]
    atmosphere = scene.default_atmosphere()
    sun_animation = abi.SunAnimation()
    lib().szg_sun_animation_default(C.byref(sun_animation))
    sun_animation.time = 0.62  # afternoon, the sun behind the camera (scene.cpp:546-574)
    camera = scene.default_camera()
    # the default camera sits 2 m in front of a cube face (scene.cpp:77-83): step back and look at the scene centre
    camera.cameraPosition[:] = [-22.0, -18.0, -42.0]
    camera.eulerAngles[:] = [float(v) for v in scene.eulers_from_forward((22.0, 11.0, 42.0))]
    spots = (abi.SpotLightPacked * 2)(scene.make_spot((1, 0.2, 0.1), (-20.0, -28.0, -20.0), scene.eulers_from_forward((20.0, 20.0, 20.0))),
                                      scene.make_spot((0.1, 0.3, 1), (20.0, -28.0, -20.0), scene.eulers_from_forward((-20.0, 20.0, 20.0))))

    # ---- GPU objects ----------------------------------------------------------------------------------------------
    cameras = pl.TStagedBuffer(abi.CameraPacked, 1)
    atmospheres = pl.TStagedBuffer(abi.AtmospherePacked, 1)
    lights = pl.TStagedBuffer(abi.DirectionalLightPacked, 2)
    ui_layer = None
    if args.ui_layer:  # UILayer::create at the window's extent: scene and output texture, the scene texture registered with ImGui
        ui_layer = pl.UILayer.create((W, H))
        white = ui_layer.addTexture(torch.full((1, 1, 4), 255, dtype=torch.uint8, device="cuda"))  # the font atlas's white texel
        panel_w, title_h = max(W // 5, 8), 22
        view_min = (panel_w + 6, title_h + 6)
        ui_layer.setSceneViewportExtent(W - view_min[0] - 6, H - view_min[1] - 6)  # the "Scene Viewport" window's content
        frame_times = []
        viewer = None
        if args.texture_viewer:  # editor.cpp:485-505, with a small display image instead of TEXTURE_MAX^2
            viewer = pl.TextureDisplay(ui_layer, (256, 256))
            if args.texture_viewer != "gbuffer-normal":
                texels, viewer_srgb = material[args.texture_viewer]
                viewer_map = torch.from_numpy(np.ascontiguousarray(texels)).cuda()
    target = ui_layer.sceneTexture() if ui_layer else pl.SceneTexture(W, H)
    deferred = pl.DeferredShadingPipeline((W, H), max_spot_lights=len(spots), max_shadow_maps=2 + len(spots), shadow_map_dim=args.shadow_map)
    sky = pl.SkyViewComputePipeline.create()
    if args.multiscatter:  # recordDrawCommands then records transmittance, multi-scatter, sky-view and composite
        sky.setMultiScattering({"add": abi.SZG_MULTISCATTER_ADD, "only": abi.SZG_MULTISCATTER_ONLY}[args.multiscatter])
    rect = ui_layer.sceneViewport().renderedSubregion if ui_layer else pl.rect(W, H)  # editor.cpp:720-735: the viewport's subregion
    RW, RH = rect.width, rect.height
    debug_lines = pl.DebugLines()  # Renderer::m_debugLines, DEBUGLINES_CAPACITY vertices (renderer.hpp:103)
    debug_lines.enabled, debug_lines.lineWidth = args.debug_lines, args.line_width
    try:
        present = pl.parse_present_option(args.present) if args.present else None  # (width, height, format)
    except ValueError as e:
        ap.error(f"--present {e}")
    swapchain = pl.swapchain_image(*present) if present else None
    collection = None
    if pipeline == "compute-collection":
        collection = pl.ComputeCollectionPipeline()  # Renderer::m_genericComputePipeline
        collection.selectShaderByName(shader)
        collection.writeExampleValues()

    presented = target
    t_start = time.perf_counter()
    elapsed, dt = 0.0, 1.0 / 60.0
    for frame in range(args.frames):
        # Scene::tick
        lib().szg_scene_tick_sun(C.byref(sun_animation), C.byref(atmosphere), dt * 50.0)  # 100x speed (scene.cpp:89): a slow sunset over a few hundred frames
        scene_meshes, casters = [], []
        debug_lines.clear()  # renderer.cpp:287
        for inst in instances:
            lib().szg_tick_mesh_instance(inst["animation"], inst["originals"], inst["transforms"], inst["n"], elapsed, dt, inst["models"],
                                         inst["mits"])
            scene_meshes.append(meshes.MeshInstanced(inst["vertices"], inst["indices"], [(0, len(inst["indices"]), material)],
                                                     list(inst["models"]), mipmaps=max_lod is not None))
            casters.append(abi.ShadowCaster(inst["bounds"], inst["transforms"], inst["n"], 1, 1, 0))
            for t in inst["transforms"]:
                debug_lines.pushBox(t, inst["bounds"])  # renderer.cpp:355-365
        bounds = abi.AABB()
        lib().szg_calculate_shadow_bounds((abi.ShadowCaster * len(casters))(*casters), len(casters), C.byref(bounds))
        atm, sun, moon = scene.atmosphere_baked(atmosphere, bounds)

        # Renderer::recordDraw
        for buf, items in ((cameras, [scene.camera_packed(camera, RW / RH)]), (atmospheres, [atm]), (lights, [sun, moon])):
            buf.clearStaged()
            buf.push(items)
            buf.recordCopyToDevice()
        if pipeline == "compute-collection":  # renderer.cpp:431-438: the collection only
            collection.recordDrawCommands(None, target, rect)
        else:
            if max_lod is not None:  # the meshes of a frame are new uploads: their chains are registered with them
                meshes.register_texture_mips(deferred, scene_meshes, max_lod, max_anisotropy=max_anisotropy)
            deferred.recordDrawCommandsMeshes(None, rect, target, 1, lights, spots, 0, cameras, scene_meshes)
            sky.recordDrawCommands(None, target, rect, deferred.gbuffer(), deferred.shadowMaps(), 0, atmospheres, 0, cameras, 0, lights)
            debug_lines.pushBox(tuple(bounds.center), (0.0, 0.0, 0.0, 1.0), tuple(bounds.half_extent))  # renderer.cpp:417-423
            debug_lines.recordDraw(None, 0, target, rect, cameras)  # renderer.cpp:425-427, :445-476 (only when enabled)
        presented = target
        if ui_layer:  # editor.cpp:736-748: the UI draw, then endFrame on uiOutput.texture
            frame_times = (frame_times + [4.0 + 10.0 * abs(np.sin(0.37 * frame))])[-60:]
            dl = ui.DrawList(white)
            dl.add_rect_filled((0, 0), (W, title_h), ui.col32(41, 74, 122, 255))  # title bar
            uv_min, uv_max = ui_layer.sceneViewportUV()
            dl.add_image(ui_layer.sceneTextureHandle(), view_min, (view_min[0] + RW, view_min[1] + RH), uv_min, uv_max)
            dl.push_clip_rect((0, title_h), (panel_w, H), True)
            dl.add_rect_filled((0, title_h), (panel_w, H), ui.col32(20, 20, 24, 230))  # side panel
            bar_w = (panel_w - 16) / 60.0
            for i, ms in enumerate(frame_times):  # frame-time graph
                x = 8 + i * bar_w
                dl.add_rect_filled((x, H - 12 - 4.0 * ms), (x + bar_w * 0.8, H - 12), ui.col32(230, 180, 60, 200))
            if viewer:  # editor.cpp:684-692 -> texturedisplay.cpp:164-195, :291-304
                if args.texture_viewer == "gbuffer-normal":
                    viewer.select(None, deferred.gbuffer().normal, srcRegion=rect)
                else:
                    viewer.select(None, viewer_map, srgb=viewer_srgb)
                side = float(panel_w - 16)
                size = viewer.imageSize(side)
                dl.add_rect_filled((6, title_h + 6), (10 + side, title_h + 10 + size[1]), ui.col32(41, 74, 122, 255))
                dl.add_image(viewer.handle, (8, title_h + 8), (8 + size[0], title_h + 8 + size[1]))
            dl.pop_clip_rect()
            presented = ui_layer.recordDraw(None, ui.DrawData((0, 0), (W, H), (1, 1), [dl])).texture
        pl.recordOETF(None, presented, W, H)
        if present:  # editor.cpp:355-361: the whole presented image onto the whole swapchain image, LINEAR
            pl.record_copy_image_to_image(None, presented, swapchain, dstFormat=present[2])
        elapsed += dt
    torch.cuda.synchronize()
    wall = time.perf_counter() - t_start
    image = presented.color_numpy()
    print(f"{args.frames} frames of {W}x{H}: {wall / args.frames * 1e3:.2f} ms per frame including host scene prep; "
          f"mean display value {image[..., :3].mean() / 65535.0:.3f}")
    if args.out and present:
        pl.write_presented_ppm(args.out, swapchain.cpu().numpy(), present[2])
        print("wrote", args.out, f"({present[0]}x{present[1]}, presented on the GPU)")
    elif args.out:
        with open(args.out, "wb") as f:
            f.write(f"P6 {W} {H} 255\n".encode())
            f.write((image[..., :3] >> 8).astype(np.uint8).tobytes())
        print("wrote", args.out)
    if args.debug_lines:
        print(f"debug lines: {debug_lines.lastFrameDrawResults.verticesDrawn // 2} lines, width {debug_lines.lineWidth}")
    if ui_layer:
        if viewer:
            viewer.cleanup()
        ui_layer.cleanup()
    debug_lines.cleanup()
    deferred.cleanup()
    sky.destroy()
    return image


if __name__ == "__main__":
    main()
