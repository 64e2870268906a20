#!/usr/bin/env python3
"""Load a glTF 2.0 / GLB file the way AssetLibrary::loadGLTFFromPath does (include/szg/assets.h) and render it through the
whole path: shadow raster, G-buffer raster, lights, transmittance + sky-view LUTs, composite, OETF.

    python examples/render_gltf.py [model.glb | model.gltf] --out /tmp/gltf.ppm [--embedded-images]
                                   [--present 1920x1080[:rgba8|bgra8|a2b10g10r10]]
                                   [--pipeline compute-collection[:booleanpush|gradient_color|sparse_push_constant|matrix_color]]

--pipeline compute-collection[:NAME] records the editor's other rendering pipeline (renderer.cpp:431-438,
include/szg/compute_collection.h) over the scene colour instead of the deferred frame: one program of the collection
(default gradient_color) with a visible block; the asset is still loaded and uploaded. The OETF and --present follow.

--present ends the frame as the reference's editor does (editor.cpp:355-361, include/szg/present.h): the scene colour is
blitted on the GPU, LINEAR, onto a swapchain-sized image of the given format, and --out is written from that image.

Without a file a textured sphere is written first (the reference's own assets/sphere.glb is a git-LFS pointer in this
checkout). Meshes are scaled to 8 m and set on the editor's floor plane. Needs an MI355X (no CPU fallback).
"""
import argparse
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def write_sphere(path):
    from tests import gltf_writer as gw  # the test suite's independent encoder

    pos, nrm, uv, idx = gw.uv_sphere(32, 64)
    b = gw.GltfBuilder()
    y, x = np.mgrid[0:128, 0:256]
    stripes = ((x // 16 + y // 16) % 2).astype(np.uint8)
    color = np.stack([80 + 150 * stripes, 60 + 40 * stripes, 200 - 150 * stripes, np.full_like(stripes, 255)], -1).astype(np.uint8)
    bump = np.stack([127 + 50 * np.sin(x / 2.0), 127 + 50 * np.sin(y / 2.0), np.full(x.shape, 235.0), np.zeros(x.shape)], -1).astype(np.uint8)
    orm = np.zeros((2, 2, 4), np.uint8)
    orm[..., 1], orm[..., 2] = 90, 255  # glossy metal
    textures = [b.texture(b.image_uri(gw.data_uri_png(gw.png_rgba8(t)))) for t in (color, bump, orm)]
    b.doc["materials"] = [{"name": "striped", "pbrMetallicRoughness": {"baseColorTexture": {"index": textures[0]},
                                                                       "metallicRoughnessTexture": {"index": textures[2]}},
                           "normalTexture": {"index": textures[1]}}]
    b.doc["meshes"] = [{"name": "Sphere", "primitives": [{"attributes": {"POSITION": b.accessor(pos), "NORMAL": b.accessor(nrm),
                                                                        "TEXCOORD_0": b.accessor(uv)},
                                                          "indices": b.accessor(idx.astype(np.uint16)), "material": 0}]}]
    with open(path, "wb") as f:
        f.write(b.glb())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?", default="")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--out", default="")
    ap.add_argument("--embedded-images", action="store_true", help="also decode images stored in GLB buffer views (the reference does not)")
    ap.add_argument("--present", default="", metavar="WxH[:format]",
                    help="blit the frame onto a WxH swapchain image (rgba8, bgra8 or a2b10g10r10) on the GPU and write --out from it")
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
    ap.add_argument("--jpeg", nargs="?", const="host", default=None, choices=("host", "device"), metavar="host|device",
                    help="decode JPEG material maps (szg/jpeg.h; default: PNG only, as before): on the host, or the entropy decode on "
                         "the host and IDCT, upsampling and colour conversion on the GPU")
    args = ap.parse_args(argv)

    import torch

    from syzygy_amd import abi, assets, lib, meshes, pipelines as pl, scene

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

    path = args.path
    if not path:
        path = os.path.join(tempfile.mkdtemp(), "sphere.glb")
        write_sphere(path)
    flags = abi.SZG_GLTF_DECODE_BUFFER_VIEW_IMAGES if args.embedded_images else 0
    flags |= {None: 0, "host": abi.SZG_GLTF_DECODE_JPEG, "device": abi.SZG_GLTF_JPEG_FOR_DEVICE}[args.jpeg]
    asset = assets.load_gltf(path, flags)
    for line in asset.warnings:
        print("[warning]", line)
    print(f"{path}: {len(asset.meshes)} meshes, {len(asset.materials)} materials")
    if not asset.meshes:
        raise SystemExit("nothing to render")

    # every mesh scaled to 8 m and set on the floor (y = -1, +y down), side by side
    scene_meshes, casters, keep = [], [], []
    for k, m in enumerate(asset.meshes):
        centre, half = m.bounds
        s = 4.0 / max(float(half.max()), 1e-6)
        x = (k - (len(asset.meshes) - 1) / 2.0) * 10.0
        tr = abi.Transform()
        tr.translation[:] = [x - s * float(centre[0]), -1.0 - s * float(centre[1] + half[1]), -s * float(centre[2])]
        tr.eulerAnglesRadians[:] = [0.0, 0.0, 0.0]
        tr.scale[:] = [s, s, s]
        model = meshes.transform_matrix(tuple(tr.translation), (0, 0, 0), (s, s, s))
        scene_meshes.append(asset.instanced(k, [model]))
        bounds = abi.AABB()
        bounds.center[:], bounds.half_extent[:] = [float(v) for v in centre], [float(v) for v in half]
        transforms = (abi.Transform * 1)(tr)
        keep.append(transforms)
        casters.append(abi.ShadowCaster(bounds, transforms, 1, 1, 1, 0))
        print(f"  {m.name}: {len(m.vertices)} vertices, {len(m.indices) // 3} triangles, {len(m.surfaces)} surfaces")
    floor = meshes.reference_default_scene()[2]
    scene_meshes.append(floor)

    W, H = args.width, args.height
    atmosphere = scene.default_atmosphere()
    sun_animation = abi.SunAnimation()
    lib().szg_sun_animation_default(C.byref(sun_animation))
    sun_animation.time = 0.62
    lib().szg_scene_tick_sun(C.byref(sun_animation), C.byref(atmosphere), 0.0)
    camera = scene.default_camera()
    camera.cameraPosition[:] = [-9.0, -9.0, -16.0]
    camera.eulerAngles[:] = [float(v) for v in scene.eulers_from_forward((9.0, 4.0, 16.0))]
    shadow_bounds = abi.AABB()
    lib().szg_calculate_shadow_bounds((abi.ShadowCaster * len(casters))(*casters), len(casters), C.byref(shadow_bounds))
    atm, sun, moon = scene.atmosphere_baked(atmosphere, shadow_bounds)
    spots = (abi.SpotLightPacked * 1)(scene.make_spot((1.0, 0.9, 0.7), (10.0, -14.0, -10.0), scene.eulers_from_forward((-10.0, 10.0, 10.0))))

    cameras = pl.TStagedBuffer(abi.CameraPacked, 1)
    atmospheres = pl.TStagedBuffer(abi.AtmospherePacked, 1)
    lights = pl.TStagedBuffer(abi.DirectionalLightPacked, 2)
    for buf, items in ((cameras, [scene.camera_packed(camera, W / H)]), (atmospheres, [atm]), (lights, [sun, moon])):
        buf.push(items)
        buf.recordCopyToDevice()
    target = pl.SceneTexture(W, H)
    deferred = pl.DeferredShadingPipeline((W, H), max_spot_lights=1, max_shadow_maps=3, shadow_map_dim=2048)
    sky = pl.SkyViewComputePipeline.create()
    if args.multiscatter:  # recordDrawCommands then records transmittance, multi-scatter, sky-view and composite
        sky.setMultiScattering({"add": abi.SZG_MULTISCATTER_ADD, "only": abi.SZG_MULTISCATTER_ONLY}[args.multiscatter])
    rect = pl.rect(W, H)
    if pipeline == "compute-collection":  # renderer.cpp:431-438: the collection only
        collection = pl.ComputeCollectionPipeline()
        collection.selectShaderByName(shader)
        collection.writeExampleValues()
        collection.recordDrawCommands(None, target, rect)
    else:
        if max_lod is not None:
            for m in scene_meshes:
                m.mipmaps = True  # chains are built with the upload, or now for a mesh that is already on the device
            count = meshes.register_texture_mips(deferred, scene_meshes, max_lod, max_anisotropy=max_anisotropy)
            print(f"mip chains for {count} textures, max_lod {max_lod:g}, max_anisotropy {max_anisotropy:g}")
        deferred.recordDrawCommandsMeshes(None, rect, target, 1, lights, spots, 0, cameras, scene_meshes)
        sky.recordDrawCommands(None, target, rect, deferred.gbuffer(), deferred.shadowMaps(), 0, atmospheres, 0, cameras, 0, lights)
    pl.recordOETF(None, target, W, H)
    try:
        present = pl.parse_present_option(args.present) if args.present else None  # (width, height, format)
    except ValueError as e:
        ap.error(f"--present {e}")
    if present:
        swapchain = pl.swapchain_image(*present)
        pl.record_copy_image_to_image(None, target, swapchain, dstFormat=present[2])
    torch.cuda.synchronize()
    image = target.color_numpy()
    covered = float((target.depth.cpu().numpy() > 0).mean())
    print(f"rendered {W}x{H}: geometry covers {covered:.1%} of the frame, mean display value {image[..., :3].mean() / 65535.0:.3f}")
    if args.out and present:
        pl.write_presented_ppm(args.out, swapchain.cpu().numpy(), present[2])
        print("wrote", args.out, f"({present[0]}x{present[1]}, presented on the GPU)")
    elif args.out:
        with open(args.out, "wb") as f:
            f.write(f"P6 {W} {H} 255\n".encode())
            f.write((image[..., :3] >> 8).astype(np.uint8).tobytes())
        print("wrote", args.out)
    deferred.cleanup()
    sky.destroy()
    return image, covered


if __name__ == "__main__":
    main()
