// kernels_scene_fill.hip — the analytic scene (a ground plane and boxes) cast into the G-buffer and into the shadow
// maps, for gfx950: stand-ins for the reference's fixed-function raster passes.
//
//   k_gbuffer_fill : output conventions of deferred/offscreen.frag:61-79 with the
//                    raster state of renderer/pipelines/deferred.cpp:342-392
//                    (analytic ray cast instead of the fixed-function rasteriser)
//   k_shadow_prep  : per shadow-map slot, the light's projection * view and its inverse
//   k_shadow_fill  : depth of the boxes' back faces as the light sees them
//
// The two ray/box slab loops differ on purpose: k_gbuffer_fill compares and assigns, to know the entry axis, where
// k_shadow_fill takes fmaxf / fminf, and a NaN goes another way through each.

#include "szg_formats.hpp"
#include "szg_launch.hpp"
#include "szg_pixel.hpp"
#include "szg_vec.hpp"

namespace szg
{
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gbuffer_fill(szg_image depth, GBufferPtrs g, unsigned drawW, unsigned drawH,
                                                      unsigned localRows, RowMap rm,
                                                      const szg_camera_packed* __restrict__ cameras, unsigned cameraIndex,
                                                      float ground_y, float ground_half_extent, float checker_cell,
                                                      float ground_roughness, const szg_fill_box* __restrict__ boxes,
                                                      unsigned boxCount)
{
    unsigned x, y;
    pixel_of_thread(x, y);
    if (x >= drawW || y >= localRows)
    {
        return;
    }
    unsigned const gy = global_row(rm, y);
    const szg_camera_packed* cam = cameras + cameraIndex;
    M4 const inverseProjection = load_m4(cam->inverseProjection);
    M4 const rotation = load_m4(cam->rotation);
    V3 const origin = mk3(cam->position[0], cam->position[1], cam->position[2]);

    float const ndcx = (((float)x + 0.5f) / (float)drawW - 0.5f) * 2.0f;
    float const ndcy = (((float)gy + 0.5f) / (float)drawH - 0.5f) * 2.0f;
    V4 const dv = mul(inverseProjection, ndcx, ndcy, 1.0f, 1.0f);
    V4 const dw = mul(rotation, dv.x, dv.y, dv.z, dv.w);
    V3 const dir = normalize(mk3(dw.x, dw.y, dw.z));

    float best_t = 3.0e38f;
    V3 best_n = splat(0.0f);
    float best_metallic = 0.0f, best_roughness = 0.0f;
    bool hit = false;

    if (dir.y != 0.0f)
    {
        float const t = (ground_y - origin.y) / dir.y;
        if (t > 0.0f)
        {
            V3 const p = origin + t * dir;
            if (fabsf(p.x) <= ground_half_extent && fabsf(p.z) <= ground_half_extent && t < best_t)
            {
                best_t = t;
                best_n = mk3(0.0f, -1.0f, 0.0f);
                best_metallic = 0.0f;
                best_roughness = ground_roughness;
                hit = true;
            }
        }
    }
    float const o[3] = {origin.x, origin.y, origin.z};
    float const d[3] = {dir.x, dir.y, dir.z};
    for (unsigned b = 0; b < boxCount; b++)
    {
        szg_fill_box const box = boxes[b];
        float tmin = -3.0e38f, tmax = 3.0e38f;
        int axis_min = 0;
        float sign_min = 0.0f;
        bool miss = false;
#pragma unroll
        for (int ax = 0; ax < 3; ax++)
        {
            float const lo = box.center[ax] - box.half_extent[ax];
            float const hi = box.center[ax] + box.half_extent[ax];
            if (d[ax] == 0.0f)
            {
                if (o[ax] < lo || o[ax] > hi)
                {
                    miss = true;
                }
                continue;
            }
            float t0 = (lo - o[ax]) / d[ax];
            float t1 = (hi - o[ax]) / d[ax];
            float s = -1.0f;
            if (t0 > t1)
            {
                float const tmp = t0;
                t0 = t1;
                t1 = tmp;
                s = 1.0f;
            }
            if (t0 > tmin)
            {
                tmin = t0;
                axis_min = ax;
                sign_min = s;
            }
            if (t1 < tmax)
            {
                tmax = t1;
            }
        }
        if (miss || tmin > tmax || tmin <= 0.0f)
        {
            continue;
        }
        if (tmin < best_t)
        {
            best_t = tmin;
            best_n = mk3(axis_min == 0 ? sign_min : 0.0f, axis_min == 1 ? sign_min : 0.0f, axis_min == 2 ? sign_min : 0.0f);
            best_metallic = box.metallic;
            best_roughness = box.roughness;
            hit = true;
        }
    }

    float depthOut = 0.0f;
    float4 pos4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint2 nrm = pack_half4(0.0f, 0.0f, 0.0f, 0.0f), dif = nrm, orm = nrm;
    if (hit)
    {
        V3 const p = origin + best_t * dir;
        M4 const projection = load_m4(cam->projection);
        M4 const view = load_m4(cam->view);
        V4 const pv = mul(view, p.x, p.y, p.z, 1.0f);
        V4 const clip = mul(projection, pv.x, pv.y, pv.z, pv.w);
        float const dz = clip.z / clip.w;
        if (dz > 0.0f && dz <= 1.0f)
        {
            depthOut = dz;
            float const cx = floorf(p.x / checker_cell), cy = floorf(p.y / checker_cell), cz = floorf(p.z / checker_cell);
            float const s = cx + cy + cz;
            bool const light = (s - 2.0f * floorf(s * 0.5f)) == 0.0f;
            float const grey = light ? (200.0f / 255.0f) : (100.0f / 255.0f);
            pos4 = make_float4(p.x, p.y, p.z, 1.0f);
            nrm = pack_half4(best_n.x, best_n.y, best_n.z, 0.0f);
            dif = pack_half4(grey, grey, grey, 1.0f);
            orm = pack_half4(1.0f, best_roughness, best_metallic, 1.0f);
        }
    }
    row_ptr<uint2>(g.diffuse, y)[x] = dif;
    row_ptr<uint2>(g.specular, y)[x] = dif;
    row_ptr<uint2>(g.normal, y)[x] = nrm;
    row_ptr<uint2>(g.orm, y)[x] = orm;
    row_ptr<float4>(g.position, y)[x] = pos4;
    row_ptr<float>(depth, y)[x] = depthOut;
}

// ---------------------------------------------------------------------------
// Shadow-map generation for the analytic scene (abi.h szg_deferred_record_shadow_maps).
__global__ void k_shadow_prep(const szg_directional_light_packed* __restrict__ dirs, unsigned dirCount,
                              const szg_spot_light_packed* __restrict__ spots, unsigned spotCount,
                              const ShadowSlot* __restrict__ owned, unsigned slotCount, ShadowGen* __restrict__ gen)
{
    unsigned const i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= slotCount)
    {
        return;
    }
    ShadowGen g;
    g.map = nullptr;
    g.dim = g.pitchFloats = g.pad = 0u;
    M4 pv;
#pragma unroll
    for (int k = 0; k < 16; k++)
    {
        pv.m[k] = 0.0f;
    }
    if (i < dirCount + spotCount && owned[i].map != nullptr)
    {
        // light.projection * light.view (shadowpass.cpp:207-215)
        // (a host-side product in the reference: glm semantics, not the shaders' contraction rule)
        pv = (i < dirCount) ? mulGlm(load_m4(dirs[i].projection), load_m4(dirs[i].view))
                            : mulGlm(load_m4(spots[i - dirCount].projection), load_m4(spots[i - dirCount].view));
        g.map = const_cast<float*>(owned[i].map);
        g.dim = owned[i].width;
        g.pitchFloats = owned[i].pitchFloats;
    }
    M4 const inv = inverse4(pv);
#pragma unroll
    for (int k = 0; k < 16; k++)
    {
        g.projView[k] = pv.m[k];
        g.invProjView[k] = inv.m[k];
    }
    gen[i] = g;
}

__global__ __launch_bounds__(256) void k_shadow_fill(const ShadowGen* __restrict__ gen, const szg_fill_box* __restrict__ boxes,
                                                     unsigned boxCount)
{
    const ShadowGen* G = gen + blockIdx.z;
    if (G->map == nullptr)
    {
        return;
    }
    unsigned x, y;
    pixel_of_thread(x, y);
    unsigned const dim = G->dim;
    if (x >= dim || y >= dim)
    {
        return;
    }
    M4 pv, inv;
#pragma unroll
    for (int k = 0; k < 16; k++)
    {
        pv.m[k] = G->projView[k];
        inv.m[k] = G->invProjView[k];
    }
    // texel centre -> NDC (inverse of TO_TEX_COORD_MAT, shadowmap.glinl:2-7): s = 0.5 ndc + 0.5
    float const ndcx = (((float)x + 0.5f) / (float)dim) * 2.0f - 1.0f;
    float const ndcy = (((float)y + 0.5f) / (float)dim) * 2.0f - 1.0f;
    V4 const h1 = mul(inv, ndcx, ndcy, 1.0f, 1.0f); // reverse-Z: depth 1 = near plane
    V4 const h2 = mul(inv, ndcx, ndcy, 0.5f, 1.0f);
    V3 const p1 = mk3(h1.x / h1.w, h1.y / h1.w, h1.z / h1.w);
    V3 const p2 = mk3(h2.x / h2.w, h2.y / h2.w, h2.z / h2.w);
    V3 const dir = normalize(p2 - p1);
    float const o[3] = {p1.x, p1.y, p1.z};
    float const d[3] = {dir.x, dir.y, dir.z};
    float best = 0.0f; // cleared depth = far
    for (unsigned b = 0; b < boxCount; b++)
    {
        szg_fill_box const box = boxes[b];
        float tmin = -3.0e38f, tmax = 3.0e38f;
        bool miss = false;
#pragma unroll
        for (int ax = 0; ax < 3; ax++)
        {
            float const lo = box.center[ax] - box.half_extent[ax];
            float const hi = box.center[ax] + box.half_extent[ax];
            if (d[ax] == 0.0f)
            {
                if (o[ax] < lo || o[ax] > hi)
                {
                    miss = true;
                }
                continue;
            }
            float t0 = (lo - o[ax]) / d[ax];
            float t1 = (hi - o[ax]) / d[ax];
            if (t0 > t1)
            {
                float const tmp = t0;
                t0 = t1;
                t1 = tmp;
            }
            tmin = fmaxf(tmin, t0);
            tmax = fminf(tmax, t1);
        }
        if (miss || tmin > tmax || tmax <= 0.0f)
        {
            continue;
        }
        V3 const pe = p1 + tmax * dir; // back face: what front-face culling leaves (pipelines.cpp:656-659)
        V4 const clip = mul(pv, pe.x, pe.y, pe.z, 1.0f);
        float const depth = clip.z / clip.w;
        if (depth > 0.0f && depth <= 1.0f && depth >= best) // GREATER_OR_EQUAL (pipelines.cpp:661)
        {
            best = depth;
        }
    }
    G->map[(size_t)y * G->pitchFloats + x] = best;
}

// ---------------------------------------------------------------------------
hipError_t launch_gbuffer_fill(hipStream_t s, const szg_scene_texture& scene, unsigned drawW, unsigned drawH, TileArgs tile,
                               const szg_gbuffer& g, const szg_camera_packed* d_cam, unsigned camIndex, float ground_y,
                               float ground_half_extent, float checker_cell, float ground_roughness,
                               const szg_fill_box* d_boxes, unsigned boxCount)
{
    unsigned const rows = tile.local_rows;
    if (rows == 0u || drawW == 0u)
    {
        return hipSuccess;
    }
    RowMap const rm{tile.block_rows, tile.rank, tile.nranks};
    hipLaunchKernelGGL(k_gbuffer_fill, pixel_grid(drawW, rows), dim3(256), 0, s, scene.depth, gptrs(g), drawW, drawH, rows, rm, d_cam,
                       camIndex, ground_y, ground_half_extent, checker_cell, ground_roughness, d_boxes, boxCount);
    return hipGetLastError();
}

hipError_t launch_shadow_prep(hipStream_t s, const szg_directional_light_packed* d_dir, unsigned dirCount,
                              const szg_spot_light_packed* d_spot, unsigned spotCount, const ShadowSlot* d_ownedSlots,
                              unsigned slotCount, ShadowGen* d_gen)
{
    if (slotCount == 0u)
    {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_shadow_prep, dim3((slotCount + 63u) / 64u), dim3(64), 0, s, d_dir, dirCount, d_spot, spotCount, d_ownedSlots,
                       slotCount, d_gen);
    return hipGetLastError();
}

hipError_t launch_shadow_maps(hipStream_t s, const szg_directional_light_packed* d_dir, unsigned dirCount,
                              const szg_spot_light_packed* d_spot, unsigned spotCount, const ShadowSlot* d_ownedSlots,
                              unsigned slotCount, ShadowGen* d_gen, const szg_fill_box* d_boxes, unsigned boxCount, unsigned maxDim)
{
    if (slotCount == 0u || maxDim == 0u)
    {
        return hipSuccess;
    }
    hipError_t const e = launch_shadow_prep(s, d_dir, dirCount, d_spot, spotCount, d_ownedSlots, slotCount, d_gen);
    if (e != hipSuccess)
    {
        return e;
    }
    hipLaunchKernelGGL(k_shadow_fill, pixel_grid(maxDim, maxDim, slotCount), dim3(256), 0, s, d_gen, d_boxes, boxCount);
    return hipGetLastError();
}
} // namespace szg

