// api_deferred.cpp — DeferredShadingPipeline behind the C-ABI (include/szg/abi.h): renderer/pipelines/deferred.cpp:145-337, :435-792.

#include <new>

#include "api_common.hpp"
#include "szg/light_tiles.h"
#include "szg_light_tiles.hpp"

using namespace szg;

extern "C" {

// ---------------------------------------------------------------------------
// DeferredShadingPipeline
// ---------------------------------------------------------------------------
int szg_deferred_create(szg_deferred_t** out, const szg_deferred_desc* desc, int device)
{
    if (out == nullptr || desc == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_create: NULL argument");
    }
    *out = nullptr;
    if (desc->capacity_width == 0u || desc->capacity_height == 0u || desc->capacity_width > 32768u ||
        desc->capacity_height > 32768u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_create: capacity %ux%u out of range", desc->capacity_width,
                    desc->capacity_height);
    }
    if (desc->max_spot_lights > 65536u || desc->max_shadow_maps > 65536u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_create: light/shadow capacity out of range");
    }
    SZG_TRY_RC(select_device(device));
    szg_deferred* p = new (std::nothrow) szg_deferred();
    if (p == nullptr)
    {
        return fail(SZG_ERR_OUT_OF_MEMORY, "szg_deferred_create: host allocation failed");
    }
    p->device = device;
    p->desc = *desc;
    unsigned const W = desc->capacity_width, H = desc->capacity_height;
    unsigned const fmts[5] = {SZG_FORMAT_RGBA16_SFLOAT, SZG_FORMAT_RGBA16_SFLOAT, SZG_FORMAT_RGBA16_SFLOAT,
                              SZG_FORMAT_RGBA32_SFLOAT, SZG_FORMAT_RGBA16_SFLOAT};
#define SZG_TRY(expr) SZG_HIP_OR(expr, szg_deferred_destroy(p), "szg_deferred_create: device allocation")
    for (int i = 0; i < 5; i++)
    {
        // attachments are cleared to 0 at the start of every G-buffer pass (deferred.cpp:493-560)
        SZG_TRY(p->d_gbufferPlanes[i].alloc((size_t)W * H * texel_bytes(fmts[i]), true));
    }
    unsigned const nSpots = desc->max_spot_lights > 0u ? desc->max_spot_lights : 1u;
    unsigned const nSlots = desc->max_shadow_maps > 0u ? desc->max_shadow_maps : 1u;
    SZG_TRY(p->d_spots.alloc(nSpots));
    SZG_TRY(p->d_slots.alloc(nSlots, true));
    SZG_TRY(p->d_lightRecs.alloc((size_t)nSpots + p->maxDirectional));
    // written in full by k_light_tiles before k_lights reads it: no clear
    SZG_TRY(p->d_lightTileMasks.alloc(lightTileMaskWords(W, H, (size_t)nSpots + p->maxDirectional)));
    SZG_TRY(p->d_boxes.alloc(p->maxBoxes));
    SZG_TRY(p->d_ownedSlots.alloc(nSlots, true));
    SZG_TRY(p->d_shadowGen.alloc(nSlots));
    p->shadowImages.assign(desc->max_shadow_maps, szg_image{nullptr, 0u, 0u, 0u, SZG_FORMAT_D32_SFLOAT});
    if (desc->shadow_map_dim > 0u && desc->max_shadow_maps > 0u)
    {
        // D32F array, cleared to 0 = far = unoccluded (shadowpass.cpp:188-248). Producing the
        // depth (triangle raster) is outside this path.
        size_t const one = (size_t)desc->shadow_map_dim * desc->shadow_map_dim * 4u;
        SZG_TRY(p->d_ownedShadowMaps.alloc(one * desc->max_shadow_maps, true));
        std::vector<ShadowSlot> owned(desc->max_shadow_maps);
        for (unsigned i = 0; i < desc->max_shadow_maps; i++)
        {
            p->shadowImages[i] = make_image(static_cast<unsigned char*>(p->d_ownedShadowMaps.get()) + one * i, desc->shadow_map_dim,
                                            desc->shadow_map_dim, SZG_FORMAT_D32_SFLOAT);
            owned[i] = ShadowSlot{static_cast<const float*>(p->shadowImages[i].data), desc->shadow_map_dim,
                                  desc->shadow_map_dim, desc->shadow_map_dim, 0u};
        }
        SZG_TRY(hipMemcpy(p->d_ownedSlots, owned.data(), owned.size() * sizeof(ShadowSlot), hipMemcpyHostToDevice));
        // from pageable memory the call may return when the source has been staged, before the device holds it; the
        // first record call may come on a non-blocking stream, which does not wait for the null stream
        SZG_TRY(hipStreamSynchronize(nullptr));
    }
#undef SZG_TRY
    size_t stagingBytes = (size_t)nSpots * sizeof(szg_spot_light_packed);
    if ((size_t)nSlots * sizeof(szg::ShadowSlot) > stagingBytes)
    {
        stagingBytes = (size_t)nSlots * sizeof(szg::ShadowSlot);
    }
    if ((size_t)p->maxBoxes * sizeof(szg_fill_box) > stagingBytes)
    {
        stagingBytes = (size_t)p->maxBoxes * sizeof(szg_fill_box);
    }
    int const src = p->staging.init(stagingBytes);
    if (src != SZG_OK)
    {
        szg_deferred_destroy(p);
        return src;
    }
    p->gbuffer.diffuse = make_image(p->d_gbufferPlanes[0], W, H, SZG_FORMAT_RGBA16_SFLOAT);
    p->gbuffer.specular = make_image(p->d_gbufferPlanes[1], W, H, SZG_FORMAT_RGBA16_SFLOAT);
    p->gbuffer.normal = make_image(p->d_gbufferPlanes[2], W, H, SZG_FORMAT_RGBA16_SFLOAT);
    p->gbuffer.worldPosition = make_image(p->d_gbufferPlanes[3], W, H, SZG_FORMAT_RGBA32_SFLOAT);
    p->gbuffer.occlusionRoughnessMetallic = make_image(p->d_gbufferPlanes[4], W, H, SZG_FORMAT_RGBA16_SFLOAT);
    p->shadowMaps.count = desc->max_shadow_maps;
    p->shadowMaps.padding = 0;
    p->shadowMaps.maps = p->shadowImages.empty() ? nullptr : p->shadowImages.data();
    *out = p;
    return SZG_OK;
}

void szg_deferred_destroy(szg_deferred_t* p)
{
    if (p == nullptr)
    {
        return;
    }
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    delete p;
}

const szg_gbuffer* szg_deferred_gbuffer(szg_deferred_t* p) { return p != nullptr ? &p->gbuffer : nullptr; }
const szg_shadowmaps* szg_deferred_shadow_maps(szg_deferred_t* p) { return p != nullptr ? &p->shadowMaps : nullptr; }

int szg_deferred_set_shadow_map(szg_deferred_t* p, uint32_t index, const szg_image* map)
{
    if (p == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_shadow_map: NULL pipeline");
    }
    if (index >= p->shadowImages.size())
    {
        return fail(SZG_ERR_CAPACITY, "szg_deferred_set_shadow_map: slot %u >= capacity %zu", index, p->shadowImages.size());
    }
    if (map == nullptr || map->data == nullptr)
    {
        p->shadowImages[index] = szg_image{nullptr, 0u, 0u, 0u, SZG_FORMAT_D32_SFLOAT};
        return SZG_OK;
    }
    if (!check_image(*map, SZG_FORMAT_D32_SFLOAT, 1u, 1u, "shadow map"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    p->shadowImages[index] = *map;
    return SZG_OK;
}

int szg_deferred_get_configuration(const szg_deferred_t* p, szg_deferred_configuration* out)
{
    if (p == nullptr || out == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_get_configuration: NULL argument");
    }
    *out = p->config;
    return SZG_OK;
}

int szg_deferred_set_configuration(szg_deferred_t* p, const szg_deferred_configuration* cfg)
{
    if (p == nullptr || cfg == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_configuration: NULL argument");
    }
    p->config = *cfg;
    return SZG_OK;
}

int szg_deferred_record_gbuffer_fill(szg_deferred_t* p, void* stream, szg_rect draw_rect, const szg_rowtile* tile,
                                     const szg_scene_texture* scene_texture, uint32_t view_camera_index,
                                     const szg_camera_packed* d_cameras, const szg_fill_scene* geometry)
{
    if (p == nullptr || d_cameras == nullptr || geometry == nullptr || scene_texture == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_record_gbuffer_fill: NULL argument");
    }
    if (!check_rect(draw_rect, "szg_deferred_record_gbuffer_fill"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    DeviceGuard const guard(p->device);
    if (draw_rect.width == 0u || draw_rect.height == 0u)
    {
        return SZG_OK;
    }
    szg::TileArgs t{};
    if (!resolve_tile(tile, draw_rect.height, t))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    // the whole scene texture, not only the depth this pass writes: the lights pass of the same frame would refuse it
    if (!check_gbuffer(&p->gbuffer, draw_rect.width, t.local_rows) || !check_scene(scene_texture, draw_rect.width, t.local_rows, true))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    if (geometry->box_count > p->maxBoxes || (geometry->box_count > 0u && geometry->boxes == nullptr))
    {
        return fail(SZG_ERR_CAPACITY, "szg_deferred_record_gbuffer_fill: %u boxes (capacity %u)", geometry->box_count, p->maxBoxes);
    }
    if (!(geometry->checker_cell > 0.0f))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_record_gbuffer_fill: checker_cell must be > 0");
    }
    hipStream_t const s = static_cast<hipStream_t>(stream);
    SZG_TRY_RC(p->staging.upload(s, p->d_boxes, geometry->boxes, (size_t)geometry->box_count * sizeof(szg_fill_box)));
    SZG_HIP(szg::launch_gbuffer_fill(s, *scene_texture, draw_rect.width, draw_rect.height, t, p->gbuffer, d_cameras,
                                     view_camera_index, geometry->ground_y, geometry->ground_half_extent, geometry->checker_cell,
                                     geometry->ground_roughness, p->d_boxes, geometry->box_count));
    return SZG_OK;
}

} // extern "C"

// Every refusal of an image or light argument of szg_deferred_record_lights, with nothing recorded, reported under the
// name of the entry point that was called: szg_deferred_record_draw_commands[_meshes] ask first, so that a frame whose lights
// pass would be refused has not already had its G-buffer and depth rewritten. (What the geometry passes refuse about
// their geometry itself - a bad checker cell, a malformed mesh table - is still found after the shadow passes, which write
// only maps the pipeline owns.)
int szg::validate_lights(const char* caller, szg_deferred_t* p, szg_rect draw_rect, const szg_rowtile* tile,
                         const szg_scene_texture* scene_texture, uint32_t atmospheric_directional_lights_count,
                         const szg_directional_light_packed* d_directional_lights, uint32_t directional_light_count,
                         const szg_spot_light_packed* h_spot_lights, uint32_t spot_light_count, const szg_camera_packed* d_cameras,
                         bool needDepth, LightsPlan* plan)
{
    if (p == nullptr || d_cameras == nullptr || scene_texture == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: NULL argument", caller);
    }
    if (!check_rect(draw_rect, caller))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    if (directional_light_count > 0u && d_directional_lights == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: directional lights NULL", caller);
    }
    if (spot_light_count > 0u && h_spot_lights == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: spot lights NULL", caller);
    }
    if (spot_light_count > p->desc.max_spot_lights)
    {
        return fail(SZG_ERR_CAPACITY, "%s: %u spot lights exceed the capacity %u", caller, spot_light_count, p->desc.max_spot_lights);
    }
    unsigned const skip = atmospheric_directional_lights_count;
    LightsPlan out{};
    out.nDir = directional_light_count > skip ? directional_light_count - skip : 0u;
    if (out.nDir > p->maxDirectional)
    {
        return fail(SZG_ERR_CAPACITY, "%s: %u directional lights exceed the capacity %u", caller, out.nDir, p->maxDirectional);
    }
    out.empty = draw_rect.width == 0u || draw_rect.height == 0u;
    if (!out.empty)
    {
        if (!resolve_tile(tile, draw_rect.height, out.tile))
        {
            return SZG_ERR_INVALID_ARGUMENT;
        }
        if (!check_scene(scene_texture, draw_rect.width, out.tile.local_rows, needDepth) ||
            !check_gbuffer(&p->gbuffer, draw_rect.width, out.tile.local_rows))
        {
            return SZG_ERR_INVALID_ARGUMENT;
        }
    }
    if (plan != nullptr)
    {
        *plan = out;
    }
    return SZG_OK;
}

extern "C" {

int szg_deferred_record_lights(szg_deferred_t* p, void* stream, szg_rect draw_rect, const szg_rowtile* tile,
                               const szg_scene_texture* scene_texture, uint32_t atmospheric_directional_lights_count,
                               const szg_directional_light_packed* d_directional_lights, uint32_t directional_light_count,
                               const szg_spot_light_packed* h_spot_lights, uint32_t spot_light_count, uint32_t view_camera_index,
                               const szg_camera_packed* d_cameras)
{
    LightsPlan plan{};
    SZG_TRY_RC(validate_lights("szg_deferred_record_lights", p, draw_rect, tile, scene_texture, atmospheric_directional_lights_count,
                               d_directional_lights, directional_light_count, h_spot_lights, spot_light_count, d_cameras, false, &plan));
    if (plan.empty)
    {
        return SZG_OK;
    }
    DeviceGuard const guard(p->device);
    unsigned const skip = atmospheric_directional_lights_count;
    unsigned const nDir = plan.nDir;
    szg::TileArgs const t = plan.tile;
    hipStream_t const s = static_cast<hipStream_t>(stream);

    // deferred.cpp:458-474: upload the spot lights to the pipeline's own buffer
    SZG_TRY_RC(p->staging.upload(s, p->d_spots, h_spot_lights, (size_t)spot_light_count * sizeof(szg_spot_light_packed)));
    // shadow-map slot table (descriptor array of shadowpass.cpp:300-340)
    unsigned const slotCount = (unsigned)p->shadowImages.size();
    if (slotCount > 0u)
    {
        std::vector<szg::ShadowSlot> slots(slotCount);
        for (unsigned i = 0; i < slotCount; i++)
        {
            const szg_image& m = p->shadowImages[i];
            slots[i] = szg::ShadowSlot{static_cast<const float*>(m.data), m.width, m.height, m.pitch_bytes / 4u, 0u};
        }
        SZG_TRY_RC(p->staging.upload(s, p->d_slots, slots.data(), slots.size() * sizeof(szg::ShadowSlot)));
    }
    SZG_HIP(szg::launch_light_prep(s, d_directional_lights, directional_light_count, skip, p->d_spots, spot_light_count, p->d_slots,
                                   slotCount, p->d_lightRecs));
    // Only spot lights can be culled: without one the tile pre-pass is not launched and k_lights visits every light.
    unsigned const lightCount = nDir + spot_light_count;
    bool const masked = spot_light_count > 0u;
    if (masked)
    {
        SZG_HIP(szg::launch_light_tiles(s, draw_rect.width, draw_rect.height, t, p->gbuffer, p->d_lightRecs, lightCount,
                                        p->d_lightTileMasks));
        p->lightTilesX = (draw_rect.width + LIGHT_TILE_DIM - 1u) / LIGHT_TILE_DIM;
        p->lightTilesY = (t.local_rows + LIGHT_TILE_DIM - 1u) / LIGHT_TILE_DIM;
        p->lightTileBatches = (lightCount + LIGHT_TILE_BATCH - 1u) / LIGHT_TILE_BATCH;
    }
    SZG_HIP(szg::launch_lights(s, *scene_texture, draw_rect.width, draw_rect.height, t, p->gbuffer, d_cameras, view_camera_index,
                               p->d_lightRecs, lightCount, masked ? p->d_lightTileMasks.get() : nullptr));
    return SZG_OK;
}

int szg_deferred_debug_light_tile_masks(szg_deferred_t* p, void* stream, uint64_t* out_words, uint64_t capacity_words,
                                        uint32_t* out_tiles_x, uint32_t* out_tiles_y, uint32_t* out_batches)
{
    if (p == nullptr || out_tiles_x == nullptr || out_tiles_y == nullptr || out_batches == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_debug_light_tile_masks: NULL argument");
    }
    *out_tiles_x = p->lightTilesX;
    *out_tiles_y = p->lightTilesY;
    *out_batches = p->lightTileBatches;
    uint64_t const words = (uint64_t)p->lightTilesX * p->lightTilesY * p->lightTileBatches;
    if (out_words == nullptr || words == 0u)
    {
        return SZG_OK;
    }
    if (capacity_words < words)
    {
        return fail(SZG_ERR_CAPACITY, "szg_deferred_debug_light_tile_masks: %llu words, room for %llu", (unsigned long long)words,
                    (unsigned long long)capacity_words);
    }
    DeviceGuard const guard(p->device);
    hipStream_t const s = static_cast<hipStream_t>(stream);
    SZG_HIP(hipMemcpyAsync(out_words, p->d_lightTileMasks.get(), words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    SZG_HIP(hipStreamSynchronize(s));
    return SZG_OK;
}

int szg_deferred_record_shadow_maps(szg_deferred_t* p, void* stream, const szg_directional_light_packed* d_directional_lights,
                                    uint32_t directional_light_count, const szg_spot_light_packed* h_spot_lights,
                                    uint32_t spot_light_count, const szg_fill_scene* geometry)
{
    if (p == nullptr || geometry == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_record_shadow_maps: NULL argument");
    }
    DeviceGuard const guard(p->device);
    if ((directional_light_count > 0u && d_directional_lights == nullptr) || (spot_light_count > 0u && h_spot_lights == nullptr))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_record_shadow_maps: light array NULL");
    }
    if (spot_light_count > p->desc.max_spot_lights)
    {
        return fail(SZG_ERR_CAPACITY, "szg_deferred_record_shadow_maps: %u spot lights exceed the capacity %u", spot_light_count,
                    p->desc.max_spot_lights);
    }
    if (geometry->box_count > p->maxBoxes || (geometry->box_count > 0u && geometry->boxes == nullptr))
    {
        return fail(SZG_ERR_CAPACITY, "szg_deferred_record_shadow_maps: %u boxes (capacity %u)", geometry->box_count, p->maxBoxes);
    }
    if (p->d_ownedShadowMaps == nullptr)
    {
        return SZG_OK; // the pipeline owns no shadow maps (shadow_map_dim == 0): nothing to render into
    }
    unsigned const lights = directional_light_count + spot_light_count;
    unsigned const slots = lights < p->desc.max_shadow_maps ? lights : p->desc.max_shadow_maps; // shadowpass.cpp:219-225
    if (slots == 0u)
    {
        return SZG_OK;
    }
    hipStream_t const s = static_cast<hipStream_t>(stream);
    SZG_TRY_RC(p->staging.upload(s, p->d_spots, h_spot_lights, (size_t)spot_light_count * sizeof(szg_spot_light_packed)));
    SZG_TRY_RC(p->staging.upload(s, p->d_boxes, geometry->boxes, (size_t)geometry->box_count * sizeof(szg_fill_box)));
    SZG_HIP(szg::launch_shadow_maps(s, d_directional_lights, directional_light_count, p->d_spots, spot_light_count, p->d_ownedSlots,
                                    slots, p->d_shadowGen, p->d_boxes, geometry->box_count, p->desc.shadow_map_dim));
    return SZG_OK;
}

int szg_deferred_record_draw_commands(szg_deferred_t* p, void* stream, szg_rect draw_rect, const szg_rowtile* tile,
                                      const szg_scene_texture* scene_texture, uint32_t atmospheric_directional_lights_count,
                                      const szg_directional_light_packed* d_directional_lights,
                                      uint32_t directional_light_count, const szg_spot_light_packed* h_spot_lights,
                                      uint32_t spot_light_count, uint32_t view_camera_index, const szg_camera_packed* d_cameras,
                                      const szg_fill_scene* geometry)
{
    SZG_TRY_RC(validate_lights("szg_deferred_record_draw_commands", p, draw_rect, tile, scene_texture, atmospheric_directional_lights_count,
                               d_directional_lights, directional_light_count, h_spot_lights, spot_light_count, d_cameras,
                               geometry != nullptr, nullptr));
    if (geometry != nullptr)
    {
        // deferred.cpp:480-490 shadow maps, then :493-713 the G-buffer pass
        SZG_TRY_RC(szg_deferred_record_shadow_maps(p, stream, d_directional_lights, directional_light_count, h_spot_lights,
                                                 spot_light_count, geometry));
        SZG_TRY_RC(szg_deferred_record_gbuffer_fill(p, stream, draw_rect, tile, scene_texture, view_camera_index, d_cameras, geometry));
    }
    return szg_deferred_record_lights(p, stream, draw_rect, tile, scene_texture, atmospheric_directional_lights_count,
                                      d_directional_lights, directional_light_count, h_spot_lights, spot_light_count,
                                      view_camera_index, d_cameras);
}

} // extern "C"
