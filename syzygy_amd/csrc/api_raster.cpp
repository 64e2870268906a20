// api_raster.cpp — the mesh passes of the deferred pipeline (szg/raster.h), the mip chains they sample (szg/mipmaps.h) and the
// sampler's anisotropy (szg/anisotropy.h).

#include <algorithm>
#include <functional>

#include "api_common.hpp"

using namespace szg;

namespace
{
// Flatten the rendered meshes into the reference's draw calls (deferred.cpp:624-699 / pipelines.cpp:738-800):
// one draw per (mesh, surface), primitives numbered instance-major.
// `mips` (G-buffer pass only): the pipeline's table of szg/mipmaps.h; `anyMips` = some draw carries more than one level.
int collect_draws(const char* who, const szg_mesh_instanced* meshes, uint32_t meshCount, bool shadow,
                  std::vector<szg::RasterDraw>& draws, uint32_t& primCount, const szg_deferred* mips = nullptr,
                  bool* anyMips = nullptr)
{
    draws.clear();
    uint64_t prims = 0;
    for (uint32_t i = 0; i < meshCount; i++)
    {
        szg_mesh_instanced const& m = meshes[i];
        // collectGeometryCullFlags (deferred.cpp:394-428): render flag, mesh and both model buffers present
        if (m.render == 0u || m.d_vertices == nullptr || m.d_indices == nullptr || m.d_models == nullptr ||
            m.d_model_inverse_transposes == nullptr || m.instance_count == 0u)
        {
            continue;
        }
        if (shadow && m.casts_shadow == 0u) // pipelines.cpp:742
        {
            continue;
        }
        if (m.surface_count > 0u && m.surfaces == nullptr)
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "%s: mesh %u has %u surfaces but a NULL surface array", who, i, m.surface_count);
        }
        for (uint32_t k = 0; k < m.surface_count; k++)
        {
            szg_surface const& surf = m.surfaces[k];
            uint32_t const avail = surf.first_index >= m.index_count ? 0u : m.index_count - surf.first_index;
            uint32_t const tris = (surf.index_count < avail ? surf.index_count : avail) / 3u;
            if (tris == 0u)
            {
                continue;
            }
            szg::RasterDraw d{};
            d.vertices = m.d_vertices;
            d.indices = m.d_indices;
            d.models = m.d_models;
            d.mits = m.d_model_inverse_transposes;
            d.vertexCount = m.vertex_count;
            d.firstIndex = surf.first_index;
            d.triCount = tris;
            d.instanceCount = m.instance_count;
            d.firstPrim = (uint32_t)prims;
            d.tex[0] = surf.material.color;
            d.tex[1] = surf.material.normal;
            d.tex[2] = surf.material.orm;
            for (szg_texture const& t : d.tex)
            {
                // (no refusal of a t.data that is not aligned to its 4-byte texels: layout_ok is given no pointer)
                if (t.data != nullptr && (t.width == 0u || t.height == 0u || t.width > 32768u || t.height > 32768u ||
                                          !layout_ok(nullptr, t.width, t.pitch_bytes, 4u)))
                {
                    return fail(SZG_ERR_INVALID_ARGUMENT, "%s: mesh %u surface %u has a malformed texture", who, i, k);
                }
            }
            d.maxLod = 0.0f;
            d.maxAnisotropy = mips != nullptr ? mips->textureMaxAnisotropy : SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE;
            for (int t = 0; t < 3; t++)
            {
                d.mipChain[t] = nullptr;
                d.mipLevels[t] = 1u;
                if (mips == nullptr || d.tex[t].data == nullptr)
                {
                    continue;
                }
                // sorted by level0_data (szg_deferred_set_texture_mips)
                auto const it = std::lower_bound(mips->textureMips.begin(), mips->textureMips.end(), d.tex[t].data,
                                                 [](szg_texture_mips const& e, const void* key) { return std::less<const void*>()(e.level0_data, key); });
                if (it == mips->textureMips.end() || it->level0_data != d.tex[t].data)
                {
                    continue;
                }
                uint32_t const full = szg_mip_level_count(d.tex[t].width, d.tex[t].height);
                if (it->level_count > full)
                {
                    return fail(SZG_ERR_INVALID_ARGUMENT,
                                "%s: mesh %u surface %u map %d is %ux%u (%u levels) but its mip table entry has level_count %u", who, i, k, t,
                                d.tex[t].width, d.tex[t].height, full, it->level_count);
                }
                d.mipChain[t] = it->d_chain;
                d.mipLevels[t] = it->level_count;
                d.maxLod = mips->textureMaxLod;
                if (it->level_count > 1u && anyMips != nullptr)
                {
                    *anyMips = true;
                }
            }
            prims += (uint64_t)tris * m.instance_count;
            if (prims > 0x40000000ull)
            {
                return fail(SZG_ERR_CAPACITY, "%s: more than 2^30 primitives", who);
            }
            draws.push_back(d);
        }
    }
    primCount = (uint32_t)prims;
    return SZG_OK;
}

int ensure_raster_capacity(szg_deferred* p, hipStream_t s, size_t draws, size_t prims)
{
    if (draws > p->rasterDrawCapacity)
    {
        SZG_HIP(hipStreamSynchronize(s));
        p->rasterDrawCapacity = 0; // (a failing allocation below must not leave the old capacity behind a NULL pointer)
        size_t const n = draws * 2u;
        SZG_HIP(p->d_rasterDraws.alloc(n));
        p->rasterDrawCapacity = n;
    }
    if (prims > p->raster.capacity)
    {
        SZG_HIP(hipStreamSynchronize(s));
        p->raster = RasterBuffers{}; // capacity 0 until every buffer below is there
        p->rasterStorage = {};       // frees the old buffers before the first new one is allocated
        auto& own = p->rasterStorage;
        size_t const n = ((prims * 3u / 2u) + 4095u) / 4096u * 4096u;
        SZG_HIP(own.prims.alloc(n));
        SZG_HIP(own.boxes.alloc(n));
        SZG_HIP(own.keysA.alloc(n));
        SZG_HIP(own.keysB.alloc(n));
        SZG_HIP(own.valsA.alloc(n));
        SZG_HIP(own.valsB.alloc(n));
        SZG_HIP(own.orderedBoxes.alloc(n));
        SZG_HIP(own.chunkBoxes.alloc(n / 64u));
        SZG_HIP(own.superBoxes.alloc(n / 4096u));
        // radix-sort temp storage for up to n pairs (a function of the count only)
        size_t sortTempBytes = 0;
        SZG_HIP(raster_sort_temp_bytes((unsigned)n, sortTempBytes));
        SZG_HIP(own.sortTemp.alloc(sortTempBytes > 0u ? sortTempBytes : 16u));
        // the view the launch interface takes (`order` is set by launch_raster_setup)
        RasterBuffers& rb = p->raster;
        rb.prims = own.prims;
        rb.boxes = own.boxes;
        rb.keysA = own.keysA;
        rb.keysB = own.keysB;
        rb.valsA = own.valsA;
        rb.valsB = own.valsB;
        rb.orderedBoxes = own.orderedBoxes;
        rb.chunkBoxes = own.chunkBoxes;
        rb.superBoxes = own.superBoxes;
        rb.sortTemp = own.sortTemp;
        rb.sortTempBytes = sortTempBytes;
        rb.capacity = n;
    }
    return SZG_OK;
}

int upload_draws(szg_deferred* p, hipStream_t s, const std::vector<szg::RasterDraw>& draws)
{
    size_t const per = p->staging.bytes / sizeof(szg::RasterDraw);
    if (per == 0u)
    {
        return fail(SZG_ERR_CAPACITY, "staging ring smaller than one draw record");
    }
    for (size_t i = 0; i < draws.size(); i += per)
    {
        size_t const n = draws.size() - i < per ? draws.size() - i : per;
        SZG_TRY_RC(p->staging.upload(s, p->d_rasterDraws + i, draws.data() + i, n * sizeof(szg::RasterDraw)));
    }
    return SZG_OK;
}
} // namespace

extern "C" {

int szg_deferred_record_gbuffer_raster(szg_deferred_t* p, void* stream, szg_rect draw_rect, const szg_rowtile* tile,
                                       const szg_scene_texture* scene_texture, uint32_t view_camera_index,
                                       const szg_camera_packed* d_cameras, const szg_mesh_instanced* meshes, uint32_t mesh_count)
{
    if (p == nullptr || d_cameras == nullptr || scene_texture == nullptr || (mesh_count > 0u && meshes == nullptr))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_record_gbuffer_raster: NULL argument");
    }
    if (!check_rect(draw_rect, "szg_deferred_record_gbuffer_raster"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    DeviceGuard const guard(p->device);
    if (draw_rect.width == 0u || draw_rect.height == 0u)
    {
        return SZG_OK;
    }
    if (draw_rect.width > 32768u || draw_rect.height > 32768u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_record_gbuffer_raster: draw extent above 32768");
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
    std::vector<szg::RasterDraw> draws;
    uint32_t primCount = 0;
    // k_raster_tile<true> only when some draw of this call has a chain (szg/mipmaps.h); k_raster_tile_aniso only when, on top of
    // that, the pipeline's maxAnisotropy is above 1 (szg/anisotropy.h)
    bool anyMips = false;
    SZG_TRY_RC(collect_draws("szg_deferred_record_gbuffer_raster", meshes, mesh_count, false, draws, primCount, p, &anyMips));
    hipStream_t const s = static_cast<hipStream_t>(stream);
    SZG_TRY_RC(ensure_raster_capacity(p, s, draws.size(), primCount));
    SZG_TRY_RC(upload_draws(p, s, draws));
    SZG_HIP(szg::launch_raster_setup(s, false, p->d_rasterDraws, (unsigned)draws.size(), primCount, d_cameras, view_camera_index, nullptr,
                                     draw_rect.width, draw_rect.height, p->raster));
    SZG_HIP(szg::launch_raster_tile(s, *scene_texture, draw_rect.width, draw_rect.height, t, p->gbuffer, p->d_rasterDraws, p->raster,
                                    primCount, d_cameras, view_camera_index, anyMips,
                                    p->textureMaxAnisotropy > SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE));
    return SZG_OK;
}

// ---------------------------------------------------------------------------
// Mip-mapped material textures (szg/mipmaps.h)
// ---------------------------------------------------------------------------
uint32_t szg_mip_level_count(uint32_t w, uint32_t h)
{
    if (w == 0u || h == 0u)
    {
        return 0u;
    }
    uint32_t levels = 1u;
    for (uint32_t m = w > h ? w : h; m > 1u; m >>= 1)
    {
        levels++;
    }
    return levels;
}

size_t szg_mip_chain_bytes(uint32_t w, uint32_t h)
{
    size_t bytes = 0;
    uint32_t const levels = szg_mip_level_count(w, h);
    for (uint32_t k = 1u; k < levels; k++)
    {
        size_t const wk = (w >> k) > 0u ? (w >> k) : 1u, hk = (h >> k) > 0u ? (h >> k) : 1u;
        bytes += wk * hk * 4u;
    }
    return bytes;
}

int szg_record_generate_mipmaps(void* stream, const szg_texture* level0, void* d_chain, size_t chain_bytes)
{
    if (level0 == nullptr || level0->data == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_generate_mipmaps: NULL level0 or level0->data");
    }
    if (level0->width == 0u || level0->height == 0u || level0->width > 32768u || level0->height > 32768u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_generate_mipmaps: extent %ux%u outside 1..32768", level0->width, level0->height);
    }
    if (!layout_ok(nullptr, level0->width, level0->pitch_bytes, 4u)) // the pointer's alignment has its own sentence below
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_generate_mipmaps: pitch %u is smaller than a row of %u texels or no multiple of 4",
                    level0->pitch_bytes, level0->width);
    }
    if (reinterpret_cast<uintptr_t>(level0->data) % 4u != 0u || reinterpret_cast<uintptr_t>(d_chain) % 4u != 0u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_generate_mipmaps: level0->data and d_chain must be aligned to 4 bytes");
    }
    size_t const need = szg_mip_chain_bytes(level0->width, level0->height);
    if (chain_bytes < need)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_generate_mipmaps: chain_bytes %zu, the chain of %ux%u needs %zu", chain_bytes,
                    level0->width, level0->height, need);
    }
    if (need == 0u)
    {
        return SZG_OK;
    }
    if (d_chain == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_generate_mipmaps: NULL d_chain");
    }
    SZG_HIP(szg::launch_generate_mipmaps(static_cast<hipStream_t>(stream), *level0, d_chain));
    return SZG_OK;
}

int szg_deferred_set_texture_mips(szg_deferred_t* p, const szg_texture_mips* entries, uint32_t count, float max_lod)
{
    // the arguments first, the pipeline last: every refusal below names its cause without a device
    if (count > 0u && entries == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_texture_mips: NULL entries with count %u", count);
    }
    if (!(max_lod >= 0.0f))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_texture_mips: max_lod is negative or NaN");
    }
    for (uint32_t i = 0; i < count; i++)
    {
        if (entries[i].level0_data == nullptr)
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_texture_mips: entry %u has a NULL level0_data", i);
        }
        if (entries[i].level_count == 0u)
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_texture_mips: entry %u has level_count 0", i);
        }
        if (reinterpret_cast<uintptr_t>(entries[i].level0_data) % 4u != 0u || reinterpret_cast<uintptr_t>(entries[i].d_chain) % 4u != 0u)
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_texture_mips: entry %u: level0_data and d_chain must be aligned to 4 bytes", i);
        }
        if (entries[i].level_count > 1u && entries[i].d_chain == nullptr)
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_texture_mips: entry %u has %u levels and a NULL d_chain", i,
                        entries[i].level_count);
        }
        for (uint32_t j = 0; j < i; j++)
        {
            if (entries[j].level0_data == entries[i].level0_data)
            {
                return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_texture_mips: entries %u and %u have the same level0_data (duplicate)",
                            j, i);
            }
        }
    }
    if (p == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_texture_mips: NULL pipeline");
    }
    p->textureMips.assign(entries, entries + count);
    std::sort(p->textureMips.begin(), p->textureMips.end(),
              [](szg_texture_mips const& a, szg_texture_mips const& b) { return std::less<const void*>()(a.level0_data, b.level0_data); });
    p->textureMaxLod = max_lod;
    return SZG_OK;
}

// ---------------------------------------------------------------------------
// Anisotropic filtering (szg/anisotropy.h)
// ---------------------------------------------------------------------------
int szg_deferred_set_sampler_anisotropy(szg_deferred_t* p, float max_anisotropy)
{
    // the argument first, the pipeline last, as szg_deferred_set_texture_mips
    if (max_anisotropy != max_anisotropy)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_sampler_anisotropy: max_anisotropy is NaN");
    }
    if (max_anisotropy < SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE || max_anisotropy > SZG_SAMPLER_MAX_ANISOTROPY_LIMIT)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_sampler_anisotropy: max_anisotropy %g outside 1..16", (double)max_anisotropy);
    }
    if (p == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_set_sampler_anisotropy: NULL pipeline");
    }
    p->textureMaxAnisotropy = max_anisotropy;
    return SZG_OK;
}

int szg_deferred_record_shadow_raster(szg_deferred_t* p, void* stream, const szg_directional_light_packed* d_directional_lights,
                                      uint32_t directional_light_count, const szg_spot_light_packed* h_spot_lights,
                                      uint32_t spot_light_count, const szg_mesh_instanced* meshes, uint32_t mesh_count)
{
    if (p == nullptr || (mesh_count > 0u && meshes == nullptr))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_record_shadow_raster: NULL argument");
    }
    DeviceGuard const guard(p->device);
    if ((directional_light_count > 0u && d_directional_lights == nullptr) || (spot_light_count > 0u && h_spot_lights == nullptr))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_deferred_record_shadow_raster: light array NULL");
    }
    if (spot_light_count > p->desc.max_spot_lights)
    {
        return fail(SZG_ERR_CAPACITY, "szg_deferred_record_shadow_raster: %u spot lights exceed the capacity %u", spot_light_count,
                    p->desc.max_spot_lights);
    }
    if (p->d_ownedShadowMaps == nullptr)
    {
        return SZG_OK; // the pipeline owns no shadow maps
    }
    unsigned const lights = directional_light_count + spot_light_count;
    unsigned const slots = lights < p->desc.max_shadow_maps ? lights : p->desc.max_shadow_maps; // shadowpass.cpp:219-225
    if (slots == 0u)
    {
        return SZG_OK;
    }
    std::vector<szg::RasterDraw> draws;
    uint32_t primCount = 0;
    SZG_TRY_RC(collect_draws("szg_deferred_record_shadow_raster", meshes, mesh_count, true, draws, primCount));
    hipStream_t const s = static_cast<hipStream_t>(stream);
    SZG_TRY_RC(ensure_raster_capacity(p, s, draws.size(), primCount));
    SZG_TRY_RC(p->staging.upload(s, p->d_spots, h_spot_lights, (size_t)spot_light_count * sizeof(szg_spot_light_packed)));
    SZG_TRY_RC(upload_draws(p, s, draws));
    SZG_HIP(szg::launch_shadow_prep(s, d_directional_lights, directional_light_count, p->d_spots, spot_light_count, p->d_ownedSlots, slots,
                                    p->d_shadowGen));
    unsigned const dim = p->desc.shadow_map_dim;
    for (unsigned slot = 0; slot < slots; slot++)
    {
        // the primitive buffers are reused slot after slot: stream order keeps setup(k+1) behind tile(k)
        SZG_HIP(szg::launch_raster_setup(s, true, p->d_rasterDraws, (unsigned)draws.size(), primCount, nullptr, 0u, p->d_shadowGen + slot, dim,
                                         dim, p->raster));
        SZG_HIP(szg::launch_shadow_tile(s, p->d_shadowGen + slot, dim, p->raster, primCount, p->config.depthBiasConstant,
                                        p->config.depthBiasSlope));
    }
    return SZG_OK;
}

int szg_deferred_record_draw_commands_meshes(szg_deferred_t* p, void* stream, szg_rect draw_rect, const szg_rowtile* tile,
                                             const szg_scene_texture* scene_texture, uint32_t atmospheric_directional_lights_count,
                                             const szg_directional_light_packed* d_directional_lights,
                                             uint32_t directional_light_count, const szg_spot_light_packed* h_spot_lights,
                                             uint32_t spot_light_count, uint32_t view_camera_index, const szg_camera_packed* d_cameras,
                                             const szg_mesh_instanced* meshes, uint32_t mesh_count)
{
    // deferred.cpp:480-490 shadow maps, :493-713 G-buffer pass, :715-787 lights
    SZG_TRY_RC(validate_lights("szg_deferred_record_draw_commands_meshes", p, draw_rect, tile, scene_texture,
                               atmospheric_directional_lights_count, d_directional_lights, directional_light_count, h_spot_lights,
                               spot_light_count, d_cameras, true, nullptr));
    SZG_TRY_RC(szg_deferred_record_shadow_raster(p, stream, d_directional_lights, directional_light_count, h_spot_lights, spot_light_count,
                                               meshes, mesh_count));
    SZG_TRY_RC(szg_deferred_record_gbuffer_raster(p, stream, draw_rect, tile, scene_texture, view_camera_index, d_cameras, meshes, mesh_count));
    return szg_deferred_record_lights(p, stream, draw_rect, tile, scene_texture, atmospheric_directional_lights_count,
                                      d_directional_lights, directional_light_count, h_spot_lights, spot_light_count, view_camera_index,
                                      d_cameras);
}

} // extern "C"
