// api_skyview.cpp — SkyViewComputePipeline behind the C-ABI (include/szg/abi.h): renderer/pipelines/skyview.cpp:713-965.

#include <new>

#include "api_common.hpp"
#include "lut_state.hpp"
#include "szg/multiscatter_sky.h"

using namespace szg;

struct szg_skyview
{
    int device = 0;
    szg_skyview_desc desc{};
    DeviceBuffer<float> d_transmittance, d_skyview, d_multiscatter, d_aerialLuminance, d_aerialTransmittance;
    float aerialMaxDistance = 0.0f; // 0 = never recorded
    uint32_t multiscatter = SZG_MULTISCATTER_OFF; // szg/multiscatter_sky.h: the mode of the sky-view and aerial LUT passes
    // mutable: the accessors that hand texels out take the ABI's const handle, and handing out is an event
    mutable LutState luts;
    DeviceBuffer<unsigned> d_slutStatusAll; // szg::SLUT_STATUS_RANKS dwords: the ranks' slice status words (szg_skyview_allgather_lut_rows)
    // LUT reuse across frames (szg_launch.hpp "LUT reuse"; off by default = the reference's recompute-every-frame)
    bool lutReuse = false;
    DeviceBuffer<unsigned> d_lutKey; // LUT_KEY_DWORDS dwords of device state
    // szg::frame_prep_bytes() each: per-frame constants (k_frame_prep), one block per pass, because a caller may record the
    // LUT pass of frame k+1 on another stream than the composite of frame k (rowtile.py does)
    DeviceBuffer<void> d_framePrep;     // sky-view LUT pass
    DeviceBuffer<void> d_framePrepDraw; // composite
};

static hipError_t ensure_tlut_status(szg_skyview* p, hipStream_t s)
{
    hipError_t e = hipSuccess;
    p->luts.ensure_tlut_status([&] {
        e = launch_lut_range(s, p->d_transmittance, p->desc.transmittance_width, p->desc.transmittance_height);
        return e == hipSuccess;
    });
    return e;
}

// A LUT pass with a mode set reads the multi-scattering LUT: somebody must have written it (szg/multiscatter_sky.h "WHERE").
static bool multiscatter_ready(const szg_skyview* p, const char* call)
{
    if (p->multiscatter != SZG_MULTISCATTER_OFF && !p->luts.multiscatterPresent)
    {
        fail(SZG_ERR_INVALID_ARGUMENT,
             "%s: multi-scattering mode %u is set but this pipeline holds no multi-scattering LUT: record one with "
             "szg_skyview_record_multiscatter_lut (or upload one through szg_skyview_multiscatter_lut) first",
             call, p->multiscatter);
        return false;
    }
    return true;
}

static hipError_t ensure_slut_status(szg_skyview* p, hipStream_t s)
{
    hipError_t e = hipSuccess;
    p->luts.ensure_slut_status([&] {
        e = launch_slut_check(s, p->d_skyview, p->desc.skyview_width, p->desc.skyview_height);
        return e == hipSuccess;
    });
    return e;
}

extern "C" {

// ---------------------------------------------------------------------------
// SkyViewComputePipeline
// ---------------------------------------------------------------------------
int szg_skyview_create(szg_skyview_t** out, const szg_skyview_desc* desc, int device)
{
    if (out == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_create: out is NULL");
    }
    *out = nullptr;
    szg_skyview_desc d{512u, 128u, 2048u, 1024u, 0u, 0u};
    if (desc != nullptr)
    {
        d = *desc;
    }
    if (d.transmittance_width < 2u || d.transmittance_height < 2u || d.skyview_width < 2u || d.skyview_height < 2u ||
        d.transmittance_width > 16384u || d.transmittance_height > 16384u || d.skyview_width > 16384u ||
        d.skyview_height > 16384u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_create: LUT extents out of range");
    }
    if (d.flags != 0u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_create: unknown flags 0x%x", d.flags);
    }
    SZG_TRY_RC(select_device(device));
    szg_skyview* p = new (std::nothrow) szg_skyview();
    if (p == nullptr)
    {
        return fail(SZG_ERR_OUT_OF_MEMORY, "szg_skyview_create: host allocation failed");
    }
    p->device = device;
    p->desc = d;
#define SZG_TRY(expr) SZG_HIP_OR(expr, szg_skyview_destroy(p), "szg_skyview_create: hipMalloc")
    size_t const aerialTexels = (size_t)SZG_AERIAL_W * SZG_AERIAL_H * SZG_AERIAL_D;
    SZG_TRY(p->d_transmittance.alloc(tlut_block_bytes(d.transmittance_width, d.transmittance_height) / sizeof(float)));
    SZG_TRY(p->d_skyview.alloc(slut_block_bytes(d.skyview_width, d.skyview_height) / sizeof(float)));
    SZG_TRY(p->d_multiscatter.alloc((size_t)SZG_MULTISCATTER_DIM * SZG_MULTISCATTER_DIM * 4u));
    SZG_TRY(p->d_aerialLuminance.alloc(aerialTexels * 4u));
    SZG_TRY(p->d_aerialTransmittance.alloc(aerialTexels * 4u));
    SZG_TRY(p->d_lutKey.alloc(LUT_KEY_DWORDS, true));
    SZG_TRY(p->d_framePrep.alloc(frame_prep_bytes()));
    SZG_TRY(p->d_slutStatusAll.alloc(SLUT_STATUS_RANKS));
    SZG_TRY(p->d_framePrepDraw.alloc(frame_prep_bytes()));
#undef SZG_TRY
    *out = p;
    return SZG_OK;
}

int szg_skyview_set_lut_reuse(szg_skyview_t* p, int enable)
{
    if (p == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_set_lut_reuse: NULL argument");
    }
    p->lutReuse = enable != 0;
    // whatever was computed while reuse was off has no key on the device: the first frame after a switch recomputes
    p->luts.reuse_switched();
    return SZG_OK;
}

int szg_skyview_set_multiscatter(szg_skyview_t* p, uint32_t mode)
{
    if (p == nullptr || mode > SZG_MULTISCATTER_ONLY)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_set_multiscatter: NULL pipeline or unknown mode %u", mode);
    }
    if (mode != p->multiscatter)
    {
        p->multiscatter = mode;
        p->luts.multiscatter_mode_changed();
    }
    return SZG_OK;
}

int szg_skyview_get_multiscatter(const szg_skyview_t* p, uint32_t* mode)
{
    if (p == nullptr || mode == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_get_multiscatter: NULL argument");
    }
    *mode = p->multiscatter;
    return SZG_OK;
}

int szg_skyview_invalidate_luts(szg_skyview_t* p, uint32_t which)
{
    if (p == nullptr || (which & ~(SZG_LUT_TRANSMITTANCE | SZG_LUT_SKYVIEW)) != 0u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_invalidate_luts: NULL pipeline or unknown LUT bits 0x%x", which);
    }
    if ((which & SZG_LUT_TRANSMITTANCE) != 0u)
    {
        p->luts.transmittance_exposed();
    }
    if ((which & SZG_LUT_SKYVIEW) != 0u)
    {
        p->luts.skyview_exposed();
    }
    return SZG_OK;
}

void szg_skyview_destroy(szg_skyview_t* p)
{
    if (p == nullptr)
    {
        return;
    }
    (void)hipSetDevice(p->device);
    delete p;
}

int szg_skyview_transmittance_lut(const szg_skyview_t* p, szg_image* out)
{
    if (p == nullptr || out == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_transmittance_lut: NULL argument");
    }
    *out = make_image(p->d_transmittance, p->desc.transmittance_width, p->desc.transmittance_height, SZG_FORMAT_RGBA32_SFLOAT);
    p->luts.transmittance_exposed(); // the caller may write the texels through this view
    return SZG_OK;
}

int szg_skyview_skyview_lut(const szg_skyview_t* p, szg_image* out)
{
    if (p == nullptr || out == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_skyview_lut: NULL argument");
    }
    *out = make_image(p->d_skyview, p->desc.skyview_width, p->desc.skyview_height, SZG_FORMAT_RGBA32_SFLOAT);
    p->luts.skyview_exposed(); // the caller may write the texels through this view (row slices gathered from other ranks)
    return SZG_OK;
}

int szg_skyview_record_transmittance(szg_skyview_t* p, void* stream, uint32_t atmosphere_index,
                                     const szg_atmosphere_packed* d_atmospheres)
{
    if (p == nullptr || d_atmospheres == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_record_transmittance: NULL argument");
    }
    DeviceGuard const guard(p->device);
    hipStream_t const s = static_cast<hipStream_t>(stream);
    const unsigned* dirty = nullptr;
    if (p->lutReuse)
    {
        // the status dword of texels written behind our back must be settled before a clean verdict may keep them
        SZG_HIP(szg::launch_lut_key(s, d_atmospheres, atmosphere_index, nullptr, 0u, p->d_lutKey, 0u, p->luts.forceTransmittance,
                                    p->d_transmittance, p->desc.transmittance_width, p->desc.transmittance_height));
        dirty = p->d_lutKey + 69;
    }
    SZG_HIP(szg::launch_transmittance(s, d_atmospheres, atmosphere_index, p->d_transmittance, p->desc.transmittance_width,
                                      p->desc.transmittance_height, dirty));
    p->luts.transmittance_recorded();
    return SZG_OK;
}

int szg_skyview_record_skyview_lut_rows(szg_skyview_t* p, void* stream, uint32_t atmosphere_index,
                                        const szg_atmosphere_packed* d_atmospheres, uint32_t view_camera_index,
                                        const szg_camera_packed* d_cameras, uint32_t row_begin, uint32_t row_end)
{
    if (p == nullptr || d_atmospheres == nullptr || d_cameras == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_record_skyview_lut_rows: NULL argument");
    }
    if (row_begin > row_end || row_end > p->desc.skyview_height)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_record_skyview_lut_rows: rows [%u, %u) outside the %u-row LUT", row_begin,
                    row_end, p->desc.skyview_height);
    }
    if (!multiscatter_ready(p, "szg_skyview_record_skyview_lut_rows"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    DeviceGuard const guard(p->device);
    hipStream_t const s = static_cast<hipStream_t>(stream);
    bool const whole = LutState::whole(row_begin, row_end, p->desc.skyview_height);
    SZG_HIP(ensure_tlut_status(p, s));
    const unsigned* dirty = nullptr;
    if (p->lutReuse && whole)
    {
        SZG_HIP(szg::launch_lut_key(s, d_atmospheres, atmosphere_index, d_cameras, view_camera_index, p->d_lutKey, 1u, p->luts.forceSkyview,
                                    p->d_skyview, p->desc.skyview_width, p->desc.skyview_height));
        dirty = p->d_lutKey + 70;
    }
    SZG_HIP(szg::launch_frame_prep(s, d_atmospheres, atmosphere_index, p->desc.transmittance_width, p->desc.transmittance_height,
                                   p->d_framePrep));
    if (p->multiscatter == SZG_MULTISCATTER_OFF)
    {
        SZG_HIP(szg::launch_skyview(s, d_atmospheres, atmosphere_index, d_cameras, view_camera_index, p->d_transmittance,
                                    p->desc.transmittance_width, p->desc.transmittance_height, p->d_skyview, p->desc.skyview_width,
                                    p->desc.skyview_height, row_begin, row_end, dirty, p->d_framePrep));
    }
    else
    {
        SZG_HIP(szg::launch_skyview_ms(s, p->multiscatter, d_atmospheres, atmosphere_index, d_cameras, view_camera_index,
                                       p->d_transmittance, p->desc.transmittance_width, p->desc.transmittance_height,
                                       p->d_multiscatter, p->d_skyview, p->desc.skyview_width, p->desc.skyview_height, row_begin,
                                       row_end, dirty, p->d_framePrep));
    }
    // (a slice is never launched behind a reuse key: launch_skyview cleared the status dword, the slice's waves set it)
    p->luts.skyview_rows_recorded(row_begin, row_end, p->desc.skyview_height);
    return SZG_OK;
}

int szg_skyview_lut_row_slice(const szg_skyview_t* p, uint32_t rank, uint32_t nranks, uint32_t* row_begin, uint32_t* row_end)
{
    if (p == nullptr || row_begin == nullptr || row_end == nullptr || nranks == 0u || rank >= nranks)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_lut_row_slice: NULL argument or rank outside [0, nranks)");
    }
    if (p->desc.skyview_height % nranks != 0u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_lut_row_slice: %u LUT rows do not divide over %u ranks", p->desc.skyview_height,
                    nranks);
    }
    uint32_t const n = p->desc.skyview_height / nranks;
    *row_begin = rank * n;
    *row_end = (rank + 1u) * n;
    return SZG_OK;
}

int szg_skyview_allgather_lut_rows(szg_skyview_t* p, szg_rowtile_comm_t* comm, void* stream)
{
    if (p == nullptr || comm == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_allgather_lut_rows: NULL argument");
    }
    int const nranks = szg_rowtile_comm_size(comm);
    if (nranks < 1 || p->desc.skyview_height % (uint32_t)nranks != 0u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_allgather_lut_rows: %u LUT rows do not divide over %d ranks",
                    p->desc.skyview_height, nranks);
    }
    if (nranks > (int)szg::SLUT_STATUS_RANKS)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_allgather_lut_rows: more than %u ranks", szg::SLUT_STATUS_RANKS);
    }
    DeviceGuard const guard(p->device);
    hipStream_t const s = static_cast<hipStream_t>(stream);
    size_t const slice = (size_t)(p->desc.skyview_height / (uint32_t)nranks) * p->desc.skyview_width * 16u;
    // this rank's status word first (the dword behind the texels is overwritten by nobody: the slices end in front of it).
    // It is known when the dword describes the whole LUT, or exactly the rows this rank contributes.
    unsigned const rank = (unsigned)szg_rowtile_comm_rank(comm);
    bool const known = p->luts.slice_status_known(rank, (uint32_t)nranks, p->desc.skyview_height);
    SZG_HIP(szg::launch_slut_status_stage(s, p->d_slutStatusAll, rank, p->d_skyview, p->desc.skyview_width,
                                          p->desc.skyview_height, known));
    int rc = szg_rowtile_allgather(comm, stream, p->d_skyview, slice);
    if (rc == SZG_OK)
    {
        // ... and the ranks' status words beside the slices: the LUT's status dword becomes their OR, so the composite needs
        // no 32 MiB re-scan of texels other ranks wrote. Every rank makes this second, 4-byte exchange unconditionally.
        rc = szg_rowtile_allgather(comm, stream, p->d_slutStatusAll, sizeof(unsigned));
    }
    if (rc == SZG_OK)
    {
        SZG_HIP(szg::launch_slut_status_reduce(s, p->d_slutStatusAll, (unsigned)nranks, p->d_skyview, p->desc.skyview_width,
                                               p->desc.skyview_height));
    }
    p->luts.rows_gathered(rc == SZG_OK);
    return rc;
}

int szg_skyview_record_skyview_lut(szg_skyview_t* p, void* stream, uint32_t atmosphere_index,
                                   const szg_atmosphere_packed* d_atmospheres, uint32_t view_camera_index,
                                   const szg_camera_packed* d_cameras)
{
    if (p == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_record_skyview_lut: NULL argument");
    }
    return szg_skyview_record_skyview_lut_rows(p, stream, atmosphere_index, d_atmospheres, view_camera_index, d_cameras, 0u,
                                               p->desc.skyview_height);
}

static int record_composite(szg_skyview_t* p, void* stream, const szg_scene_texture* scene_texture, szg_rect draw_rect,
                            const szg_rowtile* tile, const szg_gbuffer* gbuffer, const szg_shadowmaps* shadow_maps,
                            uint32_t atmosphere_index, const szg_atmosphere_packed* d_atmospheres, uint32_t view_camera_index,
                            const szg_camera_packed* d_cameras, uint32_t sun_light_index,
                            const szg_directional_light_packed* d_lights, bool fast)
{
    if (p == nullptr || d_atmospheres == nullptr || d_cameras == nullptr || d_lights == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_record_composite: NULL argument");
    }
    if (!check_rect(draw_rect, "szg_skyview_record_composite"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    DeviceGuard const guard(p->device);
    if (draw_rect.width == 0u || draw_rect.height == 0u)
    {
        return SZG_OK; // empty extent: nothing to dispatch (computeDispatchCount(0) == 0)
    }
    szg::TileArgs t{};
    if (!resolve_tile(tile, draw_rect.height, t))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    if (!check_scene(scene_texture, draw_rect.width, t.local_rows, true) || !check_gbuffer(gbuffer, draw_rect.width, t.local_rows))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    // camera.comp:369 indexes shadowMaps[sunLightIndex]; only that slot is needed.
    szg::ShadowSlot sun{nullptr, 0u, 0u, 0u, 0u};
    if (shadow_maps != nullptr && shadow_maps->maps != nullptr && sun_light_index < shadow_maps->count &&
        shadow_maps->maps[sun_light_index].data != nullptr)
    {
        const szg_image& m = shadow_maps->maps[sun_light_index];
        if (!check_image(m, SZG_FORMAT_D32_SFLOAT, 1u, 1u, "shadow map"))
        {
            return SZG_ERR_INVALID_ARGUMENT;
        }
        sun = szg::ShadowSlot{static_cast<const float*>(m.data), m.width, m.height, m.pitch_bytes / 4u, 0u};
    }
    szg::AerialLut aerial{nullptr, SZG_AERIAL_W, SZG_AERIAL_H, SZG_AERIAL_D, 0.0f};
    if (fast)
    {
        if (!(p->aerialMaxDistance > 0.0f))
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_record_composite_fast: no aerial LUT has been recorded");
        }
        aerial.luminance = p->d_aerialLuminance;
        aerial.maxDistance = p->aerialMaxDistance;
    }
    SZG_HIP(ensure_tlut_status(p, static_cast<hipStream_t>(stream)));
    SZG_HIP(ensure_slut_status(p, static_cast<hipStream_t>(stream)));
    SZG_HIP(szg::launch_frame_prep(static_cast<hipStream_t>(stream), d_atmospheres, atmosphere_index, p->desc.transmittance_width,
                                   p->desc.transmittance_height, p->d_framePrepDraw,
                                   sun.map != nullptr ? d_lights + sun_light_index : nullptr, d_cameras, view_camera_index,
                                   draw_rect.width, draw_rect.height));
    SZG_HIP(szg::launch_composite(static_cast<hipStream_t>(stream), *scene_texture, draw_rect.width, draw_rect.height, t, *gbuffer,
                                  sun, d_atmospheres, atmosphere_index, d_cameras, view_camera_index, d_lights, sun_light_index,
                                  p->d_transmittance, p->desc.transmittance_width, p->desc.transmittance_height, p->d_skyview,
                                  p->desc.skyview_width, p->desc.skyview_height, aerial, p->d_framePrepDraw));
    return SZG_OK;
}

int szg_skyview_record_composite(szg_skyview_t* p, void* stream, const szg_scene_texture* scene_texture, szg_rect draw_rect,
                                 const szg_rowtile* tile, const szg_gbuffer* gbuffer, const szg_shadowmaps* shadow_maps,
                                 uint32_t atmosphere_index, const szg_atmosphere_packed* d_atmospheres,
                                 uint32_t view_camera_index, const szg_camera_packed* d_cameras, uint32_t sun_light_index,
                                 const szg_directional_light_packed* d_lights)
{
    return record_composite(p, stream, scene_texture, draw_rect, tile, gbuffer, shadow_maps, atmosphere_index, d_atmospheres,
                            view_camera_index, d_cameras, sun_light_index, d_lights, false);
}

int szg_skyview_record_composite_fast(szg_skyview_t* p, void* stream, const szg_scene_texture* scene_texture, szg_rect draw_rect,
                                      const szg_rowtile* tile, const szg_gbuffer* gbuffer, const szg_shadowmaps* shadow_maps,
                                      uint32_t atmosphere_index, const szg_atmosphere_packed* d_atmospheres,
                                      uint32_t view_camera_index, const szg_camera_packed* d_cameras, uint32_t sun_light_index,
                                      const szg_directional_light_packed* d_lights)
{
    return record_composite(p, stream, scene_texture, draw_rect, tile, gbuffer, shadow_maps, atmosphere_index, d_atmospheres,
                            view_camera_index, d_cameras, sun_light_index, d_lights, true);
}

int szg_skyview_record_multiscatter_lut(szg_skyview_t* p, void* stream, uint32_t atmosphere_index,
                                        const szg_atmosphere_packed* d_atmospheres)
{
    if (p == nullptr || d_atmospheres == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_record_multiscatter_lut: NULL argument");
    }
    DeviceGuard const guard(p->device);
    SZG_HIP(ensure_tlut_status(p, static_cast<hipStream_t>(stream)));
    SZG_HIP(szg::launch_multiscatter(static_cast<hipStream_t>(stream), d_atmospheres, atmosphere_index, p->d_transmittance,
                                     p->desc.transmittance_width, p->desc.transmittance_height, p->d_multiscatter,
                                     SZG_MULTISCATTER_DIM));
    p->luts.multiscatter_recorded(p->multiscatter != SZG_MULTISCATTER_OFF);
    return SZG_OK;
}

int szg_skyview_multiscatter_lut(const szg_skyview_t* p, szg_image* out)
{
    if (p == nullptr || out == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_multiscatter_lut: NULL argument");
    }
    *out = make_image(p->d_multiscatter, SZG_MULTISCATTER_DIM, SZG_MULTISCATTER_DIM, SZG_FORMAT_RGBA32_SFLOAT);
    p->luts.multiscatter_exposed(p->multiscatter != SZG_MULTISCATTER_OFF); // the caller may write the texels through this view
    return SZG_OK;
}

int szg_skyview_record_aerial_lut(szg_skyview_t* p, void* stream, uint32_t atmosphere_index,
                                  const szg_atmosphere_packed* d_atmospheres, uint32_t view_camera_index,
                                  const szg_camera_packed* d_cameras, float max_distance_mm)
{
    if (p == nullptr || d_atmospheres == nullptr || d_cameras == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_record_aerial_lut: NULL argument");
    }
    if (!(max_distance_mm > 0.0f) || !(max_distance_mm < 1.0e6f))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_record_aerial_lut: max_distance_mm must be in (0, 1e6)");
    }
    if (!multiscatter_ready(p, "szg_skyview_record_aerial_lut"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    DeviceGuard const guard(p->device);
    SZG_HIP(ensure_tlut_status(p, static_cast<hipStream_t>(stream)));
    if (p->multiscatter == SZG_MULTISCATTER_OFF)
    {
        SZG_HIP(szg::launch_aerial_lut(static_cast<hipStream_t>(stream), d_atmospheres, atmosphere_index, d_cameras, view_camera_index,
                                       p->d_transmittance, p->desc.transmittance_width, p->desc.transmittance_height,
                                       p->d_aerialLuminance, p->d_aerialTransmittance, SZG_AERIAL_W, SZG_AERIAL_H, SZG_AERIAL_D,
                                       max_distance_mm));
    }
    else
    {
        SZG_HIP(szg::launch_aerial_lut_ms(static_cast<hipStream_t>(stream), p->multiscatter, d_atmospheres, atmosphere_index, d_cameras,
                                          view_camera_index, p->d_transmittance, p->desc.transmittance_width,
                                          p->desc.transmittance_height, p->d_multiscatter, p->d_aerialLuminance,
                                          p->d_aerialTransmittance, SZG_AERIAL_W, SZG_AERIAL_H, SZG_AERIAL_D, max_distance_mm));
    }
    p->aerialMaxDistance = max_distance_mm;
    return SZG_OK;
}

int szg_skyview_aerial_lut(const szg_skyview_t* p, szg_image* out_luminance, szg_image* out_transmittance)
{
    if (p == nullptr || out_luminance == nullptr || out_transmittance == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_skyview_aerial_lut: NULL argument");
    }
    *out_luminance = make_image(p->d_aerialLuminance, SZG_AERIAL_W, SZG_AERIAL_H * SZG_AERIAL_D, SZG_FORMAT_RGBA32_SFLOAT);
    *out_transmittance = make_image(p->d_aerialTransmittance, SZG_AERIAL_W, SZG_AERIAL_H * SZG_AERIAL_D, SZG_FORMAT_RGBA32_SFLOAT);
    return SZG_OK;
}

int szg_skyview_record_draw_commands(szg_skyview_t* p, void* stream, const szg_scene_texture* scene_texture, szg_rect draw_rect,
                                     const szg_rowtile* tile, const szg_gbuffer* gbuffer, const szg_shadowmaps* shadow_maps,
                                     uint32_t atmosphere_index, const szg_atmosphere_packed* d_atmospheres,
                                     uint32_t view_camera_index, const szg_camera_packed* d_cameras, uint32_t sun_light_index,
                                     const szg_directional_light_packed* d_lights)
{
    // skyview.cpp:795-845, :847-893, :895-910: three dispatches in this order, every frame.
    SZG_TRY_RC(szg_skyview_record_transmittance(p, stream, atmosphere_index, d_atmospheres));
    if (p != nullptr && p->multiscatter != SZG_MULTISCATTER_OFF)
    {
        // szg/multiscatter_sky.h: the LUT the sky-view pass is about to read, from this frame's transmittance LUT
        SZG_TRY_RC(szg_skyview_record_multiscatter_lut(p, stream, atmosphere_index, d_atmospheres));
    }
    SZG_TRY_RC(szg_skyview_record_skyview_lut(p, stream, atmosphere_index, d_atmospheres, view_camera_index, d_cameras));
    return szg_skyview_record_composite(p, stream, scene_texture, draw_rect, tile, gbuffer, shadow_maps, atmosphere_index,
                                        d_atmospheres, view_camera_index, d_cameras, sun_light_index, d_lights);
}

} // extern "C"
