// szg/pipelines.hpp — header-only C++ mirror of the reference's render-pass classes for
// the deferred-shading + atmosphere path, over the C-ABI of szg/abi.h.
//
// A caller written against the reference (Renderer::recordDraw, renderer.cpp:278-443)
// ports one to one:
//
//   reference                                              this header
//   ------------------------------------------------------ -----------------------------
//   VkCommandBuffer cmd                                    hipStream_t cmd
//   TStagedBuffer<T>            buffers.hpp:209-299        szg::TStagedBuffer<T>
//   SceneTexture                scenetexture.hpp:11-81     szg::SceneTexture
//   GBuffer / ShadowPassArray   gbuffer.hpp, shadowpass.hpp szg_gbuffer / szg_shadowmaps
//   DeferredShadingPipeline     pipelines/deferred.hpp:23  szg::DeferredShadingPipeline
//   SkyViewComputePipeline      pipelines/skyview.hpp:24   szg::SkyViewComputePipeline
//   DebugLineGraphicsPipeline   pipelines.hpp:238-268      szg::DebugLineGraphicsPipeline (szg/debuglines.h)
//   recordCopyImageToImage      imageoperations.cpp:45-176 szg::recordCopyImageToImage (szg/present.h)
//   Editor::endFrame's tail     editor.cpp:303-361         szg::recordPresent
//   ComputeCollectionPipeline   pipelines.hpp:166-235      szg::ComputeCollectionPipeline (szg/compute_collection.h)
//   UILayer                     editor/uilayer.hpp:36-114  szg::UILayer (szg/ui_layer.hpp, included at the end; szg/ui_layer.h)
//   TextureDisplay              ui/texturedisplay.hpp      szg::TextureDisplay (szg/texture_display.hpp, included at the end;
//                                                          szg/texture_display.h)
//   std::span<MeshInstanced const> sceneGeometry           szg_fill_scene const* (synthetic)
//
// Error behaviour follows the reference: construction failures give an invalid object /
// nullptr plus a log line; record* return void and never throw.
#pragma once

#include <hip/hip_runtime_api.h>

#include <array>
#include <cstdio>
#include <cstring>
#include <memory>
#include <span>
#include <string_view>
#include <vector>

#include "szg/abi.h"
#include "szg/anisotropy.h"
#include "szg/compute_collection.h"
#include "szg/debuglines.h"
#include "szg/mipmaps.h"
#include "szg/multiscatter_sky.h"
#include "szg/present.h"
#include "szg/raster.h"
#include "szg/texture_display.h"
#include "szg/host.h"

namespace szg
{
using CameraPacked = szg_camera_packed;
using AtmospherePacked = szg_atmosphere_packed;
using DirectionalLightPacked = szg_directional_light_packed;
using SpotLightPacked = szg_spot_light_packed;

// buffers.hpp:209-299 — host staging + device copy, recordCopyToDevice on a stream.
// recordCopyToDevice is asynchronous: the copy runs in stream order, possibly behind a whole frame of kernels, while the
// caller goes on to stage the next frame. The reference guards its staging memory with the frame fences (two frames in
// flight, framebuffer.cpp:134); here the staged bytes are handed to the stream through a small ring of pinned slots, and a
// slot is rewritten only after the event recorded behind its last copy has completed.
template <typename T> struct TStagedBuffer
{
    static constexpr int RING_SLOTS = 3;
    TStagedBuffer() = default;
    TStagedBuffer(TStagedBuffer const&) = delete;
    auto operator=(TStagedBuffer const&) -> TStagedBuffer& = delete;
    TStagedBuffer(TStagedBuffer&& o) noexcept { *this = std::move(o); }
    auto operator=(TStagedBuffer&& o) noexcept -> TStagedBuffer&
    {
        destroy();
        m_host = o.m_host;
        m_device = o.m_device;
        m_capacity = o.m_capacity;
        m_staged = o.m_staged;
        m_deviceSize = o.m_deviceSize;
        m_dirty = o.m_dirty;
        m_next = o.m_next;
        for (int i = 0; i < RING_SLOTS; i++)
        {
            m_ring[i] = o.m_ring[i];
            m_done[i] = o.m_done[i];
            m_used[i] = o.m_used[i];
            o.m_ring[i] = nullptr;
            o.m_done[i] = nullptr;
            o.m_used[i] = false;
        }
        o.m_host = nullptr;
        o.m_device = nullptr;
        o.m_capacity = 0;
        return *this;
    }
    ~TStagedBuffer() { destroy(); }

    static auto allocate(size_t capacity) -> TStagedBuffer<T>
    {
        TStagedBuffer<T> b;
        bool ok = hipHostMalloc(reinterpret_cast<void**>(&b.m_host), capacity * sizeof(T), hipHostMallocDefault) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void**>(&b.m_device), capacity * sizeof(T)) == hipSuccess;
        for (int i = 0; ok && i < RING_SLOTS; i++)
        {
            ok = hipHostMalloc(reinterpret_cast<void**>(&b.m_ring[i]), capacity * sizeof(T), hipHostMallocDefault) == hipSuccess &&
                 hipEventCreateWithFlags(&b.m_done[i], hipEventDisableTiming) == hipSuccess;
        }
        if (!ok)
        {
            std::fprintf(stderr, "[szg] TStagedBuffer::allocate(%zu) failed\n", capacity);
            b.destroy();
            return b;
        }
        b.m_capacity = capacity;
        return b;
    }
    void clearStaged()
    {
        m_staged = 0;
        m_dirty = true;
    }
    void push(T const& value) { push(std::span<T const>{&value, 1}); }
    void push(std::span<T const> data)
    {
        if (m_staged + data.size() > m_capacity)
        {
            std::fprintf(stderr, "[szg] TStagedBuffer::push exceeds capacity\n");
            return;
        }
        std::memcpy(m_host + m_staged, data.data(), data.size_bytes());
        m_staged += data.size();
        m_dirty = true;
    }
    void stage(std::span<T const> data)
    {
        clearStaged();
        push(data);
    }
    void pop(size_t count) { m_staged = count > m_staged ? 0 : m_staged - count; }
    void recordCopyToDevice(hipStream_t cmd)
    {
        if (m_staged > 0)
        {
            int const slot = m_next;
            m_next = (m_next + 1) % RING_SLOTS;
            if (m_used[slot])
            {
                (void)hipEventSynchronize(m_done[slot]); // the copy that last read this slot has run
            }
            std::memcpy(m_ring[slot], m_host, m_staged * sizeof(T));
            (void)hipMemcpyAsync(m_device, m_ring[slot], m_staged * sizeof(T), hipMemcpyHostToDevice, cmd);
            (void)hipEventRecord(m_done[slot], cmd);
            m_used[slot] = true;
        }
        m_deviceSize = m_staged;
        m_dirty = false;
    }
    [[nodiscard]] auto deviceAddress() const -> T const* { return m_device; }
    [[nodiscard]] auto deviceSize() const -> size_t { return m_deviceSize; }
    [[nodiscard]] auto stagedSize() const -> size_t { return m_staged; }
    [[nodiscard]] auto stagingCapacity() const -> size_t { return m_capacity; }
    [[nodiscard]] auto isDirty() const -> bool { return m_dirty; }
    [[nodiscard]] auto readValidStaged() const -> std::span<T const>
    {
        if (m_dirty)
        {
            std::fprintf(stderr, "[szg] Dirty buffer was accessed with a read\n"); // buffers.hpp:252-260
        }
        return {m_host, m_staged};
    }
    [[nodiscard]] auto valid() const -> bool { return m_capacity > 0; }

private:
    void destroy()
    {
        for (int i = 0; i < RING_SLOTS; i++)
        {
            if (m_used[i])
            {
                (void)hipEventSynchronize(m_done[i]);
            }
            if (m_done[i] != nullptr)
            {
                (void)hipEventDestroy(m_done[i]);
            }
            if (m_ring[i] != nullptr)
            {
                (void)hipHostFree(m_ring[i]);
            }
            m_ring[i] = nullptr;
            m_done[i] = nullptr;
            m_used[i] = false;
        }
        if (m_host != nullptr)
        {
            (void)hipHostFree(m_host);
        }
        if (m_device != nullptr)
        {
            (void)hipFree(m_device);
        }
        m_host = nullptr;
        m_device = nullptr;
        m_capacity = 0;
    }
    T* m_host{nullptr};
    T* m_device{nullptr};
    T* m_ring[RING_SLOTS]{};
    hipEvent_t m_done[RING_SLOTS]{};
    bool m_used[RING_SLOTS]{};
    int m_next{0};
    size_t m_capacity{0};
    size_t m_staged{0};
    size_t m_deviceSize{0};
    bool m_dirty{false};
};

// scenetexture.hpp:11-81 — colour RGBA16 UNORM + depth D32F at a capacity extent.
struct SceneTexture
{
    SceneTexture() = default;
    SceneTexture(SceneTexture const&) = delete;
    auto operator=(SceneTexture const&) -> SceneTexture& = delete;
    ~SceneTexture()
    {
        (void)hipFree(m_texture.color.data);
        (void)hipFree(m_texture.depth.data);
        (void)hipFree(m_texture.debug_color.data);
    }
    static auto create(uint32_t width, uint32_t height, bool debugColor = false) -> std::unique_ptr<SceneTexture>
    {
        auto t = std::make_unique<SceneTexture>();
        auto image = [&](szg_image& im, uint32_t fmt, uint32_t texel) {
            im = szg_image{nullptr, width, height, width * texel, fmt};
            // (the fill runs on the null stream and is not promised to be complete on return; the first pass may be recorded on
            // a non-blocking stream, which does not wait for the null stream: wait here, once)
            return hipMalloc(&im.data, (size_t)width * height * texel) == hipSuccess &&
                   hipMemset(im.data, 0, (size_t)width * height * texel) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
        };
        bool ok = image(t->m_texture.color, SZG_FORMAT_RGBA16_UNORM, 8) && image(t->m_texture.depth, SZG_FORMAT_D32_SFLOAT, 4);
        if (ok && debugColor)
        {
            ok = image(t->m_texture.debug_color, SZG_FORMAT_RGBA32_SFLOAT, 16);
        }
        if (!ok)
        {
            std::fprintf(stderr, "[szg] SceneTexture::create(%u, %u) failed\n", width, height);
            return nullptr;
        }
        return t;
    }
    [[nodiscard]] auto texture() const -> szg_scene_texture const& { return m_texture; }
    [[nodiscard]] auto color() const -> szg_image const& { return m_texture.color; }
    [[nodiscard]] auto depth() const -> szg_image const& { return m_texture.depth; }

private:
    szg_scene_texture m_texture{};
};

// The reference's record calls return void and log what goes wrong (SZG_ERROR); so do these wrappers: a negative status of
// the C-ABI call is printed once per call site to stderr with szg_last_error()'s text and kept in the pipeline's
// lastStatus(), so that a refused pass (e.g. a draw rect with a non-zero offset, szg/abi.h) is never a silently
// unrendered frame.
namespace detail
{
inline auto note(int status, char const* what, int& last) -> int
{
    last = status;
    if (status < 0)
    {
        std::fprintf(stderr, "[szg] %s failed with status %d: %s\n", what, status, szg_last_error());
    }
    return status;
}
} // namespace detail

// pipelines/deferred.hpp:23-119
struct DeferredShadingPipeline
{
    using Configuration = szg_deferred_configuration;

    // deferred.hpp:26-32. Invalid (valid() == false) on failure, like the reference's
    // shaders that stay "invalid" (deferred.cpp:153-163).
    DeferredShadingPipeline(uint32_t capacityWidth, uint32_t capacityHeight, uint32_t maxSpotLights = 16,
                            uint32_t maxShadowMaps = 10, uint32_t shadowMapDimension = 0, int device = 0)
    {
        szg_deferred_desc const desc{capacityWidth, capacityHeight, maxSpotLights, maxShadowMaps, shadowMapDimension, 0};
        if (szg_deferred_create(&m_handle, &desc, device) != SZG_OK)
        {
            m_handle = nullptr;
        }
    }
    DeferredShadingPipeline(DeferredShadingPipeline const&) = delete;
    auto operator=(DeferredShadingPipeline const&) -> DeferredShadingPipeline& = delete;
    ~DeferredShadingPipeline() { cleanup(); }

    // deferred.hpp:34-44
    void recordDrawCommands(hipStream_t cmd, szg_rect drawRect, SceneTexture& sceneTexture,
                            uint32_t atmosphericDirectionalLightsCount,
                            TStagedBuffer<DirectionalLightPacked> const& directionalLights,
                            std::span<SpotLightPacked const> spotLights, uint32_t viewCameraIndex,
                            TStagedBuffer<CameraPacked> const& cameras, szg_fill_scene const* sceneGeometry,
                            szg_rowtile const* tile = nullptr)
    {
        detail::note(szg_deferred_record_draw_commands(m_handle, cmd, drawRect, tile, &sceneTexture.texture(),
                                                atmosphericDirectionalLightsCount, directionalLights.deviceAddress(),
                                                static_cast<uint32_t>(directionalLights.deviceSize()), spotLights.data(),
                                                static_cast<uint32_t>(spotLights.size()), viewCameraIndex,
                                                cameras.deviceAddress(), sceneGeometry), "szg_deferred_record_draw_commands", m_lastStatus);
    }
    // deferred.hpp:34-44 with the reference's own last argument, std::span<MeshInstanced const> sceneGeometry
    // (szg/raster.h): shadow raster, G-buffer raster, lights.
    void recordDrawCommands(hipStream_t cmd, szg_rect drawRect, SceneTexture& sceneTexture,
                            uint32_t atmosphericDirectionalLightsCount,
                            TStagedBuffer<DirectionalLightPacked> const& directionalLights,
                            std::span<SpotLightPacked const> spotLights, uint32_t viewCameraIndex,
                            TStagedBuffer<CameraPacked> const& cameras, std::span<szg_mesh_instanced const> sceneGeometry,
                            szg_rowtile const* tile = nullptr)
    {
        detail::note(szg_deferred_record_draw_commands_meshes(m_handle, cmd, drawRect, tile, &sceneTexture.texture(),
                                                       atmosphericDirectionalLightsCount, directionalLights.deviceAddress(),
                                                       static_cast<uint32_t>(directionalLights.deviceSize()), spotLights.data(),
                                                       static_cast<uint32_t>(spotLights.size()), viewCameraIndex,
                                                       cameras.deviceAddress(), sceneGeometry.data(),
                                                       static_cast<uint32_t>(sceneGeometry.size())), "szg_deferred_record_draw_commands_meshes", m_lastStatus);
    }
    [[nodiscard]] auto lastStatus() const -> int { return m_lastStatus; } // status of the last record call (SZG_OK or negative)
    [[nodiscard]] auto gbuffer() -> szg_gbuffer const& { return *szg_deferred_gbuffer(m_handle); }          // deferred.hpp:46
    [[nodiscard]] auto shadowMaps() -> szg_shadowmaps const& { return *szg_deferred_shadow_maps(m_handle); } // deferred.hpp:47
    void cleanup() // deferred.hpp:49
    {
        szg_deferred_destroy(m_handle);
        m_handle = nullptr;
    }
    [[nodiscard]] auto getConfiguration() const -> Configuration // deferred.hpp:114
    {
        Configuration c{};
        (void)szg_deferred_get_configuration(m_handle, &c);
        return c;
    }
    void setConfiguration(Configuration c) { (void)szg_deferred_set_configuration(m_handle, &c); } // deferred.hpp:115
    // szg/mipmaps.h: the mip chains of the material textures (copied; an empty span clears the table) and the sampler's
    // maxLod: SZG_SAMPLER_MAX_LOD_REFERENCE is what the reference's sampler has (vulkanstructs.cpp:147-183).
    auto setTextureMips(std::span<szg_texture_mips const> entries, float maxLod = SZG_SAMPLER_MAX_LOD_NONE) -> int
    {
        return detail::note(szg_deferred_set_texture_mips(m_handle, entries.data(), static_cast<uint32_t>(entries.size()), maxLod),
                            "szg_deferred_set_texture_mips", m_lastStatus);
    }
    // szg/anisotropy.h: the sampler's maxAnisotropy, SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE (1.0, the reference's:
    // vulkanstructs.cpp:171-172) to SZG_SAMPLER_MAX_ANISOTROPY_LIMIT; it applies to the maps that have a chain.
    auto setSamplerAnisotropy(float maxAnisotropy) -> int
    {
        return detail::note(szg_deferred_set_sampler_anisotropy(m_handle, maxAnisotropy), "szg_deferred_set_sampler_anisotropy", m_lastStatus);
    }
    [[nodiscard]] auto valid() const -> bool { return m_handle != nullptr; }

private:
    szg_deferred_t* m_handle{nullptr};
    int m_lastStatus{SZG_OK};
};

// pipelines/skyview.hpp:24-51
struct SkyViewComputePipeline
{
    auto operator=(SkyViewComputePipeline&&) -> SkyViewComputePipeline& = delete;
    SkyViewComputePipeline(SkyViewComputePipeline const&) = delete;
    auto operator=(SkyViewComputePipeline const&) -> SkyViewComputePipeline& = delete;
    SkyViewComputePipeline(SkyViewComputePipeline&& o) noexcept : m_handle(o.m_handle) { o.m_handle = nullptr; }
    ~SkyViewComputePipeline() { szg_skyview_destroy(m_handle); }

    // skyview.hpp:36-37; nullptr on any failure (skyview.cpp:713-740)
    [[nodiscard]] static auto create(int device = 0, szg_skyview_desc const* desc = nullptr)
        -> std::unique_ptr<SkyViewComputePipeline>
    {
        szg_skyview_t* h = nullptr;
        if (szg_skyview_create(&h, desc, device) != SZG_OK)
        {
            return nullptr;
        }
        return std::unique_ptr<SkyViewComputePipeline>(new SkyViewComputePipeline(h));
    }

    // skyview.hpp:39-51
    void recordDrawCommands(hipStream_t cmd, SceneTexture& sceneTexture, szg_rect drawRect, szg_gbuffer const& gbuffer,
                            szg_shadowmaps const& shadowMaps, uint32_t atmosphereIndex,
                            TStagedBuffer<AtmospherePacked> const& atmospheres, uint32_t viewCameraIndex,
                            TStagedBuffer<CameraPacked> const& cameras, uint32_t sunLightIndex,
                            TStagedBuffer<DirectionalLightPacked> const& lights, szg_rowtile const* tile = nullptr)
    {
        detail::note(szg_skyview_record_draw_commands(m_handle, cmd, &sceneTexture.texture(), drawRect, tile, &gbuffer, &shadowMaps,
                                               atmosphereIndex, atmospheres.deviceAddress(), viewCameraIndex,
                                               cameras.deviceAddress(), sunLightIndex, lights.deviceAddress()), "szg_skyview_record_draw_commands", m_lastStatus);
    }
    // ---- extensions without a reference counterpart (szg/abi.h) ----
    // LUT reuse across frames whose atmosphere / sun / camera position are unchanged (identical results)
    [[nodiscard]] auto lastStatus() const -> int { return m_lastStatus; } // status of the last record call (SZG_OK or negative)
    void setLUTReuse(bool enable) { (void)szg_skyview_set_lut_reuse(m_handle, enable ? 1 : 0); }
    void invalidateLUTs(uint32_t which = SZG_LUT_TRANSMITTANCE | SZG_LUT_SKYVIEW) { (void)szg_skyview_invalidate_luts(m_handle, which); }
    // szg/multiscatter_sky.h: SZG_MULTISCATTER_OFF (the reference's single scattering, the default), _ADD or _ONLY. With a mode
    // set recordDrawCommands records the multi-scattering LUT between the transmittance and the sky-view LUT.
    auto setMultiScattering(uint32_t mode) -> int
    {
        return detail::note(szg_skyview_set_multiscatter(m_handle, mode), "szg_skyview_set_multiscatter", m_lastStatus);
    }
    [[nodiscard]] auto multiScattering() const -> uint32_t
    {
        uint32_t mode = SZG_MULTISCATTER_OFF;
        (void)szg_skyview_get_multiscatter(m_handle, &mode);
        return mode;
    }
    // Row-tiled multi-GPU frame: transmittance LUT, this rank's slice of the sky-view LUT, the all-gather of the slices on
    // `lutStream` (ordered behind `cmd` by an event), then the composite on `cmd` once the LUT is complete.
    void recordDrawCommandsTiled(hipStream_t cmd, hipStream_t lutStream, hipEvent_t scratchEvent, szg_rowtile_comm_t* comm,
                                 SceneTexture& sceneTexture, szg_rect drawRect, szg_gbuffer const& gbuffer,
                                 szg_shadowmaps const& shadowMaps, uint32_t atmosphereIndex,
                                 TStagedBuffer<AtmospherePacked> const& atmospheres, uint32_t viewCameraIndex,
                                 TStagedBuffer<CameraPacked> const& cameras, uint32_t sunLightIndex,
                                 TStagedBuffer<DirectionalLightPacked> const& lights, szg_rowtile const& tile)
    {
        uint32_t begin = 0, end = 0;
        detail::note(szg_skyview_record_transmittance(m_handle, cmd, atmosphereIndex, atmospheres.deviceAddress()), "szg_skyview_record_transmittance", m_lastStatus);
        if (szg_skyview_lut_row_slice(m_handle, tile.rank, tile.nranks, &begin, &end) == SZG_OK)
        {
            detail::note(szg_skyview_record_skyview_lut_rows(m_handle, cmd, atmosphereIndex, atmospheres.deviceAddress(), viewCameraIndex,
                                                      cameras.deviceAddress(), begin, end), "szg_skyview_record_skyview_lut_rows", m_lastStatus);
            (void)hipEventRecord(scratchEvent, cmd);
            (void)hipStreamWaitEvent(lutStream, scratchEvent, 0);
            detail::note(szg_skyview_allgather_lut_rows(m_handle, comm, lutStream), "szg_skyview_allgather_lut_rows", m_lastStatus);
            (void)hipEventRecord(scratchEvent, lutStream);
            (void)hipStreamWaitEvent(cmd, scratchEvent, 0);
        }
        else
        {
            // the LUT's rows do not divide over the ranks (every rank sees that alike): each rank computes the whole LUT,
            // as the single-GPU frame does, and the optional second collective is skipped
            detail::note(szg_skyview_record_skyview_lut(m_handle, cmd, atmosphereIndex, atmospheres.deviceAddress(), viewCameraIndex,
                                                 cameras.deviceAddress()), "szg_skyview_record_skyview_lut", m_lastStatus);
        }
        detail::note(szg_skyview_record_composite(m_handle, cmd, &sceneTexture.texture(), drawRect, &tile, &gbuffer, &shadowMaps,
                                           atmosphereIndex, atmospheres.deviceAddress(), viewCameraIndex, cameras.deviceAddress(),
                                           sunLightIndex, lights.deviceAddress()), "szg_skyview_record_composite", m_lastStatus);
    }
    [[nodiscard]] auto transmittanceLUT() const -> szg_image
    {
        szg_image im{};
        (void)szg_skyview_transmittance_lut(m_handle, &im);
        return im;
    }
    [[nodiscard]] auto skyviewLUT() const -> szg_image
    {
        szg_image im{};
        (void)szg_skyview_skyview_lut(m_handle, &im);
        return im;
    }

private:
    explicit SkyViewComputePipeline(szg_skyview_t* h) : m_handle(h) {}
    szg_skyview_t* m_handle{nullptr};
    int m_lastStatus{SZG_OK};
};

// pipelines.hpp:39-44
struct DrawResultsGraphics
{
    size_t drawCalls{0};
    size_t verticesDrawn{0};
    size_t indicesDrawn{0};
};

// pipelines.hpp:238-268 over szg/debuglines.h: the debug-line pass. Without the Vulkan handles: no image formats, no depth
// attachment (compare ALWAYS into a renderer-private image nothing reads, szg/debuglines.h), no index buffer (the
// reference binds it and draws non-indexed).
struct DebugLineGraphicsPipeline
{
    using VertexPacked = szg_vertex_packed;

    explicit DebugLineGraphicsPipeline(uint32_t vertexCapacity = SZG_DEBUG_LINES_CAPACITY, int device = 0)
    {
        if (szg_debug_lines_create(&m_handle, vertexCapacity, device) != SZG_OK)
        {
            std::fprintf(stderr, "[szg] DebugLineGraphicsPipeline: %s\n", szg_last_error());
            m_handle = nullptr;
        }
    }
    ~DebugLineGraphicsPipeline() { cleanup(); }
    DebugLineGraphicsPipeline(DebugLineGraphicsPipeline const&) = delete;
    auto operator=(DebugLineGraphicsPipeline const&) -> DebugLineGraphicsPipeline& = delete;

    [[nodiscard]] auto valid() const -> bool { return m_handle != nullptr; }
    [[nodiscard]] auto lastStatus() const -> int { return m_lastStatus; }

    // pipelines.cpp:463-581: endpoints.deviceSize() vertices as a line list over the scene colour
    auto recordDrawCommands(hipStream_t cmd, float lineWidth, szg_rect drawRect, SceneTexture& sceneTexture, uint32_t cameraIndex,
                            TStagedBuffer<CameraPacked> const& cameras, TStagedBuffer<VertexPacked> const& endpoints,
                            szg_rowtile const* tile = nullptr) -> DrawResultsGraphics
    {
        uint32_t const n = static_cast<uint32_t>(endpoints.deviceSize());
        if (detail::note(szg_debug_lines_record(m_handle, cmd, lineWidth, drawRect, tile, &sceneTexture.texture(), cameraIndex,
                                                cameras.deviceAddress(), endpoints.deviceAddress(), n),
                         "szg_debug_lines_record", m_lastStatus) != SZG_OK)
        {
            return DrawResultsGraphics{};
        }
        return DrawResultsGraphics{1, n, n};
    }

    void cleanup()
    {
        szg_debug_lines_destroy(m_handle);
        m_handle = nullptr;
    }

  private:
    szg_debug_lines_t* m_handle{nullptr};
    int m_lastStatus{SZG_OK};
};
// ---- present pass (szg/present.h) ----
// Free functions, as in the reference. They return the C-ABI status, log a negative one like the pipelines' record calls
// and keep it in lastPresentStatus() (per thread).
namespace detail
{
inline auto presentStatus() -> int&
{
    thread_local int status{SZG_OK};
    return status;
}
} // namespace detail
[[nodiscard]] inline auto lastPresentStatus() -> int { return detail::presentStatus(); }

// imageoperations.cpp:87-119: the VkRect2D form, VK_FILTER_LINEAR (:81). Scales srcSize of `source` (RGBA16_UNORM) onto
// dstSize of `destination` (RGBA8 / BGRA8 / A2B10G10R10) and converts; both offsets are honoured. `encode` is this
// library's addition: a transfer function applied to the taps, so that the source keeps its linear values.
inline auto recordCopyImageToImage(hipStream_t cmd, szg_image const& source, szg_image const& destination, szg_rect srcSize,
                                   szg_rect dstSize, uint32_t encode = SZG_PRESENT_ENCODE_NONE) -> int
{
    szg_present_info const info{srcSize, dstSize, SZG_FILTER_LINEAR, encode};
    return detail::note(szg_record_present(cmd, &source, &destination, &info), "szg_record_present", detail::presentStatus());
}
// imageoperations.cpp:141-176: the form behind Image::recordCopyEntire / recordCopyRect (image.cpp:185-229), corners instead
// of rectangles and VK_FILTER_NEAREST (:169). The aspect mask is dropped (colour only); a max corner below its min corner (a
// flipped blit, which a szg_rect cannot express) is refused. An RGBA16_SFLOAT destination (the texture viewer's display image,
// the reference's own use of this form) is the image copy of szg/texture_display.h; every other one the present pass, as ever.
struct Offset2D
{
    int32_t x, y;
};
inline auto recordCopyImageToImage(hipStream_t cmd, szg_image const& src, szg_image const& dst, Offset2D srcMin, Offset2D srcMax,
                                   Offset2D dstMin, Offset2D dstMax) -> int
{
    if (srcMax.x < srcMin.x || srcMax.y < srcMin.y || dstMax.x < dstMin.x || dstMax.y < dstMin.y)
    {
        std::fprintf(stderr, "[szg] recordCopyImageToImage: flipped regions are not supported\n");
        return detail::presentStatus() = SZG_ERR_INVALID_ARGUMENT;
    }
    szg_present_info const info{
        szg_rect{srcMin.x, srcMin.y, static_cast<uint32_t>(srcMax.x - srcMin.x), static_cast<uint32_t>(srcMax.y - srcMin.y)},
        szg_rect{dstMin.x, dstMin.y, static_cast<uint32_t>(dstMax.x - dstMin.x), static_cast<uint32_t>(dstMax.y - dstMin.y)},
        SZG_FILTER_NEAREST, SZG_PRESENT_ENCODE_NONE};
    if (dst.format == SZG_FORMAT_RGBA16_SFLOAT)
    {
        return detail::note(szg_record_copy_image(cmd, &src, &dst, info.src_region, info.dst_region), "szg_record_copy_image",
                            detail::presentStatus());
    }
    return detail::note(szg_record_present(cmd, &src, &dst, &info), "szg_record_present", detail::presentStatus());
}

// What Editor::endFrame records once the frame is drawn (editor.cpp:303-361): the OETF in place on the scene texture, then
// the LINEAR blit of sourceSubregion onto the WHOLE swapchain image. The reference dispatches the OETF over the top-left
// SWAPCHAIN extent of the scene texture, not over sourceSubregion (editor.cpp:328-337): with an offset or a scaled subregion
// the encoded texels are not the presented ones. That is the reference's behaviour and is kept on purpose; the extent is
// clamped to the texture, as the shader's out-of-range stores are dropped.
inline auto recordPresent(hipStream_t cmd, SceneTexture& sceneTexture, szg_rect sourceSubregion, szg_image const& swapchainImage,
                          uint32_t gammaFunction = SZG_OETF_SRGB) -> int
{
    szg_image const& color = sceneTexture.color();
    uint32_t const w = swapchainImage.width < color.width ? swapchainImage.width : color.width;
    uint32_t const h = swapchainImage.height < color.height ? swapchainImage.height : color.height;
    if (detail::note(szg_record_oetf(cmd, &color, w, h, gammaFunction), "szg_record_oetf", detail::presentStatus()) != SZG_OK)
    {
        return detail::presentStatus();
    }
    return recordCopyImageToImage(cmd, color, swapchainImage, sourceSubregion,
                                  szg_rect{0, 0, swapchainImage.width, swapchainImage.height});
}
// The same frame end in one pass: the transfer function is applied to the blit's taps (szg/present.h ENCODE), exactly the
// texels that are presented, and the scene texture keeps its linear values. 12 B/px at 1:1 instead of 16 + 12.
inline auto recordPresentEncoded(hipStream_t cmd, SceneTexture const& sceneTexture, szg_rect sourceSubregion,
                                 szg_image const& swapchainImage, uint32_t encode = SZG_OETF_SRGB) -> int
{
    return recordCopyImageToImage(cmd, sceneTexture.color(), swapchainImage, sourceSubregion,
                                  szg_rect{0, 0, swapchainImage.width, swapchainImage.height}, encode);
}

// ---- compute-collection pipeline (szg/compute_collection.h) ----
// The class the reference calls ComputeCollectionPipeline (renderer/pipelines.hpp:166-235, pipelines.cpp:223-368), with its
// public names, over szg_record_compute_collection. Here the collection is a fixed table of four programs
// (renderer.cpp:238-243) that the library describes, so an object is one array of {reflection, byte block} entries and a
// cursor: there are no Vulkan handles, no shader paths and nothing to load, the constructor touches no device, and the
// collection is never empty. Every block is zero-filled at construction and keeps its bytes while another program is
// selected.
struct ComputeCollectionPipeline
{
    // what the reference's ShaderReflectionData::PushConstant tells the editor about one program
    using PushConstant = szg_cc_reflection;

    ComputeCollectionPipeline()
    {
        for (uint32_t program = 0; program < SZG_COMPUTE_COLLECTION_SHADER_COUNT; program++)
        {
            // on failure the entry keeps a zero block size: its spans are empty and a record call is refused by the library
            if (szg_compute_collection_reflect(program, &m_reflections[program]) != SZG_OK)
            {
                std::fprintf(stderr, "[szg] ComputeCollectionPipeline: %s\n", szg_last_error());
                m_reflections[program] = PushConstant{};
                m_valid = false;
            }
        }
    }

    [[nodiscard]] auto valid() const -> bool { return m_valid; }
    [[nodiscard]] auto lastStatus() const -> int { return m_lastStatus; }

    // The selected program over the top-left drawExtent of the scene colour (only the extent of the rectangle is used, as the
    // reference passes sceneSubregion.extent). The library copies the bytes before it returns and replaces their first 16
    // with offset (0, 0) and the extent (szg/compute_collection.h, RECORD).
    void recordDrawCommands(hipStream_t cmd, SceneTexture& sceneTexture, szg_rect drawExtent) const
    {
        recordDrawCommands(cmd, sceneTexture.color(), drawExtent.width, drawExtent.height);
    }
    void recordDrawCommands(hipStream_t cmd, szg_image const& color, uint32_t width, uint32_t height) const
    {
        detail::note(szg_record_compute_collection(cmd, m_selected, m_blocks[m_selected].data(), blockBytes(), &color, width, height),
                     "szg_record_compute_collection", m_lastStatus);
    }

    void cleanup() {} // nothing is owned on the device

    // the selected program's block: editable in place / read-only
    auto mapPushConstantBytes() -> std::span<uint8_t> { return {m_blocks[m_selected].data(), blockBytes()}; }
    [[nodiscard]] auto readPushConstantBytes() const -> std::span<uint8_t const> { return {m_blocks[m_selected].data(), blockBytes()}; }

    [[nodiscard]] auto currentShader() const -> PushConstant const& { return m_reflections[m_selected]; }

    // An index outside the table is reported and ignored: the selection stays where it was.
    void selectShader(size_t index)
    {
        if (index < m_reflections.size())
        {
            m_selected = static_cast<uint32_t>(index);
            return;
        }
        std::fprintf(stderr, "[szg] ComputeCollectionPipeline::selectShader(%zu): the collection has %zu programs, selection unchanged\n",
                     index, m_reflections.size());
    }
    [[nodiscard]] auto shaderIndex() const -> size_t { return m_selected; }
    [[nodiscard]] auto shaderCount() const -> size_t { return m_reflections.size(); }
    [[nodiscard]] auto shaders() const -> std::span<PushConstant const> { return m_reflections; }

    // This library's addition: write `values` (floats; for a bool member 32-bit words, true = 1) into member `name` of the
    // selected block, found in the reflection table. False when there is no such member or the count is not the member's.
    template <typename T> auto writePushConstant(std::string_view name, std::span<T const> values) -> bool
    {
        static_assert(sizeof(T) == 4, "members are made of 32-bit components");
        PushConstant const& reflection = currentShader();
        for (uint32_t i = 0; i < reflection.member_count; i++)
        {
            szg_cc_member const& member = reflection.members[i];
            if (name == member.name)
            {
                if (values.size_bytes() != member.size_bytes || member.offset_bytes + member.size_bytes > blockBytes())
                {
                    return false;
                }
                std::memcpy(m_blocks[m_selected].data() + member.offset_bytes, values.data(), member.size_bytes);
                return true;
            }
        }
        return false;
    }

  private:
    using Block = std::array<uint8_t, SZG_COMPUTE_COLLECTION_MAX_BLOCK_BYTES>;
    // bytes of the selected block that belong to its program (the arrays have the size of the largest block)
    [[nodiscard]] auto blockBytes() const -> uint32_t { return m_reflections[m_selected].padded_size_bytes; }

    std::array<PushConstant, SZG_COMPUTE_COLLECTION_SHADER_COUNT> m_reflections{};
    std::array<Block, SZG_COMPUTE_COLLECTION_SHADER_COUNT> m_blocks{}; // zero-filled
    uint32_t m_selected{0};
    bool m_valid{true};
    mutable int m_lastStatus{SZG_OK};
};
} // namespace szg

// UILayer (editor/uilayer.hpp): builds on SceneTexture, TStagedBuffer and detail::note above
#include "szg/ui_layer.hpp"
// TextureDisplay (ui/texturedisplay.hpp): builds on UILayer and recordCopyImageToImage above
#include "szg/texture_display.hpp"
