// szg/ui_layer.hpp — header-only C++ mirror of the reference's UILayer (editor/uilayer.hpp:36-114) over szg/ui_layer.h: the
// part of it that is a render pass. Included by szg/pipelines.hpp.
//
//   reference                                                   this header
//   ----------------------------------------------------------- ------------------------------------------------------------
//   UILayer::create(..., VkExtent2D textureCapacity, ...)       szg::UILayer::create(textureCapacity): both textures at the
//     uilayer.cpp:285-328                                         capacity, the scene texture registered NEAREST / CLAMP_TO_BORDER
//   ImGui_ImplVulkan_Init / CreateDeviceObjects                 (inside create: szg_ui_layer_create)
//   ImGui_ImplVulkan_AddTexture(sampler, view, layout)          addTexture(image, sampler) -> szg_ui_texture_t*, usable as ImTextureID;
//                                                                 addTextureView(image, sampler, view) for a view with a component
//                                                                 mapping or a half-float image (szg/texture_display.h)
//   UILayer::sceneTexture(), sceneViewport(forceFocus)          the same names; {focused, texture, renderedSubregion}
//   UILayer::recordDraw(cmd) -> optional<UIOutputImage>         recordDraw(cmd, drawData): ImGui::GetDrawData() is the caller's
//     uilayer.cpp:513-572
//
// recordDraw is a template over the draw-data type and reads Dear ImGui's member names, so it takes a real ImDrawData
// unchanged: CmdListsCount, CmdLists[n]->VtxBuffer.Data / .Size, ->IdxBuffer.Data / .Size, ->CmdBuffer.Size and
// ->CmdBuffer[i] with .ClipRect.x .. .w, .TextureId, .VtxOffset, .IdxOffset, .ElemCount, .UserCallback; DisplayPos, DisplaySize,
// FramebufferScale (.x, .y). The lists are concatenated with the backend's global vertex and index offsets
// (ImGui_ImplVulkan_RenderDrawData) through TStagedBuffer. COMMANDS WITH A UserCallback ARE SKIPPED: a callback is not a
// draw, and ImDrawCallback_ResetRenderState has nothing to reset here. ImDrawVert must have the default 20-byte layout and
// ImDrawIdx 16 bits (thirdparty/imgui/imguiconfig.h keeps both).
//
// Widgets, layout, fonts and the ImGui context itself stay with the caller.
#pragma once

#include <algorithm>
#include <functional>
#include <optional>
#include <type_traits>
#include <utility>

#include "szg/pipelines.hpp"
#include "szg/texture_display.h"
#include "szg/ui_layer.h"

namespace szg
{
// uilayer.hpp:23-28
struct SceneViewport
{
    bool focused;
    std::reference_wrapper<SceneTexture> texture;
    szg_rect renderedSubregion;
};
// uilayer.hpp:30-34: what Editor::endFrame presents
struct UIOutputImage
{
    std::reference_wrapper<SceneTexture> texture;
    szg_rect renderedSubregion;
};

struct UILayer
{
    UILayer(UILayer const&) = delete;
    auto operator=(UILayer const&) -> UILayer& = delete;
    UILayer(UILayer&& o) noexcept { *this = std::move(o); }
    auto operator=(UILayer&& o) noexcept -> UILayer&
    {
        destroy();
        m_layer = std::exchange(o.m_layer, nullptr);
        m_sceneTexture = std::move(o.m_sceneTexture);
        m_outputTexture = std::move(o.m_outputTexture);
        m_sceneHandle = std::exchange(o.m_sceneHandle, nullptr);
        m_viewport = o.m_viewport;
        m_vertices = std::move(o.m_vertices);
        m_indices = std::move(o.m_indices);
        m_commands = std::move(o.m_commands);
        m_lastStatus = o.m_lastStatus;
        return *this;
    }
    ~UILayer() { destroy(); }

    // uilayer.cpp:285-328. triangleCapacity / commandCapacity bound one frame's draw data (szg_ui_layer_create).
    static auto create(uint32_t capacityWidth, uint32_t capacityHeight, uint32_t triangleCapacity = 1u << 16,
                       uint32_t commandCapacity = 4096u, int device = 0) -> std::optional<UILayer>
    {
        UILayer layer;
        if (szg_ui_layer_create(&layer.m_layer, triangleCapacity, commandCapacity, device) != SZG_OK)
        {
            std::fprintf(stderr, "[szg] UILayer::create failed: %s\n", szg_last_error());
            return std::nullopt;
        }
        layer.m_outputTexture = SceneTexture::create(capacityWidth, capacityHeight);
        layer.m_sceneTexture = SceneTexture::create(capacityWidth, capacityHeight);
        layer.m_vertices = TStagedBuffer<szg_ui_draw_vert>::allocate(3u * (size_t)triangleCapacity);
        layer.m_indices = TStagedBuffer<uint16_t>::allocate(3u * (size_t)triangleCapacity);
        if (layer.m_outputTexture == nullptr || layer.m_sceneTexture == nullptr || !layer.m_vertices.valid() || !layer.m_indices.valid())
        {
            std::fprintf(stderr, "[szg] Failed to allocate UI Layer textures or buffers.\n");
            return std::nullopt;
        }
        // scenetexture.cpp:104-109: the scene texture's own sampler; uilayer.cpp:318-322
        layer.m_sceneHandle = layer.addTexture(layer.m_sceneTexture->color(), szg_ui_sampler{SZG_FILTER_NEAREST, SZG_UI_ADDRESS_CLAMP_TO_BORDER});
        if (layer.m_sceneHandle == nullptr)
        {
            return std::nullopt;
        }
        layer.m_viewport = szg_rect{0, 0, capacityWidth, capacityHeight};
        return layer;
    }

    [[nodiscard]] auto sceneTexture() -> SceneTexture& { return *m_sceneTexture; }
    [[nodiscard]] auto outputTexture() -> SceneTexture& { return *m_outputTexture; }
    // m_imguiSceneTextureHandle: the ImTextureID of the scene viewport quad
    [[nodiscard]] auto sceneTextureHandle() const -> szg_ui_texture_t* { return m_sceneHandle; }

    // What the "Scene Viewport" window measures (ui/statelesswidgets.cpp:868-885): the content extent, clamped to the capacity.
    // The window itself is the caller's; its quad has uv_max = sceneViewportUVMax().
    void setSceneViewportExtent(uint32_t width, uint32_t height)
    {
        m_viewport = szg_rect{0, 0, std::min(width, m_sceneTexture->color().width), std::min(height, m_sceneTexture->color().height)};
    }
    [[nodiscard]] auto sceneViewportUVMax() const -> std::array<float, 2>
    {
        return {static_cast<float>(m_viewport.width) / static_cast<float>(m_sceneTexture->color().width),
                static_cast<float>(m_viewport.height) / static_cast<float>(m_sceneTexture->color().height)};
    }
    // uilayer.cpp:412-448
    auto sceneViewport(bool forceFocus = false) -> std::optional<SceneViewport>
    {
        if (m_sceneTexture == nullptr || m_viewport.width == 0u || m_viewport.height == 0u)
        {
            return std::nullopt;
        }
        return SceneViewport{forceFocus, *m_sceneTexture, m_viewport};
    }

    // ImGui_ImplVulkan_AddTexture / RemoveTexture; nullptr (and a log line) when refused
    auto addTexture(szg_image const& image, szg_ui_sampler sampler) -> szg_ui_texture_t*
    {
        szg_ui_texture_t* out = nullptr;
        detail::note(szg_ui_layer_add_texture(m_layer, &image, sampler, &out), "szg_ui_layer_add_texture", m_lastStatus);
        return out;
    }
    // the same with an image view (szg/texture_display.h): RGBA16_SFLOAT images too, `view` maps the components
    auto addTextureView(szg_image const& image, szg_ui_sampler sampler, szg_ui_texture_view const& view) -> szg_ui_texture_t*
    {
        szg_ui_texture_t* out = nullptr;
        detail::note(szg_ui_layer_add_texture_view(m_layer, &image, sampler, &view, &out), "szg_ui_layer_add_texture_view", m_lastStatus);
        return out;
    }
    void removeTexture(szg_ui_texture_t* texture)
    {
        detail::note(szg_ui_layer_remove_texture(m_layer, texture), "szg_ui_layer_remove_texture", m_lastStatus);
    }

    // uilayer.cpp:513-572: render area (int32)DisplayPos, (uint32)DisplaySize (:536-545), clear to (0, 0, 0, 1), draw.
    template <typename DrawData> auto recordDraw(hipStream_t cmd, DrawData const& drawData) -> std::optional<UIOutputImage>
    {
        if (m_outputTexture == nullptr)
        {
            std::fprintf(stderr, "[szg] UI Layer had no texture to render to.\n");
            return std::nullopt;
        }
        szg_rect const renderedArea{static_cast<int32_t>(drawData.DisplayPos.x), static_cast<int32_t>(drawData.DisplayPos.y),
                                    static_cast<uint32_t>(drawData.DisplaySize.x), static_cast<uint32_t>(drawData.DisplaySize.y)};
        m_vertices.clearStaged();
        m_indices.clearStaged();
        m_commands.clear();
        uint32_t globalVtx = 0, globalIdx = 0;
        for (int n = 0; n < drawData.CmdListsCount; n++)
        {
            auto const& list = *drawData.CmdLists[n];
            using Vert = std::remove_cv_t<std::remove_pointer_t<decltype(list.VtxBuffer.Data)>>;
            using Idx = std::remove_cv_t<std::remove_pointer_t<decltype(list.IdxBuffer.Data)>>;
            static_assert(sizeof(Vert) == sizeof(szg_ui_draw_vert), "ImDrawVert must keep its default layout");
            static_assert(sizeof(Idx) == sizeof(uint16_t), "ImDrawIdx must be 16 bits");
            for (int i = 0; i < list.CmdBuffer.Size; i++)
            {
                auto const& c = list.CmdBuffer[i];
                if (c.UserCallback != nullptr)
                {
                    continue;
                }
                szg_ui_draw_cmd out{};
                out.clip_rect[0] = c.ClipRect.x;
                out.clip_rect[1] = c.ClipRect.y;
                out.clip_rect[2] = c.ClipRect.z;
                out.clip_rect[3] = c.ClipRect.w;
                out.texture = toTexture(c.TextureId);
                out.vtx_offset = globalVtx + static_cast<uint32_t>(c.VtxOffset);
                out.idx_offset = globalIdx + static_cast<uint32_t>(c.IdxOffset);
                out.elem_count = static_cast<uint32_t>(c.ElemCount);
                m_commands.push_back(out);
            }
            m_vertices.push(std::span<szg_ui_draw_vert const>{reinterpret_cast<szg_ui_draw_vert const*>(list.VtxBuffer.Data),
                                                              static_cast<size_t>(list.VtxBuffer.Size)});
            m_indices.push(std::span<uint16_t const>{reinterpret_cast<uint16_t const*>(list.IdxBuffer.Data),
                                                     static_cast<size_t>(list.IdxBuffer.Size)});
            globalVtx += static_cast<uint32_t>(list.VtxBuffer.Size);
            globalIdx += static_cast<uint32_t>(list.IdxBuffer.Size);
        }
        if (m_vertices.stagedSize() != globalVtx || m_indices.stagedSize() != globalIdx)
        {
            std::fprintf(stderr, "[szg] UILayer::recordDraw: the draw data exceeds the layer's vertex / index capacity\n");
            return std::nullopt;
        }
        m_vertices.recordCopyToDevice(cmd);
        m_indices.recordCopyToDevice(cmd);
        szg_ui_draw_data data{};
        data.display_pos[0] = drawData.DisplayPos.x;
        data.display_pos[1] = drawData.DisplayPos.y;
        data.display_size[0] = drawData.DisplaySize.x;
        data.display_size[1] = drawData.DisplaySize.y;
        data.framebuffer_scale[0] = drawData.FramebufferScale.x;
        data.framebuffer_scale[1] = drawData.FramebufferScale.y;
        data.d_vertices = m_vertices.deviceAddress();
        data.vertex_count = globalVtx;
        data.d_indices = m_indices.deviceAddress();
        data.index_count = globalIdx;
        data.commands = m_commands.data();
        data.command_count = static_cast<uint32_t>(m_commands.size());
        float const clear[4] = {0.0F, 0.0F, 0.0F, 1.0F}; // uilayer.cpp:551-553
        if (detail::note(szg_ui_layer_record_draw(m_layer, cmd, &m_outputTexture->color(), renderedArea, SZG_UI_LOAD_OP_CLEAR, clear, &data),
                         "szg_ui_layer_record_draw", m_lastStatus) != SZG_OK)
        {
            return std::nullopt;
        }
        return UIOutputImage{*m_outputTexture, renderedArea};
    }

    [[nodiscard]] auto lastStatus() const -> int { return m_lastStatus; }

private:
    UILayer() = default;
    void destroy()
    {
        szg_ui_layer_destroy(m_layer);
        m_layer = nullptr;
    }
    // ImTextureID is void* by default and an integer in later versions of Dear ImGui
    template <typename Id> static auto toTexture(Id id) -> szg_ui_texture_t const*
    {
        if constexpr (std::is_pointer_v<Id>)
        {
            return static_cast<szg_ui_texture_t const*>(static_cast<void const*>(id));
        }
        else
        {
            return reinterpret_cast<szg_ui_texture_t const*>(static_cast<uintptr_t>(id));
        }
    }

    szg_ui_layer_t* m_layer{nullptr};
    std::unique_ptr<SceneTexture> m_sceneTexture;
    std::unique_ptr<SceneTexture> m_outputTexture;
    szg_ui_texture_t* m_sceneHandle{nullptr};
    szg_rect m_viewport{};
    TStagedBuffer<szg_ui_draw_vert> m_vertices;
    TStagedBuffer<uint16_t> m_indices;
    std::vector<szg_ui_draw_cmd> m_commands;
    int m_lastStatus{SZG_OK};
};
} // namespace szg
