// szg/texture_display.hpp — header-only C++ mirror of the reference's TextureDisplay (ui/texturedisplay.hpp, .cpp) over
// szg/texture_display.h: the part of the Texture Viewer window that runs on the GPU. Included by szg/pipelines.hpp.
//
//   reference                                                   this header
//   ----------------------------------------------------------- ------------------------------------------------------------
//   TextureDisplay::create(device, allocator, queue, pool,      szg::TextureDisplay::create(uiLayer, width, height, format): the
//     extent, format)  texturedisplay.cpp:23-145                  display image, cleared to opaque black before create returns
//     editor.cpp:485-505: TEXTURE_MAX^2, R16G16B16A16_SFLOAT      (the immediate submit of :147-162), registered NEAREST /
//                                                                 CLAMP_TO_BORDER through a view with alpha ONE (:69-80, :104-120)
//   uiRender's copy of the picked texture (:164-195)            recordSelect(cmd, imageView): Image::recordCopyEntire, the NEAREST
//     -> Image::recordCopyEntire                                  blit of the whole asset image onto the whole display image;
//   picking "None" -> recordClearColorImage (:147-162)            recordSelect(cmd, nullptr)
//   ImGui::Image(m_imguiDescriptor, imageSize) (:291-304)       imguiDescriptor(), imageSize(contentWidth): the widget's quad is
//                                                                 the caller's (ImGui::Image, or a quad of the draw data)
//
// The list box, the regex search, the property table and the file dialog are out of scope. Move-only; destruction removes the
// texture from the layer, which must outlive the display.
#pragma once

#include <array>
#include <cstddef>
#include <optional>
#include <utility>

#include "szg/pipelines.hpp"
#include "szg/texture_display.h"

namespace szg
{
struct TextureDisplay
{
    TextureDisplay(TextureDisplay const&) = delete;
    auto operator=(TextureDisplay const&) -> TextureDisplay& = delete;
    TextureDisplay(TextureDisplay&& o) noexcept { *this = std::move(o); }
    auto operator=(TextureDisplay&& o) noexcept -> TextureDisplay&
    {
        destroy();
        m_layer = std::exchange(o.m_layer, nullptr);
        m_image = std::exchange(o.m_image, szg_image{});
        m_descriptor = std::exchange(o.m_descriptor, nullptr);
        m_lastStatus = o.m_lastStatus;
        return *this;
    }
    ~TextureDisplay() { destroy(); }

    // texturedisplay.cpp:23-145. `format`: RGBA16_SFLOAT (the editor's), or RGBA16_UNORM for a display that only shows clears
    // and is drawn without the copy; the copy itself needs the half-float destination.
    static auto create(UILayer& uiLayer, uint32_t width, uint32_t height, uint32_t format = SZG_FORMAT_RGBA16_SFLOAT)
        -> std::optional<TextureDisplay>
    {
        if (width == 0u || height == 0u || (format != SZG_FORMAT_RGBA16_SFLOAT && format != SZG_FORMAT_RGBA16_UNORM))
        {
            std::fprintf(stderr, "[szg] TextureDisplay::create: an empty extent or a format that cannot be displayed.\n");
            return std::nullopt;
        }
        TextureDisplay display;
        display.m_layer = &uiLayer;
        display.m_image = szg_image{nullptr, width, height, width * 8u, format};
        if (hipMalloc(&display.m_image.data, (size_t)width * height * 8u) != hipSuccess)
        {
            std::fprintf(stderr, "[szg] Failed to allocate the texture display image.\n");
            return std::nullopt;
        }
        // :147-162, an immediate submit: the image is opaque black when create returns
        float const black[4] = {0.0F, 0.0F, 0.0F, 1.0F};
        if (detail::note(szg_record_clear_color_image(nullptr, &display.m_image, black), "szg_record_clear_color_image", display.m_lastStatus) != SZG_OK ||
            hipStreamSynchronize(nullptr) != hipSuccess)
        {
            return std::nullopt;
        }
        // :69-80 the sampler, :104-120 the view with components.a = VK_COMPONENT_SWIZZLE_ONE
        szg_ui_texture_view const view{{SZG_SWIZZLE_IDENTITY, SZG_SWIZZLE_IDENTITY, SZG_SWIZZLE_IDENTITY, SZG_SWIZZLE_ONE}};
        display.m_descriptor = uiLayer.addTextureView(display.m_image, szg_ui_sampler{SZG_FILTER_NEAREST, SZG_UI_ADDRESS_CLAMP_TO_BORDER}, view);
        if (display.m_descriptor == nullptr)
        {
            return std::nullopt;
        }
        return display;
    }

    // :164-195. `view` is an szg::ImageView (szg/assets.hpp) or anything whose texture() returns a szg_texture: RGBA8 texels,
    // sRGB-encoded or not by its srgb flag. Returns the C-ABI status.
    template <typename View> auto recordSelect(hipStream_t cmd, View const* view) -> int
    {
        if (view == nullptr)
        {
            return recordSelect(cmd, nullptr);
        }
        szg_texture const t = view->texture();
        return recordSelect(cmd, szg_image{const_cast<void*>(t.data), t.width, t.height, t.pitch_bytes,
                                           t.srgb != 0u ? uint32_t{SZG_FORMAT_RGBA8_SRGB} : uint32_t{SZG_FORMAT_RGBA8_UNORM}});
    }
    // "None": the display image becomes opaque black
    auto recordSelect(hipStream_t cmd, std::nullptr_t) -> int
    {
        float const black[4] = {0.0F, 0.0F, 0.0F, 1.0F};
        return detail::note(szg_record_clear_color_image(cmd, &m_image, black), "szg_record_clear_color_image", m_lastStatus);
    }
    // any image the copy accepts: a half-float plane of the G-buffer, the scene colour (RGBA16_UNORM)
    auto recordSelect(hipStream_t cmd, szg_image const& source) -> int
    {
        // Image::recordCopyEntire (image.cpp:191-206): both whole images
        m_lastStatus = recordCopyImageToImage(cmd, source, m_image, Offset2D{0, 0},
                                              Offset2D{static_cast<int32_t>(source.width), static_cast<int32_t>(source.height)}, Offset2D{0, 0},
                                              Offset2D{static_cast<int32_t>(m_image.width), static_cast<int32_t>(m_image.height)});
        return m_lastStatus;
    }

    // m_imguiDescriptor: the ImTextureID of the widget's image
    [[nodiscard]] auto imguiDescriptor() const -> szg_ui_texture_t* { return m_descriptor; }
    [[nodiscard]] auto image() const -> szg_image const& { return m_image; }
    // :291-295: ImVec2{contentWidth, aspectRatio * contentWidth} with aspectRatio = width / height. The reference's
    // expression; it is only right for a square image, and that is kept.
    [[nodiscard]] auto imageSize(float contentWidth) const -> std::array<float, 2>
    {
        float const aspectRatio = static_cast<float>(m_image.width) / static_cast<float>(m_image.height);
        return {contentWidth, aspectRatio * contentWidth};
    }
    [[nodiscard]] auto lastStatus() const -> int { return m_lastStatus; }

private:
    TextureDisplay() = default;
    void destroy()
    {
        if (m_layer != nullptr && m_descriptor != nullptr)
        {
            m_layer->removeTexture(m_descriptor);
        }
        if (m_image.data != nullptr)
        {
            (void)hipFree(m_image.data); // waits for the device: nothing reads the image any more
        }
        m_layer = nullptr;
        m_descriptor = nullptr;
        m_image = szg_image{};
    }

    UILayer* m_layer{nullptr};
    szg_image m_image{};
    szg_ui_texture_t* m_descriptor{nullptr};
    int m_lastStatus{SZG_OK};
};
} // namespace szg
