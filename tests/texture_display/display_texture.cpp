// An engine-style caller of szg::TextureDisplay (include/szg/texture_display.hpp): the editor's Texture Viewer over a hand-made
// draw-data struct in Dear ImGui's shape (member names and layouts of imgui.h v1.90.6, nothing else of it).
//   display_texture <map.bin (RGBA8)> <mapW> <mapH> <srgb> <displayW> <displayH> <frameW> <frameH> <out.bin>
// Frame 1: the map is selected (szg::ImageView -> Image::recordCopyEntire) and the viewer quad drawn over a panel.
// Frame 2: "None" is selected and the same draw data drawn again. Both output images are written, one after the other.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "szg/assets.hpp"
#include "szg/pipelines.hpp"

struct ImVec2
{
    float x, y;
};
struct ImVec4
{
    float x, y, z, w;
};
template <typename T> struct ImVector
{
    int Size = 0;
    int Capacity = 0;
    T* Data = nullptr;
    T& operator[](int i) { return Data[i]; }
    T const& operator[](int i) const { return Data[i]; }
};
using ImTextureID = void*;
using ImDrawIdx = unsigned short;
struct ImDrawList;
struct ImDrawCmd;
using ImDrawCallback = void (*)(ImDrawList const*, ImDrawCmd const*);
struct ImDrawVert
{
    ImVec2 pos;
    ImVec2 uv;
    uint32_t col;
};
struct ImDrawCmd
{
    ImVec4 ClipRect;
    ImTextureID TextureId;
    unsigned int VtxOffset;
    unsigned int IdxOffset;
    unsigned int ElemCount;
    ImDrawCallback UserCallback;
    void* UserCallbackData;
};
struct ImDrawList
{
    ImVector<ImDrawCmd> CmdBuffer;
    ImVector<ImDrawIdx> IdxBuffer;
    ImVector<ImDrawVert> VtxBuffer;
};
struct ImDrawData
{
    bool Valid;
    int CmdListsCount;
    int TotalIdxCount;
    int TotalVtxCount;
    ImVector<ImDrawList*> CmdLists;
    ImVec2 DisplayPos;
    ImVec2 DisplaySize;
    ImVec2 FramebufferScale;
};

namespace
{
struct List
{
    std::vector<ImDrawVert> v;
    std::vector<ImDrawIdx> i;
    std::vector<ImDrawCmd> c;
    ImDrawList list;
    void rect(ImVec2 a, ImVec2 b, ImVec2 uva, ImVec2 uvb, uint32_t col, ImVec4 clip, ImTextureID tex)
    {
        ImDrawIdx const base = static_cast<ImDrawIdx>(v.size());
        c.push_back(ImDrawCmd{clip, tex, 0u, static_cast<unsigned>(i.size()), 6u, nullptr, nullptr});
        for (ImDrawIdx k : {0, 1, 2, 0, 2, 3})
        {
            i.push_back(static_cast<ImDrawIdx>(base + k));
        }
        v.push_back({a, uva, col});
        v.push_back({{b.x, a.y}, {uvb.x, uva.y}, col});
        v.push_back({b, uvb, col});
        v.push_back({{a.x, b.y}, {uva.x, uvb.y}, col});
    }
    ImDrawList* finish()
    {
        list.VtxBuffer.Data = v.data();
        list.VtxBuffer.Size = static_cast<int>(v.size());
        list.IdxBuffer.Data = i.data();
        list.IdxBuffer.Size = static_cast<int>(i.size());
        list.CmdBuffer.Data = c.data();
        list.CmdBuffer.Size = static_cast<int>(c.size());
        return &list;
    }
};

bool append(FILE* f, szg_image const& image)
{
    std::vector<uint16_t> host((size_t)image.width * image.height * 4);
    return hipMemcpy(host.data(), image.data, host.size() * 2, hipMemcpyDeviceToHost) == hipSuccess &&
           std::fwrite(host.data(), 2, host.size(), f) == host.size();
}
} // namespace

int main(int argc, char** argv)
{
    if (argc != 10)
    {
        return 2;
    }
    uint32_t const mapW = std::atoi(argv[2]), mapH = std::atoi(argv[3]), srgb = std::atoi(argv[4]);
    uint32_t const displayW = std::atoi(argv[5]), displayH = std::atoi(argv[6]), frameW = std::atoi(argv[7]), frameH = std::atoi(argv[8]);
    std::vector<uint8_t> map((size_t)mapW * mapH * 4);
    FILE* f = std::fopen(argv[1], "rb");
    if (f == nullptr || std::fread(map.data(), 1, map.size(), f) != map.size())
    {
        return 3;
    }
    std::fclose(f);

    std::optional<szg::UILayer> layer = szg::UILayer::create(frameW, frameH, 64, 8);
    if (!layer.has_value())
    {
        return 4;
    }
    szg::UILayer ui = std::move(layer).value();
    std::optional<szg::TextureDisplay> created = szg::TextureDisplay::create(ui, displayW, displayH);
    if (!created.has_value() || szg::TextureDisplay::create(ui, 0, 4).has_value() ||
        szg::TextureDisplay::create(ui, 4, 4, SZG_FORMAT_RGBA8_UNORM).has_value())
    {
        return 5;
    }
    szg::TextureDisplay display = std::move(created).value(); // moves, as the reference's does
    if (display.imguiDescriptor() == nullptr || display.image().format != SZG_FORMAT_RGBA16_SFLOAT)
    {
        return 6;
    }
    std::shared_ptr<szg::ImageView const> view = szg::ImageView::upload(map.data(), mapW, mapH, srgb != 0u, "map");
    void* d_white = nullptr;
    uint32_t const white = 0xFFFFFFFFu;
    if (view == nullptr || hipMalloc(&d_white, 4) != hipSuccess || hipMemcpy(d_white, &white, 4, hipMemcpyHostToDevice) != hipSuccess)
    {
        return 7;
    }
    szg_ui_texture_t* font = ui.addTexture(szg_image{d_white, 1, 1, 4, SZG_FORMAT_RGBA8_UNORM}, szg_ui_sampler{SZG_FILTER_LINEAR, SZG_UI_ADDRESS_REPEAT});
    if (font == nullptr)
    {
        return 8;
    }

    float const fw = static_cast<float>(frameW), fh = static_cast<float>(frameH);
    ImVec4 const everything{0.0F, 0.0F, fw, fh};
    auto const size = display.imageSize(22.0F); // the widget: texturedisplay.cpp:291-304
    List a;
    a.rect({2, 2}, {fw - 2.0F, fh - 2.0F}, {0.5F, 0.5F}, {0.5F, 0.5F}, 0xFF503C28u, everything, font);
    a.rect({12, 4}, {12.0F + size[0], 4.0F + size[1]}, {-0.125F, 0.0F}, {1.0F, 1.125F}, 0xFFC8E6FFu, everything, display.imguiDescriptor());
    ImDrawList* lists[1] = {a.finish()};
    ImDrawData data{};
    data.Valid = true;
    data.CmdListsCount = 1;
    data.CmdLists.Data = lists;
    data.CmdLists.Size = 1;
    data.DisplayPos = {0.0F, 0.0F};
    data.DisplaySize = {fw, fh};
    data.FramebufferScale = {1.0F, 1.0F};

    hipStream_t stream = nullptr;
    if (hipStreamCreate(&stream) != hipSuccess)
    {
        return 9;
    }
    f = std::fopen(argv[9], "wb");
    if (f == nullptr)
    {
        return 10;
    }
    // frame 1: the map
    if (display.recordSelect(stream, view.get()) != SZG_OK)
    {
        return 11;
    }
    std::optional<szg::UIOutputImage> out = ui.recordDraw(stream, data);
    if (!out.has_value() || hipStreamSynchronize(stream) != hipSuccess || !append(f, out->texture.get().color()))
    {
        return 12;
    }
    // frame 2: "None"
    szg::ImageView const* none = nullptr;
    if (display.recordSelect(stream, none) != SZG_OK || display.recordSelect(stream, nullptr) != SZG_OK)
    {
        return 13;
    }
    out = ui.recordDraw(stream, data);
    if (!out.has_value() || hipStreamSynchronize(stream) != hipSuccess || !append(f, out->texture.get().color()))
    {
        return 14;
    }
    // the corner form of the reference's blit still refuses what neither pass takes, and says so
    szg_image const rgba8{d_white, 1, 1, 4, SZG_FORMAT_RGBA8_UNORM};
    if (szg::recordCopyImageToImage(stream, rgba8, ui.outputTexture().color(), {0, 0}, {1, 1}, {0, 0}, {1, 1}) != SZG_ERR_INVALID_ARGUMENT ||
        szg::lastPresentStatus() != SZG_ERR_INVALID_ARGUMENT || display.recordSelect(stream, ui.outputTexture().color()) != SZG_OK)
    {
        return 15;
    }
    // frame 3: an image of the frame itself, the UNORM16 output of frame 2, through recordSelect(cmd, szg_image)
    std::vector<uint16_t> shown((size_t)displayW * displayH * 4);
    if (hipStreamSynchronize(stream) != hipSuccess ||
        hipMemcpy(shown.data(), display.image().data, shown.size() * 2, hipMemcpyDeviceToHost) != hipSuccess ||
        std::fwrite(shown.data(), 2, shown.size(), f) != shown.size())
    {
        return 16;
    }
    std::fclose(f);
    (void)hipStreamDestroy(stream);
    {
        szg::TextureDisplay gone = std::move(display); // destruction removes the texture: the next draw names a stale handle
    }
    if (ui.recordDraw(nullptr, data).has_value() || ui.lastStatus() != SZG_ERR_INVALID_ARGUMENT)
    {
        return 17;
    }
    (void)hipFree(d_white);
    std::printf("OK %u %u\n", frameW, frameH);
    return 0;
}
