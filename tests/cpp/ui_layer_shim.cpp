// An engine-style caller of szg::UILayer (include/szg/ui_layer.hpp) with draw data in Dear ImGui's shape: the types below
// carry ImGui's member names and layouts (imgui.h v1.90.6: ImVector, ImVec2, ImVec4, ImDrawVert, ImDrawCmd, ImDrawList,
// ImDrawData) and nothing else of it, so the template is instantiated exactly as it would be with the real headers.
//   ui_layer_shim <scene.bin (RGBA16, capacity extent)> <capW> <capH> <contentW> <contentH> <displayW> <displayH> <out.bin>
// Two lists: a background rectangle, the scene viewport quad at uv_max = content / capacity, a command with a user callback
// (must be skipped), and in the second list a translucent rectangle under a clip rect.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

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
void callback(ImDrawList const*, ImDrawCmd const*) {}
} // namespace

int main(int argc, char** argv)
{
    if (argc != 9)
    {
        return 2;
    }
    uint32_t const capW = std::atoi(argv[2]), capH = std::atoi(argv[3]), contentW = std::atoi(argv[4]), contentH = std::atoi(argv[5]);
    float const displayW = static_cast<float>(std::atof(argv[6])), displayH = static_cast<float>(std::atof(argv[7]));
    std::vector<uint16_t> scene((size_t)capW * capH * 4);
    FILE* f = std::fopen(argv[1], "rb");
    if (f == nullptr || std::fread(scene.data(), 2, scene.size(), f) != scene.size())
    {
        return 3;
    }
    std::fclose(f);

    std::optional<szg::UILayer> layer = szg::UILayer::create(capW, capH, 1024, 16);
    if (!layer.has_value())
    {
        return 4;
    }
    szg::UILayer ui = std::move(layer).value(); // the layer moves, as the reference's does
    // the renderer's part: the scene texture gets its frame
    if (hipMemcpy(ui.sceneTexture().color().data, scene.data(), scene.size() * 2, hipMemcpyHostToDevice) != hipSuccess)
    {
        return 5;
    }
    ui.setSceneViewportExtent(contentW, contentH);
    std::optional<szg::SceneViewport> viewport = ui.sceneViewport(true);
    if (!viewport.has_value() || viewport->renderedSubregion.width != contentW || &viewport->texture.get() != &ui.sceneTexture())
    {
        return 6;
    }
    // a 1x1 white texture: what untextured primitives sample
    void* d_white = nullptr;
    uint32_t const white = 0xFFFFFFFFu;
    if (hipMalloc(&d_white, 4) != hipSuccess || hipMemcpy(d_white, &white, 4, hipMemcpyHostToDevice) != hipSuccess)
    {
        return 7;
    }
    szg_ui_texture_t* font = ui.addTexture(szg_image{d_white, 1, 1, 4, SZG_FORMAT_RGBA8_UNORM}, szg_ui_sampler{SZG_FILTER_LINEAR, SZG_UI_ADDRESS_REPEAT});
    if (font == nullptr)
    {
        return 8;
    }

    ImVec4 const everything{0.0F, 0.0F, displayW, displayH};
    auto const uvMax = ui.sceneViewportUVMax();
    List a, b;
    a.rect({0, 0}, {displayW, displayH}, {0.5F, 0.5F}, {0.5F, 0.5F}, 0xFF221E1Eu, everything, font);
    a.rect({6, 5}, {6.0F + contentW, 5.0F + contentH}, {0, 0}, {uvMax[0], uvMax[1]}, 0xFFFFFFFFu, everything, ui.sceneTextureHandle());
    a.c.push_back(ImDrawCmd{everything, nullptr, 0u, 0u, 0u, callback, nullptr}); // not a draw
    b.rect({10.5F, 8.25F}, {40.0F, 30.0F}, {0.5F, 0.5F}, {0.5F, 0.5F}, 0xA03C78F0u, {12.7F, 9.2F, 33.9F, 25.5F}, font);
    ImDrawList* lists[2] = {a.finish(), b.finish()};
    ImDrawData data{};
    data.Valid = true;
    data.CmdListsCount = 2;
    data.CmdLists.Data = lists;
    data.CmdLists.Size = 2;
    data.DisplayPos = {0.0F, 0.0F};
    data.DisplaySize = {displayW, displayH};
    data.FramebufferScale = {1.0F, 1.0F};

    hipStream_t stream = nullptr;
    if (hipStreamCreate(&stream) != hipSuccess)
    {
        return 9;
    }
    std::optional<szg::UIOutputImage> out = ui.recordDraw(stream, data);
    if (!out.has_value() || &out->texture.get() != &ui.outputTexture() || out->renderedSubregion.width != static_cast<uint32_t>(displayW))
    {
        return 10;
    }
    // a removed texture is refused by the next draw, and the layer says so
    ui.removeTexture(font);
    if (ui.recordDraw(stream, data).has_value() || ui.lastStatus() != SZG_ERR_INVALID_ARGUMENT)
    {
        return 11;
    }
    if (hipStreamSynchronize(stream) != hipSuccess)
    {
        return 12;
    }
    szg_image const& image = out->texture.get().color();
    std::vector<uint16_t> host((size_t)image.width * image.height * 4);
    if (hipMemcpy(host.data(), image.data, host.size() * 2, hipMemcpyDeviceToHost) != hipSuccess)
    {
        return 13;
    }
    f = std::fopen(argv[8], "wb");
    if (f == nullptr || std::fwrite(host.data(), 2, host.size(), f) != host.size())
    {
        return 14;
    }
    std::fclose(f);
    (void)hipStreamDestroy(stream);
    (void)hipFree(d_white);
    std::printf("OK %u %u\n", image.width, image.height);
    return 0;
}
