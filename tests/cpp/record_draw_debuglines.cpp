// record_draw_debuglines.cpp — szg::Renderer::recordDraw (include/szg/scene.hpp) on the editor's start-up scene with the
// "Debug Lines" switch off, on, and off again (reference renderer.cpp:278-476, engineui.cpp:95-109). Writes, under the
// prefix argv[1]: .off.bin / .on.bin / .off2.bin (RGBA16 scene colour of each frame), .lines.bin (the staged line list of
// the enabled frame), .camera.bin (the camera the renderer staged), .boxes.bin (the transforms and bounds the boxes were
// built from). tests/test_gpu_debuglines_renderer.py compiles it with hipcc and checks the frames against the CPU model.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "szg/assets.hpp"
#include "szg/pipelines.hpp"
#include "szg/scene.hpp"

namespace
{
bool writeFile(std::string const& path, void const* data, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (f == nullptr)
    {
        return false;
    }
    bool const ok = std::fwrite(data, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 5)
    {
        std::fprintf(stderr, "usage: %s PREFIX WIDTH HEIGHT LINE_WIDTH\n", argv[0]);
        return 2;
    }
    std::string const prefix = argv[1];
    uint32_t const W = (uint32_t)std::atoi(argv[2]), H = (uint32_t)std::atoi(argv[3]);
    float const lineWidth = (float)std::atof(argv[4]);
    auto library = szg::AssetLibrary::loadDefaultAssets();
    auto renderer = szg::Renderer::create(W, H, 512);
    auto sceneTexture = szg::SceneTexture::create(W, H);
    if (!library.has_value() || !renderer.has_value() || !sceneTexture)
    {
        std::fprintf(stderr, "setup failed: %s\n", szg_last_error());
        return 1;
    }
    szg::Scene scene = szg::Scene::defaultScene(library->defaultMesh(szg::AssetLibrary::DefaultMeshAssets::Cube));
    scene.sunAnimation.time = 0.6f; // afternoon
    scene.calculateShadowBounds();
    hipStream_t cmd = nullptr;
    (void)hipStreamCreate(&cmd);
    szg_rect const sceneSubregion{0, 0, W, H};
    szg::DebugLines& lines = renderer->debugLines();
    lines.lineWidth = lineWidth;
    char const* const names[3] = {".off.bin", ".on.bin", ".off2.bin"};
    for (int frame = 0; frame < 3; frame++)
    {
        lines.enabled = frame == 1;
        renderer->recordDraw(cmd, scene, *sceneTexture, sceneSubregion);
        if (hipStreamSynchronize(cmd) != hipSuccess)
        {
            std::fprintf(stderr, "stream failed\n");
            return 1;
        }
        std::vector<uint16_t> host((size_t)W * H * 4);
        (void)hipMemcpy2D(host.data(), (size_t)W * 8, sceneTexture->color().data, sceneTexture->color().pitch_bytes, (size_t)W * 8,
                          H, hipMemcpyDeviceToHost);
        if (!writeFile(prefix + names[frame], host.data(), host.size() * 2))
        {
            return 1;
        }
        szg::DrawResultsGraphics const r = lines.lastFrameDrawResults;
        std::printf("frame %d enabled %d staged %zu draw %zu %zu %zu\n", frame, lines.enabled ? 1 : 0, lines.vertices.stagedSize(),
                    r.drawCalls, r.verticesDrawn, r.indicesDrawn);
        if (frame == 1)
        {
            auto const staged = lines.vertices.readValidStaged();
            if (!writeFile(prefix + ".lines.bin", staged.data(), staged.size_bytes()))
            {
                return 1;
            }
        }
    }
    // the camera Renderer::recordDraw staged (renderer.cpp:302-310) and what the boxes were built from
    szg_camera_packed camera{};
    szg_camera_to_device_equivalent(&scene.camera, static_cast<float>(static_cast<double>(W) / static_cast<double>(H)), &camera);
    std::vector<float> boxes;
    for (szg::MeshInstanced const& instance : scene.geometry())
    {
        auto const mesh = instance.getMesh();
        for (szg_transform const& t : instance.transforms)
        {
            float const* p = reinterpret_cast<float const*>(&t);
            boxes.insert(boxes.end(), p, p + 9);
            float const* b = reinterpret_cast<float const*>(&mesh->vertexBounds);
            boxes.insert(boxes.end(), b, b + 6);
        }
    }
    szg_aabb const sb = scene.shadowBounds();
    float const* b = reinterpret_cast<float const*>(&sb);
    boxes.insert(boxes.end(), b, b + 6);
    if (!writeFile(prefix + ".camera.bin", &camera, sizeof camera) || !writeFile(prefix + ".boxes.bin", boxes.data(), boxes.size() * 4))
    {
        return 1;
    }
    (void)hipStreamDestroy(cmd);
    std::printf("ok\n");
    return 0;
}
