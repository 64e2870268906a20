// record_draw_compute_collection.cpp — szg::Renderer::recordDraw (include/szg/scene.hpp) with the editor's pipeline switch
// (reference renderer.cpp:379-439, ui/engineui.cpp:19-22) on the editor's start-up scene. argv: PREFIX WIDTH HEIGHT
// TEXTURE_WIDTH TEXTURE_HEIGHT; PREFIX.blocks.bin holds the four push-constant blocks back to back (80 + 48 + 80 + 208 bytes).
// One renderer never leaves DEFERRED (.reference.bin). The other is switched to COMPUTE_COLLECTION with its G-buffer and the
// scene depth poisoned, records each of the four programs (.cc0.bin .. .cc3.bin, the whole scene colour), then
// selectShader(7) and the frame again (.cc7.bin), then back to DEFERRED (.back.bin). tests/test_gpu_compute_collection_renderer.py
// compiles it with hipcc and checks the images against the CPU model.
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
bool writeColor(std::string const& path, szg::SceneTexture const& texture, hipStream_t cmd)
{
    if (hipStreamSynchronize(cmd) != hipSuccess)
    {
        std::fprintf(stderr, "stream failed\n");
        return false;
    }
    szg_image const& color = texture.color();
    std::vector<uint16_t> host((size_t)color.width * color.height * 4);
    (void)hipMemcpy2D(host.data(), (size_t)color.width * 8, color.data, color.pitch_bytes, (size_t)color.width * 8, color.height,
                      hipMemcpyDeviceToHost);
    return writeFile(path, host.data(), host.size() * 2);
}
size_t imageBytes(szg_image const& im) { return (size_t)im.pitch_bytes * im.height; }
// every byte of the image's allocation still `value`?
bool holds(szg_image const& im, int value)
{
    std::vector<unsigned char> host(imageBytes(im));
    (void)hipMemcpy(host.data(), im.data, host.size(), hipMemcpyDeviceToHost);
    for (unsigned char b : host)
    {
        if (b != (unsigned char)value)
        {
            return false;
        }
    }
    return true;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 6)
    {
        std::fprintf(stderr, "usage: %s PREFIX WIDTH HEIGHT TEXTURE_WIDTH TEXTURE_HEIGHT\n", argv[0]);
        return 2;
    }
    std::string const prefix = argv[1];
    uint32_t const W = (uint32_t)std::atoi(argv[2]), H = (uint32_t)std::atoi(argv[3]);
    uint32_t const TW = (uint32_t)std::atoi(argv[4]), TH = (uint32_t)std::atoi(argv[5]);
    std::vector<unsigned char> blocks(80 + 48 + 80 + 208);
    {
        FILE* f = std::fopen((prefix + ".blocks.bin").c_str(), "rb");
        if (f == nullptr || std::fread(blocks.data(), 1, blocks.size(), f) != blocks.size())
        {
            std::fprintf(stderr, "cannot read %s.blocks.bin\n", prefix.c_str());
            return 2;
        }
        std::fclose(f);
    }
    auto library = szg::AssetLibrary::loadDefaultAssets();
    auto reference = szg::Renderer::create(W, H, 512);
    auto renderer = szg::Renderer::create(W, H, 512);
    auto referenceTexture = szg::SceneTexture::create(TW, TH);
    auto sceneTexture = szg::SceneTexture::create(TW, TH);
    if (!library.has_value() || !reference.has_value() || !renderer.has_value() || !referenceTexture || !sceneTexture)
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

    // a renderer that never switched
    std::printf("default pipeline %d\n", (int)reference->activeRenderingPipeline());
    reference->recordDraw(cmd, scene, *referenceTexture, sceneSubregion);
    if (!writeColor(prefix + ".reference.bin", *referenceTexture, cmd))
    {
        return 1;
    }

    // the switched one: poison what the collection must not touch
    szg_gbuffer const& g = renderer->deferredShadingPipeline().gbuffer();
    szg_image const planes[5] = {g.diffuse, g.specular, g.normal, g.worldPosition, g.occlusionRoughnessMetallic};
    for (szg_image const& plane : planes)
    {
        (void)hipMemset(plane.data, 0xA5, imageBytes(plane));
    }
    (void)hipMemset(sceneTexture->depth().data, 0x5A, imageBytes(sceneTexture->depth()));
    (void)hipMemset(sceneTexture->color().data, 0xC3, imageBytes(sceneTexture->color()));
    (void)hipDeviceSynchronize();
    renderer->setActiveRenderingPipeline(szg::RenderingPipelines::COMPUTE_COLLECTION);
    szg::ComputeCollectionPipeline& collection = renderer->genericComputePipeline();
    std::printf("shaders %zu\n", collection.shaderCount());
    size_t offset = 0;
    for (size_t index = 0; index < collection.shaderCount(); index++)
    {
        collection.selectShader(index);
        std::span<uint8_t> const bytes = collection.mapPushConstantBytes();
        bool zeros = true;
        for (uint8_t b : bytes)
        {
            zeros = zeros && b == 0;
        }
        std::printf("shader %zu %s bytes %zu zeros %d\n", index, collection.currentShader().name, bytes.size(), zeros ? 1 : 0);
        std::memcpy(bytes.data(), blocks.data() + offset, bytes.size());
        offset += bytes.size();
        renderer->recordDraw(cmd, scene, *sceneTexture, sceneSubregion);
        std::memset(bytes.data(), 0xEE, bytes.size()); // push-constant semantics: the bytes were copied at record time
        if (!writeColor(prefix + ".cc" + std::to_string(index) + ".bin", *sceneTexture, cmd))
        {
            return 1;
        }
        std::memcpy(bytes.data(), blocks.data() + offset - bytes.size(), bytes.size());
    }
    bool untouched = holds(sceneTexture->depth(), 0x5A);
    for (szg_image const& plane : planes)
    {
        untouched = untouched && holds(plane, 0xA5);
    }
    std::printf("gbuffer and depth untouched %d status %d lines staged %zu drawn %zu\n", untouched ? 1 : 0, collection.lastStatus(),
                renderer->debugLines().vertices.stagedSize(), renderer->debugLines().lastFrameDrawResults.drawCalls);

    collection.selectShader(7); // outside the table: a warning and no change
    std::printf("after selectShader(7) index %zu\n", collection.shaderIndex());
    renderer->recordDraw(cmd, scene, *sceneTexture, sceneSubregion);
    if (!writeColor(prefix + ".cc7.bin", *sceneTexture, cmd))
    {
        return 1;
    }
    // the typed helper finds members in the reflection table
    collection.selectShader(1);
    float const top[4] = {0.25f, 0.5f, 0.75f, 1.0f};
    bool const wrote = collection.writePushConstant<float>("topColor", top) && !collection.writePushConstant<float>("row1", top) &&
                       !collection.writePushConstant<float>("bottomColor", std::span<float const>{top, 2});
    std::printf("writePushConstant %d\n", wrote && std::memcmp(collection.readPushConstantBytes().data() + 16, top, 16) == 0 ? 1 : 0);

    renderer->setActiveRenderingPipeline(szg::RenderingPipelines::DEFERRED);
    renderer->recordDraw(cmd, scene, *sceneTexture, sceneSubregion);
    if (!writeColor(prefix + ".back.bin", *sceneTexture, cmd))
    {
        return 1;
    }
    (void)hipStreamDestroy(cmd);
    std::printf("ok\n");
    return 0;
}
