// skyview_multiscatter.cpp — a C++ caller of SkyViewComputePipeline::setMultiScattering (include/szg/pipelines.hpp over
// szg/multiscatter_sky.h): one small frame through recordDrawCommands in the mode given on the command line, then the
// 64 x 32 sky-view LUT and the packed atmosphere and camera blocks it was computed from are written to files, so that
// tests/test_gpu_multiscatter_sky.py repeats the frame through the Python mirror on the same blocks and compares the bits.
//   skyview_multiscatter <mode> <prefix>   ->   <prefix>.skyview (64 * 32 * 4 floats), <prefix>.atmosphere, <prefix>.camera
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "szg/pipelines.hpp"

static bool writeFile(std::string const& path, const void* data, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    bool const ok = f != nullptr && std::fwrite(data, 1, bytes, f) == bytes;
    return (f == nullptr || std::fclose(f) == 0) && ok;
}

int main(int argc, char** argv)
{
    if (argc != 3)
    {
        std::fprintf(stderr, "usage: skyview_multiscatter mode prefix\n");
        return 2;
    }
    uint32_t const mode = (uint32_t)std::atoi(argv[1]);
    std::string const prefix = argv[2];
    uint32_t const W = 160, H = 90, LW = 64, LH = 32;

    szg_camera camera;
    szg_camera_default(&camera);
    szg_camera_packed cameraPacked;
    szg_camera_to_device_equivalent(&camera, (float)W / (float)H, &cameraPacked);
    szg_atmosphere atmosphere;
    szg_atmosphere_default_earth(&atmosphere);
    atmosphere.sunEulerAngles[0] = 3.14159265358979f + 35.0f * 3.14159265358979f / 180.0f;
    szg_aabb const bounds{{0.0f, -7.0f, 39.0f}, {64.0f, 8.0f, 46.0f}};
    szg_atmosphere_packed atmospherePacked;
    szg_directional_light_packed sun, moon;
    szg_atmosphere_baked(&atmosphere, &bounds, &atmospherePacked, &sun, &moon);

    auto cameras = szg::TStagedBuffer<szg::CameraPacked>::allocate(1);
    auto atmospheres = szg::TStagedBuffer<szg::AtmospherePacked>::allocate(1);
    auto lights = szg::TStagedBuffer<szg::DirectionalLightPacked>::allocate(2);
    auto sceneTexture = szg::SceneTexture::create(W, H);
    szg::DeferredShadingPipeline deferred(W, H, 1, 0, 0);
    szg_skyview_desc const desc{512u, 128u, LW, LH, 0u, 0u};
    auto skyView = szg::SkyViewComputePipeline::create(0, &desc);
    if (!cameras.valid() || !atmospheres.valid() || !lights.valid() || !sceneTexture || !deferred.valid() || !skyView)
    {
        std::fprintf(stderr, "setup failed: %s\n", szg_last_error());
        return 1;
    }
    // the mirror refuses what the C-ABI refuses, and reports what it holds
    if (skyView->multiScattering() != SZG_MULTISCATTER_OFF || skyView->setMultiScattering(3u) != SZG_ERR_INVALID_ARGUMENT ||
        skyView->multiScattering() != SZG_MULTISCATTER_OFF || skyView->setMultiScattering(mode) != SZG_OK ||
        skyView->multiScattering() != mode)
    {
        std::fprintf(stderr, "setMultiScattering / multiScattering: %s\n", szg_last_error());
        return 1;
    }

    hipStream_t cmd = nullptr;
    (void)hipStreamCreate(&cmd);
    cameras.push(cameraPacked);
    cameras.recordCopyToDevice(cmd);
    atmospheres.push(atmospherePacked);
    atmospheres.recordCopyToDevice(cmd);
    lights.push(sun);
    lights.push(moon);
    lights.recordCopyToDevice(cmd);

    szg_fill_box boxes[1] = {{{0.0f, -8.0f, 6.0f}, {5.0f, 5.0f, 5.0f}, 0.0f, 60.0f / 255.0f}};
    szg_fill_scene const geometry{-1.0f, 4000.0f, 4.0f, 60.0f / 255.0f, 1, 0, boxes};
    szg_rect const region{0, 0, W, H};
    std::vector<szg::SpotLightPacked> const noSpots;
    deferred.recordDrawCommands(cmd, region, *sceneTexture, 1, lights, noSpots, 0, cameras, &geometry);
    // transmittance -> multi-scatter -> sky-view -> composite when a mode is set (szg/multiscatter_sky.h "WHERE")
    skyView->recordDrawCommands(cmd, *sceneTexture, region, deferred.gbuffer(), deferred.shadowMaps(), 0, atmospheres, 0, cameras, 0, lights);
    if (skyView->lastStatus() != SZG_OK || hipStreamSynchronize(cmd) != hipSuccess)
    {
        std::fprintf(stderr, "frame failed: %s\n", szg_last_error());
        return 1;
    }
    szg_image const lut = skyView->skyviewLUT();
    std::vector<float> host((size_t)LW * LH * 4);
    if (lut.width != LW || lut.height != LH ||
        hipMemcpy2D(host.data(), (size_t)LW * 16, lut.data, lut.pitch_bytes, (size_t)LW * 16, LH, hipMemcpyDeviceToHost) != hipSuccess)
    {
        std::fprintf(stderr, "download failed\n");
        return 1;
    }
    if (!writeFile(prefix + ".skyview", host.data(), host.size() * sizeof(float)) ||
        !writeFile(prefix + ".atmosphere", &atmospherePacked, sizeof atmospherePacked) ||
        !writeFile(prefix + ".camera", &cameraPacked, sizeof cameraPacked))
    {
        std::fprintf(stderr, "cannot write %s.*\n", prefix.c_str());
        return 1;
    }
    std::printf("ok mode %u\n", skyView->multiScattering());
    (void)hipStreamDestroy(cmd);
    return 0;
}
