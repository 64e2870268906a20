// record_present.cpp — the frame end of include/szg/pipelines.hpp from a C++ caller (reference editor.cpp:303-361):
//   record_present IN W H SX SY SW SH DW DH FORMAT PREFIX
// uploads the W x H RGBA16 scene colour of IN into a szg::SceneTexture and records, each on a fresh upload,
//   szg::recordPresent          OETF (sRGB) in place over the top-left DW x DH + LINEAR blit of (SX, SY, SW, SH) onto DW x DH
//                               -> PREFIX.present.bin (destination), PREFIX.scene.bin (the scene colour afterwards)
//   szg::recordPresentEncoded   the same blit with the transfer function on the taps -> PREFIX.encoded.bin, and
//                               PREFIX.linear.bin (the scene colour afterwards: must equal IN)
//   szg::recordCopyImageToImage the NEAREST corner form -> PREFIX.nearest.bin
// and checks that a refused call is reported through lastPresentStatus(). tests/test_gpu_present.py compiles and runs it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "szg/pipelines.hpp"

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
bool download(std::string const& path, void const* device, size_t bytes)
{
    std::vector<unsigned char> host(bytes);
    return hipMemcpy(host.data(), device, bytes, hipMemcpyDeviceToHost) == hipSuccess && writeFile(path, host.data(), bytes);
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 12)
    {
        std::fprintf(stderr, "usage: %s IN W H SX SY SW SH DW DH FORMAT PREFIX\n", argv[0]);
        return 2;
    }
    uint32_t const W = (uint32_t)std::atoi(argv[2]), H = (uint32_t)std::atoi(argv[3]);
    szg_rect const sub{std::atoi(argv[4]), std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]), (uint32_t)std::atoi(argv[7])};
    uint32_t const DW = (uint32_t)std::atoi(argv[8]), DH = (uint32_t)std::atoi(argv[9]);
    uint32_t const format = (uint32_t)std::atoi(argv[10]);
    std::string const prefix = argv[11];

    size_t const sceneBytes = (size_t)W * H * 8u, dstBytes = (size_t)DW * DH * 4u;
    std::vector<unsigned char> input(sceneBytes);
    FILE* f = std::fopen(argv[1], "rb");
    if (f == nullptr || std::fread(input.data(), 1, sceneBytes, f) != sceneBytes)
    {
        std::fprintf(stderr, "cannot read %zu bytes from %s\n", sceneBytes, argv[1]);
        return 1;
    }
    std::fclose(f);

    auto sceneTexture = szg::SceneTexture::create(W, H);
    szg_image swapchainImage{nullptr, DW, DH, DW * 4u, format};
    hipStream_t cmd = nullptr;
    if (!sceneTexture || hipMalloc(&swapchainImage.data, dstBytes) != hipSuccess || hipStreamCreate(&cmd) != hipSuccess)
    {
        std::fprintf(stderr, "setup failed: %s\n", szg_last_error());
        return 1;
    }
    auto upload = [&]() {
        return hipMemcpy(sceneTexture->color().data, input.data(), sceneBytes, hipMemcpyHostToDevice) == hipSuccess &&
               hipMemset(swapchainImage.data, 0x5A, dstBytes) == hipSuccess;
    };
    auto finish = [&](int status, char const* what) {
        if (status != SZG_OK || szg::lastPresentStatus() != SZG_OK || hipStreamSynchronize(cmd) != hipSuccess)
        {
            std::fprintf(stderr, "%s failed: status %d, %s\n", what, status, szg_last_error());
            return false;
        }
        return true;
    };

    if (!upload() || !finish(szg::recordPresent(cmd, *sceneTexture, sub, swapchainImage, SZG_OETF_SRGB), "recordPresent") ||
        !download(prefix + ".present.bin", swapchainImage.data, dstBytes) ||
        !download(prefix + ".scene.bin", sceneTexture->color().data, sceneBytes))
    {
        return 1;
    }
    if (!upload() || !finish(szg::recordPresentEncoded(cmd, *sceneTexture, sub, swapchainImage, SZG_OETF_SRGB), "recordPresentEncoded") ||
        !download(prefix + ".encoded.bin", swapchainImage.data, dstBytes) ||
        !download(prefix + ".linear.bin", sceneTexture->color().data, sceneBytes))
    {
        return 1;
    }
    szg::Offset2D const srcMin{sub.x, sub.y}, srcMax{sub.x + (int32_t)sub.width, sub.y + (int32_t)sub.height};
    if (!upload() ||
        !finish(szg::recordCopyImageToImage(cmd, sceneTexture->color(), swapchainImage, srcMin, srcMax, szg::Offset2D{0, 0},
                                            szg::Offset2D{(int32_t)DW, (int32_t)DH}),
                "recordCopyImageToImage (NEAREST)") ||
        !download(prefix + ".nearest.bin", swapchainImage.data, dstBytes))
    {
        return 1;
    }
    // a refusal (the subregion moved out of the texture) is reported, not silently dropped
    szg_rect const outside{(int32_t)W, 0, sub.width, sub.height};
    int const refused = szg::recordCopyImageToImage(cmd, sceneTexture->color(), swapchainImage, outside, szg_rect{0, 0, DW, DH});
    if (refused != SZG_ERR_INVALID_ARGUMENT || szg::lastPresentStatus() != SZG_ERR_INVALID_ARGUMENT)
    {
        std::fprintf(stderr, "a region outside the image was not refused (status %d)\n", refused);
        return 1;
    }
    (void)hipStreamDestroy(cmd);
    (void)hipFree(swapchainImage.data);
    std::printf("record_present ok\n");
    return 0;
}
