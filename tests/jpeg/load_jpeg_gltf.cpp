// load_jpeg_gltf.cpp — the C++ mirror of include/szg/jpeg.h through its own interface (tests/test_gpu_cpp_jpeg.py):
// AssetLibrary::loadGLTFFromPath(path, SZG_GLTF_JPEG_FOR_DEVICE) and loadTextureFromPath with setDecodeJPEG, mip chains on.
// Every texture the library registered after the defaults is downloaded to <out>.<k>.rgba (and <out>.<k>.chain) and listed
// on stdout as "TEX <k> <name> <width> <height> <srgb> <mip levels>".
//
//   load_jpeg_gltf file.gltf out-prefix [file.jpg]
#include <cstdio>
#include <string>
#include <vector>

#include "szg/assets.hpp"

static bool dump(std::string const& path, void const* device, size_t bytes)
{
    std::vector<unsigned char> host(bytes);
    if (bytes > 0 && hipMemcpy(host.data(), device, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    {
        return false;
    }
    FILE* f = std::fopen(path.c_str(), "wb");
    if (f == nullptr)
    {
        return false;
    }
    std::fwrite(host.data(), 1, bytes, f);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 3)
    {
        std::fprintf(stderr, "usage: load_jpeg_gltf file.gltf out-prefix [file.jpg]\n");
        return 2;
    }
    auto library = szg::AssetLibrary::loadDefaultAssets(true);
    if (!library.has_value())
    {
        std::fprintf(stderr, "loadDefaultAssets failed: %s\n", szg_last_error());
        return 1;
    }
    size_t const defaults = library->textures().size();
    library->loadGLTFFromPath(argv[1], SZG_GLTF_JPEG_FOR_DEVICE);
    if (argc > 3)
    {
        if (library->loadTextureFromPath(true, argv[3]) != nullptr)
        {
            std::fprintf(stderr, "a JPEG file loaded although setDecodeJPEG is off\n");
            return 1;
        }
        library->setDecodeJPEG(true);
        if (library->loadTextureFromPath(true, argv[3]) == nullptr)
        {
            std::fprintf(stderr, "loadTextureFromPath failed with setDecodeJPEG on\n");
            return 1;
        }
    }
    if (hipDeviceSynchronize() != hipSuccess)
    {
        return 1;
    }
    auto const textures = library->textures();
    for (size_t k = defaults; k < textures.size(); k++)
    {
        szg::ImageView const& t = *textures[k];
        std::string const base = std::string(argv[2]) + "." + std::to_string(k - defaults);
        if (!dump(base + ".rgba", t.data, size_t{t.width} * t.height * 4) ||
            !dump(base + ".chain", t.mipChain, t.mipLevels > 1 ? szg_mip_chain_bytes(t.width, t.height) : 0))
        {
            std::fprintf(stderr, "download failed\n");
            return 1;
        }
        std::printf("TEX %zu %s %u %u %d %u\n", k - defaults, t.name.c_str(), t.width, t.height, t.srgb ? 1 : 0, t.mipLevels);
    }
    std::printf("OK %zu\n", textures.size() - defaults);
    return 0;
}
