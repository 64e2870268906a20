// asset_library_mips.cpp — the C++ mirror of szg/mipmaps.h through its own interface (tests/test_gpu_cpp_mipmaps.py):
// an AssetLibrary with the generateMips switch on owns chains for the textures it loads, textureMips() hands them to
// DeferredShadingPipeline::setTextureMips, and a library with the switch off has none.
// usage: asset_library_mips TEXTURE.png OUT_PREFIX   -> OUT_PREFIX.level0 / OUT_PREFIX.chain (the loaded texture, sRGB)
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "szg/assets.hpp"

static int fail(char const* what)
{
    std::fprintf(stderr, "asset_library_mips: %s\n", what);
    return 1;
}

int main(int argc, char** argv)
{
    if (argc != 3)
    {
        return fail("usage: asset_library_mips TEXTURE.png OUT_PREFIX");
    }
    auto plain = szg::AssetLibrary::loadDefaultAssets();
    if (!plain.has_value() || plain->generateMips() || !plain->textureMips().empty())
    {
        return fail("a library without the switch must carry no chain");
    }
    if (plain->loadTextureFromPath(true, argv[1]) == nullptr || !plain->textureMips().empty())
    {
        return fail("a texture loaded without the switch must carry no chain");
    }
    plain->setGenerateMips(true);
    if (plain->loadTextureFromPath(true, argv[1]) == nullptr || plain->textureMips().size() != 1)
    {
        return fail("setGenerateMips(true) must give the next texture a chain");
    }

    auto library = szg::AssetLibrary::loadDefaultAssets(true);
    if (!library.has_value() || !library->generateMips())
    {
        return fail("loadDefaultAssets(true)");
    }
    auto entries = library->textureMips();
    if (entries.size() != 3) // the three default maps, 64 x 64: 7 levels
    {
        return fail("the three default maps must carry chains");
    }
    for (auto const& e : entries)
    {
        if (e.level0_data == nullptr || e.d_chain == nullptr || e.level_count != szg_mip_level_count(SZG_DEFAULT_MAP_DIMENSIONS, SZG_DEFAULT_MAP_DIMENSIONS))
        {
            return fail("a default map's entry is incomplete");
        }
    }
    auto view = library->loadTextureFromPath(true, argv[1]);
    if (view == nullptr || view->mipLevels != szg_mip_level_count(view->width, view->height) || view->mipChain == nullptr)
    {
        return fail("loadTextureFromPath with the switch on must build the full chain");
    }
    entries = library->textureMips();
    if (entries.size() != 4 || entries.back().level0_data != view->data || entries.back().d_chain != view->mipChain)
    {
        return fail("textureMips() must list the loaded texture");
    }
    szg::DeferredShadingPipeline deferred(64, 64, 1, 0);
    if (!deferred.valid() || deferred.setTextureMips(entries) != SZG_OK || deferred.setTextureMips({}, SZG_SAMPLER_MAX_LOD_REFERENCE) != SZG_OK)
    {
        return fail("setTextureMips");
    }
    if (deferred.setTextureMips(entries, -1.0f) != SZG_ERR_INVALID_ARGUMENT || deferred.lastStatus() != SZG_ERR_INVALID_ARGUMENT)
    {
        return fail("a negative maxLod must be refused");
    }
    if (hipDeviceSynchronize() != hipSuccess)
    {
        return fail("hipDeviceSynchronize");
    }
    std::vector<char> level0(size_t{view->width} * view->height * 4), chain(szg_mip_chain_bytes(view->width, view->height));
    if (hipMemcpy(level0.data(), view->data, level0.size(), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(chain.data(), view->mipChain, chain.size(), hipMemcpyDeviceToHost) != hipSuccess)
    {
        return fail("hipMemcpy");
    }
    std::ofstream(std::string(argv[2]) + ".level0", std::ios::binary).write(level0.data(), (std::streamsize)level0.size());
    std::ofstream(std::string(argv[2]) + ".chain", std::ios::binary).write(chain.data(), (std::streamsize)chain.size());
    std::printf("OK %u %u %u\n", view->width, view->height, view->mipLevels);
    return 0;
}
