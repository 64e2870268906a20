// raster_anisotropy.cpp — the C++ mirror of szg/anisotropy.h through its own interface (tests/test_gpu_raster_anisotropy.py):
// DeferredShadingPipeline::setSamplerAnisotropy beside setTextureMips, then one frame of a mesh whose buffers the test wrote.
//   raster_anisotropy DIR W H MAX_ANISOTROPY
// reads DIR/{vertices,indices,models,mits,camera}.bin and, for each MAP of color, normal, orm, DIR/MAP.bin (RGBA8, square)
// and DIR/MAP_chain.bin (levels 1.., packed); writes DIR/out_{depth,diffuse,specular,normal,worldPosition,orm}.bin.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "szg/pipelines.hpp"

namespace
{
int fail(char const* what)
{
    std::fprintf(stderr, "raster_anisotropy: %s\n", what);
    return 1;
}
std::vector<char> slurp(std::string const& path)
{
    std::ifstream f(path, std::ios::binary);
    return {std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()};
}
void* upload(std::vector<char> const& bytes)
{
    void* d = nullptr;
    if (bytes.empty() || hipMalloc(&d, bytes.size()) != hipSuccess || hipMemcpy(d, bytes.data(), bytes.size(), hipMemcpyHostToDevice) != hipSuccess)
    {
        return nullptr;
    }
    return d;
}
bool download(std::string const& path, szg_image const& image, uint32_t width, uint32_t rows, uint32_t texel)
{
    std::vector<char> host((size_t)width * rows * texel);
    if (hipMemcpy2D(host.data(), (size_t)width * texel, image.data, image.pitch_bytes, (size_t)width * texel, rows, hipMemcpyDeviceToHost) != hipSuccess)
    {
        return false;
    }
    std::ofstream(path, std::ios::binary).write(host.data(), (std::streamsize)host.size());
    return true;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc != 5)
    {
        return fail("usage: raster_anisotropy DIR W H MAX_ANISOTROPY");
    }
    std::string const dir = std::string(argv[1]) + "/";
    uint32_t const W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    float const maxAnisotropy = std::strtof(argv[4], nullptr);

    std::vector<char> const vertices = slurp(dir + "vertices.bin"), indices = slurp(dir + "indices.bin");
    std::vector<char> const models = slurp(dir + "models.bin"), mits = slurp(dir + "mits.bin"), camera = slurp(dir + "camera.bin");
    if (vertices.empty() || indices.empty() || models.size() != sizeof(szg_mat4) || mits.size() != sizeof(szg_mat4) ||
        camera.size() != sizeof(szg::CameraPacked))
    {
        return fail("input files");
    }
    szg_surface surface{};
    surface.first_index = 0;
    surface.index_count = static_cast<uint32_t>(indices.size() / 4);
    std::vector<szg_texture_mips> entries;
    char const* const names[3] = {"color", "normal", "orm"};
    szg_texture* const maps[3] = {&surface.material.color, &surface.material.normal, &surface.material.orm};
    for (int m = 0; m < 3; m++)
    {
        std::vector<char> const level0 = slurp(dir + names[m] + ".bin"), chain = slurp(dir + names[m] + "_chain.bin");
        uint32_t const side = static_cast<uint32_t>(std::lround(std::sqrt((double)level0.size() / 4.0)));
        if ((size_t)side * side * 4 != level0.size() || chain.size() != szg_mip_chain_bytes(side, side))
        {
            return fail("a map is not square or its chain is not the full one");
        }
        *maps[m] = szg_texture{upload(level0), side, side, side * 4, 0};
        entries.push_back(szg_texture_mips{maps[m]->data, upload(chain), szg_mip_level_count(side, side)});
        if (entries.back().level0_data == nullptr || entries.back().d_chain == nullptr)
        {
            return fail("upload of a map");
        }
    }
    szg_mesh_instanced mesh{};
    mesh.d_vertices = static_cast<szg_vertex_packed const*>(upload(vertices));
    mesh.vertex_count = static_cast<uint32_t>(vertices.size() / sizeof(szg_vertex_packed));
    mesh.d_indices = static_cast<uint32_t const*>(upload(indices));
    mesh.index_count = surface.index_count;
    mesh.surfaces = &surface;
    mesh.surface_count = 1;
    mesh.instance_count = 1;
    mesh.d_models = static_cast<szg_mat4 const*>(upload(models));
    mesh.d_model_inverse_transposes = static_cast<szg_mat4 const*>(upload(mits));
    mesh.render = 1;
    mesh.casts_shadow = 1;
    if (mesh.d_vertices == nullptr || mesh.d_indices == nullptr || mesh.d_models == nullptr || mesh.d_model_inverse_transposes == nullptr)
    {
        return fail("upload of the mesh");
    }

    auto cameras = szg::TStagedBuffer<szg::CameraPacked>::allocate(1);
    auto lights = szg::TStagedBuffer<szg::DirectionalLightPacked>::allocate(1);
    auto target = szg::SceneTexture::create(W, H);
    szg::DeferredShadingPipeline deferred(W, H, 1, 0);
    if (!cameras.valid() || !lights.valid() || target == nullptr || !deferred.valid())
    {
        return fail("pipeline objects");
    }
    cameras.push(*reinterpret_cast<szg::CameraPacked const*>(camera.data()));
    cameras.recordCopyToDevice(nullptr);
    lights.recordCopyToDevice(nullptr);

    // every refusal keeps the status and the value; the accepted calls clear the status again
    if (deferred.setSamplerAnisotropy(0.5F) != SZG_ERR_INVALID_ARGUMENT || deferred.lastStatus() != SZG_ERR_INVALID_ARGUMENT ||
        deferred.setSamplerAnisotropy(17.0F) != SZG_ERR_INVALID_ARGUMENT || deferred.setSamplerAnisotropy(std::nanf("")) != SZG_ERR_INVALID_ARGUMENT)
    {
        return fail("a maxAnisotropy outside 1..16 must be refused");
    }
    if (deferred.setSamplerAnisotropy(SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE) != SZG_OK || deferred.setSamplerAnisotropy(maxAnisotropy) != SZG_OK ||
        deferred.lastStatus() != SZG_OK || deferred.setTextureMips(entries, SZG_SAMPLER_MAX_LOD_NONE) != SZG_OK)
    {
        return fail("setSamplerAnisotropy / setTextureMips");
    }
    deferred.recordDrawCommands(nullptr, szg_rect{0, 0, W, H}, *target, 0, lights, {}, 0, cameras, std::span<szg_mesh_instanced const>{&mesh, 1});
    if (deferred.lastStatus() != SZG_OK || hipDeviceSynchronize() != hipSuccess)
    {
        return fail("recordDrawCommands");
    }
    szg_gbuffer const& g = deferred.gbuffer();
    if (!download(dir + "out_depth.bin", target->depth(), W, H, 4) || !download(dir + "out_diffuse.bin", g.diffuse, W, H, 8) ||
        !download(dir + "out_specular.bin", g.specular, W, H, 8) || !download(dir + "out_normal.bin", g.normal, W, H, 8) ||
        !download(dir + "out_worldPosition.bin", g.worldPosition, W, H, 16) ||
        !download(dir + "out_orm.bin", g.occlusionRoughnessMetallic, W, H, 8))
    {
        return fail("download");
    }
    std::printf("OK %u %u %g\n", W, H, (double)maxAnisotropy);
    return 0;
}
