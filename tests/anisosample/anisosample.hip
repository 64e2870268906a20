// anisosample.hip — test infrastructure: the anisotropic material sampler of syzygy_amd/csrc/szg_texture.hpp
// (include/szg/anisotropy.h "SAMPLER") evaluated on the GPU over arrays of (uv, dUvDx, dUvDy), so that
// tests/test_gpu_anisotropy.py can compare every bit with tests/aniso_model.py without a rasteriser in between. The shape is
// that of tests/mipsample/mipsample.hip plus max_anisotropy: the decode tables live in LDS and are filled by the expression
// of decode8, as in k_raster_tile.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "szg_texture.hpp"

namespace
{
__global__ __launch_bounds__(256) void k_anisosample(szg_texture tex, szg::TextureMips mips, float maxAnisotropy,
                                                     const float2* __restrict__ st, const float2* __restrict__ ddx,
                                                     const float2* __restrict__ ddy, float* __restrict__ out, unsigned n)
{
    __shared__ float s_unorm[256];
    __shared__ float s_srgb[256];
    s_unorm[threadIdx.x] = szg::decode8(threadIdx.x, false);
    s_srgb[threadIdx.x] = szg::decode8(threadIdx.x, true);
    __syncthreads();
    unsigned const i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
    {
        return;
    }
    szg::V3 const r = szg::sampleTextureAniso(tex, mips, maxAnisotropy, szg::V2{st[i].x, st[i].y}, szg::V2{ddx[i].x, ddx[i].y},
                                              szg::V2{ddy[i].x, ddy[i].y}, s_unorm, s_srgb);
    out[3u * i] = r.x;
    out[3u * i + 1u] = r.y;
    out[3u * i + 2u] = r.z;
}
} // namespace

// All pointers but `tex` are device pointers; `levels` must not exceed the level count of tex's size and `d_chain` must hold
// that many levels; max_anisotropy in 1..16. Returns the HIP status after the kernel has finished.
extern "C" int szg_anisosample(const szg_texture* tex, const void* d_chain, uint32_t levels, float max_lod, float max_anisotropy,
                               const float* d_st, const float* d_ddx, const float* d_ddy, float* d_out, uint32_t n)
{
    if (n == 0u)
    {
        return 0;
    }
    hipLaunchKernelGGL(k_anisosample, dim3((n + 255u) / 256u), dim3(256), 0, nullptr, *tex, szg::TextureMips{d_chain, levels, max_lod},
                       max_anisotropy, reinterpret_cast<const float2*>(d_st), reinterpret_cast<const float2*>(d_ddx),
                       reinterpret_cast<const float2*>(d_ddy), d_out, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
    {
        e = hipDeviceSynchronize();
    }
    return (int)e;
}
