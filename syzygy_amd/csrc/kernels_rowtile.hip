// kernels_rowtile.hip — the multi-GPU row-tile compose copy for gfx950.
//
//   k_compose : HBM-bound row scatter after the RCCL gather

#include <hip/hip_runtime.h>

#include "szg_launch.hpp"

namespace szg
{
// Row scatter after the gather: rank r's packed tile holds its rows in local
// order; local row l of rank r is global row ((l / B) * N + r) * B + l % B.
// One workgroup row per global row; 16 B per lane, fully coalesced both sides.
__global__ __launch_bounds__(256) void k_compose(const uint4* __restrict__ gathered, size_t tileStrideVec, unsigned nranks,
                                                 unsigned blockRows, unsigned char* __restrict__ dst, unsigned dstPitch,
                                                 unsigned rowVecs)
{
    unsigned const gy = blockIdx.y;
    unsigned const blk = gy / blockRows;
    unsigned const rank = blk % nranks;
    unsigned const local = (blk / nranks) * blockRows + gy % blockRows;
    const uint4* src = gathered + (size_t)rank * tileStrideVec + (size_t)local * rowVecs;
    uint4* out = reinterpret_cast<uint4*>(dst + (size_t)gy * dstPitch);
    for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < rowVecs; v += gridDim.x * 256u)
    {
        out[v] = src[v];
    }
}

hipError_t launch_compose_rowtiles(hipStream_t s, const void* gathered, size_t tileStrideBytes, unsigned nranks,
                                   unsigned blockRows, const szg_image& dst, unsigned width, unsigned height)
{
    if (width == 0u || height == 0u)
    {
        return hipSuccess;
    }
    unsigned const rowBytes = width * 8u; // RGBA16_UNORM
    unsigned const rowVecs = rowBytes / 16u;
    unsigned const gx = (rowVecs + 255u) / 256u;
    hipLaunchKernelGGL(k_compose, dim3(gx > 8u ? 8u : gx, height), dim3(256), 0, s, static_cast<const uint4*>(gathered),
                       tileStrideBytes / 16u, nranks, blockRows, static_cast<unsigned char*>(dst.data), dst.pitch_bytes, rowVecs);
    return hipGetLastError();
}
} // namespace szg
