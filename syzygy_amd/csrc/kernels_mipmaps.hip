// kernels_mipmaps.hip — the mip chain builder of include/szg/mipmaps.h ("GENERATION"): k_mip_downsample makes one level
// from the stored texels of the level before it, one launch per level. It runs when an asset is loaded, not per frame, so
// the chain is NOT built in one pass through an LDS pyramid: the launches of a 4096^2 chain read 64 MiB + 1/3 once each and
// the small levels cost microseconds of launch latency, which asset loading does not notice.
//
// One thread per destination texel: four dword loads (the texel pair of two source rows) and one dword store. A wave
// covers 32 x 2 destination texels: it reads four contiguous 256-byte row segments and writes two of 128 bytes.
#include "szg_image_ops.hpp"
#include "szg_launch.hpp"

namespace szg
{
__global__ __launch_bounds__(256) void k_mip_downsample(const unsigned char* __restrict__ src, unsigned srcW, unsigned srcH,
                                                        unsigned srcPitch, unsigned char* __restrict__ dst, unsigned dstW,
                                                        unsigned dstH, unsigned srgb)
{
    // the sRGB decode of every code, once per workgroup by the sampler's expression
    __shared__ float s_srgb[256];
    if (srgb != 0u)
    {
        s_srgb[threadIdx.y * 32u + threadIdx.x] = decode8(threadIdx.y * 32u + threadIdx.x, true);
        __syncthreads();
    }
    unsigned const x = blockIdx.x * 32u + threadIdx.x;
    unsigned const y = blockIdx.y * 8u + threadIdx.y;
    if (x >= dstW || y >= dstH)
    {
        return;
    }
    unsigned const x0 = min(2u * x, srcW - 1u), x1 = min(2u * x + 1u, srcW - 1u);
    unsigned const y0 = min(2u * y, srcH - 1u), y1 = min(2u * y + 1u, srcH - 1u);
    const unsigned char* const row0 = src + (size_t)y0 * srcPitch;
    const unsigned char* const row1 = src + (size_t)y1 * srcPitch;
    unsigned const t00 = *reinterpret_cast<const unsigned*>(row0 + (size_t)x0 * 4u);
    unsigned const t10 = *reinterpret_cast<const unsigned*>(row0 + (size_t)x1 * 4u);
    unsigned const t01 = *reinterpret_cast<const unsigned*>(row1 + (size_t)x0 * 4u);
    unsigned const t11 = *reinterpret_cast<const unsigned*>(row1 + (size_t)x1 * 4u);
    unsigned out = 0u;
#pragma unroll
    for (unsigned ch = 0; ch < 4u; ch++)
    {
        unsigned const sh = ch * 8u;
        unsigned const a = (t00 >> sh) & 0xFFu, b = (t10 >> sh) & 0xFFu, c = (t01 >> sh) & 0xFFu, e = (t11 >> sh) & 0xFFu;
        unsigned code = (a + b + c + e + 2u) >> 2;
        if (srgb != 0u && ch < 3u)
        {
            float const l = ((s_srgb[a] + s_srgb[b]) + (s_srgb[c] + s_srgb[e])) * 0.25f;
            int const q = (int)floorf(encode_srgb(l) * 255.0f + 0.5f);
            code = (unsigned)min(max(q, 0), 255);
        }
        out |= code << sh;
    }
    *reinterpret_cast<unsigned*>(dst + ((size_t)y * dstW + x) * 4u) = out;
}

hipError_t launch_generate_mipmaps(hipStream_t s, const szg_texture& level0, void* d_chain)
{
    const unsigned char* src = static_cast<const unsigned char*>(level0.data);
    unsigned char* dst = static_cast<unsigned char*>(d_chain);
    unsigned w = level0.width, h = level0.height, pitch = level0.pitch_bytes;
    while (w > 1u || h > 1u)
    {
        unsigned const dw = w > 1u ? w >> 1 : 1u, dh = h > 1u ? h >> 1 : 1u;
        hipLaunchKernelGGL(k_mip_downsample, dim3((dw + 31u) / 32u, (dh + 7u) / 8u), dim3(32, 8), 0, s, src, w, h, pitch, dst, dw, dh,
                           level0.srgb);
        hipError_t const e = hipGetLastError();
        if (e != hipSuccess)
        {
            return e;
        }
        src = dst;
        dst += (size_t)dw * dh * 4u;
        w = dw;
        h = dh;
        pitch = dw * 4u;
    }
    return hipSuccess;
}
} // namespace szg
