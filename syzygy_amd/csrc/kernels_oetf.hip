// kernels_oetf.hip — the OETF pass for gfx950: transfer/oetf_srgb.comp:9-19, transfer/oetf_pure_gamma.comp:9, in place
// on RGBA16 UNORM. Two pixels (16 B) per lane per access, fully coalesced; 16 B/px of traffic.
//
//   k_oetf_table : the function's value for every UNORM16 channel value
//   k_oetf       : every colour channel of the image through that table

#include "szg/fpmath.h"
#include "szg_formats.hpp"
#include "szg_image_ops.hpp"
#include "szg_launch.hpp"

namespace szg
{
SZG_DEV float oetf(float linear, unsigned function)
{
    if (function == SZG_OETF_SRGB)
    {
        return encode_srgb(linear); // mix(higher, lower, cutoff)
    }
    // (float)(1.0 / 2.2), not 1.0f / 2.2f: the constant of the reference's SPIR-V, folded in double (oracle_oetf)
    return szg_powf(linear, (float)(1.0 / 2.2));
}
// The OETF is a pure function of a 16-bit channel value: 65 536 possible inputs. k_oetf_table evaluates the
// expression above once per input; k_oetf then maps every channel through the 128 KiB table (L2-resident gathers),
// which leaves the pass with ~20 instructions per pixel against 16 B of traffic: HBM-bound, and bit-identical to
// evaluating the three pow() per pixel.
__global__ __launch_bounds__(256) void k_oetf_table(unsigned short* __restrict__ table, unsigned function)
{
    unsigned const i = blockIdx.x * 256u + threadIdx.x; // 256 x 256 threads
    table[i] = (unsigned short)unorm16(oetf((float)i / 65535.0f, function));
}
SZG_DEV unsigned oetf_pair_lut(unsigned packed, const unsigned short* __restrict__ table, bool hiIsAlpha)
{
    unsigned const lo = table[packed & 0xFFFFu];
    unsigned const hi = hiIsAlpha ? (packed >> 16) : (unsigned)table[packed >> 16];
    return lo | (hi << 16);
}
__global__ __launch_bounds__(256) void k_oetf(unsigned char* __restrict__ data, unsigned pitch, unsigned width, unsigned height,
                                             const unsigned short* __restrict__ table)
{
    unsigned const pairs = (width + 1u) / 2u; // uint4 = 2 pixels
    for (unsigned y = blockIdx.y; y < height; y += gridDim.y)
    {
        uint4* row = reinterpret_cast<uint4*>(data + (size_t)y * pitch);
        for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < pairs; v += gridDim.x * 256u)
        {
            if (2u * v + 1u < width)
            {
                uint4 t = row[v];
                t.x = oetf_pair_lut(t.x, table, false);
                t.y = oetf_pair_lut(t.y, table, true);
                t.z = oetf_pair_lut(t.z, table, false);
                t.w = oetf_pair_lut(t.w, table, true);
                row[v] = t;
            }
            else
            {
                uint2* px = reinterpret_cast<uint2*>(row) + 2u * v; // odd width: last single pixel
                uint2 t = *px;
                t.x = oetf_pair_lut(t.x, table, false);
                t.y = oetf_pair_lut(t.y, table, true);
                *px = t;
            }
        }
    }
}

hipError_t launch_oetf_table(hipStream_t s, unsigned short* table, unsigned function)
{
    hipLaunchKernelGGL(k_oetf_table, dim3(256), dim3(256), 0, s, table, function);
    return hipGetLastError();
}

hipError_t launch_oetf(hipStream_t s, const szg_image& image, unsigned width, unsigned height, const unsigned short* table)
{
    if (width == 0u || height == 0u)
    {
        return hipSuccess;
    }
    unsigned const pairs = (width + 1u) / 2u;
    unsigned gx = (pairs + 255u) / 256u;
    gx = gx > 8u ? 8u : gx;
    unsigned const gy = height > 65535u ? 65535u : height;
    hipLaunchKernelGGL(k_oetf, dim3(gx, gy), dim3(256), 0, s, static_cast<unsigned char*>(image.data), image.pitch_bytes, width, height,
                       table);
    return hipGetLastError();
}
} // namespace szg
