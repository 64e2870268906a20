// kernels_image_copy.hip — the image copy and clear of the texture viewer (include/szg/texture_display.h): the NEAREST blit
// behind Image::recordCopyEntire (renderer/image.cpp:191-206 -> imageoperations.cpp:141-176, vkCmdBlitImage2) from an 8- or
// 16-bit image onto an RGBA16_SFLOAT one, and recordClearColorImage (rendercommands.cpp:25). The rules (coordinates in
// integers, the four loads, the half store after the fp32 rounding) are stated in the header; the CPU model is
// tests/texture_display_model.py. Nothing here belongs to a contraction class: both libraries compile the same code.
//
// The editor's case magnifies a 64^2 .. 4096^2 RGBA8 map onto 4096^2 x 8 B: 128 MiB written, the source read from cache.
// Both kernels are store-bound and shaped like k_present_scale:
//   k_image_copy   a lane owns the two destination texels of one aligned 16 bytes, computes their source offsets (the
//                  integer divisions) once and keeps them over the IMAGE_COPY_ROWS_PER_LANE rows it walks; the row's source
//                  index is wave-uniform. The 8-bit decodes are a 256-entry table of binary16 codes built once per workgroup in
//                  LDS, only for the formats that need it: an sRGB table costs 256 szg_powf per workgroup, a texel four
//                  LDS reads and no conversion.
//   k_image_clear  the same groups, one value.
// Destination texels are grouped in twos by address (RowGroups<8> of szg_image_ops.hpp): a full group of a row aligned like
// row 0 is one aligned 16-B store, every other texel one predicated 8-B store; nothing outside the region is written.
#include "szg_image_ops.hpp"
#include "szg_launch.hpp"

#include "szg/texture_display.h"

namespace szg
{
namespace
{
// STORE of the header for one channel: binary16 of the ROUNDED fp32 value (the guard of pack_half4)
SZG_DEV unsigned half_code(float x)
{
    asm volatile("" : "+v"(x));
    __half const h = __float2half_rn(x);
    return (unsigned)*reinterpret_cast<const unsigned short*>(&h);
}

using Groups = RowGroups<8>; // 8-B destination texels

// The group's two texels: one 16-B store where the group is full and this row puts it on a 16-B boundary, otherwise one
// predicated 8-B store per texel. One function body on purpose: split into the pieces of RowGroups<4>, the address of the
// first 8-B store no longer merges with the 16-B store's (+2 VGPRs, 1.1 % to 1.5 % slower; profiles/image_ops_refactor.md).
SZG_DEV void store_pair(unsigned char* drow, int c0, bool full, unsigned width, uint2 t0, uint2 t1)
{
    unsigned char* p = drow + (ptrdiff_t)c0 * 8;
    if (full && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u)
    {
        *reinterpret_cast<uint4*>(p) = make_uint4(t0.x, t0.y, t1.x, t1.y);
    }
    else
    {
        if (c0 >= 0 && (unsigned)c0 < width)
        {
            *reinterpret_cast<uint2*>(drow + (size_t)c0 * 8u) = t0;
        }
        if (c0 + 1 >= 0 && (unsigned)(c0 + 1) < width)
        {
            *reinterpret_cast<uint2*>(drow + (size_t)(c0 + 1) * 8u) = t1;
        }
    }
}

template <unsigned SRC> constexpr unsigned source_texel_bytes() { return SRC == SZG_FORMAT_RGBA8_UNORM || SRC == SZG_FORMAT_RGBA8_SRGB ? 4u : 8u; }

// LOAD and STORE of one texel. `colour` / `alpha`: the LDS tables of an 8-bit source
template <unsigned SRC> SZG_DEV uint2 convert_texel(const unsigned char* p, const unsigned short* colour, const unsigned short* alpha)
{
    if (SRC == SZG_FORMAT_RGBA16_SFLOAT)
    {
        return *reinterpret_cast<const uint2*>(p);
    }
    if (SRC == SZG_FORMAT_RGBA16_UNORM)
    {
        V4 const t = unpack_unorm16x4(*reinterpret_cast<const uint2*>(p));
        return pack_half4(t.x, t.y, t.z, t.w);
    }
    unsigned const t = *reinterpret_cast<const unsigned*>(p);
    return make_uint2((unsigned)colour[t & 0xFFu] | ((unsigned)colour[(t >> 8) & 0xFFu] << 16),
                      (unsigned)colour[(t >> 16) & 0xFFu] | ((unsigned)alpha[t >> 24] << 16));
}

// `src` points at texel (0, 0) of the source IMAGE, `dst` at the first texel of the destination region
template <unsigned SRC>
__global__ __launch_bounds__(256) void k_image_copy(const unsigned char* __restrict__ src, unsigned srcPitch, int srcW, int srcH,
                                                    SrcRegion sr, unsigned char* __restrict__ dst, unsigned dstPitch, unsigned width,
                                                    unsigned height)
{
    constexpr bool TABLE = source_texel_bytes<SRC>() == 4u;
    constexpr bool SRGB = SRC == SZG_FORMAT_RGBA8_SRGB;
    __shared__ unsigned short tables[TABLE ? (SRGB ? 512 : 256) : 1];
    if (TABLE)
    {
        unsigned const b = threadIdx.x; // 256 lanes, one code each
        tables[b] = (unsigned short)half_code(decode8(b, SRGB));
        if (SRGB)
        {
            tables[256u + b] = (unsigned short)half_code(decode8(b, false));
        }
        __syncthreads();
    }
    const unsigned short* const colour = tables;
    const unsigned short* const alpha = tables + (SRGB ? 256 : 0);

    // groups by the alignment of row 0; a row aligned otherwise (a pitch that is no multiple of 16) takes the 8-B stores
    unsigned const lead = Groups::lead_texels(dst);
    unsigned const v = blockIdx.x * 256u + threadIdx.x;
    if (v >= Groups::count(width, lead))
    {
        return;
    }
    int const c0 = Groups::first_column(v, lead);
    bool const full = Groups::full(c0, width);
    // per-column setup, once per lane; a column outside the region is computed but never stored
    unsigned off[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
    {
        int const c = min(max(c0 + i, 0), (int)width - 1);
        off[i] = (unsigned)axis_nearest(c, sr.x, sr.width, (int)width, srcW) * source_texel_bytes<SRC>();
    }
    for (unsigned y = blockIdx.y; y < height; y += gridDim.y)
    {
        int const j = axis_nearest((int)y, sr.y, sr.height, (int)height, srcH); // wave-uniform
        const unsigned char* srow = src + (size_t)j * srcPitch;
        unsigned char* drow = dst + (size_t)y * dstPitch;
        uint2 const t0 = convert_texel<SRC>(srow + off[0], colour, alpha);
        uint2 const t1 = convert_texel<SRC>(srow + off[1], colour, alpha);
        store_pair(drow, c0, full, width, t0, t1);
    }
}

// `dst` points at texel (0, 0) of the image
template <bool HALF>
__global__ __launch_bounds__(256) void k_image_clear(unsigned char* __restrict__ dst, unsigned dstPitch, unsigned width, unsigned height,
                                                     V4 color)
{
    uint2 const t = HALF ? pack_half4(color.x, color.y, color.z, color.w) : pack_unorm16x4(color.x, color.y, color.z, color.w);
    unsigned const lead = Groups::lead_texels(dst);
    unsigned const v = blockIdx.x * 256u + threadIdx.x;
    if (v >= Groups::count(width, lead))
    {
        return;
    }
    int const c0 = Groups::first_column(v, lead);
    bool const full = Groups::full(c0, width);
    for (unsigned y = blockIdx.y; y < height; y += gridDim.y)
    {
        store_pair(dst + (size_t)y * dstPitch, c0, full, width, t, t);
    }
}

// the grid of both kernels: 256 groups per workgroup along x, IMAGE_COPY_ROWS_PER_LANE rows per lane along y
dim3 group_grid(unsigned width, unsigned height)
{
    return dim3((Groups::count(width) + 255u) / 256u, (height + IMAGE_COPY_ROWS_PER_LANE - 1u) / IMAGE_COPY_ROWS_PER_LANE);
}

template <unsigned SRC>
hipError_t launch_copy_fmt(hipStream_t s, const szg_image& src, const szg_image& dst, const szg_rect& sr, const szg_rect& dr)
{
    unsigned char* dstRegion = static_cast<unsigned char*>(dst.data) + (size_t)dr.y * dst.pitch_bytes + (size_t)dr.x * 8u;
    SrcRegion const region{sr.x, sr.y, (int)sr.width, (int)sr.height};
    hipLaunchKernelGGL((k_image_copy<SRC>), group_grid(dr.width, dr.height), dim3(256), 0, s, static_cast<const unsigned char*>(src.data),
                       src.pitch_bytes, (int)src.width, (int)src.height, region, dstRegion, dst.pitch_bytes, dr.width, dr.height);
    return hipGetLastError();
}
} // namespace

// Arguments are validated by szg_record_copy_image (api_texture_display.cpp).
hipError_t launch_image_copy(hipStream_t s, const szg_image& src, const szg_image& dst, const szg_rect& sr, const szg_rect& dr)
{
    if (sr.width == 0u || sr.height == 0u || dr.width == 0u || dr.height == 0u)
    {
        return hipSuccess;
    }
    switch (src.format)
    {
    case SZG_FORMAT_RGBA8_UNORM:
        return launch_copy_fmt<SZG_FORMAT_RGBA8_UNORM>(s, src, dst, sr, dr);
    case SZG_FORMAT_RGBA8_SRGB:
        return launch_copy_fmt<SZG_FORMAT_RGBA8_SRGB>(s, src, dst, sr, dr);
    case SZG_FORMAT_RGBA16_UNORM:
        return launch_copy_fmt<SZG_FORMAT_RGBA16_UNORM>(s, src, dst, sr, dr);
    case SZG_FORMAT_RGBA16_SFLOAT:
        return launch_copy_fmt<SZG_FORMAT_RGBA16_SFLOAT>(s, src, dst, sr, dr);
    default:
        return hipErrorInvalidValue;
    }
}

// Arguments are validated by szg_record_clear_color_image.
hipError_t launch_image_clear(hipStream_t s, const szg_image& image, const float color[4])
{
    if (image.width == 0u || image.height == 0u)
    {
        return hipSuccess;
    }
    V4 const c{color[0], color[1], color[2], color[3]};
    unsigned char* data = static_cast<unsigned char*>(image.data);
    if (image.format == SZG_FORMAT_RGBA16_SFLOAT)
    {
        hipLaunchKernelGGL(k_image_clear<true>, group_grid(image.width, image.height), dim3(256), 0, s, data, image.pitch_bytes, image.width,
                           image.height, c);
    }
    else
    {
        hipLaunchKernelGGL(k_image_clear<false>, group_grid(image.width, image.height), dim3(256), 0, s, data, image.pitch_bytes, image.width,
                           image.height, c);
    }
    return hipGetLastError();
}
} // namespace szg
