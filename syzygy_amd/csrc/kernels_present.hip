// kernels_present.hip — the present pass (include/szg/present.h): the scaled, format-converting blit that ends the
// reference's frame (editor/editor.cpp:355-361 -> renderer/imageoperations.cpp:45-119, vkCmdBlitImage2), from the
// RGBA16_UNORM scene colour to an 8- or 10-bit swapchain format. The rule (coordinates in integers, taps clamped to the
// image, every fp32 operation rounded on its own, UNORM store by round-to-nearest-even) is stated in the header; the CPU
// model is tests/present_model.py. Nothing here belongs to a contraction class: both libraries compile the same code.
//
// Two kernels, both pure streaming:
//   k_present_copy   regions of equal extent (the editor's normal case). Every weight is 1 or 0, so the texel is converted
//                    without a filter. A lane converts 4 texels: 32 B loaded (two 16-B loads), 16 B stored; 12 B/px.
//   k_present_scale  everything else. A lane owns 4 adjacent destination columns, computes their taps and weights once
//                    and keeps them over the rows it walks; the row's taps and weight are wave-uniform. Taps are 8-B
//                    gathers (for a magnification they hit the same lines again; a 4K source fits the Infinity Cache).
// Destination texels are grouped in fours by address (RowGroups<4> of szg_image_ops.hpp): a full group is one aligned 16-B
// store, the groups at the region's edges store texel by texel; nothing outside the region is read (1:1) or written.
#include "szg_image_ops.hpp"
#include "szg_launch.hpp"

#include "szg/present.h"

namespace szg
{
namespace
{
// 16 bytes that are only known to be 8-B aligned (a source row starts at any texel): lets the compiler use one 16-B load
// where the target allows it without promising an alignment the address does not have
struct alignas(8) Quad8
{
    unsigned x, y, z, w;
};

// STORE of the header: clamp, scale by 2^b - 1, round to nearest even
SZG_DEV unsigned unorm_bits(float x, float scale)
{
    float const c = fminf(fmaxf(x, 0.0f), 1.0f); // NaN -> 0
    return (unsigned)__float2int_rn(c * scale);
}
template <unsigned FMT> SZG_DEV unsigned pack_texel(V4 c)
{
    if (FMT == SZG_FORMAT_A2B10G10R10_UNORM)
    {
        return unorm_bits(c.x, 1023.0f) | (unorm_bits(c.y, 1023.0f) << 10) | (unorm_bits(c.z, 1023.0f) << 20) |
               (unorm_bits(c.w, 3.0f) << 30);
    }
    unsigned const r = unorm_bits(c.x, 255.0f), g = unorm_bits(c.y, 255.0f), b = unorm_bits(c.z, 255.0f);
    unsigned const a = unorm_bits(c.w, 255.0f);
    return FMT == SZG_FORMAT_BGRA8_UNORM ? (b | (g << 8) | (r << 16) | (a << 24)) : (r | (g << 8) | (b << 16) | (a << 24));
}

// One source texel as four floats; ENCODE maps R, G, B through the table of szg_record_oetf first (alpha passes)
template <bool ENC> SZG_DEV V4 load_tap(uint2 t, const unsigned short* __restrict__ table)
{
    unsigned r = t.x & 0xFFFFu, g = t.x >> 16, b = t.y & 0xFFFFu;
    unsigned const a = t.y >> 16;
    if (ENC)
    {
        r = table[r];
        g = table[g];
        b = table[b];
    }
    return V4{unorm16_to_float(r), unorm16_to_float(g), unorm16_to_float(b), unorm16_to_float(a)};
}
template <unsigned FMT, bool ENC> SZG_DEV unsigned convert_texel(uint2 t, const unsigned short* __restrict__ table)
{
    return pack_texel<FMT>(load_tap<ENC>(t, table));
}

using Groups = RowGroups<4>; // 4-B destination texels

// `src` / `dst` point at the first texel of the regions
template <unsigned FMT, bool ENC>
__global__ __launch_bounds__(256) void k_present_copy(const unsigned char* __restrict__ src, unsigned srcPitch,
                                                      unsigned char* __restrict__ dst, unsigned dstPitch, unsigned width,
                                                      unsigned height, const unsigned short* __restrict__ table)
{
    for (unsigned y = blockIdx.y; y < height; y += gridDim.y)
    {
        const unsigned char* srow = src + (size_t)y * srcPitch;
        unsigned char* drow = dst + (size_t)y * dstPitch;
        unsigned const lead = Groups::lead_texels(drow); // of this row: its full groups are aligned whatever the pitch
        unsigned const groups = Groups::count(width, lead);
        for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < groups; v += gridDim.x * 256u)
        {
            int const c0 = Groups::first_column(v, lead);
            if (Groups::full(c0, width))
            {
                const Quad8* s = reinterpret_cast<const Quad8*>(srow + (size_t)c0 * 8u);
                Quad8 const p01 = s[0];
                Quad8 const p23 = s[1];
                uint4 out;
                out.x = convert_texel<FMT, ENC>(make_uint2(p01.x, p01.y), table);
                out.y = convert_texel<FMT, ENC>(make_uint2(p01.z, p01.w), table);
                out.z = convert_texel<FMT, ENC>(make_uint2(p23.x, p23.y), table);
                out.w = convert_texel<FMT, ENC>(make_uint2(p23.z, p23.w), table);
                Groups::store_aligned(Groups::address(drow, c0), out); // 16-B aligned: `lead` is this row's
            }
            else
            {
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    int const c = c0 + i;
                    if (Groups::holds(c, width)) // nothing outside the region is read either
                    {
                        uint2 const t = *reinterpret_cast<const uint2*>(srow + (size_t)c * 8u);
                        Groups::store_texel(drow, c, width, convert_texel<FMT, ENC>(t, table));
                    }
                }
            }
        }
    }
}

// `src` points at texel (0, 0) of the source IMAGE (taps may leave the region), `dst` at the first texel of the region
template <unsigned FMT, bool ENC, bool LINEAR>
__global__ __launch_bounds__(256) void k_present_scale(const unsigned char* __restrict__ src, unsigned srcPitch, int srcW, int srcH,
                                                       SrcRegion sr, unsigned char* __restrict__ dst, unsigned dstPitch,
                                                       unsigned width, unsigned height, const unsigned short* __restrict__ table)
{
    // groups by the alignment of row 0; with a pitch that is a multiple of 16 every row has the same one, otherwise the
    // rows that do not take the per-texel stores below
    unsigned const lead = Groups::lead_texels(dst);
    unsigned const v = blockIdx.x * 256u + threadIdx.x;
    if (v >= Groups::count(width, lead))
    {
        return;
    }
    int const c0 = Groups::first_column(v, lead);
    // per-column setup, once per lane: byte offsets of the two taps, the weight and its complement
    unsigned off0[4], off1[4];
    float alpha[4], oneMinusAlpha[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
        int const c = min(max(c0 + i, 0), (int)width - 1); // columns outside the region are computed but never stored
        if (LINEAR)
        {
            int i0, i1;
            axis_linear(c, sr.x, sr.width, (int)width, srcW, i0, i1, alpha[i]);
            off0[i] = (unsigned)i0 * 8u;
            off1[i] = (unsigned)i1 * 8u;
            oneMinusAlpha[i] = 1.0f - alpha[i];
        }
        else
        {
            off0[i] = (unsigned)axis_nearest(c, sr.x, sr.width, (int)width, srcW) * 8u;
            off1[i] = off0[i];
            alpha[i] = 0.0f;
            oneMinusAlpha[i] = 1.0f;
        }
    }
    for (unsigned y = blockIdx.y; y < height; y += gridDim.y)
    {
        unsigned char* drow = dst + (size_t)y * dstPitch;
        unsigned out[4];
        if (LINEAR)
        {
            int j0, j1;
            float beta;
            axis_linear((int)y, sr.y, sr.height, (int)height, srcH, j0, j1, beta); // wave-uniform
            float const oneMinusBeta = 1.0f - beta;
            const unsigned char* r0 = src + (size_t)j0 * srcPitch;
            const unsigned char* r1 = src + (size_t)j1 * srcPitch;
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                V4 const t00 = load_tap<ENC>(*reinterpret_cast<const uint2*>(r0 + off0[i]), table);
                V4 const t10 = load_tap<ENC>(*reinterpret_cast<const uint2*>(r0 + off1[i]), table);
                V4 const t01 = load_tap<ENC>(*reinterpret_cast<const uint2*>(r1 + off0[i]), table);
                V4 const t11 = load_tap<ENC>(*reinterpret_cast<const uint2*>(r1 + off1[i]), table);
                V4 const top = blend(t00, t10, oneMinusAlpha[i], alpha[i]);
                V4 const bot = blend(t01, t11, oneMinusAlpha[i], alpha[i]);
                out[i] = pack_texel<FMT>(blend(top, bot, oneMinusBeta, beta));
            }
        }
        else
        {
            int const j = axis_nearest((int)y, sr.y, sr.height, (int)height, srcH);
            const unsigned char* r0 = src + (size_t)j * srcPitch;
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                out[i] = convert_texel<FMT, ENC>(*reinterpret_cast<const uint2*>(r0 + off0[i]), table);
            }
        }
        Groups::store(drow, c0, width, make_uint4(out[0], out[1], out[2], out[3]));
    }
}

template <unsigned FMT, bool ENC>
hipError_t launch_present_fmt(hipStream_t s, const szg_image& src, const szg_image& dst, const szg_present_info& info,
                              const unsigned short* table)
{
    szg_rect const& sr = info.src_region;
    szg_rect const& dr = info.dst_region;
    unsigned char* dstRegion = static_cast<unsigned char*>(dst.data) + (size_t)dr.y * dst.pitch_bytes + (size_t)dr.x * 4u;
    unsigned const gx = (Groups::count(dr.width) + 255u) / 256u;
    if (sr.width == dr.width && sr.height == dr.height)
    {
        const unsigned char* srcRegion = static_cast<const unsigned char*>(src.data) + (size_t)sr.y * src.pitch_bytes + (size_t)sr.x * 8u;
        hipLaunchKernelGGL((k_present_copy<FMT, ENC>), dim3(gx > 8u ? 8u : gx, dr.height), dim3(256), 0, s, srcRegion, src.pitch_bytes,
                           dstRegion, dst.pitch_bytes, dr.width, dr.height, table);
        return hipGetLastError();
    }
    // 8 rows per lane: the per-column setup (four integer divisions) is paid once for them
    dim3 const grid(gx, (dr.height + 7u) / 8u);
    SrcRegion const region{sr.x, sr.y, (int)sr.width, (int)sr.height};
    const unsigned char* srcImage = static_cast<const unsigned char*>(src.data);
    if (info.filter == SZG_FILTER_LINEAR)
    {
        hipLaunchKernelGGL((k_present_scale<FMT, ENC, true>), grid, dim3(256), 0, s, srcImage, src.pitch_bytes, (int)src.width,
                           (int)src.height, region, dstRegion, dst.pitch_bytes, dr.width, dr.height, table);
    }
    else
    {
        hipLaunchKernelGGL((k_present_scale<FMT, ENC, false>), grid, dim3(256), 0, s, srcImage, src.pitch_bytes, (int)src.width,
                           (int)src.height, region, dstRegion, dst.pitch_bytes, dr.width, dr.height, table);
    }
    return hipGetLastError();
}
template <unsigned FMT>
hipError_t launch_present_enc(hipStream_t s, const szg_image& src, const szg_image& dst, const szg_present_info& info,
                              const unsigned short* table)
{
    return table != nullptr ? launch_present_fmt<FMT, true>(s, src, dst, info, table)
                            : launch_present_fmt<FMT, false>(s, src, dst, info, nullptr);
}
} // namespace

// Arguments are validated by szg_record_present (api_image_passes.cpp); `table` is the OETF table of info.encode or NULL for
// SZG_PRESENT_ENCODE_NONE.
hipError_t launch_present(hipStream_t s, const szg_image& src, const szg_image& dst, const szg_present_info& info,
                          const unsigned short* table)
{
    if (info.src_region.width == 0u || info.src_region.height == 0u || info.dst_region.width == 0u || info.dst_region.height == 0u)
    {
        return hipSuccess;
    }
    switch (dst.format)
    {
    case SZG_FORMAT_RGBA8_UNORM:
        return launch_present_enc<SZG_FORMAT_RGBA8_UNORM>(s, src, dst, info, table);
    case SZG_FORMAT_BGRA8_UNORM:
        return launch_present_enc<SZG_FORMAT_BGRA8_UNORM>(s, src, dst, info, table);
    case SZG_FORMAT_A2B10G10R10_UNORM:
        return launch_present_enc<SZG_FORMAT_A2B10G10R10_UNORM>(s, src, dst, info, table);
    default:
        return hipErrorInvalidValue;
    }
}
} // namespace szg
