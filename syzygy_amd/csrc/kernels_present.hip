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
// Destination texels are grouped in fours by ADDRESS, not by column: group g of a row covers the 16 aligned bytes
// 16 g .. 16 g + 15 counted from the 16-B boundary at or below the row's first texel, so that a full group is one aligned
// 16-B store whatever the region offset and the pitch. The groups that straddle the region's left or right edge fall back
// to one predicated 4-B store per texel: nothing outside the region is read (1:1) or written.
#include "szg_device.hpp"
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

// float(code) / 65535.0f, the UNORM16 load of the library. RN(1 / 65535) is 0x1.0001p-16, and with it divR0 (Markstein)
// returns the correctly rounded quotient for every one of the 65 536 codes: checked exhaustively in exact arithmetic by
// tests/test_present_model.py and on the device by tests/test_gpu_present.py. 3 instructions instead of the ~11 of `/`.
SZG_DEV float unorm16_to_float(unsigned code) { return divR0((float)code, 65535.0f, 0x1.0001p-16f); }

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

// texels of a row's first group that lie in front of the region (0..3): the row starts `lead` texels after a 16-B boundary
SZG_DEV unsigned lead_texels(const unsigned char* row) { return ((unsigned)reinterpret_cast<uintptr_t>(row) & 15u) >> 2; }

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
        unsigned const lead = lead_texels(drow);
        unsigned const groups = (width + lead + 3u) / 4u;
        for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < groups; v += gridDim.x * 256u)
        {
            int const c0 = (int)(4u * v) - (int)lead; // first column of the group; < 0 only for v == 0
            if (c0 >= 0 && (unsigned)c0 + 4u <= width)
            {
                const Quad8* s = reinterpret_cast<const Quad8*>(srow + (size_t)c0 * 8u);
                Quad8 const p01 = s[0];
                Quad8 const p23 = s[1];
                uint4 out;
                out.x = convert_texel<FMT, ENC>(make_uint2(p01.x, p01.y), table);
                out.y = convert_texel<FMT, ENC>(make_uint2(p01.z, p01.w), table);
                out.z = convert_texel<FMT, ENC>(make_uint2(p23.x, p23.y), table);
                out.w = convert_texel<FMT, ENC>(make_uint2(p23.z, p23.w), table);
                *reinterpret_cast<uint4*>(drow + (size_t)c0 * 4u) = out; // 16-B aligned by construction of the groups
            }
            else
            {
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    int const c = c0 + i;
                    if (c >= 0 && (unsigned)c < width)
                    {
                        uint2 const t = *reinterpret_cast<const uint2*>(srow + (size_t)c * 8u);
                        *reinterpret_cast<unsigned*>(drow + (size_t)c * 4u) = convert_texel<FMT, ENC>(t, table);
                    }
                }
            }
        }
    }
}

// COORDINATES of the header for one axis: destination index k of n onto source texels [s0, s0 + sw) of an image of
// `extent` texels. All products stay below 2^30 (extents <= 16384).
SZG_DEV void axis_linear(int k, int s0, int sw, int n, int extent, int& i0, int& i1, float& alpha)
{
    int const num = (2 * k + 1) * sw + (2 * s0 - 1) * n;
    int const den = 2 * n;
    int q = num / den; // truncates; num >= -n, so only q == 0 with a negative remainder needs the floor fix
    int rem = num - q * den;
    if (rem < 0)
    {
        rem += den;
        q -= 1;
    }
    alpha = (float)rem / (float)den;
    i0 = min(max(q, 0), extent - 1);
    i1 = min(max(q + 1, 0), extent - 1);
}
SZG_DEV int axis_nearest(int k, int s0, int sw, int n, int extent)
{
    int const i = s0 + ((2 * k + 1) * sw) / (2 * n);
    return min(max(i, 0), extent - 1);
}

struct SrcRegion
{
    int x, y, width, height;
};

// `src` points at texel (0, 0) of the source IMAGE (taps may leave the region), `dst` at the first texel of the region
template <unsigned FMT, bool ENC, bool LINEAR>
__global__ __launch_bounds__(256) void k_present_scale(const unsigned char* __restrict__ src, unsigned srcPitch, int srcW, int srcH,
                                                       SrcRegion sr, unsigned char* __restrict__ dst, unsigned dstPitch,
                                                       unsigned width, unsigned height, const unsigned short* __restrict__ table)
{
    // groups by the alignment of row 0; with a pitch that is a multiple of 16 every row has the same one, otherwise the
    // rows that do not take the per-texel stores below
    unsigned const lead = lead_texels(dst);
    unsigned const groups = (width + lead + 3u) / 4u;
    unsigned const v = blockIdx.x * 256u + threadIdx.x;
    if (v >= groups)
    {
        return;
    }
    int const c0 = (int)(4u * v) - (int)lead;
    bool const full = c0 >= 0 && (unsigned)c0 + 4u <= width;
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
                float const a = alpha[i], na = oneMinusAlpha[i];
                V4 const top{t00.x * na + t10.x * a, t00.y * na + t10.y * a, t00.z * na + t10.z * a, t00.w * na + t10.w * a};
                V4 const bot{t01.x * na + t11.x * a, t01.y * na + t11.y * a, t01.z * na + t11.z * a, t01.w * na + t11.w * a};
                V4 const r{top.x * oneMinusBeta + bot.x * beta, top.y * oneMinusBeta + bot.y * beta,
                           top.z * oneMinusBeta + bot.z * beta, top.w * oneMinusBeta + bot.w * beta};
                out[i] = pack_texel<FMT>(r);
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
        unsigned char* p = drow + (ptrdiff_t)c0 * 4;
        if (full && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u)
        {
            *reinterpret_cast<uint4*>(p) = make_uint4(out[0], out[1], out[2], out[3]);
        }
        else
        {
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                int const c = c0 + i;
                if (c >= 0 && (unsigned)c < width)
                {
                    *reinterpret_cast<unsigned*>(drow + (size_t)c * 4u) = out[i];
                }
            }
        }
    }
}

template <unsigned FMT, bool ENC>
hipError_t launch_present_fmt(hipStream_t s, const szg_image& src, const szg_image& dst, const szg_present_info& info,
                              const unsigned short* table)
{
    szg_rect const& sr = info.src_region;
    szg_rect const& dr = info.dst_region;
    unsigned char* dstRegion = static_cast<unsigned char*>(dst.data) + (size_t)dr.y * dst.pitch_bytes + (size_t)dr.x * 4u;
    unsigned const groups = (dr.width + 3u + 3u) / 4u; // at most 3 leading texels
    unsigned const gx = (groups + 255u) / 256u;
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

// Arguments are validated by szg_record_present (szg_api.cpp); `table` is the OETF table of info.encode or NULL for
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
