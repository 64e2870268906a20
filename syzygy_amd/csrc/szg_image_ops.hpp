// szg_image_ops.hpp — the device rules that the image passes share, each stated once: the texel codec, the integer
// coordinates of a blit, the two-tap blend and the aligned store of a destination row. Used by kernels_present.hip,
// kernels_image_copy.hip, kernels_ui_layer.hip and kernels_mipmaps.hip; every one of them is built with -ffp-contract=off,
// so each operation below rounds once. The CPU models (tests/present_model.py, tests/texture_display_model.py,
// tests/ui_layer_model.py) state the same rules and the GPU tests hold the kernels to them bit for bit.
#ifndef SZG_IMAGE_OPS_HPP
#define SZG_IMAGE_OPS_HPP

#include "szg/fpmath.h"
#include "szg_formats.hpp"
#include "szg_lean.hpp"
#include "szg_texture.hpp"
#include "szg_vec.hpp"

namespace szg
{
// ---- texel codec (the 8-bit UNORM load is decode8(b, false) of szg_texture.hpp) ----
// float(code) / 65535.0f, the UNORM16 load of the library. RN(1 / 65535) is 0x1.0001p-16, and with it divR0 (Markstein)
// returns the correctly rounded quotient for every one of the 65 536 codes: checked exhaustively in exact arithmetic by
// tests/test_present_model.py and on the device by tests/test_gpu_present.py and tests/test_gpu_ui_layer.py. 3 instructions
// instead of the ~11 of `/`.
SZG_DEV float unorm16_to_float(unsigned code) { return divR0((float)code, 65535.0f, 0x1.0001p-16f); }
// a texel as pack_unorm16x4 stores it: r | g << 16, b | a << 16
SZG_DEV V4 unpack_unorm16x4(uint2 t)
{
    return V4{unorm16_to_float(t.x & 0xFFFFu), unorm16_to_float(t.x >> 16), unorm16_to_float(t.y & 0xFFFFu), unorm16_to_float(t.y >> 16)};
}

// SZG_OETF_SRGB of szg_record_oetf (transfer/oetf_srgb.comp:9-19); kernels_oetf.hip evaluates it through this function too.
SZG_DEV float encode_srgb(float linear)
{
    float const lower = 12.92f * linear;
    float const higher = szg_powf(linear, (float)(1.0 / 2.4)) * 1.055f - 0.055f;
    return (linear <= 0.0031308f) ? lower : higher;
}

// ---- blit coordinates: COORDINATES of szg/present.h and szg/texture_display.h ----
// One axis: destination index k of n onto source texels [s0, s0 + sw) of an image of `extent` texels; taps are clamped to
// the image. All products stay below 2^30 (extents <= 16384).
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

// ---- two-tap blend: x wx + y wy per channel, two products and one sum, each rounded. The callers pass the complement
// they computed first (1 - w, w): LINEAR of szg/present.h and of szg/ui_layer.h ----
SZG_DEV V4 blend(V4 x, V4 y, float wx, float wy)
{
    return V4{x.x * wx + y.x * wy, x.y * wx + y.y * wy, x.z * wx + y.z * wy, x.w * wx + y.w * wy};
}

// ---- aligned row groups ----
// Destination texels of BYTES bytes (4 or 8) are grouped by ADDRESS, not by column: group v of a row covers the 16 aligned
// bytes 16 v .. 16 v + 15 counted from the 16-B boundary at or below the row's first texel, so that a full group is one
// aligned 16-B store whatever the region offset and the pitch. A group that straddles the region's left or right edge, and
// every group of a row aligned otherwise than the row `lead` was taken from (a pitch that is no multiple of 16), falls back
// to one predicated store per texel: nothing outside the region is written. The arithmetic serves both texel sizes.
template <unsigned BYTES> struct RowGroups
{
    static_assert(BYTES == 4u || BYTES == 8u, "RGBA8-sized or RGBA16-sized texels");
    static constexpr unsigned G = 16u / BYTES; // texels of a group

    // texels of a row's first group that lie in front of the region: 0 .. G - 1
    static SZG_DEV unsigned lead_texels(const unsigned char* row) { return ((unsigned)reinterpret_cast<uintptr_t>(row) & 15u) / BYTES; }
    // groups of a row of `width` texels; a launch sizes its grid for the most leading texels a row can have
    static __host__ __device__ constexpr unsigned count(unsigned width, unsigned lead = G - 1u) { return (width + lead + G - 1u) / G; }

    // first column of group v; < 0 only for group 0
    static SZG_DEV int first_column(unsigned v, unsigned lead) { return (int)(G * v) - (int)lead; }
    // every texel of the group that starts at column c0 lies in the region
    static SZG_DEV bool full(int c0, unsigned width) { return c0 >= 0 && (unsigned)c0 + G <= width; }
    static SZG_DEV bool holds(int c, unsigned width) { return c >= 0 && (unsigned)c < width; }
    // of the group's 16 bytes; `drow`: the first texel of the region's row
    static SZG_DEV unsigned char* address(unsigned char* drow, int c0) { return drow + (ptrdiff_t)c0 * (int)BYTES; }

    // The store of a group of 4-B texels in its two pieces; `words`: the group's 16 bytes in address order. (The 8-B texels'
    // store is store_pair of kernels_image_copy.hip.)
    // A full group at an address the caller knows to be 16-B aligned, in one store ...
    static SZG_DEV void store_aligned(unsigned char* p, uint4 words) { *reinterpret_cast<uint4*>(p) = words; }
    // ... and texel c of the row, if it lies in the region
    static SZG_DEV void store_texel(unsigned char* drow, int c, unsigned width, unsigned word)
    {
        static_assert(BYTES == 4u, "one word per texel");
        if (holds(c, width))
        {
            *reinterpret_cast<unsigned*>(drow + (size_t)c * BYTES) = word;
        }
    }
    // A group of any row: one store where it is full and this row puts it on a 16-B boundary, texel by texel otherwise
    static SZG_DEV void store(unsigned char* drow, int c0, unsigned width, uint4 words)
    {
        unsigned char* p = address(drow, c0);
        if (full(c0, width) && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u)
        {
            store_aligned(p, words);
            return;
        }
        store_texel(drow, c0, width, words.x);
        store_texel(drow, c0 + 1, width, words.y);
        store_texel(drow, c0 + 2, width, words.z);
        store_texel(drow, c0 + 3, width, words.w);
    }
};
} // namespace szg

#endif // SZG_IMAGE_OPS_HPP
