// szg_formats.hpp — the store formats of the images (UNORM16, fp16) and the linear image views the kernels take by value.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "szg_vec.hpp"

namespace szg
{
// ---------------------------------------------------------------------------
// Formats
// ---------------------------------------------------------------------------
// imageStore on rgba16 (UNORM16): clamp, scale, round to nearest even.
SZG_DEV unsigned unorm16(float x)
{
    float const c = fminf(fmaxf(x, 0.0f), 1.0f); // NaN -> 0
    return (unsigned)__float2int_rn(c * 65535.0f);
}
SZG_DEV uint2 pack_unorm16x4(float r, float g, float b, float a)
{
    return make_uint2(unorm16(r) | (unorm16(g) << 16), unorm16(b) | (unorm16(a) << 16));
}
SZG_DEV V4 unpack_half4(uint2 v)
{
    __half2 const lo = *reinterpret_cast<const __half2*>(&v.x);
    __half2 const hi = *reinterpret_cast<const __half2*>(&v.y);
    float2 const a = __half22float2(lo);
    float2 const b = __half22float2(hi);
    return V4{a.x, a.y, b.x, b.y};
}
SZG_DEV uint2 pack_half4(float r, float g, float b, float a)
{
    // The stored value is RNE(fp16) of the ROUNDED fp32 value. Keep the compiler from folding a producing fp32
    // multiply into the conversion (v_fma_mixlo_f16 rounds the exact product once: a different result at ties).
    asm volatile("" : "+v"(r), "+v"(g), "+v"(b), "+v"(a));
    __half2 const lo = __floats2half2_rn(r, g);
    __half2 const hi = __floats2half2_rn(b, a);
    uint2 o;
    o.x = *reinterpret_cast<const unsigned*>(&lo);
    o.y = *reinterpret_cast<const unsigned*>(&hi);
    return o;
}

// Linear image view passed by value to kernels.
struct Img
{
    const unsigned char* data;
    unsigned width, height, pitch;
};
struct ImgRW
{
    unsigned char* data;
    unsigned width, height, pitch;
};

// szg_rowtile: local row -> global row
struct RowMap
{
    unsigned block_rows, rank, nranks;
};
SZG_DEV unsigned global_row(const RowMap& m, unsigned local)
{
    if (m.nranks <= 1u)
    {
        return local;
    }
    return ((local / m.block_rows) * m.nranks + m.rank) * m.block_rows + local % m.block_rows;
}

} // namespace szg
