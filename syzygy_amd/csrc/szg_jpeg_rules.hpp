// szg_jpeg_rules.hpp — the reconstruction rules of include/szg/jpeg.h (3 IDCT, 4 UPSAMPLING, 5 COLOUR) as functions, compiled
// into the host path (host_jpeg.cpp, g++) and into the kernels (kernels_jpeg.hip, hipcc): one text, so the two cannot drift.
// Everything is 32-bit two's complement that wraps: the arithmetic is done on uint32_t, and a value is looked at as signed
// only by asr() and by the clamps. No signed overflow reaches the compiler.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SZG_JPEG_FN __host__ __device__ inline
#else
#define SZG_JPEG_FN inline
#endif

namespace szg
{
namespace jpeg
{
// arithmetic shift right of the reinterpreted value
SZG_JPEG_FN int32_t asr(uint32_t v, int n)
{
    return static_cast<int32_t>(v) >> n;
}

SZG_JPEG_FN uint32_t clamp255(int32_t v)
{
    return static_cast<uint32_t>(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// clamp255(asr(v, n)) for n <= 22, written as a clamp of the unshifted value and a logical shift: the same result for every
// v. (The shift-then-saturate form is what hipcc turns into gfx950's v_ashr_pk_u8_i32, whose packed result came back from the
// MI355X with bits above the two bytes set and corrupted the bytes or-ed in next to it)
SZG_JPEG_FN uint32_t shiftClamp255(uint32_t v, int n)
{
    int32_t const x = static_cast<int32_t>(v);
    int32_t const top = static_cast<int32_t>((256u << n) - 1u);
    return static_cast<uint32_t>(x < 0 ? 0 : (x > top ? top : x)) >> n;
}

// (int)(c * 4096 + 0.5) of the twelve constants of jpeg.h rule 3, negative ones as their two's complement
constexpr uint32_t K(int32_t c)
{
    return static_cast<uint32_t>(c);
}
constexpr uint32_t C_0_541 = K(2217), C_N1_847 = K(-7567), C_0_765 = K(3135), C_1_175 = K(4816), C_0_298 = K(1223),
                   C_2_053 = K(8410), C_3_072 = K(12586), C_1_501 = K(6149), C_N0_899 = K(-3685), C_N2_562 = K(-10497),
                   C_N1_961 = K(-8034), C_N0_390 = K(-1597);

// One 8-point pass. s: the eight inputs; bias: what is added to the even part before the butterflies (512 for the column
// pass, 65536 + (128 << 17) for the row pass). o[k] is output k BEFORE its shift.
SZG_JPEG_FN void idct1d(const uint32_t s[8], uint32_t bias, uint32_t o[8])
{
    uint32_t p2 = s[2], p3 = s[6];
    uint32_t p1 = (p2 + p3) * C_0_541;
    uint32_t t2 = p1 + p3 * C_N1_847;
    uint32_t t3 = p1 + p2 * C_0_765;
    p2 = s[0];
    p3 = s[4];
    uint32_t t0 = (p2 + p3) * 4096u;
    uint32_t t1 = (p2 - p3) * 4096u;
    uint32_t const x0 = t0 + t3 + bias, x3 = t0 - t3 + bias, x1 = t1 + t2 + bias, x2 = t1 - t2 + bias;
    t0 = s[7];
    t1 = s[5];
    t2 = s[3];
    t3 = s[1];
    p3 = t0 + t2;
    uint32_t p4 = t1 + t3;
    p1 = t0 + t3;
    p2 = t1 + t2;
    uint32_t const p5 = (p3 + p4) * C_1_175;
    t0 = t0 * C_0_298;
    t1 = t1 * C_2_053;
    t2 = t2 * C_3_072;
    t3 = t3 * C_1_501;
    p1 = p5 + p1 * C_N0_899;
    p2 = p5 + p2 * C_N2_562;
    p3 = p3 * C_N1_961;
    p4 = p4 * C_N0_390;
    t3 += p1 + p4;
    t2 += p2 + p3;
    t1 += p2 + p4;
    t0 += p1 + p3;
    o[0] = x0 + t3;
    o[7] = x0 - t3;
    o[1] = x1 + t2;
    o[6] = x1 - t2;
    o[2] = x2 + t1;
    o[5] = x2 - t1;
    o[3] = x3 + t0;
    o[4] = x3 - t0;
}

constexpr uint32_t COLUMN_BIAS = 512u;
constexpr int COLUMN_SHIFT = 10;
constexpr uint32_t ROW_BIAS = 65536u + (128u << 17);
constexpr int ROW_SHIFT = 17;

// One component's 8-bit sample plane, as rule 4 sees it
struct Plane
{
    const uint8_t* samples;
    uint32_t pitch; // blocks_w * 8
    uint32_t hs, vs; // h_max / h, v_max / v
    uint32_t ch;     // sample rows that exist: ceil(H * v / v_max)
    uint32_t wl;     // source samples a row needs: ceil(W / hs)
};

// The upsampled value of the component at output texel (x, j), x < W, j < H (rule 4). Clamps go to ch - 1 and wl - 1.
SZG_JPEG_FN uint32_t upsampled(const Plane& p, uint32_t x, uint32_t j)
{
    uint32_t nearRow = j / p.vs;
    nearRow = nearRow < p.ch - 1u ? nearRow : p.ch - 1u;
    const uint8_t* const n = p.samples + static_cast<size_t>(nearRow) * p.pitch;
    if (p.vs == 2u && p.hs <= 2u)
    {
        uint32_t farRow;
        if ((j & 1u) == 0u)
        {
            farRow = nearRow > 0u ? nearRow - 1u : 0u;
        }
        else
        {
            farRow = nearRow + 1u < p.ch ? nearRow + 1u : p.ch - 1u;
        }
        const uint8_t* const f = p.samples + static_cast<size_t>(farRow) * p.pitch;
        if (p.hs == 1u)
        {
            return (3u * n[x] + f[x] + 2u) >> 2;
        }
        uint32_t const s = x >> 1;
        uint32_t const ts = 3u * n[s] + f[s];
        if ((x & 1u) == 0u)
        {
            if (s == 0u)
            {
                return (ts + 2u) >> 2;
            }
            return (3u * ts + (3u * n[s - 1u] + f[s - 1u]) + 8u) >> 4;
        }
        if (s == p.wl - 1u)
        {
            return (ts + 2u) >> 2;
        }
        return (3u * ts + (3u * n[s + 1u] + f[s + 1u]) + 8u) >> 4;
    }
    if (p.hs == 2u && p.vs == 1u)
    {
        uint32_t const s = x >> 1;
        if ((x & 1u) == 0u)
        {
            if (s == 0u)
            {
                return n[0];
            }
            if (s == p.wl - 1u)
            {
                return (3u * n[s - 1u] + n[s] + 2u) >> 2; // the reference's last pair weights wl - 2 (rule 4, "quirk")
            }
            return (3u * n[s] + n[s - 1u] + 2u) >> 2;
        }
        if (s == p.wl - 1u)
        {
            return n[s];
        }
        return (3u * n[s] + n[s + 1u] + 2u) >> 2;
    }
    return n[x / p.hs];
}

// f(x) = ((int)(x * 4096.0f + 0.5f)) << 8 of rule 5
constexpr uint32_t F_1_402 = 1470208u, F_0_714 = 748800u, F_0_344 = 360960u, F_1_772 = 1858048u;

// three samples -> the texel as a little-endian dword (R lowest), alpha 255; ycbcr == false: the samples are R, G, B
SZG_JPEG_FN uint32_t texel(uint32_t c0, uint32_t c1, uint32_t c2, bool ycbcr)
{
    if (!ycbcr)
    {
        return c0 | (c1 << 8) | (c2 << 16) | 0xFF000000u;
    }
    uint32_t const yf = (c0 << 20) + (1u << 19);
    uint32_t const cr = c2 - 128u, cb = c1 - 128u;
    uint32_t const r = yf + cr * F_1_402;
    uint32_t const g = yf - cr * F_0_714 + (((0u - cb) * F_0_344) & 0xFFFF0000u);
    uint32_t const b = yf + cb * F_1_772;
    return shiftClamp255(r, 20) | (shiftClamp255(g, 20) << 8) | (shiftClamp255(b, 20) << 16) | 0xFF000000u;
}
} // namespace jpeg
} // namespace szg
