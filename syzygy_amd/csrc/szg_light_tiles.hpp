// szg_light_tiles.hpp — the lights pass's two culls of a (position, spot light) pair, for device AND host code:
//
//   pairCull         : what k_lights' light loop decides for ONE position ("this pixel surely lies outside the cone and
//                      its term is an exact zero"), the code the loop itself runs
//   tileMaySkipLight : the same decision for EVERY position of an axis-aligned box at once, what k_light_tiles runs once
//                      per 64 x 64 screen tile and light
//
// No HIP type appears here: tests/lights_tiles/light_tile_bounds.cpp compiles this header with g++ and holds the second
// against the first on sampled boxes.
#pragma once

#include <math.h>
#include <stddef.h>

#include "szg/contraction.h"

#if defined(__HIPCC__)
#define SZG_HD __host__ __device__ __forceinline__
#else
#define SZG_HD inline
#endif

namespace szg
{
constexpr unsigned LIGHT_TILE_DIM = 64u;   // pixels per side of a screen tile of k_light_tiles
constexpr unsigned LIGHT_TILE_BATCH = 64u; // lights per mask word

// The three rows of the shadow matrix the cone test needs (x, y, w), the light's position and falloff constant, the spot flag.
struct LightCull
{
    float rx[4], ry[4], rw[4];
    float position[3], falloffBound;
    unsigned isSpot;
};

// One pair's cull: rows x, y and w of shadowMatrix * vec4(p, 1), each summed left to right as the shader does, the squared
// distance to the light, and `skip`: the light is a spot light whose record says its own factors are finite (`flags` bit 0 of
// LightRec::leanOK), falloffBound * d^2 >= 2^-28, and the position surely lies outside the cone. (The caller may act on `skip`
// only where every pixel of its wave is finite, kernels_lights.hip.)
struct PairCull
{
    float cx, cy, cw, d2;
    bool skip;
};
SZG_HD bool surelyOutsideCone(float cx, float cy, float cw)
{
    float const acw = fabsf(cw);
    float const ax = fabsf(cx - 0.5f * cw);
    float const ay = fabsf(cy - 0.5f * cw);
    // (one axis outside implies q = dx^2 + dy^2 >= 0.25 only if the other axis is a number. It is: the test is only consulted
    // for a `cullable` pair - every position of the wave finite and <= 2^30, every row of the light <= 2^28 - so the three
    // projected coordinates are finite numbers below 2^60 and no inf - inf can occur.)
    return acw > 0.0f && (ax > 0.505f * acw || ay > 0.505f * acw);
}
SZG_HD PairCull pairCull(const LightCull& c, unsigned flags, float px, float py, float pz)
{
    PairCull r;
    // (M * vec4(p, 1)).row as the oracle's operator* evaluates it: an fma chain over x, y, z, then + m3 * 1
    r.cx = SZG_CON(SZG_C_MATVEC, c.rx[2], pz, SZG_CON(SZG_C_MATVEC, c.rx[1], py, c.rx[0] * px)) + c.rx[3];
    r.cy = SZG_CON(SZG_C_MATVEC, c.ry[2], pz, SZG_CON(SZG_C_MATVEC, c.ry[1], py, c.ry[0] * px)) + c.ry[3];
    r.cw = SZG_CON(SZG_C_MATVEC, c.rw[2], pz, SZG_CON(SZG_C_MATVEC, c.rw[1], py, c.rw[0] * px)) + c.rw[3];
    // A pixel outside the cone contributes (colour * strength / falloff) * 0 * ...: an exact zero ONLY while the quotient
    // is finite. The falloff factor * (distance / falloffDistance)^2 is 0 AT the light's position and underflows next to
    // it, and inf * 0 = NaN poisons the pixel in the reference (found in round 3 by a test that puts G-buffer positions
    // on the lights: rounds 1 and 2 returned 0 there). So the squared distance is formed in front of the cone test, and
    // the two cone culls - like the back-face cull - require falloffBound * d^2 >= 2^-28 (falloff >= 2^-30 with a factor of
    // 4 for the roundings): closer pixels are evaluated in full.
    float const tx = c.position[0] - px, ty = c.position[1] - py, tz = c.position[2] - pz;
    r.d2 = SZG_CON(SZG_C_LDOT, tz, tz, SZG_CON(SZG_C_LDOT, ty, ty, tx * tx));
    bool const falloffAwayFromZero = c.falloffBound * r.d2 >= 0x1p-28f;
    r.skip = c.isSpot != 0u && (flags & 1u) != 0u && falloffAwayFromZero && surelyOutsideCone(r.cx, r.cy, r.cw);
    return r;
}

// The positions of a screen tile: componentwise bounds, and `finite`: every position is a number of magnitude <= 2^30
// (k_lights' positionModerate). lo and hi mean nothing when it is false.
struct TileBox
{
    float lo[3], hi[3];
    bool finite;
};

// true: pairCull(c, flags, p).skip holds for EVERY float position p with lo <= p <= hi, so a wave of that tile whose pixels
// are all finite would `continue` past this light with every lane, and need not visit it.
//
// With k = rx - 0.5 rw the per-pixel test on the x axis is |k.p + k3| > 0.505 |rw.p + rw3| up to the roundings of its float
// evaluation. Over the box an affine form a.p + a3 lies within (its value at the centre) +- sum |a_i| half_i. The test here
// asks for
//     |F(centre)| - radius_F - m  >  0.51 (|W(centre)| + radius_W + m)     and     |W(centre)| - radius_W - m > 0
// with F = k.p + k3 and W = rw.p + rw3 (the sign of W stays open as per pixel, but it must not be zero anywhere in the box:
// the per-pixel test does not reject cw == 0), the same with ry for the y axis, one axis rejecting the whole box. m is the
// rounding margin: every float sum of four products a_i p_i formed per pixel or here is within 4 ulp-fractions (4 * 2^-24) of
// S = sum |a_i| max|p_i| + |a3| of the real value, the centre and half extents add 2 more each, and the per-pixel comparison
// itself rounds twice (1 + 2^-23); fewer than 30 * 2^-24 S in all over both sides of the inequality against m = 64 * 2^-24 (S_xy
// + S_w), plus 2^-100 for products that underflow. 0.51 against the per-pixel 0.505 is another 1 % to spare.
// The falloff guard holds when the nearest point of the box is far enough: per axis |light - p| >= g = max(lo - light, light -
// hi, 0), float subtraction is monotone, so the per-pixel d^2 is at least the sum of the g^2 up to the rounding of three
// additions; the guard is asked with a factor of 2 to spare.
SZG_HD bool tileMaySkipLight(const LightCull& c, unsigned flags, const TileBox& b)
{
    if (!b.finite || c.isSpot == 0u || (flags & 1u) == 0u)
    {
        return false;
    }
    float kx[4], ky[4];
    for (int i = 0; i < 4; i++)
    {
        kx[i] = c.rx[i] - 0.5f * c.rw[i];
        ky[i] = c.ry[i] - 0.5f * c.rw[i];
    }
    float fc = kx[3], gc = ky[3], wc = c.rw[3];                           // the forms at the centre
    float rf = 0.0f, rg = 0.0f, rwr = 0.0f;                               // their radii over the box
    float sx = fabsf(c.rx[3]), sy = fabsf(c.ry[3]), sw = fabsf(c.rw[3]); // the magnitudes the margins scale with
    float d2 = 0.0f;
    for (int i = 0; i < 3; i++)
    {
        float const centre = 0.5f * b.lo[i] + 0.5f * b.hi[i];
        float const half = fmaxf(b.hi[i] - centre, centre - b.lo[i]);
        float const mag = fmaxf(fabsf(b.lo[i]), fabsf(b.hi[i]));
        fc += kx[i] * centre;
        gc += ky[i] * centre;
        wc += c.rw[i] * centre;
        rf += fabsf(kx[i]) * half;
        rg += fabsf(ky[i]) * half;
        rwr += fabsf(c.rw[i]) * half;
        sx += fabsf(c.rx[i]) * mag;
        sy += fabsf(c.ry[i]) * mag;
        sw += fabsf(c.rw[i]) * mag;
        float const g = fmaxf(fmaxf(b.lo[i] - c.position[i], c.position[i] - b.hi[i]), 0.0f);
        d2 += g * g;
    }
    if (!(c.falloffBound * d2 >= 0x1p-27f))
    {
        return false;
    }
    float const mw = 0x1p-18f * sw + 0x1p-100f;
    if (!(fabsf(wc) - rwr - mw > 0.0f))
    {
        return false;
    }
    float const mx = 0x1p-18f * (sx + sw) + 0x1p-100f, my = 0x1p-18f * (sy + sw) + 0x1p-100f;
    bool const outsideX = fabsf(fc) - rf - mx > 0.51f * (fabsf(wc) + rwr + mx);
    bool const outsideY = fabsf(gc) - rg - my > 0.51f * (fabsf(wc) + rwr + my);
    return outsideX || outsideY;
}

// Words of mask storage for an image of at most capacityW x capacityH pixels and `lights` lights.
inline size_t lightTileMaskWords(unsigned capacityW, unsigned capacityH, size_t lights)
{
    size_t const tiles = (size_t)((capacityW + LIGHT_TILE_DIM - 1u) / LIGHT_TILE_DIM) * ((capacityH + LIGHT_TILE_DIM - 1u) / LIGHT_TILE_DIM);
    return tiles * ((lights + LIGHT_TILE_BATCH - 1u) / LIGHT_TILE_BATCH);
}
} // namespace szg
