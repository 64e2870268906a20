// szg_texture.hpp — the material sampler of the G-buffer raster pass as device functions, shared by k_raster_tile
// (kernels_raster.hip), the image passes through szg_image_ops.hpp (decode8: the mip builder, the image copy, the UI layer)
// and the sampler test kernels (tests/mipsample/mipsample.hip, tests/anisosample/anisosample.hip). The rules are those of
// include/szg/raster.h "textures" (one level), include/szg/mipmaps.h "SAMPLER" (a registered chain) and
// include/szg/anisotropy.h "SAMPLER" (a chain under maxAnisotropy > 1); every translation unit that includes this is built
// with -ffp-contract=off, so each operation below rounds once.
#ifndef SZG_TEXTURE_HPP
#define SZG_TEXTURE_HPP

#include "szg/fpmath.h"
#include "szg/raster.h"
#include "szg_vec.hpp"

namespace szg
{
// raster.h "textures": RGBA8, LINEAR, REPEAT, one level
SZG_DEV float decode8(unsigned b, bool srgb)
{
    float const c = (float)b / 255.0f;
    if (!srgb)
    {
        return c;
    }
    return c <= 0.04045f ? c / 12.92f : szg_powf((c + 0.055f) / 1.055f, 2.4f);
}
SZG_DEV int wrapIndex(float f, int n)
{
    float const fn = (float)n;
    float const m = f - fn * floorf(f / fn);
    int i = (int)m;
    if (i >= n || i < 0)
    {
        i = 0;
    }
    return i;
}
// `unormTable[b]` = decode8(b, false), `srgbTable[b]` = decode8(b, true): the 36 texel decodes of a pixel are LDS
// look-ups of values each computed once per workgroup by the same expression.
SZG_DEV V3 sampleTexture(const szg_texture& tex, V2 st, const float* unormTable, const float* srgbTable)
{
    if (tex.data == nullptr || tex.width == 0u || tex.height == 0u)
    {
        return splat(0.0f);
    }
    int const W = (int)tex.width, H = (int)tex.height;
    float const u = st.x * (float)W - 0.5f;
    float const v = st.y * (float)H - 0.5f;
    float const fu = floorf(u), fv = floorf(v);
    float const a = u - fu, b = v - fv;
    int const i0 = wrapIndex(fu, W), j0 = wrapIndex(fv, H);
    int const i1 = (i0 + 1 == W) ? 0 : i0 + 1, j1 = (j0 + 1 == H) ? 0 : j0 + 1;
    const unsigned char* base = static_cast<const unsigned char*>(tex.data);
    unsigned const t00 = *reinterpret_cast<const unsigned*>(base + (size_t)j0 * tex.pitch_bytes + (size_t)i0 * 4u);
    unsigned const t10 = *reinterpret_cast<const unsigned*>(base + (size_t)j0 * tex.pitch_bytes + (size_t)i1 * 4u);
    unsigned const t01 = *reinterpret_cast<const unsigned*>(base + (size_t)j1 * tex.pitch_bytes + (size_t)i0 * 4u);
    unsigned const t11 = *reinterpret_cast<const unsigned*>(base + (size_t)j1 * tex.pitch_bytes + (size_t)i1 * 4u);
    const float* const table = tex.srgb != 0u ? srgbTable : unormTable;
    float const w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    float r[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
    {
        unsigned const sh = (unsigned)ch * 8u;
        r[ch] = w00 * table[(t00 >> sh) & 0xFFu] + w10 * table[(t10 >> sh) & 0xFFu] + w01 * table[(t01 >> sh) & 0xFFu] +
                w11 * table[(t11 >> sh) & 0xFFu];
    }
    return mk3(r[0], r[1], r[2]);
}

// ---- mipmaps.h "SAMPLER" ----
// The chain registered for one map: levels 1..levels-1 packed behind `chain` (mipmaps.h "CHAIN LAYOUT"); levels <= 1 or a
// null chain means the one-level rule above.
struct TextureMips
{
    const void* chain;
    unsigned levels;
    float maxLod;
};

// lambda of mipmaps.h from the fine quad derivatives, clamped to [0, min(maxLod, levels - 1)]
SZG_DEV float mipLambda(unsigned W, unsigned H, unsigned levels, float maxLod, V2 dUvDx, V2 dUvDy)
{
    float const mux = dUvDx.x * (float)W, mvx = dUvDx.y * (float)H;
    float const muy = dUvDy.x * (float)W, mvy = dUvDy.y * (float)H;
    float const r2 = fmaxf(mux * mux + mvx * mvx, muy * muy + mvy * mvy);
    float const lam = !(r2 > 0.0f) ? 0.0f : 0.5f * (szg_logf(r2) * 1.44269504f);
    return fminf(fmaxf(lam, 0.0f), fminf(maxLod, (float)(levels - 1u)));
}

// Level k of a texture as a one-level texture (k == 0: the image itself, any pitch).
SZG_DEV szg_texture mipLevel(const szg_texture& tex, const void* chain, int k)
{
    if (k <= 0)
    {
        return tex;
    }
    size_t offset = 0;
    for (int j = 1; j < k; j++)
    {
        offset += (size_t)max(1u, tex.width >> j) * max(1u, tex.height >> j) * 4u;
    }
    szg_texture lv;
    lv.data = static_cast<const unsigned char*>(chain) + offset;
    lv.width = max(1u, tex.width >> k);
    lv.height = max(1u, tex.height >> k);
    lv.pitch_bytes = lv.width * 4u;
    lv.srgb = tex.srgb;
    return lv;
}

SZG_DEV V3 sampleTextureMips(const szg_texture& tex, TextureMips mips, V2 st, V2 dUvDx, V2 dUvDy, const float* unormTable,
                             const float* srgbTable)
{
    if (mips.levels <= 1u || mips.chain == nullptr || tex.data == nullptr || tex.width == 0u || tex.height == 0u)
    {
        return sampleTexture(tex, st, unormTable, srgbTable); // lambda clamps to 0 there: the same value, without the log
    }
    float const lam = mipLambda(tex.width, tex.height, mips.levels, mips.maxLod, dUvDx, dUvDy);
    int const d = (int)floorf(lam);
    float const f = lam - (float)d;
    V3 const lo = sampleTexture(mipLevel(tex, mips.chain, d), st, unormTable, srgbTable);
    if (f == 0.0f)
    {
        return lo;
    }
    V3 const hi = sampleTexture(mipLevel(tex, mips.chain, d + 1), st, unormTable, srgbTable);
    float const g = 1.0f - f;
    return mk3(g * lo.x + f * hi.x, g * lo.y + f * hi.y, g * lo.z + f * hi.z);
}

// ---- anisotropy.h "SAMPLER" ----
// The level behind `lv` = level k of `tex` (k >= 0), without walking the chain again.
SZG_DEV szg_texture mipLevelAfter(const szg_texture& tex, const void* chain, const szg_texture& lv, int k)
{
    szg_texture next;
    next.data = k == 0 ? chain : static_cast<const unsigned char*>(lv.data) + (size_t)lv.width * lv.height * 4u;
    next.width = max(1u, tex.width >> (k + 1));
    next.height = max(1u, tex.height >> (k + 1));
    next.pitch_bytes = next.width * 4u;
    next.srgb = tex.srgb;
    return next;
}

// One trilinear tap between two levels already looked up: f == 0 reads `lo` alone.
SZG_DEV V3 trilinearTap(const szg_texture& lo, const szg_texture& hi, float f, V2 st, const float* unormTable,
                        const float* srgbTable)
{
    V3 const a = sampleTexture(lo, st, unormTable, srgbTable);
    if (f == 0.0f)
    {
        return a;
    }
    V3 const b = sampleTexture(hi, st, unormTable, srgbTable);
    float const g = 1.0f - f;
    return mk3(g * a.x + f * b.x, g * a.y + f * b.y, g * a.z + f * b.z);
}

// maxAnisotropy in [1, 16] (szg_deferred_set_sampler_anisotropy). Lambda, d, f and the two level descriptors are made once
// per map; the tap loop runs to the largest N of the wave with the other lanes masked off, and a wave whose lanes all have
// N == 1 branches over it.
SZG_DEV V3 sampleTextureAniso(const szg_texture& tex, TextureMips mips, float maxAnisotropy, V2 st, V2 dUvDx, V2 dUvDy,
                              const float* unormTable, const float* srgbTable)
{
    if (mips.levels <= 1u || mips.chain == nullptr || tex.data == nullptr || tex.width == 0u || tex.height == 0u)
    {
        return sampleTexture(tex, st, unormTable, srgbTable);
    }
    float const mux = dUvDx.x * (float)tex.width, mvx = dUvDx.y * (float)tex.height;
    float const muy = dUvDy.x * (float)tex.width, mvy = dUvDy.y * (float)tex.height;
    float const px2 = mux * mux + mvx * mvx, py2 = muy * muy + mvy * mvy;
    float const r2 = fmaxf(px2, py2), s2 = fminf(px2, py2);
    float eta = 1.0f;
    if (maxAnisotropy != 1.0f && r2 > 0.0f && r2 != __builtin_inff())
    {
        eta = fminf(sqrtf(r2 / s2), maxAnisotropy);
    }
    int const N = (int)ceilf(eta);
    float lam = !(r2 > 0.0f) ? 0.0f : 0.5f * (szg_logf(r2) * 1.44269504f); // mipmaps.h, and all of it when N == 1
    if (N > 1)
    {
        lam = lam - szg_logf(eta) * 1.44269504f;
    }
    lam = fminf(fmaxf(lam, 0.0f), fminf(mips.maxLod, (float)(mips.levels - 1u)));
    int const d = (int)floorf(lam);
    float const f = lam - (float)d;
    szg_texture const lo = mipLevel(tex, mips.chain, d);
    szg_texture const hi = mipLevelAfter(tex, mips.chain, lo, d); // fetched only where f != 0, and then d + 1 < levels
    if (N == 1)
    {
        return trilinearTap(lo, hi, f, st, unormTable, srgbTable);
    }
    V2 const major = px2 >= py2 ? dUvDx : dUvDy;
    float const parts = (float)(N + 1);
    V3 acc = splat(0.0f);
    for (int i = 1; i <= N; i++)
    {
        float const t = (float)i / parts - 0.5f;
        V3 const tap = trilinearTap(lo, hi, f, V2{st.x + t * major.x, st.y + t * major.y}, unormTable, srgbTable);
        acc = i == 1 ? tap : mk3(acc.x + tap.x, acc.y + tap.y, acc.z + tap.z);
    }
    float const n = (float)N;
    return mk3(acc.x / n, acc.y / n, acc.z / n);
}
} // namespace szg

#endif // SZG_TEXTURE_HPP
