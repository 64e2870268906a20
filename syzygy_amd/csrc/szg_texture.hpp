// szg_texture.hpp — the material sampler of the G-buffer raster pass as device functions, shared by k_raster_tile
// (kernels_raster.hip), the image passes through szg_image_ops.hpp (decode8: the mip builder, the image copy, the UI layer)
// and the sampler test kernel (tests/mipsample/mipsample.hip). The rules are those of include/szg/raster.h "textures" (one level) and
// include/szg/mipmaps.h "SAMPLER" (a registered chain); every translation unit that includes this is built with
// -ffp-contract=off, so each operation below rounds once.
#ifndef SZG_TEXTURE_HPP
#define SZG_TEXTURE_HPP

#include "szg/raster.h"
#include "szg_device.hpp"

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
} // namespace szg

#endif // SZG_TEXTURE_HPP
