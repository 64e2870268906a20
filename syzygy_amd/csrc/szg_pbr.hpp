// szg_pbr.hpp — the material, BRDF and shadow-map functions of the lights pass and the composite.
#pragma once

#include "szg/fpmath.h"
#include "szg_lean.hpp"
#include "szg_vec.hpp"

namespace szg
{
// ---------------------------------------------------------------------------
// PBR (gbuffer/pbrFunctions.glinl) and shadow maps (shadowmap.glinl)
// ---------------------------------------------------------------------------
struct Material
{
    V3 position;
    V3 normal;
    V3 subscattering;
    V3 reflectance;
    float occlusion;
    float specularPower;
    float metallic;
    // per-pixel invariants of the BRDF: diffuseBRDF() = subscattering / pi (pbrFunctions.glinl:38) and the
    // Blinn-Phong normalisation (specularPower + 2) / 8 (pbrFunctions.glinl:49)
    V3 diffuse;
    float normalization;
};

// Per-pixel precondition of convertPBR<true> (the caller asks it of every lane of the wave): the largest specular component,
// the denominator of the three reflectance quotients, a positive moderate number - a black specular makes it 0 - and their
// numerators, like the three of subscattering / pi, zeros or moderate numbers; pow(160, 1 - roughness) inside powLean's
// domain - a roughness of 1 makes the exponent 0.
SZG_DEV bool convertPBRLeanOK(V4 diffuse, V4 specular, V4 orm)
{
    float const mx = fmaxf(fmaxf(specular.x, specular.y), specular.z);
    return inRange(mx, 0x1p-60f, 0x1p60f) && leanQuotientOperand(0.5f * specular.x) && leanQuotientOperand(0.5f * specular.y) &&
           leanQuotientOperand(0.5f * specular.z) && leanQuotientOperand(diffuse.x) && leanQuotientOperand(diffuse.y) && leanQuotientOperand(diffuse.z) &&
           powLeanOK(160.0f, 1.0f - orm.y);
}
// pbrFunctions.glinl:3-20. LEAN (convertPBRLeanOK on every lane): the quotients with one shared reciprocal per denominator and
// the sign IEEE gives a zero quotient, pow() without its special cases - the same values.
template <bool LEAN = false> SZG_DEV Material convertPBR(V4 position, V4 normal, V4 diffuse, V4 specular, V4 orm)
{
    Material m;
    V3 const spec = mk3(specular.x, specular.y, specular.z);
    float const mx = fmaxf(fmaxf(spec.x, spec.y), spec.z);
    V3 const halfSpec = splat(0.5f) * spec;
    float const rcpMx = LEAN ? rcpN(mx) : 0.0f;
    V3 const metallicReflectance = LEAN ? mk3(divR(halfSpec.x, mx, rcpMx), divR(halfSpec.y, mx, rcpMx), divR(halfSpec.z, mx, rcpMx))
                                        : halfSpec / mx;
    m.position = mk3(position.x, position.y, position.z);
    m.normal = mk3(normal.x, normal.y, normal.z);
    m.subscattering = mk3(diffuse.x, diffuse.y, diffuse.z);
    m.metallic = orm.z;
    m.reflectance = mix(splat(0.04f), metallicReflectance, splat(m.metallic));
    m.occlusion = orm.x;
    m.specularPower = LEAN ? powLean(160.0f, 1.0f - orm.y) : szg_powf(160.0f, 1.0f - orm.y);
    float const pi = 3.14159265359f;
    float const rcpPi = LEAN ? rcpN(pi) : 0.0f;
    m.diffuse = LEAN ? mk3(divR(m.subscattering.x, pi, rcpPi), divR(m.subscattering.y, pi, rcpPi), divR(m.subscattering.z, pi, rcpPi))
                     : m.subscattering / pi;
    m.normalization = (m.specularPower + 2.0f) / 8.0f;
    return m;
}

// computeLightContribution's BRDF part (lights.comp:93-108 / camera.comp:258-271):
// mix(diffuseBRDF, specularBRDF, fresnel) for outgoing light/view directions. LEAN: the caller has checked
// that |lightDir + viewDir|^2 >= 2^-40 (normalisation with the lean exact ops). POWS: both pow() without their special-case
// selects when no lane of the wave has a zero / denormal base or an exponent outside powLean's domain (as lightContribution
// of the lights pass does).
template <bool LEAN = false, bool POWS = false> SZG_DEV V3 brdfMix(const Material& m, V3 lightDir, V3 viewDir)
{
    V3 const hs = lightDir + viewDir;
    float const hd = dotP(hs, hs);
    V3 const h = hs * divX<LEAN>(1.0f, sqrtX<LEAN>(hd));
    float const baseSpecular = clampf(dotP(h, m.normal), 0.0f, 1.0f);
    float const baseFresnel = 1.0f - clampf(dotP(h, lightDir), 0.0f, 1.0f);
    bool const powsLean = POWS && waveAll(powLeanOK(baseSpecular, m.specularPower) && powLeanOK(baseFresnel, 5.0f));
    float const microfacet = powsLean ? powLean(baseSpecular, m.specularPower) : szg_powf(baseSpecular, m.specularPower);
    V3 const specular = splat(m.normalization * microfacet);
    float const p = powsLean ? powLean(baseFresnel, 5.0f) : szg_powf(baseFresnel, 5.0f);
    V3 const fresnel = m.reflectance + (splat(1.0f) - m.reflectance) * p;
    return mix(m.diffuse, specular, fresnel);
}

// pbrFunctions.glinl:22-32
SZG_DEV V3 computeFresnel(const Material& m, V3 lightOutgoing, V3 viewOutgoing)
{
    V3 const h = normalizeP(lightOutgoing + viewOutgoing);
    float const p = szg_powf(1.0f - clampf(dotP(h, lightOutgoing), 0.0f, 1.0f), 5.0f);
    return m.reflectance + (splat(1.0f) - m.reflectance) * p;
}

// shadowmap.glinl:32-64 with NEAREST / CLAMP_TO_BORDER(0) (shadowpass.cpp:29-35).
// `coord` is shadowCoord / w, (ndx, ndy) the two sqrt terms of computeShadowFrame.
SZG_DEV float sampleShadowMap(const float* __restrict__ map, unsigned W, unsigned H, unsigned pitchFloats, V3 coord, float fdx,
                              float fdy)
{
    float const fragmentDepth = coord.z;
    float const fW = (float)(int)W;
    float const fH = (float)(int)H;
    float const dx = 1.5f * fdx / fW;
    float const dy = 1.5f * fdy / fH;
    float summed = 0.0f;
#pragma unroll
    for (int y = -2; y <= 2; y++)
    {
#pragma unroll
        for (int x = -2; x <= 2; x++)
        {
            float const s = coord.x + (float)x * dx;
            float const t = coord.y + (float)y * dy;
            float const fx = floorf(s * fW);
            float const fy = floorf(t * fH);
            float occluder = 0.0f;
            if (fx >= 0.0f && fy >= 0.0f && fx < fW && fy < fH)
            {
                occluder = map[(unsigned)fy * pitchFloats + (unsigned)fx];
            }
            if (occluder > 0.0f && occluder > fragmentDepth)
            {
                summed += 1.0f;
            }
        }
    }
    return 1.0f - summed / 25.0f;
}

} // namespace szg
