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

// pbrFunctions.glinl:3-20
SZG_DEV Material convertPBR(V4 position, V4 normal, V4 diffuse, V4 specular, V4 orm)
{
    Material m;
    V3 const spec = mk3(specular.x, specular.y, specular.z);
    float const mx = fmaxf(fmaxf(spec.x, spec.y), spec.z);
    V3 const metallicReflectance = (splat(0.5f) * spec) / mx;
    m.position = mk3(position.x, position.y, position.z);
    m.normal = mk3(normal.x, normal.y, normal.z);
    m.subscattering = mk3(diffuse.x, diffuse.y, diffuse.z);
    m.metallic = orm.z;
    m.reflectance = mix(splat(0.04f), metallicReflectance, splat(m.metallic));
    m.occlusion = orm.x;
    m.specularPower = szg_powf(160.0f, 1.0f - orm.y);
    m.diffuse = m.subscattering / 3.14159265359f;
    m.normalization = (m.specularPower + 2.0f) / 8.0f;
    return m;
}

// computeLightContribution's BRDF part (lights.comp:93-108 / camera.comp:258-271):
// mix(diffuseBRDF, specularBRDF, fresnel) for outgoing light/view directions. LEAN: the caller has checked
// that |lightDir + viewDir|^2 >= 2^-40 (normalisation with the lean exact ops).
template <bool LEAN = false> SZG_DEV V3 brdfMix(const Material& m, V3 lightDir, V3 viewDir)
{
    V3 const hs = lightDir + viewDir;
    float const hd = dotP(hs, hs);
    V3 const h = hs * divX<LEAN>(1.0f, sqrtX<LEAN>(hd));
    float const microfacet = szg_powf(clampf(dotP(h, m.normal), 0.0f, 1.0f), m.specularPower);
    V3 const specular = splat(m.normalization * microfacet);
    float const p = szg_powf(1.0f - clampf(dotP(h, lightDir), 0.0f, 1.0f), 5.0f);
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
