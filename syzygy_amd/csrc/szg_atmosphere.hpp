// szg_atmosphere.hpp — the atmosphere block and its per-frame constants, extinction, the ray / sphere intersections and the
// transmittance-LUT samplers (atmosphere/common.glinl).
#pragma once

#include "szg/abi.h"
#include "szg/fpmath.h"
#include "szg_lean.hpp"
#include "szg_vec.hpp"

namespace szg
{
// ---------------------------------------------------------------------------
// Atmosphere block in registers/SGPRs + per-atmosphere constants
// (types/atmosphere.glinl:3-32)
// ---------------------------------------------------------------------------
struct Atm
{
    V3 scatteringRayleigh;
    float densityScaleRayleigh;
    V3 absorptionRayleigh;
    float planetRadius;
    V3 scatteringMie;
    float densityScaleMie;
    float atmosphereRadius;
    V3 incidentDirectionSun;
    V3 scatteringOzone;
    V3 absorptionOzone;
    V3 sunIntensitySpectrum;
    float sunAngularRadius;
    // hoisted sub-expressions of common.glinl:42-46
    float Ra2, Rp2, H;
    // refined reciprocals for divR (valid when `lean`)
    float rcpH, rcpDsR, rcpDsM, rcp15;
    bool lean; // leanAtmosphere(): every atmosphere-level precondition of the lean ops holds
    // Squared radius floor of the lean paths: >= 0.9 Rp (the x_mu denominator) and >= Rp - 80 min(Hr, Hm), so that both
    // densities exp(-altitude / H) stay finite (<= e^80) wherever a lean path evaluates them.
    float leanFloor2;
    // Zero coefficient vectors (Earth defaults: Rayleigh absorption and ozone scattering are 0, scene.cpp:62-70). With
    // finite densities their terms are exactly +0, and acc + (+0) == acc for every acc but -0, which a sum of
    // products of sign-clear coefficients and non-negative densities cannot be: the lean paths skip those terms.
    bool zeroAbsorptionRayleigh, zeroScatteringOzone;
    bool signClearCoefficients;
    // the extinction sum stays in [2^-40, 2^52] for radii in [sqrt(extFloor2), sqrt(extCeil2)] (lean division of the
    // in-scatter integral): coefficients <= 2^10, densities <= e^27, Rayleigh scattering alone >= 2^-40 at the shell's top
    bool extModerate;
    // the sun direction is a unit vector to 1 % and the sun's angular radius a sane positive number: with extModerate and a
    // moderate transmittance LUT, what makes every environment sample (sky-view LUT, sun disc, ground march) finite for
    // any finite ray — the phase functions see a true cosine (phaseMie's pow(1 + g^2 - 2 g c, 1.5) is NaN for c > 1.025)
    bool sunSane;
    float extFloor2, extCeil2; // Rayleigh / Mie scattering and Rayleigh absorption carry no sign bit: partial sums are never -0
    // Squared radius ceiling of the INNER lean march (marchLoop<true, true>): min(Ra (1 - 2^-10), Rp + 85 min(Hr, Hm)).
    // Below it (a) every transmittance-LUT coordinate has a discriminant r^2 (mu^2 - 1) + Ra^2 >= 2^-10 Ra^2, far above its
    // rounding error, so the clamp to 0 under its square root never acts (the clamp of the distance itself stays: NaN cosines
    // of zero-length segments rely on it), and (b) both densities exp(-altitude / H) have arguments in [-85, 80], where the
    // clamp of exp's argument is the identity.
    float innerCeil2;
    // Frame-uniform operands of the march setup (scatteringIntegral), formed here - once per frame where the block comes from
    // k_frame_prep - with the functions the setup used to call on the same inputs: szg_sinf / szg_cosf(sunAngularRadius),
    // dotA(sun, sun), and its square root by the generic operator (lengthA) and by the lean one (sqrtP; meaningful when
    // leanLength2(sun2) holds, which is the only case the lean setup reads it in).
    float sinSunRadius, cosSunRadius, sun2, sunLength, sunLengthLean;
};
SZG_DEV bool plusZero3(V3 v)
{
    return (__builtin_bit_cast(unsigned, v.x) | __builtin_bit_cast(unsigned, v.y) | __builtin_bit_cast(unsigned, v.z)) == 0u;
}
SZG_DEV bool signClear3(V3 v) // no component negative, -0 or NaN-with-sign; (+NaN passes and poisons every sum alike)
{
    return ((__builtin_bit_cast(unsigned, v.x) | __builtin_bit_cast(unsigned, v.y) | __builtin_bit_cast(unsigned, v.z)) >> 31) == 0u;
}
SZG_DEV Atm load_atm(const szg_atmosphere_packed* p)
{
    Atm a;
    a.scatteringRayleigh = mk3(p->scatteringRayleighPerMm[0], p->scatteringRayleighPerMm[1], p->scatteringRayleighPerMm[2]);
    a.densityScaleRayleigh = p->densityScaleRayleighMm;
    a.absorptionRayleigh = mk3(p->absorptionRayleighPerMm[0], p->absorptionRayleighPerMm[1], p->absorptionRayleighPerMm[2]);
    a.planetRadius = p->planetRadiusMm;
    a.scatteringMie = mk3(p->scatteringMiePerMm[0], p->scatteringMiePerMm[1], p->scatteringMiePerMm[2]);
    a.densityScaleMie = p->densityScaleMieMm;
    a.atmosphereRadius = p->atmosphereRadiusMm;
    a.incidentDirectionSun = mk3(p->incidentDirectionSun[0], p->incidentDirectionSun[1], p->incidentDirectionSun[2]);
    a.scatteringOzone = mk3(p->scatteringOzonePerMm[0], p->scatteringOzonePerMm[1], p->scatteringOzonePerMm[2]);
    a.absorptionOzone = mk3(p->absorptionOzonePerMm[0], p->absorptionOzonePerMm[1], p->absorptionOzonePerMm[2]);
    a.sunIntensitySpectrum = mk3(p->sunIntensitySpectrum[0], p->sunIntensitySpectrum[1], p->sunIntensitySpectrum[2]);
    a.sunAngularRadius = p->sunAngularRadius;
    a.Ra2 = a.atmosphereRadius * a.atmosphereRadius;
    a.Rp2 = a.planetRadius * a.planetRadius;
    a.H = safeSqrt(a.Ra2 - a.Rp2);
    // Preconditions of the lean ops that depend only on the atmosphere: radii, H and density scales of moderate
    // magnitude, and the x_mu denominator rho + H - (Ra - r) bounded away from 0 for every r >= 0.9 Rp.
    float const lo = 0x1p-30f, hi = 0x1p30f;
    // The density scales must also be large against the rounding of a radius (a few ulps of Rp): the zero-coefficient
    // shortcuts and expX<true> count on exp(-altitude / scale) staying finite for samples the lean floor admits, and an
    // altitude that comes out a few ulps below that floor must not be e^100 scale heights deep.
    float const scaleFloor = a.planetRadius * 0x1p-18f;
    a.lean = inRange(a.planetRadius, lo, hi) && inRange(a.atmosphereRadius, lo, hi) && inRange(a.H, lo, hi) &&
             inRange(a.densityScaleRayleigh, fmaxf(lo, scaleFloor), hi) && inRange(a.densityScaleMie, fmaxf(lo, scaleFloor), hi) &&
             (a.H - a.atmosphereRadius + 0.9f * a.planetRadius >= 0x1p-20f);
    // coefficients finite and of moderate magnitude: no NaN / inf can enter the extinction sum on a lean path
    // (expX<true> relies on that)
    V3 const* const coefficients[5] = {&a.scatteringRayleigh, &a.absorptionRayleigh, &a.scatteringMie, &a.scatteringOzone, &a.absorptionOzone};
#pragma unroll
    for (int i = 0; i < 5; i++)
    {
        a.lean = a.lean && inRange(fabsf(coefficients[i]->x), 0.0f, hi) && inRange(fabsf(coefficients[i]->y), 0.0f, hi) &&
                 inRange(fabsf(coefficients[i]->z), 0.0f, hi);
    }
    float const rFloor = fmaxf(0.9f * a.planetRadius, a.planetRadius - 80.0f * fminf(a.densityScaleRayleigh, a.densityScaleMie));
    a.leanFloor2 = rFloor * rFloor;
    bool const signs = signClear3(a.scatteringRayleigh) && signClear3(a.scatteringMie);
    a.signClearCoefficients = signs && signClear3(a.absorptionRayleigh);
    a.zeroAbsorptionRayleigh = signs && plusZero3(a.absorptionRayleigh);
    a.zeroScatteringOzone = signs && signClear3(a.absorptionRayleigh) && plusZero3(a.scatteringOzone);
    {
        float const shell = a.atmosphereRadius - a.planetRadius;
        float const minRayleigh = fminf(fminf(a.scatteringRayleigh.x, a.scatteringRayleigh.y), a.scatteringRayleigh.z);
        float const thinnest = szg_expf(-1.02f * (shell / a.densityScaleRayleigh)) * 0.5f;
        bool small = true;
#pragma unroll
        for (int i = 0; i < 5; i++)
        {
            small = small && coefficients[i]->x <= 0x1p10f && coefficients[i]->y <= 0x1p10f && coefficients[i]->z <= 0x1p10f;
        }
        a.extModerate = a.lean && a.signClearCoefficients && signClear3(a.scatteringOzone) && signClear3(a.absorptionOzone) && small &&
                        inRange(shell, lo, hi) && (minRayleigh * thinnest >= 0x1p-40f);
        float const sun2 = dot(a.incidentDirectionSun, a.incidentDirectionSun);
        // (and its azimuth exists: normalize(vec2(-sun.x, -sun.z)) of skyview_LUT.comp:60-61 / camera.comp:113-114 is 0/0 for an
        // exactly vertical sun)
        float const sunHorizontal2 = a.incidentDirectionSun.x * a.incidentDirectionSun.x + a.incidentDirectionSun.z * a.incidentDirectionSun.z;
        a.sunSane = inRange(sun2, 0.98f, 1.02f) && inRange(a.sunAngularRadius, 0x1p-30f, 1.5f) && sunHorizontal2 >= 0x1p-100f;
        float const eFloor = fmaxf(0.9f * a.planetRadius, a.planetRadius - 27.0f * fminf(a.densityScaleRayleigh, a.densityScaleMie));
        float const eCeil = a.atmosphereRadius + shell * 0.005f;
        a.extFloor2 = eFloor * eFloor;
        a.extCeil2 = eCeil * eCeil;
        float const iCeil = fminf(a.atmosphereRadius * (1.0f - 0x1p-10f),
                                  a.planetRadius + 85.0f * fminf(a.densityScaleRayleigh, a.densityScaleMie));
        a.innerCeil2 = iCeil * iCeil;
    }
    a.rcpH = rcpN(a.lean ? a.H : 1.0f);
    a.rcpDsR = rcpN(a.lean ? a.densityScaleRayleigh : 1.0f);
    a.rcpDsM = rcpN(a.lean ? a.densityScaleMie : 1.0f);
    a.rcp15 = rcpN(15.0f);
    a.sinSunRadius = szg_sinf(a.sunAngularRadius);
    a.cosSunRadius = szg_cosf(a.sunAngularRadius);
    a.sun2 = dotA(a.incidentDirectionSun, a.incidentDirectionSun);
    a.sunLength = lengthA(a.incidentDirectionSun);
    a.sunLengthLean = sqrtP(a.sun2);
    return a;
}

// common.glinl:194-216. Mie absorption uses the Rayleigh coefficient (line 202).
struct Extinction
{
    V3 scatteringRayleigh;
    V3 scatteringMie;
    V3 extinction;
};
template <bool LEAN>
SZG_DEV Extinction extinctionFromDensities(const Atm& a, float altitude, float densityRayleigh, float densityMie, bool belowOzone);
template <bool LEAN = false, bool INNER = false> SZG_DEV Extinction sampleExtinction(const Atm& a, float altitude, bool belowOzone = false)
{
    // (the lean paths never see a NaN altitude: every radius along the ray is finite and above the lean floor)
    if (LEAN && INNER)
    {
        // radii in [lean floor, inner ceiling]: -altitude / H in [-85, 80] for both scale heights (Atm::innerCeil2)
        float const densityRayleigh = expInner(divR0(-altitude, a.densityScaleRayleigh, a.rcpDsR));
        float const densityMie = expInner(divR0(-altitude, a.densityScaleMie, a.rcpDsM));
        return extinctionFromDensities<true>(a, altitude, densityRayleigh, densityMie, belowOzone);
    }
    float const densityRayleigh = expX<LEAN>(divRX<LEAN>(-altitude, a.densityScaleRayleigh, a.rcpDsR));
    float const densityMie = expX<LEAN>(divRX<LEAN>(-altitude, a.densityScaleMie, a.rcpDsM));
    return extinctionFromDensities<LEAN>(a, altitude, densityRayleigh, densityMie, belowOzone);
}
// belowOzone (wave-uniform, MarchSetup): every sample of the ray lies below 9.9 km, so altitude * 1000 - 25 <= -15.09 and the
// test |h - 25 km| >= 15 km below holds at every step without being evaluated
template <bool LEAN>
SZG_DEV Extinction extinctionFromDensities(const Atm& a, float altitude, float densityRayleigh, float densityMie, bool belowOzone)
{
    V3 const scatteringRayleigh = a.scatteringRayleigh * densityRayleigh;
    V3 const absorptionRayleigh = a.absorptionRayleigh * densityRayleigh;
    V3 const scatteringMie = a.scatteringMie * densityMie;
    V3 const absorptionMie = a.absorptionRayleigh * densityMie;
    Extinction e;
    e.scatteringRayleigh = scatteringRayleigh;
    e.scatteringMie = scatteringMie;
    if (LEAN && belowOzone && a.signClearCoefficients)
    {
        e.extinction = a.zeroAbsorptionRayleigh ? (scatteringRayleigh + scatteringMie)
                                                : (((scatteringRayleigh + absorptionRayleigh) + scatteringMie) + absorptionMie);
        return e;
    }
    float const ozoneOffset = fabsf(altitude * 1000.0f - 25.0f);
    // Outside the ozone tent (|h - 25 km| >= 15 km) the density is max(0, 1 - q) with q >= 1, i.e. +0, and both ozone
    // products are +-0: adding them to a partial sum that is not -0 (sign-clear coefficients) changes nothing. When that holds for the whole wave (aerial-perspective marches
    // near the ground, high-altitude samples) the tent, its division and the two terms are skipped.
    bool const noOzone = LEAN && a.signClearCoefficients && waveAll(ozoneOffset >= 15.0f);
    if (noOzone)
    {
        e.extinction = a.zeroAbsorptionRayleigh ? (scatteringRayleigh + scatteringMie)
                                                : (((scatteringRayleigh + absorptionRayleigh) + scatteringMie) + absorptionMie);
        return e;
    }
    float const densityOzone = fmaxf(0.0f, 1.0f - divRX<LEAN>(ozoneOffset, 15.0f, a.rcp15));
    V3 const scatteringOzone = a.scatteringOzone * densityOzone;
    V3 const absorptionOzone = a.absorptionOzone * densityOzone;
    if (LEAN && a.zeroAbsorptionRayleigh && a.zeroScatteringOzone)
    {
        // + absorptionRayleigh, + absorptionMie (= absorptionRayleigh coefficient, Q1) and + scatteringOzone add exact +0
        e.extinction = (scatteringRayleigh + scatteringMie) + absorptionOzone;
    }
    else if (LEAN && a.zeroAbsorptionRayleigh)
    {
        e.extinction = ((scatteringRayleigh + scatteringMie) + scatteringOzone) + absorptionOzone;
    }
    else
    {
        e.extinction = scatteringRayleigh + absorptionRayleigh + scatteringMie + absorptionMie + scatteringOzone + absorptionOzone;
    }
    return e;
}

// common.glinl:220-260
SZG_DEV bool raySphere(V3 f, V3 d, float radius, float& t0, float& t1)
{
    float const b = -1.0f * dotA(f, d);
    V3 const chord = f + b * d;
    float const discriminant = radius * radius - dotA(chord, chord);
    float const c = dotA(f, f) - radius * radius;
    if (discriminant < 0.0f)
    {
        return false;
    }
    float q = b;
    float const s = sqrtf(discriminant);
    q = (b < 0.0f) ? (q - s) : (q + s);
    float a0 = c / q;
    float a1 = q;
    if (a0 > a1)
    {
        float const tmp = a0;
        a0 = a1;
        a1 = tmp;
    }
    t0 = a0;
    t1 = a1;
    return true;
}

// common.glinl:284-307
SZG_DEV float raycastAtmosphere(const Atm& a, V3 origin, V3 direction)
{
    float at0 = 0.0f, at1 = 0.0f;
    bool const hitAtmosphere = raySphere(origin, direction, a.atmosphereRadius, at0, at1) && at1 > 0.0f;
    at0 = fmaxf(0.0f, at0);
    float pt0 = 0.0f, pt1 = 0.0f;
    bool const hitPlanet = raySphere(origin, direction, a.planetRadius, pt0, pt1) && pt0 > 0.0f;
    if (hitPlanet)
    {
        at1 = fminf(pt0, at1);
    }
    return hitAtmosphere ? (at1 - at0) : 0.0f;
}

// ---------------------------------------------------------------------------
// Transmittance LUT sampler: LINEAR / CLAMP_TO_EDGE / fp32 weights
// (renderer/pipelines/skyview.cpp:199-207, :339-346)
// ---------------------------------------------------------------------------
struct TLut
{
    const float4* texels; // RGBA32F, row-major, pitch = width texels
    int width, height;
    float fwidth, fheight;
    // textureCoordFromUnitRange constants (common.glinl:29-32)
    float u_bias, u_scale, v_bias, v_scale;
    // every texel's rgb lies in [2^-50, 2] (status dword behind the texels, szg_launch.hpp "transmittance LUT block"):
    // any bilinear tap then lies in [2^-51, 2.01], inside the operand domain of the lean exact division
    bool moderate;
    // wave-uniform, from k_frame_prep (FramePrep::rowsInterior): for every radius of an INNER march (radius^2 <= Atm::innerCeil2,
    // with a margin of 2^-16) both LUT rows of a tap, floor(v) and floor(v) + 1, lie inside [0, H - 1] - the two clamps of
    // radiusPart are identities there and the row offsets can be formed in float
    bool rowsInterior;
};
SZG_DEV bool tlutTexelModerate(float x, float y, float z)
{
    return inRange(x, 0x1p-50f, 2.0f) && inRange(y, 0x1p-50f, 2.0f) && inRange(z, 0x1p-50f, 2.0f);
}
// a sky-view LUT texel the composite may leave unsampled: a finite number well inside the fp32 range
SZG_DEV bool slutTexelFinite(float r, float g, float b) { return fabsf(r) <= 0x1p100f && fabsf(g) <= 0x1p100f && fabsf(b) <= 0x1p100f; }
SZG_DEV TLut make_tlut(const float4* texels, int w, int h)
{
    TLut t;
    t.moderate = reinterpret_cast<const unsigned*>(texels + (size_t)w * (size_t)h)[0] == 0u;
    t.texels = texels;
    t.width = w;
    t.height = h;
    t.fwidth = (float)w;
    t.fheight = (float)h;
    t.u_bias = 0.5f / (float)w;
    t.u_scale = 1.0f - 1.0f / (float)w;
    t.v_bias = 0.5f / (float)h;
    t.v_scale = 1.0f - 1.0f / (float)h;
    t.rowsInterior = false;
    return t;
}

// Per-frame constants (k_frame_prep, one lane, launched in front of the composite and the sky-view LUT kernel): everything
// load_atm() and make_tlut() derive from the atmosphere block and the LUT extent - ~300 instructions that every wave of
// those kernels would otherwise repeat - computed once and read back through scalar loads. Same code, same values.
struct FramePrep
{
    Atm a;
    float fwidth, fheight, u_bias, u_scale, v_bias, v_scale;
    // camera.comp:366-369: TO_TEX_COORD_MAT * (sun.projection * sun.view), the shadow frame's matrix of the composite - two 4x4
    // products that are the same for every pixel (round 2 formed them per lane, ~300 VALU instructions per geometry pixel when a
    // sun shadow map is bound). Same mul(), same order; read back through scalar loads. Valid when the composite has a sun map.
    float sunShadow[16];
    // TLut::rowsInterior (k_frame_prep evaluates the LUT's v coordinate at both ends of the INNER radius range: the map is
    // monotone, every operation in it being correctly rounded)
    unsigned rowsInterior;
    // What phase A of the composite derives from the camera block, the atmosphere block and the draw extent alone
    // (camera.comp:320-322, :75-77, :113, :125-126, :144-147, common.glinl:114-136), formed by k_frame_prep with the generic
    // operators - which are right in every operand domain, and what the lean ones return inside theirs - through the same
    // functions on the same inputs. Valid in the block of a record call that hands k_frame_prep a camera (the composite's).
    // Read in phase A only: nothing of it is live across the march.
    struct Camera
    {
        V3 position;                 // camera position / 1e6, y flipped, + planetRadius
        float r2, sinHorizon;        // dot(position, position); planetRadius / length(position)
        float horizonZenith, cosHorizonZenith, piMinusHorizon; // sampleMap_Direction's horizon terms for a ray from the camera
        V2 projectedLight;           // normalize(vec2(-sun.x, -sun.z))
        float sunLength;             // length(-sun) (SZG_C_DOT; Atm::sunLength is the SZG_C_ATMODOT one)
        V3 lightDirection;           // normalize(-sun)
        // radiusPart(lengthA(position)) of sampleT_Segment's `from` side, field by field, and rcpN of its denominator for the
        // lean form (meaningful where the lean gate of the call holds, which is the only case it is read in)
        float lenFrom, from_r2, from_d_min, from_denom, from_rcpDenom, from_b, from_omb;
        unsigned from_row0, from_row1;
        float rcpDrawW, rcpDrawH;    // rcpN((float)drawW), rcpN((float)drawH): the clip coordinates' shared reciprocals
    } camera;
};
// The block arrives through scalar loads; its floats then move to vector registers, where the per-wave derivation used to
// leave them: a VALU instruction of gfx950 reads at most one scalar operand, and ~70 constants held in scalar registers
// through the march loops spill (v_writelane / v_readlane inside the loops). The flags stay scalar: they steer wave-uniform
// branches.
SZG_DEV float inVector(float x)
{
    asm volatile("" : "+v"(x));
    return x;
}
SZG_DEV V3 inVector(V3 v) { return V3{inVector(v.x), inVector(v.y), inVector(v.z)}; }
SZG_DEV Atm load_atm(const FramePrep& f)
{
    Atm a = f.a;
    a.scatteringRayleigh = inVector(a.scatteringRayleigh);
    a.densityScaleRayleigh = inVector(a.densityScaleRayleigh);
    a.absorptionRayleigh = inVector(a.absorptionRayleigh);
    a.planetRadius = inVector(a.planetRadius);
    a.scatteringMie = inVector(a.scatteringMie);
    a.densityScaleMie = inVector(a.densityScaleMie);
    a.atmosphereRadius = inVector(a.atmosphereRadius);
    a.incidentDirectionSun = inVector(a.incidentDirectionSun);
    a.scatteringOzone = inVector(a.scatteringOzone);
    a.absorptionOzone = inVector(a.absorptionOzone);
    a.sunIntensitySpectrum = inVector(a.sunIntensitySpectrum);
    a.sunAngularRadius = inVector(a.sunAngularRadius);
    a.Ra2 = inVector(a.Ra2);
    a.Rp2 = inVector(a.Rp2);
    a.H = inVector(a.H);
    a.rcpH = inVector(a.rcpH);
    a.rcpDsR = inVector(a.rcpDsR);
    a.rcpDsM = inVector(a.rcpDsM);
    a.rcp15 = inVector(a.rcp15);
    a.leanFloor2 = inVector(a.leanFloor2);
    a.extFloor2 = inVector(a.extFloor2);
    a.extCeil2 = inVector(a.extCeil2);
    a.innerCeil2 = inVector(a.innerCeil2);
    return a;
}
SZG_DEV TLut make_tlut(const float4* texels, int w, int h, const FramePrep& f)
{
    TLut t;
    t.moderate = reinterpret_cast<const unsigned*>(texels + (size_t)w * (size_t)h)[0] == 0u;
    t.texels = texels;
    t.width = w;
    t.height = h;
    t.fwidth = inVector(f.fwidth);
    t.fheight = inVector(f.fheight);
    t.u_bias = inVector(f.u_bias);
    t.u_scale = inVector(f.u_scale);
    t.v_bias = inVector(f.v_bias);
    t.v_scale = inVector(f.v_scale);
    t.rowsInterior = f.rowsInterior != 0u;
    return t;
}

SZG_DEV V3 bilinear_rgb(const float4* __restrict__ texels, int W, int H, float fW, float fH, float s, float t)
{
    float const u = SZG_CON(SZG_C_TEXCOORD, s, fW, -0.5f);
    float const v = SZG_CON(SZG_C_TEXCOORD, t, fH, -0.5f);
    float const fu = floorf(u);
    float const fv = floorf(v);
    float const a = u - fu;
    float const b = v - fv;
    int i0 = (int)fu, j0 = (int)fv;
    int i1 = i0 + 1, j1 = j0 + 1;
    i0 = min(max(i0, 0), W - 1);
    i1 = min(max(i1, 0), W - 1);
    j0 = min(max(j0, 0), H - 1);
    j1 = min(max(j1, 0), H - 1);
    float4 const t00 = texels[j0 * W + i0];
    float4 const t10 = texels[j0 * W + i1];
    float4 const t01 = texels[j1 * W + i0];
    float4 const t11 = texels[j1 * W + i1];
    float const w00 = (1.0f - a) * (1.0f - b);
    float const w10 = a * (1.0f - b);
    float const w01 = (1.0f - a) * b;
    float const w11 = a * b;
    V3 r;
    r.x = SZG_CON(SZG_C_BILINEAR, w11, t11.x, SZG_CON(SZG_C_BILINEAR, w01, t01.x, SZG_CON(SZG_C_BILINEAR, w10, t10.x, w00 * t00.x)));
    r.y = SZG_CON(SZG_C_BILINEAR, w11, t11.y, SZG_CON(SZG_C_BILINEAR, w01, t01.y, SZG_CON(SZG_C_BILINEAR, w10, t10.y, w00 * t00.y)));
    r.z = SZG_CON(SZG_C_BILINEAR, w11, t11.z, SZG_CON(SZG_C_BILINEAR, w01, t01.z, SZG_CON(SZG_C_BILINEAR, w10, t10.z, w00 * t00.z)));
    return r;
}

// transmittanceLUT_RMu_to_UV (common.glinl:40-66) + the bilinear fetch, split into the
// part that depends only on the radius (v coordinate, row pair and row weights) and the
// part that depends on mu. Two taps at the same radius share the first part; every
// operation and its order are those of the unsplit evaluation.
struct Rgb
{
    float x, y, z;
};
struct RadiusPart
{
    float r, r2;        // radius, radius * radius
    float d_min, denom; // atmosphereRadius - radius, (rho + H) - d_min
    float rcpDenom;     // rcpN(denom) when LEAN
    unsigned row0;      // texel index of the start of rows j0, j1 (clamped); 32-bit so that the taps use
    unsigned row1;      // SGPR-base + VGPR-offset addressing instead of 64-bit VALU address arithmetic
    float b, omb;       // v weight and 1 - b
};
SZG_DEV RadiusPart cameraRadiusPart(const FramePrep::Camera& c)
{
    RadiusPart p;
    p.r = c.lenFrom;
    p.r2 = c.from_r2;
    p.d_min = c.from_d_min;
    p.denom = c.from_denom;
    p.rcpDenom = c.from_rcpDenom;
    p.row0 = c.from_row0;
    p.row1 = c.from_row1;
    p.b = c.from_b;
    p.omb = c.from_omb;
    return p;
}
template <bool LEAN = false, bool INNER = false> SZG_DEV RadiusPart radiusPart(const TLut& L, const Atm& a, float radius)
{
    RadiusPart p;
    p.r = radius;
    p.r2 = radius * radius;
    float const rho = safeSqrtX<LEAN>(p.r2 - a.Rp2);
    p.d_min = a.atmosphereRadius - radius;
    float const d_max = rho + a.H;
    p.denom = d_max - p.d_min;
    p.rcpDenom = LEAN ? rcpN(p.denom) : 0.0f;
    float const x_radius = divRX<LEAN>(rho, a.H, a.rcpH);
    float const t = SZG_CON(SZG_C_LUTMAP, x_radius, L.v_scale, L.v_bias);
    float const v = SZG_CON(SZG_C_TEXCOORD, t, L.fheight, -0.5f);
    float const fv = floorf(v);
    p.b = v - fv;
    p.omb = 1.0f - p.b;
    // clamp((int)fv, 0, H-1) and clamp((int)fv + 1, 0, H-1) with the clamp done in float by v_med3_f32 (one instruction
    // instead of two integer ones per index): the same indices for every finite fv (integer-valued; beyond 2^24
    // fv + 1 == fv and both land on the same edge, as the saturating conversion does). For a NaN fv the weights are NaN
    // and so is the result, whichever texels are fetched.
    if (LEAN && INNER && L.rowsInterior)
    {
        // 0 <= fv <= H - 2 for every radius of this march (TLut::rowsInterior): the clamped indices are fv and fv + 1 themselves,
        // and fv * W is an exact float product below 2^24 (the flag also says W * H <= 2^24): one conversion, one full-rate
        // multiply and one add instead of two clamps, two conversions and two integer multiplies. (A NaN fv converts to row 0
        // and has NaN weights: a NaN tap whichever texels are fetched, as above.)
        p.row0 = (unsigned)(int)(fv * L.fwidth);
        p.row1 = p.row0 + (unsigned)L.width;
        return p;
    }
    float const hm1 = L.fheight - 1.0f;
    int const j0 = (int)__builtin_amdgcn_fmed3f(fv, 0.0f, hm1);
    int const j1 = (int)__builtin_amdgcn_fmed3f(fv + 1.0f, 0.0f, hm1);
    p.row0 = (unsigned)(j0 * L.width);
    p.row1 = (unsigned)(j1 * L.width);
    return p;
}
template <bool LEAN = false, bool INNER = false> SZG_DEV V3 sampleT_at(const TLut& L, const Atm& a, const RadiusPart& p, float mu)
{
    // INNER (radius^2 <= Atm::innerCeil2): for a mu that is a number the discriminant is >= 2^-10 Ra^2 against rounding
    // errors of 2^-22 relative, so max(., 0) inside safeSqrt and sqrtN's own guard never act. The clamp of d STAYS: mu is NaN
    // where a march segment has length 0 (geometry nearer than 32 ulps of the planet radius, ~15 m: normalize(0) = NaN,
    // common.glinl:114-136), and max(NaN, 0) = 0 is what the reference then samples with (found by the 6 000-seed sweep of
    // round 2: a version without this clamp let the NaN through to the texel weights in 8 of 6 000 random frames).
    float const disc = SZG_CON(SZG_C_LUTDIST, p.r2, SZG_CON(SZG_C_LUTDIST, mu, mu, -1.0f), a.Ra2);
    float const d = fmaxf(SZG_CON(SZG_C_LUTDIST, -p.r, mu, (LEAN && INNER) ? sqrtP(disc) : safeSqrtX<LEAN>(disc)), 0.0f);
    float const x_mu = divRX<LEAN>(d - p.d_min, p.denom, p.rcpDenom);
    float const s = SZG_CON(SZG_C_LUTMAP, x_mu, L.u_scale, L.u_bias);
    float const u = SZG_CON(SZG_C_TEXCOORD, s, L.fwidth, -0.5f);
    float const fu = floorf(u);
    float const al = u - fu;
    float const wm1 = L.fwidth - 1.0f;
    // only .rgb is consumed (common.glinl:111, :142): 12-byte loads keep 16 VGPRs per step out of flight
    const char* const base = reinterpret_cast<const char*>(L.texels);
    unsigned o00, o10, o01, o11; // byte offsets of the four texels
    // (0 <= fu <= W - 2 as ONE unsigned compare of the converted index: a negative fu converts to a negative int = a huge
    // unsigned, an fu beyond int range saturates to INT_MAX, and a NaN fu, which converts to 0, has NaN weights and gives
    // a NaN texel average on either path)
    unsigned const iu = (unsigned)(int)fu;
    if (LEAN && INNER && waveAll(iu <= (unsigned)(L.width - 2)))
    {
        // interior column for the whole wave (the rule; the clamps only act for rays that point into the ground, x_mu > 1, or
        // on a rounding below 0): i0 = fu and i1 = fu + 1 are the unclamped indices and the right-hand texel of each row is
        // the next 16 bytes: one conversion and two full-rate adds instead of two clamps, two conversions and two shifts
        unsigned const i0 = iu;
        o00 = (p.row0 + i0) << 4;
        o01 = (p.row1 + i0) << 4;
        o10 = o00 + 16u;
        o11 = o01 + 16u;
    }
    else
    {
        int const i0 = (int)__builtin_amdgcn_fmed3f(fu, 0.0f, wm1); // see radiusPart
        int const i1 = (int)__builtin_amdgcn_fmed3f(fu + 1.0f, 0.0f, wm1);
        o00 = (p.row0 + (unsigned)i0) << 4;
        o10 = (p.row0 + (unsigned)i1) << 4;
        o01 = (p.row1 + (unsigned)i0) << 4;
        o11 = (p.row1 + (unsigned)i1) << 4;
    }
    Rgb t00, t10, t01, t11;
    {
        t00 = *reinterpret_cast<const Rgb*>(base + o00);
        t10 = *reinterpret_cast<const Rgb*>(base + o10);
        t01 = *reinterpret_cast<const Rgb*>(base + o01);
        t11 = *reinterpret_cast<const Rgb*>(base + o11);
    }
    float const oma = 1.0f - al;
    float const w00 = oma * p.omb;
    float const w10 = al * p.omb;
    float const w01 = oma * p.b;
    float const w11 = al * p.b;
    V3 r;
    r.x = SZG_CON(SZG_C_BILINEAR, w11, t11.x, SZG_CON(SZG_C_BILINEAR, w01, t01.x, SZG_CON(SZG_C_BILINEAR, w10, t10.x, w00 * t00.x)));
    r.y = SZG_CON(SZG_C_BILINEAR, w11, t11.y, SZG_CON(SZG_C_BILINEAR, w01, t01.y, SZG_CON(SZG_C_BILINEAR, w10, t10.y, w00 * t00.y)));
    r.z = SZG_CON(SZG_C_BILINEAR, w11, t11.z, SZG_CON(SZG_C_BILINEAR, w01, t01.z, SZG_CON(SZG_C_BILINEAR, w10, t10.z, w00 * t00.z)));
    return r;
}

// common.glinl:40-66 + :138-143 : sample at (radius, mu)
template <bool LEAN = false> SZG_DEV V3 sampleT_RadiusMu(const TLut& L, const Atm& a, float radius, float mu)
{
    RadiusPart const p = radiusPart<LEAN>(L, a, radius);
    return sampleT_at<LEAN>(L, a, p, mu);
}

// Wave-uniform precondition of the LEAN forms of the samplers below, given the squared radii / lengths they take square roots
// and quotients of: the atmosphere admits the lean ops (Atm::lean), every radius is above the lean floor and every
// length a normal number of moderate size.
SZG_DEV bool leanLength2(float x) { return inRange(x, 0x1p-60f, 0x1p60f); }
SZG_DEV bool leanRadius2(const Atm& a, float r2) { return r2 >= a.leanFloor2 && r2 <= 0x1p60f; }

// common.glinl:104-112
template <bool LEAN = false> SZG_DEV V3 sampleT_Ray(const TLut& L, const Atm& a, V3 position, V3 direction)
{
    if (LEAN)
    {
        // lengthA() = sqrt(dot) and the quotient, with the lean exact operators (same values)
        float const radius = sqrtP(dotA(position, position));
        float const mu = divN0(dotA(position, direction), radius * sqrtP(dotA(direction, direction)));
        return sampleT_RadiusMu<true>(L, a, radius, mu);
    }
    float const radius = lengthA(position);
    float const mu = dotA(position, direction) / (lengthA(position) * lengthA(direction));
    return sampleT_RadiusMu(L, a, radius, mu);
}

// common.glinl:114-136. The flipped branch samples with -direction, whose mu is the exact
// negation of the unflipped one (negation commutes with every rounding), so one code path
// with a sign select reproduces both branches.
template <bool LEAN = false, bool INNER = false>
SZG_DEV V3 segmentRatio(const TLut& L, const Atm& a, const RadiusPart& pFrom, float fromDotDir, float lenFrom,
                        const RadiusPart& pTo, float toDotDir, float lenTo, float lenDir)
{
    bool const flip = fromDotDir < 0.0f;
    float const muFrom = divX<LEAN>(fromDotDir, lenFrom * lenDir);
    float const muTo = divX<LEAN>(toDotDir, lenTo * lenDir);
    // flip ? -mu : mu as a sign-bit XOR (one VALU op instead of a compare/select pair through VCC); for the
    // ratio, numerator and denominator are swapped by selecting the operands once rather than two quotients
    unsigned const signFlip = flip ? 0x80000000u : 0u;
    V3 const Tf = sampleT_at<LEAN, INNER>(L, a, pFrom, xorSign(muFrom, signFlip));
    V3 const Tt = sampleT_at<LEAN, INNER>(L, a, pTo, xorSign(muTo, signFlip));
    if (LEAN && L.moderate)
    {
        // both taps lie in [2^-51, 2.01]; the quotient is clamped to [0, 1] and then consumed sign-blind
        V3 const ql = flip ? V3{divN0(Tt.x, Tf.x), divN0(Tt.y, Tf.y), divN0(Tt.z, Tf.z)}
                           : V3{divN0(Tf.x, Tt.x), divN0(Tf.y, Tt.y), divN0(Tf.z, Tt.z)};
        return clamp01(ql);
    }
    V3 const q = flip ? (Tt / Tf) : (Tf / Tt);
    return clamp01(q);
}
// sampleT_Segment with the radius part and the length of the `from` side handed in (FramePrep::Camera: the camera's, once per
// frame): radiusPart<LEAN>(L, a, lenFrom) and lenFrom = |from| as the form below derives them
template <bool LEAN = false> SZG_DEV V3 sampleT_Segment(const TLut& L, const Atm& a, V3 from, const RadiusPart& pf, float lenFrom, V3 to)
{
    if (LEAN)
    {
        V3 const segment = to - from;
        V3 const direction = segment * divN0(1.0f, sqrtP(dotA(segment, segment))); // normalizeA()
        float const lenTo = sqrtP(dotA(to, to));
        RadiusPart const pt = radiusPart<true>(L, a, lenTo);
        return segmentRatio<true>(L, a, pf, dotA(from, direction), lenFrom, pt, dotA(to, direction), lenTo, sqrtP(dotA(direction, direction)));
    }
    V3 const direction = normalizeA(to - from);
    float const lenTo = lengthA(to);
    RadiusPart const pt = radiusPart<false>(L, a, lenTo);
    return segmentRatio<false>(L, a, pf, dotA(from, direction), lenFrom, pt, dotA(to, direction), lenTo, lengthA(direction));
}
template <bool LEAN = false> SZG_DEV V3 sampleT_Segment(const TLut& L, const Atm& a, V3 from, V3 to)
{
    if (LEAN)
    {
        V3 const segment = to - from;
        V3 const direction = segment * divN0(1.0f, sqrtP(dotA(segment, segment))); // normalizeA()
        float const lenFrom = sqrtP(dotA(from, from));
        float const lenTo = sqrtP(dotA(to, to));
        RadiusPart const pf = radiusPart<true>(L, a, lenFrom);
        RadiusPart const pt = radiusPart<true>(L, a, lenTo);
        return segmentRatio<true>(L, a, pf, dotA(from, direction), lenFrom, pt, dotA(to, direction), lenTo, sqrtP(dotA(direction, direction)));
    }
    V3 const direction = normalizeA(to - from);
    float const lenFrom = lengthA(from);
    float const lenTo = lengthA(to);
    RadiusPart const pf = radiusPart<false>(L, a, lenFrom);
    RadiusPart const pt = radiusPart<false>(L, a, lenTo);
    return segmentRatio<false>(L, a, pf, dotA(from, direction), lenFrom, pt, dotA(to, direction), lenTo, lengthA(direction));
}

} // namespace szg
