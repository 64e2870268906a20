// szg_march.hpp — the phase functions and the 32-step scattering integral shared by the composite and the LUT kernels
// (atmosphere/common.glinl).
#pragma once

#include "szg/fpmath.h"
#include "szg_atmosphere.hpp"
#include "szg_lean.hpp"
#include "szg_vec.hpp"

namespace szg
{
// common.glinl:263-279
SZG_DEV float phaseRayleigh(float cosine)
{
    float const scalar = 3.0f / (16.0f * 3.141592653589793f);
    return scalar * (1.0f + cosine * cosine);
}
SZG_DEV float phaseMie(float cosine, float g)
{
    float const scalar = 3.0f / (8.0f * 3.141592653589793f);
    float const numerator = (1.0f - g * g) * (1.0f + cosine * cosine);
    float const denominator = (2.0f + g * g) * szg_powf(1.0f + g * g - 2.0f * g * cosine, 1.5f);
    return scalar * numerator / denominator;
}

// common.glinl:364-424 computeLuminanceScatteringIntegral, 32 steps.
// Hoisted (values identical in every iteration of the GLSL loop):
//   phase functions (line 408-410), sun-disc sin/cos (147-148), the origin-side
//   LUT tap and mu_sunAndStepDirection of sampleTransmittanceLUT_RayMarchStep /
//   stepRadiusMu (325, 349/357). stepRadiusMu(originStep, t) is evaluated once
//   per step and used for both sampleStep (389) and `end` (343).
struct MarchSetup
{
    V3 origin, scatteringDir;
    float dS, pR, pM, sin_sunRadius, cos_sunRadius;
    float mu_sunAndStep, r_mu, two_r_mu, r2, r_musun;
    bool up;
    bool extLean; // wave-uniform: the extinction along this wave's rays is of moderate magnitude (Atm::extModerate)
    // wave-uniform: at EVERY sample of this wave's rays the sun disc lies entirely above the local horizon, decided once per
    // ray from bounds (scatteringIntegral); the horizon smoothstep of sampleTransmittanceLUT_Sun is then exactly 1 at every
    // step and its operands (sin / cos of the horizon angle, the two edges) need not be formed
    bool sunClear;
    // wave-uniform: every ray of the wave has a step dS >= 1e-7, so t = i * dS < 1e-7 (common.glinl:338) holds at step 0 and at
    // no other step: the per-step comparison and its select are not needed
    bool firstStepOnly;
    // wave-uniform: every radius of the wave's rays is below Rp + 9.9 km (sampleExtinction's ozone tent is 0 there)
    bool belowOzone;
    V3 T_origin;
};

// INNER: every radius of the march lies below Atm::innerCeil2 (wave-uniform, decided per ray in scatteringIntegral)
// MS: the multi-scattering mode of include/szg/multiscatter_sky.h (0 = off: `psi` is not read and the function is what it was
// before that header; 1 = the higher orders added to the result; 2 = the higher orders alone). `psi`: the SZG_MULTISCATTER_DIM^2
// RGBA32F texels of the multi-scattering LUT, in global memory or in LDS. The term reads values the three bodies form alike
// (s_musun, altitude, the two scattering coefficients, integral, T_begin), so it does not depend on the body either.
template <bool LEAN, bool INNER = false, int MS = 0>
SZG_DEV V3 marchLoop(const TLut& L, const Atm& a, const MarchSetup& m, const float4* psi = nullptr)
{
    V3 luminance = splat(0.0f);
    V3 ms = splat(0.0f);
    float const shell = a.atmosphereRadius - a.planetRadius;
    // `end` of step i and `begin` of step i+1 are the same expression (common.glinl:386-387),
    // so its length and radius part are carried from one iteration to the next.
    V3 begin = fnma(0.0f * m.dS, m.scatteringDir, m.origin);
    float lenBegin = sqrtPX<LEAN>(dotA(begin, begin));
    RadiusPart pBegin = radiusPart<LEAN, INNER>(L, a, lenBegin);
#pragma unroll 1
    for (unsigned i = 0; i < 32u; i++)
    {
        float const fi = (float)i;
        float const t = fi * m.dS;
        V3 const end = fnma((float)(i + 1u) * m.dS, m.scatteringDir, m.origin);
        float const lenEnd = sqrtPX<LEAN>(dotA(end, end));
        RadiusPart const pEnd = radiusPart<LEAN, INNER>(L, a, lenEnd);

        // stepRadiusMu(originStep, t), common.glinl:329-331
        // (on a lean path this is a squared radius above the lean floor: neither the clamp to 0 nor sqrtN's guard is needed)
        float const s_q = SZG_CON(SZG_C_STEP, m.two_r_mu, t, t * t) + m.r2;
        float const s_radius = LEAN ? sqrtP(s_q) : safeSqrt(s_q);
        float const yS = LEAN ? rcpN(s_radius) : 0.0f;
        float const s_mu = divRX<LEAN>(m.r_mu + t, s_radius, yS);
        float const s_musun = divRX<LEAN>(SZG_CON(SZG_C_STEP, t, m.mu_sunAndStep, m.r_musun), s_radius, yS);
        RadiusPart const pStep = radiusPart<LEAN, INNER>(L, a, s_radius);

        float const altitude = lenBegin - a.planetRadius;

        // sampleTransmittanceLUT_Sun, common.glinl:145-172
        V3 const T_atm = sampleT_at<LEAN, INNER>(L, a, pStep, s_musun);
        V3 T_sun;
        if (LEAN && m.sunClear)
        {
            // (the per-step test below would succeed at every step: MarchSetup::sunClear)
            T_sun = T_atm;
        }
        else
        {
            float const sin_hz = divRX<LEAN>(a.planetRadius, s_radius, yS);
            float const cos_hz = -safeSqrtX<LEAN>(1.0f - sin_hz * sin_hz);
            float const e0 = -sin_hz * m.sin_sunRadius;
            float const e1 = sin_hz * m.sin_sunRadius;
            float const ssNum = (s_musun - cos_hz * m.cos_sunRadius) - e0, ssDen = e1 - e0;
            if (LEAN && waveAll(ssNum >= ssDen && ssDen > 0.0f))
            {
                // the sun disc is entirely above the sample's horizon for the whole wave: num / den >= 1 clamps to 1,
                // smoothstep(1) = 1 * 1 * (3 - 2) = 1 and T_atm * 1 = T_atm, all exactly
                T_sun = T_atm;
            }
            else
            {
                float const ss = clampf(divX<LEAN>(ssNum, ssDen), 0.0f, 1.0f);
                float const angularFactor = ss * ss * (3.0f - 2.0f * ss);
                T_sun = T_atm * angularFactor;
            }
        }

        Extinction const ex = sampleExtinction<LEAN, INNER>(a, altitude, LEAN && m.belowOzone);

        // sampleTransmittanceLUT_RayMarchStep, common.glinl:336-361
        // (t < 1e-7 -> 1, common.glinl:338-341: true for the whole wave at step 0, where the tap and the quotients are skipped)
        V3 T_begin = splat(1.0f);
        if ((LEAN && m.firstStepOnly) ? (i != 0u) : !waveAll(t < 0.0000001f))
        {
            V3 const T_end = sampleT_at<LEAN, INNER>(L, a, pStep, xorSign(s_mu, m.up ? 0u : 0x80000000u));
            V3 ratio;
            if (LEAN && L.moderate)
            {
                ratio = clamp01(m.up ? V3{divN0(m.T_origin.x, T_end.x), divN0(m.T_origin.y, T_end.y), divN0(m.T_origin.z, T_end.z)}
                                     : V3{divN0(T_end.x, m.T_origin.x), divN0(T_end.y, m.T_origin.y), divN0(T_end.z, m.T_origin.z)});
            }
            else
            {
                ratio = clamp01(m.up ? (m.T_origin / T_end) : (T_end / m.T_origin));
            }
            // (only a wave with lanes on both sides of the threshold needs the per-lane select)
            T_begin = ((LEAN && m.firstStepOnly) || waveAll(!(t < 0.0000001f))) ? ratio : ((t < 0.0000001f) ? splat(1.0f) : ratio);
        }

        V3 const phaseTimesScattering = fma3(ex.scatteringMie, m.pM, ex.scatteringRayleigh * m.pR);

        // sampleTransmittanceLUT_Segment(begin, end), common.glinl:114-136. The segment can be arbitrarily short
        // (geometry close to the camera: end - begin may even be 0 and its normal NaN), so normalizeA() keeps the
        // generic operators unless the squared length is comfortably normal for the whole wave.
        V3 const segment = end - begin;
        float const segment2 = dotA(segment, segment);
        V3 segDir;
        if (LEAN && waveAll(inRange(segment2, 0x1p-90f, 0x1p60f)))
        {
            segDir = segment * divN0(1.0f, sqrtP(segment2)); // = segment * (1 / sqrt(dot)) of normalizeA()
        }
        else
        {
            segDir = normalizeA(segment);
        }
        V3 const T_path = segmentRatio<LEAN, INNER>(L, a, pBegin, dotA(begin, segDir), lenBegin, pEnd, dotA(end, segDir), lenEnd,
                                             sqrtPX<LEAN>(dotA(segDir, segDir)));
        // 1 - T_path is 0 or a multiple of 2^-24; the extinction is in [2^-40, 2^52] when m.extLean
        V3 const oneMinusT = splat(1.0f) - T_path;
        V3 const integral = (LEAN && m.extLean) ? V3{divN0(oneMinusT.x, ex.extinction.x), divN0(oneMinusT.y, ex.extinction.y),
                                                     divN0(oneMinusT.z, ex.extinction.z)}
                                                : oneMinusT / ex.extinction;
        luminance = fma3(phaseTimesScattering * T_sun * integral, T_begin, luminance);
        if (MS != 0)
        {
            // szg/multiscatter_sky.h "THE RULE": the sample's sun cosine with `begin`'s altitude, the pairing of the term above
            float const su = clampf(0.5f + 0.5f * s_musun, 0.0f, 1.0f);
            float const sv = clampf(altitude / shell, 0.0f, 1.0f);
            V3 const Psi = bilinear_rgb(psi, (int)SZG_MULTISCATTER_DIM, (int)SZG_MULTISCATTER_DIM, (float)SZG_MULTISCATTER_DIM,
                                        (float)SZG_MULTISCATTER_DIM, su, sv);
            ms = fma3(((ex.scatteringRayleigh + ex.scatteringMie) * Psi) * integral, T_begin, ms);
        }

        begin = end;
        lenBegin = lenEnd;
        pBegin = pEnd;
    }
    return MS == 0 ? luminance : (MS == 1 ? luminance + ms : ms);
}

template <int MS = 0>
SZG_DEV V3 scatteringIntegral(const TLut& L, const Atm& a, V3 origin, V3 direction, float sampleDistance, const float4* psi = nullptr)
{
    MarchSetup m;
    m.origin = origin;
    // The per-ray setup with the lean exact operators (same values) when the whole wave's origins lie above the lean floor
    // and the direction and sun vectors have ordinary lengths; otherwise hipcc's generic sqrtf / division.
    float const origin2 = dotA(origin, origin), direction2 = dotA(direction, direction);
    float const sun2 = a.sun2;
    bool const setupLean = waveAll(a.lean && leanRadius2(a, origin2) && leanLength2(direction2) && leanLength2(sun2));
    float radius, mu, mu_sun;
    V3 const toSun = -a.incidentDirectionSun;
    if (setupLean)
    {
        float const lenDirection = sqrtP(direction2);
        m.scatteringDir = -(direction * divN0(1.0f, lenDirection));
        radius = sqrtP(origin2);
        mu = divN0(dotA(origin, direction), radius * lenDirection);
        mu_sun = divN0(dotA(origin, toSun), radius * a.sunLengthLean);
    }
    else
    {
        m.scatteringDir = -normalizeA(direction);
        radius = lengthA(origin);
        mu = dotA(origin, direction) / (lengthA(origin) * lengthA(direction));
        mu_sun = dotA(origin, toSun) / (lengthA(origin) * a.sunLength);
    }

    float const incidentCosine = dotA(a.incidentDirectionSun, m.scatteringDir);
    m.pR = phaseRayleigh(incidentCosine);
    m.pM = phaseMie(incidentCosine, 0.8f);
    m.sin_sunRadius = a.sinSunRadius;
    m.cos_sunRadius = a.cosSunRadius;

    // stepRadiusMu invariants (common.glinl:325)
    m.mu_sunAndStep = safeSqrt(mu_sun * mu - safeSqrt((1.0f - mu_sun * mu_sun) * (1.0f - mu * mu)));
    m.r_mu = radius * mu;
    m.two_r_mu = 2.0f * radius * mu;
    m.r2 = radius * radius;
    m.r_musun = radius * mu_sun;
    m.up = mu > 0.0f;
    m.T_origin = setupLean ? sampleT_RadiusMu<true>(L, a, radius, m.up ? mu : -mu) : sampleT_RadiusMu<false>(L, a, radius, m.up ? mu : -mu);
    m.dS = sampleDistance / 32.0f;

    // leanRay: every radius met along the path stays >= 0.9 Rp and of moderate magnitude, the path length is
    // moderate, and the smoothstep span 2 * sin_hz * sin(sunRadius) is a normal number. The closest approach of
    // the segment [0, L] to the planet centre is at t* = -r*mu when that lies inside the segment.
    float const L2 = SZG_CON(SZG_C_STEP, m.two_r_mu, sampleDistance, sampleDistance * sampleDistance) + m.r2; // stepRadiusMu's form
    float const tStar = -m.r_mu;
    float const rmin2 = (tStar > 0.0f && tStar < sampleDistance) ? m.r2 * (1.0f - mu * mu) : fminf(m.r2, L2);
    // ... and the two cosines are cosines: a sun (or view) vector of length 0 or inf makes mu_sun (mu) infinite or NaN, and
    // the one-correction division returns NaN for an infinite numerator where the quotient is inf.
    bool const lean = a.lean && rmin2 >= a.leanFloor2 && inRange(radius, 0x1p-30f, 0x1p30f) && inRange(sampleDistance, 0.0f, 0x1p30f) &&
                      m.sin_sunRadius >= 0x1p-30f && leanLength2(sun2) && leanLength2(direction2) && fabsf(mu) <= 2.0f &&
                      fabsf(mu_sun) <= 2.0f;
    m.extLean = waveAll(a.extModerate && rmin2 >= a.extFloor2 && fmaxf(m.r2, L2) <= a.extCeil2);
    m.firstStepOnly = waveAll(lean && m.dS >= 0.0000001f); // then fl(i * dS) >= dS >= 1e-7 for every i >= 1
    {
        float const ozoneLow = a.planetRadius + 0.0099f; // Mm: below the 10 km foot of the tent (25 km - 15 km) with a margin
        m.belowOzone = waveAll(lean && fmaxf(m.r2, L2) <= ozoneLow * ozoneLow);
    }
    // sunClear. At step i the sun cosine handed to the smoothstep is s_musun = (r_musun + t * mu_sunAndStep) / s_radius with
    // t >= 0 and mu_sunAndStep >= 0 (a safeSqrt), so its numerator is >= r_musun, and s_radius is the radius of a point of
    // the segment: <= sqrt(max(r2, L2)) up to rounding. The test passes when s_musun >= cos_hz cos R + sin_hz sin R, and with
    // cos_hz <= 0 <= cos R the right-hand side is at most sin_hz sin R <= (Rp / lean floor) sin R <= 1.12 sin R. Hence
    // r_musun * 0.999 / r_max >= 1.25 sin R + 2^-10 implies ssNum >= ssDen > 0 at every step, with a margin (2^-10) a
    // thousand times the rounding errors of the per-step expressions (which are never formed then).
    {
        float const rMax = sqrtf(fmaxf(m.r2, L2));
        m.sunClear = waveAll(lean && m.cos_sunRadius >= 0.0f && m.sin_sunRadius > 0.0f && m.r_musun > 0.0f &&
                             m.r_musun * 0.999f >= (1.25f * m.sin_sunRadius + 0x1p-10f) * rMax);
    }
    // wave-uniform choice: one lane outside the domain sends its whole wave down the generic path
    if (waveAll(lean))
    {
        // the largest radius of the march is at one of its ends (|origin - t dir|^2 is convex in t); the cosines handed to
        // the taps are quotients bounded by Cauchy-Schwarz up to rounding (|mu| <= 1 + 2^-20 is all INNER asks for)
        if (waveAll(fmaxf(m.r2, L2) <= a.innerCeil2))
        {
            return marchLoop<true, true, MS>(L, a, m, psi);
        }
        return marchLoop<true, false, MS>(L, a, m, psi);
    }
    return marchLoop<false, false, MS>(L, a, m, psi);
}

} // namespace szg
