// kernels_composite.hip — the full-screen sky / aerial-perspective composite
// ("perspective map") for gfx950: atmosphere/camera.comp:70-395.
//
// Structure (results unchanged, see DESIGN.md "composite"):
//   phase A  classify the pixel (sky / geometry), evaluate everything that is
//            not a ray march, and record up to two march requests
//              slot 0: primary ray  (geometry aerial perspective, or a sky ray
//                      that hits the ground: sampleGround)
//              slot 1: metal reflection ray that hits the ground
//   phase B  run the 32-step scattering integral for the active slots through
//            ONE copy of the march code
//   phase C  combine in the order camera.comp adds the terms, tonemap, store.

#include "szg/fpmath.h"
#include "szg_atmosphere.hpp"
#include "szg_formats.hpp"
#include "szg_launch.hpp"
#include "szg_lean.hpp"
#include "szg_march.hpp"
#include "szg_pbr.hpp"
#include "szg_pixel.hpp"
#include "szg_vec.hpp"

// Outside the march, what depends on the camera, the atmosphere and the draw extent alone comes from FramePrep::Camera
// (k_frame_prep, once per frame), and the per-pixel quotients, square roots and pow() of phases A and C use the lean exact
// operators of szg_lean.hpp where a wave-uniform gate proves their operand domain (profiles/composite_pixel_path.md).

namespace szg
{
namespace
{
struct SkyLut
{
    const float4* texels;
    int width, height;
    bool finite; // status dword behind the texels (szg_launch.hpp "sky-view LUT block"): every texel a finite, moderate number
};

// sampleMap_Direction, camera.comp:70-121 (sky-view LUT: LINEAR, CLAMP_TO_EDGE,
// no half-texel squeeze: SURVEY Q14)
SZG_DEV V3 sampleMapDirection(const SkyLut& S, const Atm& a, V3 position, V3 direction)
{
    float const PI = 3.141592653589793f;
    V3 const normalized = normalize(direction);
    float const sinHorizonZenith = a.planetRadius / length(position);
    float const horizonZenith = PI - szg_asinf(sinHorizonZenith);
    float const cosViewZenith = normalized.y;
    float const cosHorizonZenith = -safeSqrt(1.0f - sinHorizonZenith * sinHorizonZenith);
    float const viewZenith = szg_acosf(normalized.y);
    float v;
    if (cosViewZenith > cosHorizonZenith)
    {
        float const angleFraction = viewZenith / horizonZenith;
        v = (1.0f - sqrtf(1.0f - angleFraction)) * 0.5f;
    }
    else
    {
        float const angleFraction = (viewZenith - horizonZenith) / (PI - horizonZenith);
        v = sqrtf(angleFraction) * 0.5f + 0.5f;
    }
    V2 const projectedLight = normalize(V2{-a.incidentDirectionSun.x, -a.incidentDirectionSun.z});
    V2 const projectedView = normalize(V2{direction.x, direction.z});
    float const u = clampf(dot(projectedLight, projectedView), -1.0f, 1.0f) * 0.5f + 0.5f;
    return bilinear_rgb(S.texels, S.width, S.height, (float)S.width, (float)S.height, u, v);
}

// ... for a ray that starts at the camera: the horizon terms and the projected sun direction are FramePrep::Camera's (the same
// expressions on the camera's position and the atmosphere, formed once per frame)
SZG_DEV V3 sampleMapDirection(const SkyLut& S, const FramePrep::Camera& c, V3 direction)
{
    V3 const normalized = normalize(direction);
    float const cosViewZenith = normalized.y;
    float const viewZenith = szg_acosf(normalized.y);
    float v;
    if (cosViewZenith > c.cosHorizonZenith)
    {
        float const angleFraction = viewZenith / c.horizonZenith;
        v = (1.0f - sqrtf(1.0f - angleFraction)) * 0.5f;
    }
    else
    {
        float const angleFraction = (viewZenith - c.horizonZenith) / c.piMinusHorizon;
        v = sqrtf(angleFraction) * 0.5f + 0.5f;
    }
    V2 const projectedView = normalize(V2{direction.x, direction.z});
    float const u = clampf(dot(c.projectedLight, projectedView), -1.0f, 1.0f) * 0.5f + 0.5f;
    return bilinear_rgb(S.texels, S.width, S.height, (float)S.width, (float)S.height, u, v);
}

// sampleSunDisk, camera.comp:123-140; `sunLength` is length(directionToSun) (FramePrep::Camera::sunLength) where the caller has it
SZG_DEV V3 sampleSunDisk(const TLut& L, const Atm& a, V3 position, V3 direction, float sunLength)
{
    V3 const directionToSun = -a.incidentDirectionSun;
    float const cosDirectionSun = dot(direction, directionToSun) / (length(direction) * sunLength);
    float const sinSunRadius = a.sunAngularRadius;
    float const sinDirectionSun = safeSqrt(1.0f - cosDirectionSun * cosDirectionSun);
    if (cosDirectionSun < 0.0f)
    {
        return splat(0.0f);
    }
    V3 const transmittanceToSun = sampleT_Ray(L, a, position, direction);
    return transmittanceToSun * (1.0f - smoothstep(0.2f * sinSunRadius, sinSunRadius, sinDirectionSun));
}
SZG_DEV V3 sampleSunDisk(const TLut& L, const Atm& a, V3 position, V3 direction)
{
    return sampleSunDisk(L, a, position, direction, length(-a.incidentDirectionSun));
}

// raycastDistanceToGround, camera.comp:175-192
SZG_DEV bool raycastGround(const Atm& a, V3 origin, V3 direction, float& distance)
{
    float t0 = 0.0f, t1 = 0.0f;
    bool const hit = raySphere(origin, direction, a.planetRadius, t0, t1) && t0 > 0.0f;
    distance = t0;
    return hit;
}

// The part of sampleGround (camera.comp:203-235) that is not the march:
// surfaceLuminance * transmittanceToSurface.
SZG_DEV V3 groundSurfaceTerm(const TLut& L, const Atm& a, V3 origin, V3 direction, float distanceToGround)
{
    float const PI = 3.141592653589793f;
    V3 const surfacePosition = origin + distanceToGround * direction;
    V3 const surfaceNormal = normalize(surfacePosition);
    V3 const lightDirection = -a.incidentDirectionSun;
    V3 const viewDirection = -direction;
    V3 const h = normalize(lightDirection + viewDirection);
    float const specularPower = 160.0f;
    float const microfacet = szg_powf(clampf(dot(h, surfaceNormal), 0.0f, 1.0f), specularPower);
    float const normalization = (specularPower + 2.0f) / 8.0f;
    V3 const specular = splat(normalization * microfacet);
    V3 const diffuse = splat(0.4f) / PI;
    V3 const fresnel =
        splat(0.04f) + (splat(1.0f) - splat(0.04f)) * szg_powf(1.0f - clampf(dot(h, lightDirection), 0.0f, 1.0f), 5.0f);
    V3 const albedo = mix(diffuse, specular, fresnel);
    V3 const transmittanceToSun = sampleT_Ray(L, a, surfacePosition, lightDirection);
    V3 const surfaceLuminance = (transmittanceToSun * albedo) * clampf(dot(surfaceNormal, lightDirection), 0.0f, 1.0f);
    V3 const transmittanceToSurface = sampleT_Segment(L, a, origin, surfacePosition);
    return surfaceLuminance * transmittanceToSurface;
}
} // namespace

#ifdef SZG_TAIL_DIAG
// Diagnostic build only (tools/tail_histogram.py; never part of libszg_hip.so): every wave of k_composite stamps the constant-
// frequency clock (s_memrealtime, 100 MHz) when it starts and when it ends into a buffer the tool hands over, together
// with the hardware id of where it ran, so that the launch tail can be read off a histogram (profiles/r03_tail_*.txt).
__device__ unsigned long long* g_tailStamps = nullptr; // [workgroup * 4 + wave] * 3: start, end, HW_ID
extern "C" int szg_debug_tail_buffer(void* d_buffer)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_tailStamps), &d_buffer, sizeof d_buffer);
}
struct TailStamp
{
    unsigned long long start;
    unsigned slot;
    SZG_DEV TailStamp(unsigned slot_) : start(wall_clock64()), slot(slot_) {}
    SZG_DEV ~TailStamp()
    {
        if (g_tailStamps != nullptr && (threadIdx.x & 63u) == 0u)
        {
            unsigned hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            g_tailStamps[(size_t)slot * 3u + 0u] = start;
            g_tailStamps[(size_t)slot * 3u + 1u] = wall_clock64();
            g_tailStamps[(size_t)slot * 3u + 2u] = hw;
        }
    }
};
#endif

// Trilinear fetch of the aerial-perspective luminance volume at screen position (sx, sy) in [0, 1] and distance
// `dist` (Mm): clamp-to-edge in x, y; slices at d_k = (k + .5) / D * maxDistance, linear ramp to 0 below d_0.
SZG_DEV V3 sampleAerial(const AerialLut& A, float sx, float sy, float dist)
{
    const float4* vol = reinterpret_cast<const float4*>(A.luminance);
    float const fz = dist / A.maxDistance * (float)A.D - 0.5f;
    float const ramp = fz < 0.0f ? fmaxf(dist / (0.5f * A.maxDistance / (float)A.D), 0.0f) : 1.0f;
    float const z = fminf(fmaxf(fz, 0.0f), (float)A.D - 1.0f);
    int const k0 = (int)floorf(z);
    int const k1 = min(k0 + 1, (int)A.D - 1);
    float const wz = z - (float)k0;
    V3 const l0 = bilinear_rgb(vol + (size_t)k0 * A.W * A.H, (int)A.W, (int)A.H, (float)A.W, (float)A.H, sx, sy);
    V3 const l1 = bilinear_rgb(vol + (size_t)k1 * A.W * A.H, (int)A.W, (int)A.H, (float)A.W, (float)A.H, sx, sy);
    return (l0 * (1.0f - wz) + l1 * wz) * ramp;
}

// waves per SIMD the register budget is held to (tests/test_march_kernel_resources.py pins the occupancy)
constexpr unsigned COMPOSITE_WAVES = 4u;
template <bool FAST>
__global__ __launch_bounds__(256, COMPOSITE_WAVES) void k_composite(szg_image color, szg_image depth, szg_image debug, GBufferPtrs g,
                                                   unsigned drawW, unsigned drawH, unsigned localRows, RowMap rm,
                                                   ShadowSlot sunSlot, const szg_atmosphere_packed* __restrict__ atmospheres,
                                                   unsigned atmosphereIndex, const szg_camera_packed* __restrict__ cameras,
                                                   unsigned cameraIndex,
                                                   const szg_directional_light_packed* __restrict__ dirLights,
                                                   unsigned sunLightIndex, const float4* __restrict__ tlut, int tW, int tH,
                                                   const float4* __restrict__ slut, int sW, int sH, AerialLut aerial,
                                                   const FramePrep* __restrict__ prep)
{
    unsigned const tid = threadIdx.x;
    unsigned const wave = tid >> 6; // (the pixel's column and the diagnostic build's stamp share it)
#ifdef SZG_TAIL_DIAG
    TailStamp const stamp((blockIdx.y * gridDim.x + blockIdx.x) * 4u + wave);
#endif
    // (bottom-up: the sky's workgroups, which march nothing, tend to come last and fill the tail of the launch)
    unsigned const x = pixel_column(wave, tid & 63u), y = pixel_row_bottom_up(tid);
    if (x >= drawW || y >= localRows)
    {
        return;
    }
    unsigned const gy = global_row(rm, y);

    Atm const a = load_atm(*prep); // (k_frame_prep: load_atm(atmospheres + atmosphereIndex), once per frame instead of once per wave)
    TLut const L = make_tlut(tlut, tW, tH, *prep);
    SkyLut const S{slut, sW, sH, reinterpret_cast<const unsigned*>(slut + (size_t)sW * (size_t)sH)[0] == 0u};
    const szg_camera_packed* cam = cameras + cameraIndex;

    // camera.comp:315-316 (nearest at the pixel's own texel)
    float const sceneDepth = row_ptr<const float>(depth, y)[x];

    // camera.comp:320-322
    const FramePrep::Camera& fc = prep->camera; // (scalar loads; read in phase A only)
    V3 const position = fc.position;

    // camera.comp:324-328 (no pixel-centre offset: SURVEY Q5; global row)
    // x and the row are 0 or an integer in [1, 2^32), the extents integers in [1, 2^32): inside the domain of divR0 whatever
    // the frame (no gate), and a zero quotient is +0 as IEEE gives it
    float const screenx = divR0((float)x, (float)drawW, fc.rcpDrawW), screeny = divR0((float)gy, (float)drawH, fc.rcpDrawH);
    float const clipx = (screenx - 0.5f) * 2.0f;
    float const clipy = (screeny - 0.5f) * 2.0f;
    M4 const inverseProjection = load_m4(cam->inverseProjection);
    M4 const rotation = load_m4(cam->rotation);
    V4 const dvs = mul(inverseProjection, clipx, clipy, 1.0f, 1.0f);
    V4 const rot = mul(rotation, dvs.x, dvs.y, dvs.z, dvs.w);
    // normalize() as v * (1 / sqrt(dot)) with the lean operators when every lane's squared length is a moderate number
    V3 const unrotated = mk3(rot.x, rot.y, rot.z);
    float const unrotated2 = dot(unrotated, unrotated);
    bool const viewLean = waveAll(leanLength2(unrotated2));
    V3 direction = viewLean ? unrotated * divN0(1.0f, sqrtP(unrotated2)) : normalize(unrotated);
    direction.y *= -1.0f;

    // ---- phase A ---------------------------------------------------------
    bool isSky = (sceneDepth == 0.0f);
    Material m;
    if (!isSky)
    {
        // camera.comp:346-347; a pixel with depth 0 is sky whatever the G-buffer holds (:354)
        V4 const diffuse = unpack_half4(row_ptr<const uint2>(g.diffuse, y)[x]);
        V4 const specular = unpack_half4(row_ptr<const uint2>(g.specular, y)[x]);
        V4 const normal = unpack_half4(row_ptr<const uint2>(g.normal, y)[x]);
        V4 const orm = unpack_half4(row_ptr<const uint2>(g.orm, y)[x]);
        float4 const p4 = row_ptr<const float4>(g.position, y)[x];
        // (the quotients by max(specular) and by pi and pow(160, .) with the lean operators when no lane of the wave has a black,
        // non-finite or negative-max specular, a non-finite diffuse, or a roughness of 1 or beyond fp32's moderate range)
        bool const materialLean = waveAll(convertPBRLeanOK(diffuse, specular, orm));
        m = materialLean ? convertPBR<true>(V4{p4.x, p4.y, p4.z, p4.w}, normal, diffuse, specular, orm)
                         : convertPBR<false>(V4{p4.x, p4.y, p4.z, p4.w}, normal, diffuse, specular, orm);
        isSky = m.position.y > 0.0f; // underground, +y down (:354)
    }

    V3 surfaceLuminance = splat(0.0f);
    V3 base = splat(0.0f);   // non-march part of the primary term
    V3 coef = splat(0.0f);   // transmittanceToSurface * metallic * fresnel of the reflection
    V3 env2 = splat(0.0f);   // non-march part of the reflection's environment sample
    bool hasReflection = false;
    bool march0 = false, march1 = false;
    V3 o0 = position, d0 = direction, o1 = position, d1 = direction;
    float l0 = 0.0f, l1 = 0.0f;

    if (isSky)
    {
        // sampleEnvironmentLuminanceTransfer(position, direction, 1.0), camera.comp:286-301
        float dtg;
        if (raycastGround(a, position, direction, dtg))
        {
            base = groundSurfaceTerm(L, a, position, direction, dtg);
            march0 = true;
            l0 = dtg;
        }
        else
        {
            base = sampleMapDirection(S, fc, direction) + sampleSunDisk(L, a, position, direction, fc.sunLength) * 1.0f;
        }
    }
    else
    {
        // camera.comp:364
        uint2 const prior = row_ptr<const uint2>(color, y)[x];
        // (numerators 0 or an integer in [1, 65535]: inside the domain of divR0 for every texel, no gate)
        float const rcp65535 = rcpN(65535.0f);
        surfaceLuminance = mk3(divR0((float)(prior.x & 0xFFFFu), 65535.0f, rcp65535), divR0((float)(prior.x >> 16), 65535.0f, rcp65535),
                               divR0((float)(prior.y & 0xFFFFu), 65535.0f, rcp65535));

        // camera.comp:366-369: shadow frame from the engine-space position/normal
        float shadowFactor = 1.0f;
        if (sunSlot.map != nullptr)
        {
            // TO_TEX * (sun.projection * sun.view): once per frame by k_frame_prep (FramePrep::sunShadow), wave-uniform here
            M4 sm;
#pragma unroll
            for (int k = 0; k < 16; k++)
            {
                sm.m[k] = prep->sunShadow[k];
            }
            V4 c = mul(sm, m.position.x, m.position.y, m.position.z, 1.0f);
            float const w = c.w;
            V3 const coord = mk3(c.x / w, c.y / w, c.z / w);
            V4 const pn = mul(sm, m.normal.x, m.normal.y, m.normal.z, 0.0f);
            float const fdx = sqrtf(1.0f - clampf(pn.x * pn.x, 0.0f, 1.0f));
            float const fdy = sqrtf(1.0f - clampf(pn.y * pn.y, 0.0f, 1.0f));
            shadowFactor = sampleShadowMap(sunSlot.map, sunSlot.width, sunSlot.height, sunSlot.pitchFloats, coord, fdx, fdy);
        }

        // camera.comp:371-374
        m.normal.y *= -1.0f;
        m.position.y *= -1.0f;
        // (the quotient by 10^6 stays generic: a lean form's gate would have no observable side - a coordinate beyond 2^60 or below
        // 2^-60 gives the same pixel either way - and a gate no test can see is not kept, profiles/composite_pixel_path.md)
        m.position = m.position / 1000000.0f;
        m.position.y += a.planetRadius;

        // computeGeometryLuminanceTransfer, camera.comp:237-278
        V3 const surfacePosition = m.position;
        // the two transmittance samples of this branch with the lean exact operators when the whole wave allows it
        V3 const toSurface = surfacePosition - position;
        float const cameraR2 = fc.r2; // dot(position, position)
        bool const samplesLean = waveAll(a.lean && leanRadius2(a, cameraR2) && leanRadius2(a, dot(surfacePosition, surfacePosition)) &&
                                         leanLength2(dot(toSurface, toSurface)) &&
                                         leanLength2(dot(a.incidentDirectionSun, a.incidentDirectionSun)));
        RadiusPart const cameraPart = cameraRadiusPart(fc);
        V3 const transmittanceToSurface = samplesLean ? sampleT_Segment<true>(L, a, position, cameraPart, fc.lenFrom, surfacePosition)
                                                      : sampleT_Segment<false>(L, a, position, cameraPart, fc.lenFrom, surfacePosition);
        // (normalize(), length() and the quotients below likewise: v * (1 / sqrt(dot)) and sqrt(dot) with the lean operators)
        V3 const minusDirection = -direction;
        float const direction2 = dot(minusDirection, minusDirection);
        bool const vectorsLean = samplesLean && waveAll(leanLength2(direction2));
        V3 const lightDirection = fc.lightDirection; // normalize(-a.incidentDirectionSun)
        V3 const viewDirection = vectorsLean ? minusDirection * divN0(1.0f, sqrtP(direction2)) : normalize(minusDirection);
        float pt0 = 0.0f, pt1 = 0.0f;
        bool const shadowedByPlanet = raySphere(surfacePosition, lightDirection, a.planetRadius, pt0, pt1) && pt0 > 0.0f;
        V3 const halfSum = lightDirection + viewDirection;
        bool const brdfLean = vectorsLean && waveAll(inRange(dot(halfSum, halfSum), 0x1p-40f, 8.0f));
        V3 const brdf = brdfLean ? brdfMix<true, true>(m, lightDirection, viewDirection)
                                 : brdfMix<false>(m, lightDirection, viewDirection);
        V3 const transmittanceToSun = samplesLean ? sampleT_Ray<true>(L, a, surfacePosition, lightDirection)
                                                  : sampleT_Ray<false>(L, a, surfacePosition, lightDirection);
        float const fractionOfSunVisible = vectorsLean ? divN0(a.planetRadius, sqrtP(dot(m.position, m.position)))
                                                       : a.planetRadius / length(m.position); // camera.comp:144-147
        float const scalar = (shadowFactor * fractionOfSunVisible) * (shadowedByPlanet ? 0.0f : 1.0f);
        base = ((((scalar * transmittanceToSun) * transmittanceToSurface) * m.occlusion) * brdf) *
               clampf(dot(m.normal, lightDirection), 0.0f, 1.0f);
        l0 = vectorsLean ? sqrtP(dot(toSurface, toSurface)) : length(surfacePosition - position);
        if (FAST)
        {
            // APPROXIMATE extension (abi.h): aerial perspective from the froxel LUT instead of the inline march
            base = base + sampleAerial(aerial, screenx, screeny, l0);
        }
        else
        {
            march0 = true;
        }

        // camera.comp:379-386: single-bounce reflection. With metallic == 0 the term is 0 * fresnel * environment: an
        // exact zero that may be skipped — unless the environment could be NaN or inf (0 * NaN = NaN poisons the pixel in
        // the reference). It cannot when the extinction is bounded away from 0 along every ray of the shell
        // (Atm::extModerate), the transmittance LUT is moderate, and both the camera (whose sky-view LUT is sampled)
        // and the surface (origin of the reflection ray) lie inside the shell, and the reflection direction itself is finite
        // (it is built from the G-buffer normal; found by tests/sweeps/random_sweep_mesh_frames.py: a NaN normal from a degenerate
        // triangle leaves the sun term at 0 through the clamps but makes the environment sample NaN); otherwise the term
        // is evaluated.
        float const surfaceR2 = dot(surfacePosition, surfacePosition);
        float const nBig = 0x1p60f;
        bool const normalFinite = fabsf(m.normal.x) <= nBig && fabsf(m.normal.y) <= nBig && fabsf(m.normal.z) <= nBig;
        // Both horizon angles asin(Rp / r) must exist: the camera's (every texel of the sky-view LUT depends on it) and the
        // surface's (where the LUT is sampled from); same expressions as skyview_LUT.comp:106-112 and camera.comp:75-77.
        float const cameraSinHorizon = fc.sinHorizon; // a.planetRadius / length(position)
        bool const aboveGround = cameraSinHorizon <= 1.0f && fractionOfSunVisible <= 1.0f;
        bool const environmentFinite = a.extModerate && a.sunSane && L.moderate && S.finite && normalFinite && aboveGround &&
                                       inRange(cameraR2, a.extFloor2, a.extCeil2) && inRange(surfaceR2, a.extFloor2, a.extCeil2);
        if (m.metallic != 0.0f || !environmentFinite)
        {
            hasReflection = true;
            V3 const negDir = -direction;
            V3 const parallel = dot(m.normal, negDir) * m.normal;
            V3 const reflectionDirection = 2.0f * parallel - negDir;
            coef = (transmittanceToSurface * m.metallic) * computeFresnel(m, negDir, reflectionDirection);
            float dtg2;
            if (raycastGround(a, m.position, reflectionDirection, dtg2))
            {
                env2 = groundSurfaceTerm(L, a, m.position, reflectionDirection, dtg2);
                march1 = true;
                o1 = m.position;
                d1 = reflectionDirection;
                l1 = dtg2;
            }
            else
            {
                env2 = sampleMapDirection(S, a, m.position, reflectionDirection) +
                       sampleSunDisk(L, a, m.position, reflectionDirection) * shadowFactor;
            }
        }
    }

    // ---- phase B ---------------------------------------------------------
    // The march needs ~125 VGPRs by itself. Everything per-pixel that phase C wants back (12 floats), the two march
    // requests (origin, direction, length), their results and the three flags wait in LDS meanwhile - a queue of two slots
    // per thread - so that nothing of phases A and C is live across the march (LDS is otherwise unused here; every thread
    // touches only its own [k][tid] slots: conflict-free, no barrier, and the early return above stays legal).
    __shared__ float s_park[12][256];
    __shared__ float s_request[2][7][256];
    __shared__ float s_result[2][3][256];
    __shared__ unsigned s_flags[256];
    {
        float const park[12] = {base.x, base.y, base.z, coef.x, coef.y, coef.z, env2.x, env2.y, env2.z,
                                surfaceLuminance.x, surfaceLuminance.y, surfaceLuminance.z};
#pragma unroll
        for (int k = 0; k < 12; k++)
        {
            s_park[k][tid] = park[k];
        }
        float const request[2][7] = {{o0.x, o0.y, o0.z, d0.x, d0.y, d0.z, l0}, {o1.x, o1.y, o1.z, d1.x, d1.y, d1.z, l1}};
#pragma unroll
        for (int k = 0; k < 2; k++)
        {
#pragma unroll
            for (int c = 0; c < 7; c++)
            {
                s_request[k][c][tid] = request[k][c];
            }
        }
        s_flags[tid] = (march0 ? 1u : 0u) | (march1 ? 2u : 0u) | (hasReflection ? 4u : 0u);
    }
    // (the compiler must not forward the stores above to the loads below: the values would stay in registers)
    asm volatile("" ::: "memory");
    // The frame's constants move from the scalar block to vector registers again (load_atm: ~45 moves per wave), so that
    // phase A's copies die with phase A instead of being spilled around the march.
#pragma unroll 1
    for (unsigned k = 0; k < 2u; k++)
    {
        // ... and once per slot, behind a fence that keeps the loads from being hoisted out of the loop: constants that only
        // the per-ray set-up reads would otherwise stay live across slot 0's march for slot 1's set-up, in scratch. The loads
        // are scalar and do not depend on which slots the wave runs.
        asm volatile("" ::: "memory");
        Atm const aB = load_atm(*prep);
        TLut const LB = make_tlut(tlut, tW, tH, *prep);
        if (((s_flags[tid] >> k) & 1u) != 0u)
        {
            V3 const o = mk3(s_request[k][0][tid], s_request[k][1][tid], s_request[k][2][tid]);
            V3 const d = mk3(s_request[k][3][tid], s_request[k][4][tid], s_request[k][5][tid]);
            V3 const r = scatteringIntegral(LB, aB, o, d, s_request[k][6][tid]);
            s_result[k][0][tid] = r.x;
            s_result[k][1][tid] = r.y;
            s_result[k][2][tid] = r.z;
        }
    }
    asm volatile("" ::: "memory");

    // Phase C addresses its pixel and its LDS slots from the thread index again, through a copy the compiler cannot see
    // through: x, y and the slot addresses of phase A would otherwise wait for it in scratch across the march.
    unsigned tidC = tid;
    asm volatile("" : "+v"(tidC));
    unsigned const xC = pixel_column(tidC), yC = pixel_row_bottom_up(tidC);
    unsigned const flags = s_flags[tidC];
    march0 = (flags & 1u) != 0u;
    march1 = (flags & 2u) != 0u;
    hasReflection = (flags & 4u) != 0u;
    V3 const ap0 = march0 ? mk3(s_result[0][0][tidC], s_result[0][1][tidC], s_result[0][2][tidC]) : splat(0.0f);
    V3 const ap1 = march1 ? mk3(s_result[1][0][tidC], s_result[1][1][tidC], s_result[1][2][tidC]) : splat(0.0f);
    base = mk3(s_park[0][tidC], s_park[1][tidC], s_park[2][tidC]);
    coef = mk3(s_park[3][tidC], s_park[4][tidC], s_park[5][tidC]);
    env2 = mk3(s_park[6][tidC], s_park[7][tidC], s_park[8][tidC]);
    surfaceLuminance = mk3(s_park[9][tidC], s_park[10][tidC], s_park[11][tidC]);
    // ---- phase C ---------------------------------------------------------
    // sky:      transfer = env(position, direction)
    // geometry: transfer = (surfaceTransfer + AP) + coef * env(reflection)
    V3 transfer = march0 ? (base + ap0) : base;
    if (hasReflection)
    {
        V3 const e2 = march1 ? (env2 + ap1) : env2;
        transfer = transfer + coef * e2;
    }
    // (read again from the frame block, scalar loads, instead of holding three registers across the march)
    V3 const luminance = transfer * mk3(prep->a.sunIntensitySpectrum.x, prep->a.sunIntensitySpectrum.y, prep->a.sunIntensitySpectrum.z);
    V3 const pre = luminance * 10.0f + surfaceLuminance;
    // (pow() without its special cases when every lane's three values are positive normal numbers: a black, denormal, negative or
    // NaN component sends its wave down the generic form)
    bool const tonemapLean = waveAll(powLeanOK(pre.x, 1.2f) && powLeanOK(pre.y, 1.2f) && powLeanOK(pre.z, 1.2f));
    V3 const out = tonemapLean ? mk3(powLean(pre.x, 1.2f), powLean(pre.y, 1.2f), powLean(pre.z, 1.2f))
                               : mk3(szg_powf(pre.x, 1.2f), szg_powf(pre.y, 1.2f), szg_powf(pre.z, 1.2f));
    row_ptr<uint2>(color, yC)[xC] = pack_unorm16x4(out.x, out.y, out.z, 1.0f);
    if (debug.data != nullptr)
    {
        row_ptr<float4>(debug, yC)[xC] = make_float4(out.x, out.y, out.z, 1.0f);
    }
}

hipError_t launch_composite(hipStream_t s, const szg_scene_texture& scene, unsigned drawW, unsigned drawH, TileArgs tile,
                            const szg_gbuffer& g, ShadowSlot sunSlot, const szg_atmosphere_packed* d_atm, unsigned atmIndex, const szg_camera_packed* d_cam,
                            unsigned camIndex, const szg_directional_light_packed* d_dir, unsigned sunIndex, const float* tlut,
                            unsigned tW, unsigned tH, const float* slut, unsigned sW, unsigned sH, AerialLut aerial, const void* d_prep)
{
    unsigned const rows = tile.local_rows;
    if (rows == 0u || drawW == 0u)
    {
        return hipSuccess;
    }
    dim3 const grid = pixel_grid(drawW, rows);
    RowMap const rm{tile.block_rows, tile.rank, tile.nranks};
    GBufferPtrs const gp = gptrs(g);
    if (aerial.luminance != nullptr)
    {
        hipLaunchKernelGGL(k_composite<true>, grid, dim3(256), 0, s, scene.color, scene.depth, scene.debug_color, gp, drawW, drawH,
                           rows, rm, sunSlot, d_atm, atmIndex, d_cam, camIndex, d_dir, sunIndex,
                           reinterpret_cast<const float4*>(tlut), (int)tW, (int)tH, reinterpret_cast<const float4*>(slut),
                           (int)sW, (int)sH, aerial, static_cast<const FramePrep*>(d_prep));
    }
    else
    {
        hipLaunchKernelGGL(k_composite<false>, grid, dim3(256), 0, s, scene.color, scene.depth, scene.debug_color, gp, drawW, drawH,
                           rows, rm, sunSlot, d_atm, atmIndex, d_cam, camIndex, d_dir, sunIndex,
                           reinterpret_cast<const float4*>(tlut), (int)tW, (int)tH, reinterpret_cast<const float4*>(slut),
                           (int)sW, (int)sH, aerial, static_cast<const FramePrep*>(d_prep));
    }
    return hipGetLastError();
}
} // namespace szg
