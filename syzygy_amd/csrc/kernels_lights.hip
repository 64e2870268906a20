// kernels_lights.hip — the deferred lights pass for gfx950.
//
//   k_light_prep   : per-light invariants of deferred/lights.comp:141-161
//   k_light_tiles  : per 64x64 screen tile, which lights k_lights has to visit
//   k_lights       : deferred/lights.comp:110-164, fused with the clear of the
//                    scene colour (deferred.cpp:715-717)

#include "szg/fpmath.h"
#include "szg_formats.hpp"
#include "szg_launch.hpp"
#include "szg_lean.hpp"
#include "szg_light_tiles.hpp"
#include "szg_pbr.hpp"
#include "szg_pixel.hpp"
#include "szg_vec.hpp"

namespace szg
{
// ---------------------------------------------------------------------------
// One thread per light. Slot numbering follows lights.comp:138-161: the shadow
// map index starts at directionalLightSkipCount and runs over the directional
// lights [skip, count) then the spot lights.
__global__ void k_light_prep(const szg_directional_light_packed* __restrict__ dirs, unsigned dirCount, unsigned dirSkip,
                             const szg_spot_light_packed* __restrict__ spots, unsigned spotCount,
                             const ShadowSlot* __restrict__ slots, unsigned slotCount, LightRec* __restrict__ out)
{
    unsigned const i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned const nDir = dirCount > dirSkip ? dirCount - dirSkip : 0u;
    if (i >= nDir + spotCount)
    {
        return;
    }
    // shadowmap.glinl:2-7
    M4 toTex;
    {
        float const t[16] = {0.5f, 0.0f, 0.0f, 0.0f, 0.0f, 0.5f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.5f, 0.5f, 0.0f, 1.0f};
#pragma unroll
        for (int k = 0; k < 16; k++)
        {
            toTex.m[k] = t[k];
        }
    }
    LightRec r;
    M4 projection, view;
    V3 forward, color;
    float strength;
    if (i < nDir)
    {
        const szg_directional_light_packed* l = dirs + dirSkip + i;
        projection = load_m4(l->projection);
        view = load_m4(l->view);
        forward = mk3(l->forward[0], l->forward[1], l->forward[2]);
        color = mk3(l->color[0], l->color[1], l->color[2]);
        strength = l->strength;
        r.isSpot = 0u;
        r.falloffFactor = 0.0f;
        r.falloffDistance = 1.0f;
        r.position[0] = r.position[1] = r.position[2] = 0.0f;
    }
    else
    {
        const szg_spot_light_packed* l = spots + (i - nDir);
        projection = load_m4(l->projection);
        view = load_m4(l->view);
        forward = mk3(l->forward[0], l->forward[1], l->forward[2]);
        color = mk3(l->color[0], l->color[1], l->color[2]);
        strength = l->strength;
        r.isSpot = 1u;
        r.falloffFactor = l->falloffFactor;
        r.falloffDistance = l->falloffDistance;
        r.position[0] = l->position[0];
        r.position[1] = l->position[1];
        r.position[2] = l->position[2];
    }
    // computeShadowFrame(light.projection * light.view, ...): TO_TEX * (projection * view)
    M4 const shadowMatrix = mul(toTex, mul(projection, view));
#pragma unroll
    for (int row = 0; row < 4; row++)
    {
#pragma unroll
        for (int col = 0; col < 4; col++)
        {
            r.shadowRows[row * 4 + col] = shadowMatrix.m[col * 4 + row];
        }
    }
    V3 const dirUnit = normalizeL(-forward);
    r.dir[0] = dirUnit.x;
    r.dir[1] = dirUnit.y;
    r.dir[2] = dirUnit.z;
    V3 const cs = color * strength;
    r.colorStrength[0] = cs.x;
    r.colorStrength[1] = cs.y;
    r.colorStrength[2] = cs.z;
    unsigned const slot = dirSkip + i;
    if (slot < slotCount && slots[slot].map != nullptr)
    {
        r.map = slots[slot].map;
        r.mapWidth = slots[slot].width;
        r.mapHeight = slots[slot].height;
        r.mapPitchFloats = slots[slot].pitchFloats;
    }
    else
    {
        r.map = nullptr;
        r.mapWidth = r.mapHeight = r.mapPitchFloats = 0u;
    }
    {
        float const lo = 0x1p-30f, hi = 0x1p30f;
        // colour * strength is the numerator of lean divisions (an infinite one would come out NaN instead of inf) and a
        // factor of the culled term: a spot light's term for a pixel outside its cone is (colour * strength / falloff) * 0 *
        // brdf, an exact zero only if every factor is finite. The light's own factors are checked here, the pixel's in k_lights.
        auto numerator = [&](float a) { return a == 0.0f || (fabsf(a) >= lo && fabsf(a) <= hi); };
        // rows of the shadow matrix: with |position| <= 2^30 (checked per pixel) entries up to 2^28 keep every projected
        // coordinate — the numerators of the lean divisions by w — below 2^60
        bool rowsModerate = true;
        for (int k = 0; k < 16; k++)
        {
            rowsModerate = rowsModerate && fabsf(r.shadowRows[k]) <= 0x1p28f;
        }
        bool const finite = numerator(r.colorStrength[0]) && numerator(r.colorStrength[1]) && numerator(r.colorStrength[2]) &&
                            fabsf(r.position[0]) <= hi && fabsf(r.position[1]) <= hi && fabsf(r.position[2]) <= hi &&
                            fabsf(r.dir[0]) <= 2.0f && fabsf(r.dir[1]) <= 2.0f && fabsf(r.dir[2]) <= 2.0f;
        r.leanOK = (r.isSpot != 0u && finite && rowsModerate && inRange(r.falloffDistance, lo, hi) && inRange(r.falloffFactor, lo, hi)) ? 1u : 0u;
    }
    r.rcpFalloffDistance = r.leanOK != 0u ? rcpN(r.falloffDistance) : 0.0f;
    r.falloffBound = r.falloffFactor * r.rcpFalloffDistance * r.rcpFalloffDistance;
    // The falloff of a lean pair is falloffBound * d^2 up to rounding, with d^2 in [2^-30, 2^30] (tested per pair): it is the
    // denominator of colour * strength / falloff, so it has to stay inside the domain of the exact reciprocal, [2^-60, 2^60]
    // (round 3: factor and distance were only bounded one by one before, which admitted falloffs up to 2^120 and quotients in
    // the denormal range, where the one-correction division is not the IEEE quotient).
    if (r.leanOK != 0u && !inRange(r.falloffBound, 0x1p-30f, 0x1p30f))
    {
        r.leanOK = 0u;
        r.rcpFalloffDistance = 0.0f;
        r.falloffBound = 0.0f;
    }
    if (r.leanOK != 0u)
    {
        bool tight = fabsf(r.position[0]) <= 0x1p12f && fabsf(r.position[1]) <= 0x1p12f && fabsf(r.position[2]) <= 0x1p12f &&
                     inRange(r.falloffBound, 0x1p-20f, 0x1p20f);
        for (int k = 0; k < 16; k++)
        {
            tight = tight && fabsf(r.shadowRows[k]) <= 0x1p14f;
        }
        r.leanOK |= tight ? 2u : 0u;
    }
    out[i] = r;
}

// ---------------------------------------------------------------------------
// deferred/lights.comp:110-164.
//
// Light records are wave-uniform, so they are read with scalar loads into SGPRs (VALU operands for free,
// no VGPR or LDS cost); the next light's cull rows are prefetched while the current light is evaluated.
// Per light a lane first runs a division-free conservative test ("surely outside the cone"), then the exact
// evaluation (the reference's arithmetic, including its exact zero for pixels outside the cone), in
// ascending light order, so the per-pixel sum adds the same non-zero terms in the same order as the reference
// loop. Measured on the C3 scene: 29 % of pixel-light pairs are lit (~19 lights per pixel), so most of the pass is the
// exact BRDF evaluation; of the 64 lights a wave evaluates 14 for some lane, and the other visits - every lane surely
// outside the cone - were a fifth of the VALU instructions the kernel issued. k_light_tiles decides those once per 64 x 64 screen tile, and
// the loop visits only the lights whose bit the tile's mask word has set (profiles/lights_tile_masks.md). An LDS-staged
// variant (records copied to LDS once per workgroup, broadcast reads) was measured 20 % slower than scalar loads and dropped.
//
// A spot light contributes exactly 0 when distance(st, 0.5) / 0.5 >= 1 (lights.comp:84-88). |s - 0.5| > 0.505 on
// either axis implies that with a 1 % margin, far above any rounding of the exact evaluation, so rejecting there
// never changes a result — unless the other axis is NaN. cw == 0 (st = inf/NaN) is not rejected.

// Runtime (wave-uniform) selection between the lean exact ops of szg_lean.hpp and the generic operators;
// both give the IEEE correctly rounded result, the lean ones only inside their operand ranges.
SZG_DEV float divU(bool lean, float a, float b, float y) { return lean ? divR(a, b, y) : a / b; }
// numerator of a lean division: 0, or not tiny (the residual of the one-correction division underflows below ~2^-100; its
// upper bound comes from the light's rows, checked once in k_light_prep)
SZG_DEV bool leanNumerator(float a) { return a == 0.0f || fabsf(a) >= 0x1p-60f; }
SZG_DEV float sqrtU(bool lean, float x) { return lean ? sqrtN(x) : sqrtf(x); }

// One light's term of the sum (lights.comp:141-161), exact.
// `clip`: shadowMatrix * vec4(position, 1), rows x, y, w summed left to right (pairCull, szg_light_tiles.hpp: the cone test and the
// exact evaluation share one evaluation of the three rows; R[k] * 1.0f of the shader's product is R[k] itself)
// `backCull` (per lane): the pixel's own factors are of ordinary magnitude (k_lights, pixelModerate), so that a term whose last
// factor clamp(N.L, 0, 1) is 0 is an exact zero and its BRDF (half of the cost of a lit pair) need not be evaluated.
//
// OPTIMISTIC (k_lights' first pass, only for lights whose record is "tight" and waves whose pixels all are, see there): the lean
// exact operators are used without testing their operand ranges pair by pair. Upper bounds hold by construction; the LOWER
// bounds (|w| and d^2 >= 2^-30, |half vector|^2 >= 2^-40, projected numerators >= 2^-60 in magnitude - a numerator of exactly
// 0 counts as out of range here, which only costs time) are folded into `track`, a running minimum per lane, scaled to the
// common threshold 2^-30: three v_min3 and three multiplies instead of fourteen compares and the mask arithmetic around
// them. Every operand is a finite number on this path (no NaN can hide from the minimum). k_lights checks `track` once after
// the loop and repeats the wave's loop with the tested form if it ever fell below the threshold.
template <bool OPTIMISTIC>
SZG_DEV V3 lightContribution(const LightRec& L, const Material& m, bool positionModerate, V3 viewDirection, bool cullable, V3 clip,
                             bool backCull, float d2, float& track)
{
    const float* R = L.shadowRows;
    float const cx = clip.x, cy = clip.y, cw = clip.z;
    bool const isSpot = L.isSpot != 0u;
    V3 const lightDir = mk3(L.dir[0], L.dir[1], L.dir[2]);
    // (d2 = dot(toLight, toLight) of distance(), lights.comp:80, formed by the caller in front of the cone test)
    // The surface faces away from the light: clamp(dot(N, L), 0, 1) = 0 (also for a NaN, fmax(NaN, 0) = 0) is the last factor
    // of ((occlusion * brdf) * spectral) * clamp(N.L) (lights.comp:106-107), so the term is +-0 - and sum + (+-0) == sum, the sum
    // being never -0 - provided the other factors are finite numbers whose product does not overflow:
    //   |occlusion * brdf| < 2^36 for a pixel of ordinary magnitude (k_lights, pixelModerate; clamp() turns a NaN half
    //   vector into 0, so brdf is a number whatever the directions are);
    //   spectral = ((colour * strength / falloff) * edge) * shadow with colour * strength <= 2^30 (k_light_prep, leanOK), edge and
    //   shadow in [0, 1] whatever the projected coordinates are, and falloff = factor * (dist / falloffDistance)^2 >= 2^-30:
    //   tested as falloffBound * d^2 >= 2^-28, the same quantity up to rounding, with a factor of 4 to spare (an infinite
    //   falloff gives spectral = 0).
    // Then nothing of this light needs evaluating for the pixel: a quarter of the lit pixel-light pairs of the bench scenes.
    float const ndl = dotL(m.normal, lightDir);
    if (backCull && cullable && isSpot && (OPTIMISTIC || L.leanOK != 0u) && !(ndl > 0.0f) && L.falloffBound * d2 >= 0x1p-28f)
    {
        return splat(0.0f);
    }
    V3 const hs = lightDir + viewDirection;
    float const hd = dotP(hs, hs);
    // Operand ranges of the lean ops used below: w of the projected position, squared distance to the light
    // (=> lightFalloff = factor * (dist / falloffDistance)^2 with the per-light constants checked by k_light_prep),
    // the half-vector length, and the position magnitude. One lane outside sends the wave down the generic path.
    float const lo = 0x1p-30f, hi = 0x1p30f;
    // (numerators too: the one-correction division returns NaN for an infinite numerator where the quotient is inf — a
    // projection with entries near FLT_MAX — and is not verified for denormal ones)
    float const cz = (L.map != nullptr)
                         ? SZG_CON(SZG_C_MATVEC, R[10], m.position.z, SZG_CON(SZG_C_MATVEC, R[9], m.position.y, R[8] * m.position.x)) + R[11]
                         : 0.0f;
    bool lean = true;
    if (OPTIMISTIC)
    {
        track = fminf(track, fminf(fabsf(cw), d2));
        track = fminf(track, fminf(hd * 0x1p10f, fabsf(cx) * 0x1p30f));
        track = fminf(track, fabsf(cy) * 0x1p30f);
        if (L.map != nullptr)
        {
            track = fminf(track, fabsf(cz) * 0x1p30f);
        }
    }
    else
    {
        lean = waveAll(L.leanOK != 0u && positionModerate && inRange(fabsf(cw), lo, hi) && inRange(d2, lo, hi) &&
                       inRange(hd, 0x1p-40f, 8.0f) && leanNumerator(cx) && leanNumerator(cy) && leanNumerator(cz));
    }

    float const ycw = lean ? rcpN(cw) : 0.0f;
    // (OPTIMISTIC: the quotients below are never zero - numerators >= 2^-60 over denominators < 2^28, positive lengths - so the
    // sign fix of a zero quotient, divR's last instruction, has nothing to do: divR0; and the square roots of d^2 and |h|^2 are
    // of numbers >= 2^-40: sqrtP)
    float const sx = OPTIMISTIC ? divR0(cx, cw, ycw) : divU(lean, cx, cw, ycw);
    float const sy = OPTIMISTIC ? divR0(cy, cw, ycw) : divU(lean, cy, cw, ycw);
    float edgeSoftening = 1.0f;
    float lightFalloff = 1.0f;
    if (isSpot)
    {
        // lights.comp:80-85. distanceUV = clamp(sqrt(q) / 0.5, 0, 1) and edgeSoftening = 1 - distanceUV^2 is
        // exactly 0 iff sqrt(q) * 2 >= 1 iff q >= 0.25 (sqrt is monotonic, sqrt(0.25) = 0.5 exactly), so the
        // cull needs no square root. x / 0.5 == x * 2 exactly.
        float const ddx = sx - 0.5f, ddy = sy - 0.5f;
        float const q = SZG_CON(SZG_C_LDOT, ddy, ddy, ddx * ddx); // dot(d, d) of distance()
        // (an exact zero only while colour * strength / falloff is finite: see falloffAwayFromZero in pairCull, szg_light_tiles.hpp)
        if (q >= 0.25f && cullable && L.falloffBound * d2 >= 0x1p-28f)
        {
            return splat(0.0f);
        }
        float const distanceUV = clampf(sqrtU(lean, q) * 2.0f, 0.0f, 1.0f);
        edgeSoftening = 1.0f - distanceUV * distanceUV;
        float const dist = OPTIMISTIC ? sqrtP(d2) : sqrtU(lean, d2);
        float const nd = OPTIMISTIC ? divR0(dist, L.falloffDistance, L.rcpFalloffDistance)
                                    : (lean ? divR(dist, L.falloffDistance, L.rcpFalloffDistance) : dist / L.falloffDistance);
        lightFalloff = L.falloffFactor * nd * nd;
    }
    float shadow = 1.0f;
    if (L.map != nullptr)
    {
        float const sz = OPTIMISTIC ? divR0(cz, cw, ycw) : divU(lean, cz, cw, ycw);
        // projectedNormal = shadowMatrix * vec4(normal, 0)
        float const nx = SZG_CON(SZG_C_MATVEC, R[3], 0.0f, SZG_CON(SZG_C_MATVEC, R[2], m.normal.z, SZG_CON(SZG_C_MATVEC, R[1], m.normal.y, R[0] * m.normal.x)));
        float const ny = SZG_CON(SZG_C_MATVEC, R[7], 0.0f, SZG_CON(SZG_C_MATVEC, R[6], m.normal.z, SZG_CON(SZG_C_MATVEC, R[5], m.normal.y, R[4] * m.normal.x)));
        float const fdx = sqrtf(1.0f - clampf(nx * nx, 0.0f, 1.0f));
        float const fdy = sqrtf(1.0f - clampf(ny * ny, 0.0f, 1.0f));
        shadow = sampleShadowMap(L.map, L.mapWidth, L.mapHeight, L.mapPitchFloats, mk3(sx, sy, sz), fdx, fdy);
    }
    V3 const cs = mk3(L.colorStrength[0], L.colorStrength[1], L.colorStrength[2]);
    // lights.comp:68 / :87-88
    V3 spectral;
    if (isSpot)
    {
        float const yf = lean ? rcpN(lightFalloff) : 0.0f;
        V3 const perFalloff = mk3(divU(lean, cs.x, lightFalloff, yf), divU(lean, cs.y, lightFalloff, yf), divU(lean, cs.z, lightFalloff, yf));
        spectral = (perFalloff * edgeSoftening) * shadow;
    }
    else
    {
        spectral = cs * shadow;
    }
    // computeLightContribution, lights.comp:93-108 (brdfMix of szg_pbr.hpp with the half vector shared above)
    float const hinv = OPTIMISTIC ? divN0(1.0f, sqrtP(hd)) : (lean ? divN(1.0f, sqrtN(hd)) : 1.0f / sqrtf(hd));
    V3 const h = hs * hinv;
    // both pow() without their special-case selects when no lane of the wave has a zero / denormal / non-finite base or a
    // zero exponent (szg_lean.hpp powLean: the same values)
    float const baseSpecular = clampf(dotP(h, m.normal), 0.0f, 1.0f);
    float const baseFresnel = 1.0f - clampf(dotP(h, lightDir), 0.0f, 1.0f);
    // (OPTIMISTIC: both bases lie in [0, 1] and must be >= 2^-126 for powLean: tracked like the other lower bounds, x * 2^96
    // against 2^-30; the exponent's range is part of the wave's precondition in k_lights)
    bool powsLean = true;
    if (OPTIMISTIC)
    {
        track = fminf(track, fminf(baseSpecular * 0x1p96f, baseFresnel * 0x1p96f));
    }
    else
    {
        powsLean = waveAll(powLeanOK(baseSpecular, m.specularPower) && powLeanOK(baseFresnel, 5.0f));
    }
    float const microfacet = powsLean ? powLean(baseSpecular, m.specularPower) : szg_powf(baseSpecular, m.specularPower);
    V3 const specular = splat(m.normalization * microfacet);
    float const p = powsLean ? powLean(baseFresnel, 5.0f) : szg_powf(baseFresnel, 5.0f);
    V3 const fresnel = m.reflectance + (splat(1.0f) - m.reflectance) * p;
    V3 const brdf = mix(m.diffuse, specular, fresnel);
    // lights.comp:106-107
    return ((m.occlusion * brdf) * spectral) * clampf(ndl, 0.0f, 1.0f);
}

// The three rows of the shadow matrix the cone test needs (x, y, w) + the spot flag (LightCull, szg_light_tiles.hpp).
SZG_DEV LightCull loadCull(const LightRec* __restrict__ L)
{
    LightCull c;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        c.rx[k] = L->shadowRows[k];
        c.ry[k] = L->shadowRows[4 + k];
        c.rw[k] = L->shadowRows[12 + k];
    }
    c.position[0] = L->position[0];
    c.position[1] = L->position[1];
    c.position[2] = L->position[2];
    c.falloffBound = L->falloffBound;
    c.isSpot = L->isSpot;
    return c;
}
// The loop over the lights for one pixel (lights.comp:141-161): terms added in ascending light order.
// `tileWords` (wave-uniform, may be null): the words k_light_tiles wrote for this pixel's 64 x 64 tile, one per 64 lights, a
// clear bit = every position of the tile fails pairCull for that light. Read with one scalar load per 64 lights; the set
// bits are visited from the lowest up, so the sum keeps its order of terms. A wave with a non-finite pixel visits every light,
// as it ignores the per-pixel cull.
template <bool OPTIMISTIC>
SZG_DEV V3 lightLoop(const LightRec* lights, unsigned lightCount, const unsigned long long* __restrict__ tileWords, const Material& m,
                     bool positionModerate, V3 viewDirection, bool waveFinite, bool pixelModerate, float& track)
{
    V3 sum = splat(0.0f);
#pragma unroll 1
    for (unsigned base = 0, batch = 0; base < lightCount; base += LIGHT_TILE_BATCH, batch++)
    {
        unsigned const n = lightCount - base;
        unsigned long long word = n >= LIGHT_TILE_BATCH ? ~0ull : (1ull << n) - 1ull;
        if (waveFinite && tileWords != nullptr)
        {
            word = tileWords[batch]; // (bits of lights past lightCount are clear)
        }
#pragma unroll 1
        while (word != 0ull)
        {
            unsigned const i = base + (unsigned)__builtin_ctzll(word);
            word &= word - 1ull;
            const LightRec* __restrict__ L = lights + i;
            LightCull const cur = loadCull(L); // (prefetching light i+1's rows here measured 20 % slower)
            unsigned const flags = L->leanOK;
            bool const cullable = waveFinite && (flags & 1u) != 0u;
            // rows x, y, w of the shadow-space position and the squared distance, formed in front of the cone test
            // (szg_light_tiles.hpp: why the culls ask for falloffBound * d^2 >= 2^-28)
            PairCull const pc = pairCull(cur, flags, m.position.x, m.position.y, m.position.z);
            if (waveFinite && pc.skip)
            {
                continue;
            }
            V3 const clip = mk3(pc.cx, pc.cy, pc.cw);
            if (OPTIMISTIC && (flags & 2u) != 0u)
            {
                sum = sum + lightContribution<true>(*L, m, positionModerate, viewDirection, cullable, clip, pixelModerate, pc.d2, track);
            }
            else
            {
                sum = sum + lightContribution<false>(*L, m, positionModerate, viewDirection, cullable, clip, pixelModerate, pc.d2, track);
            }
        }
    }
    return sum;
}

// ---------------------------------------------------------------------------
// One workgroup per 64 x 64-pixel tile of the local image (partial at the right and bottom edges): the tile's G-buffer
// positions - background texels included, which only widens the box - are reduced to an axis-aligned box and the flag "every
// position finite and <= 2^30"; then wave 0 tests 64 light records at a time against the box, one light per lane
// (tileMaySkipLight, szg_light_tiles.hpp), and writes one 64-bit word per 64 lights: bit set = visit this light.
// masks[(tileY * tilesX + tileX) * batches + batch]; every word of every tile of the launch is written, so the storage needs
// no clear. A non-finite box keeps every bit; so do directional lights and records without flag bit 0.
__global__ __launch_bounds__(256) void k_light_tiles(szg_image position, unsigned drawW, unsigned localRows,
                                                     const LightRec* __restrict__ lights, unsigned lightCount,
                                                     unsigned long long* __restrict__ masks)
{
    __shared__ float s_box[4][6];
    __shared__ unsigned s_bad[4];
    unsigned const lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned const x = blockIdx.x * LIGHT_TILE_DIM + lane;
    unsigned const y0 = blockIdx.y * LIGHT_TILE_DIM;
    float const inf = __builtin_inff();
    float box[6] = {inf, inf, inf, -inf, -inf, -inf};
    bool ok = true;
    if (x < drawW)
    {
        for (unsigned r = wave; r < LIGHT_TILE_DIM && y0 + r < localRows; r += 4u)
        {
            float4 const p = row_ptr<const float4>(position, y0 + r)[x];
            ok = ok && fabsf(p.x) <= 0x1p30f && fabsf(p.y) <= 0x1p30f && fabsf(p.z) <= 0x1p30f; // false for a NaN
            box[0] = fminf(box[0], p.x);
            box[1] = fminf(box[1], p.y);
            box[2] = fminf(box[2], p.z);
            box[3] = fmaxf(box[3], p.x);
            box[4] = fmaxf(box[4], p.y);
            box[5] = fmaxf(box[5], p.z);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++)
    {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
        {
            float const other = __shfl_xor(box[k], d, 64);
            box[k] = k < 3 ? fminf(box[k], other) : fmaxf(box[k], other);
        }
    }
    bool const waveOk = waveAll(ok);
    if (lane == 0u)
    {
#pragma unroll
        for (int k = 0; k < 6; k++)
        {
            s_box[wave][k] = box[k];
        }
        s_bad[wave] = waveOk ? 0u : 1u;
    }
    __syncthreads();
    if (wave != 0u)
    {
        return;
    }
    TileBox b;
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        b.lo[k] = fminf(fminf(s_box[0][k], s_box[1][k]), fminf(s_box[2][k], s_box[3][k]));
        b.hi[k] = fmaxf(fmaxf(s_box[0][3 + k], s_box[1][3 + k]), fmaxf(s_box[2][3 + k], s_box[3][3 + k]));
    }
    b.finite = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) == 0u && b.lo[0] <= b.hi[0] && b.lo[1] <= b.hi[1] && b.lo[2] <= b.hi[2];
    unsigned const batches = (lightCount + LIGHT_TILE_BATCH - 1u) / LIGHT_TILE_BATCH;
    unsigned long long* out = masks + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * batches;
    for (unsigned batch = 0; batch < batches; batch++)
    {
        unsigned const i = batch * LIGHT_TILE_BATCH + lane;
        bool visit = false;
        if (i < lightCount)
        {
            const LightRec* __restrict__ L = lights + i;
            visit = !tileMaySkipLight(loadCull(L), L->leanOK, b);
        }
        unsigned long long const word = __builtin_amdgcn_ballot_w64(visit);
        if (lane == 0u)
        {
            out[batch] = word;
        }
    }
}

// `tileMasks` (may be null: no spot lights, nothing to cull): the words of k_light_tiles, `tilesX` tiles per row of tiles.
__global__ __launch_bounds__(256, 6) void k_lights(szg_image color, szg_image debug, GBufferPtrs g, unsigned drawW,
                                                unsigned localRows, const szg_camera_packed* __restrict__ cameras,
                                                unsigned cameraIndex, const LightRec* __restrict__ lights, unsigned lightCount,
                                                const unsigned long long* __restrict__ tileMasks, unsigned tilesX)
{
    unsigned x, y;
    pixel_of_thread_bottom_up(x, y);
    if (x >= drawW || y >= localRows)
    {
        return;
    }
    V4 const diffuse = unpack_half4(row_ptr<const uint2>(g.diffuse, y)[x]);
    V3 sum = splat(0.0f);
    // lights.comp:126-129: background texels keep the clear colour (0,0,0,1)
    if (!(diffuse.w < 1.0f))
    {
        V4 const specular = unpack_half4(row_ptr<const uint2>(g.specular, y)[x]);
        V4 const normal = unpack_half4(row_ptr<const uint2>(g.normal, y)[x]);
        V4 const orm = unpack_half4(row_ptr<const uint2>(g.orm, y)[x]);
        float4 const p4 = row_ptr<const float4>(g.position, y)[x];
        Material const m = convertPBR(V4{p4.x, p4.y, p4.z, p4.w}, normal, diffuse, specular, orm);
        const szg_camera_packed* cam = cameras + cameraIndex;
        V3 const viewDirection = normalizeL(mk3(cam->position[0], cam->position[1], cam->position[2]) - m.position);

        float const hi = 0x1p30f;
        bool const positionModerate = fabsf(m.position.x) <= hi && fabsf(m.position.y) <= hi && fabsf(m.position.z) <= hi;
        // every per-pixel factor of a light's term is finite (see k_light_prep): only then is 0 * term an exact zero and a
        // pixel outside a spot light's cone may skip that light (a NaN anywhere poisons the sum in the reference)
        float const big = 0x1p120f;
        bool const pixelFinite = positionModerate && fabsf(viewDirection.x) <= 2.0f && fabsf(viewDirection.y) <= 2.0f &&
                                 fabsf(viewDirection.z) <= 2.0f && fabsf(m.normal.x) <= big && fabsf(m.normal.y) <= big &&
                                 fabsf(m.normal.z) <= big && fabsf(m.diffuse.x) <= big && fabsf(m.diffuse.y) <= big &&
                                 fabsf(m.diffuse.z) <= big && fabsf(m.reflectance.x) <= big && fabsf(m.reflectance.y) <= big &&
                                 fabsf(m.reflectance.z) <= big && fabsf(m.occlusion) <= big && fabsf(m.normalization) <= big &&
                                 fabsf(m.specularPower) <= big;
        // ... and of ordinary magnitude (every real material: roughness in [0, 1] gives a specular power <= 160): then
        // |occlusion * mix(diffuse, specular, fresnel)| < 2^36, see lightContribution's back-face test
        bool const pixelModerate = pixelFinite && fabsf(m.diffuse.x) <= 0x1p16f && fabsf(m.diffuse.y) <= 0x1p16f &&
                                   fabsf(m.diffuse.z) <= 0x1p16f && fabsf(m.reflectance.x) <= 4.0f && fabsf(m.reflectance.y) <= 4.0f &&
                                   fabsf(m.reflectance.z) <= 4.0f && fabsf(m.occlusion) <= 0x1p16f && fabsf(m.normalization) <= 0x1p8f &&
                                   fabsf(m.normal.x) <= 0x1p16f && fabsf(m.normal.y) <= 0x1p16f && fabsf(m.normal.z) <= 0x1p16f;
        // Light records are wave-uniform: they are fetched with scalar loads and live in SGPRs. Culling is decided per
        // wave: when some pixel of the wave has a non-finite factor the whole wave evaluates every light (no term of its
        // sum may be dropped); the flag of the light itself is wave-uniform anyway.
        bool const waveFinite = waveAll(pixelFinite);
        // The optimistic pass (lightContribution<true>): every pixel of the wave finite and within 4096 units of the origin.
        bool const tightPixel = pixelFinite && fabsf(m.position.x) <= 0x1p12f && fabsf(m.position.y) <= 0x1p12f && fabsf(m.position.z) <= 0x1p12f &&
                                inRange(fabsf(m.specularPower), 0x1p-100f, 0x1p20f); // (the exponent half of powLeanOK)
        // The workgroup's 32 x 8 pixels lie in one 64 x 64 tile: its mask words are found from the workgroup's first column
        // and first row (pixel_row_bottom_up's, szg_pixel.hpp) alone, in scalar registers.
        const unsigned long long* tileWords = nullptr;
        if (tileMasks != nullptr)
        {
            unsigned const tileX = (blockIdx.x * PIXEL_GROUP_W) / LIGHT_TILE_DIM;
            unsigned const tileY = (pixel_group_bottom_up() * PIXEL_GROUP_H) / LIGHT_TILE_DIM;
            unsigned const batches = (lightCount + LIGHT_TILE_BATCH - 1u) / LIGHT_TILE_BATCH;
            tileWords = tileMasks + (size_t)(tileY * tilesX + tileX) * batches;
        }
        bool done = false;
        if (waveAll(tightPixel))
        {
            float track = 0x1p100f;
            sum = lightLoop<true>(lights, lightCount, tileWords, m, positionModerate, viewDirection, waveFinite, pixelModerate, track);
            done = waveAll(track >= 0x1p-30f);
        }
        if (!done)
        {
            float unused = 0.0f;
            sum = lightLoop<false>(lights, lightCount, tileWords, m, positionModerate, viewDirection, waveFinite, pixelModerate, unused);
        }
    }
    row_ptr<uint2>(color, y)[x] = pack_unorm16x4(sum.x, sum.y, sum.z, 1.0f);
    if (debug.data != nullptr)
    {
        row_ptr<float4>(debug, y)[x] = make_float4(sum.x, sum.y, sum.z, 1.0f);
    }
}

// ---------------------------------------------------------------------------
hipError_t launch_light_prep(hipStream_t s, const szg_directional_light_packed* d_dir, unsigned dirCount, unsigned dirSkip,
                             const szg_spot_light_packed* d_spot, unsigned spotCount, const ShadowSlot* d_slots,
                             unsigned slotCount, LightRec* d_out)
{
    unsigned const nDir = dirCount > dirSkip ? dirCount - dirSkip : 0u;
    unsigned const n = nDir + spotCount;
    if (n == 0u)
    {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_light_prep, dim3((n + 63u) / 64u), dim3(64), 0, s, d_dir, dirCount, dirSkip, d_spot, spotCount, d_slots,
                       slotCount, d_out);
    return hipGetLastError();
}

hipError_t launch_lights(hipStream_t s, const szg_scene_texture& scene, unsigned drawW, unsigned drawH, TileArgs tile,
                         const szg_gbuffer& g, const szg_camera_packed* d_cam, unsigned camIndex, const LightRec* d_lights,
                         unsigned lightCount, const unsigned long long* d_tileMasks)
{
    unsigned const rows = tile.local_rows;
    if (rows == 0u || drawW == 0u)
    {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_lights, pixel_grid(drawW, rows), dim3(256), 0, s, scene.color, scene.debug_color, gptrs(g), drawW, rows, d_cam, camIndex,
                       d_lights, lightCount, d_tileMasks, (drawW + LIGHT_TILE_DIM - 1u) / LIGHT_TILE_DIM);
    return hipGetLastError();
}

hipError_t launch_light_tiles(hipStream_t s, unsigned drawW, unsigned drawH, TileArgs tile, const szg_gbuffer& g,
                              const LightRec* d_lights, unsigned lightCount, unsigned long long* d_tileMasks)
{
    unsigned const rows = tile.local_rows;
    if (rows == 0u || drawW == 0u || lightCount == 0u)
    {
        return hipSuccess;
    }
    dim3 const grid((drawW + LIGHT_TILE_DIM - 1u) / LIGHT_TILE_DIM, (rows + LIGHT_TILE_DIM - 1u) / LIGHT_TILE_DIM);
    hipLaunchKernelGGL(k_light_tiles, grid, dim3(256), 0, s, g.worldPosition, drawW, rows, d_lights, lightCount, d_tileMasks);
    return hipGetLastError();
}
} // namespace szg
