// szg_lut_rays.hpp — the ray of a sky-view LUT texel and of an aerial-perspective froxel: what k_skyview / k_aerial_lut
// (kernels_lut.hip) and their multi-scattering twins (kernels_lut_ms.hip) march along.
#pragma once

#include "szg/fpmath.h"
#include "szg_atmosphere.hpp"
#include "szg_vec.hpp"

namespace szg
{
// skyview_LUT.comp:100-119: origin and direction of texel (x, y) of a W x H sky-view LUT
SZG_DEV void skyviewTexelRay(const Atm& a, const szg_camera_packed* cam, int x, int y, int W, int H, V3& origin, V3& direction)
{
    float const PI = 3.141592653589793f;

    // skyview_LUT.comp:100-101
    float const u = ((float)x + 0.5f) / (float)W;
    float const v = ((float)y + 0.5f) / (float)H;

    // skyview_LUT.comp:110-112
    origin = mk3(cam->position[0], cam->position[1], cam->position[2]) / 1000000.0f;
    origin.y *= -1.0f;
    origin.y += a.planetRadius;

    // uv_to_azimuthElevation, skyview_LUT.comp:51-89
    float const radius = length(origin);
    float const sinHorizonZenith = a.planetRadius / radius;
    float const horizonZenith = PI - szg_asinf(sinHorizonZenith);
    float const cosineViewLightProjected = (u - 0.5f) * 2.0f;
    V2 const lightDirectionProjected = normalize(V2{-a.incidentDirectionSun.x, -a.incidentDirectionSun.z});
    float azimuthSun = szg_asinf(lightDirectionProjected.x);
    if (lightDirectionProjected.y < 0.0f)
    {
        azimuthSun = PI - azimuthSun;
    }
    float const azimuth = szg_acosf(clampf(cosineViewLightProjected, -1.0f, 1.0f)) + azimuthSun;
    float viewZenith;
    float const unnormalized_v = 2.0f * v - 1.0f;
    if (v < 0.5f)
    {
        float const angleFraction = 1.0f - unnormalized_v * unnormalized_v;
        viewZenith = angleFraction * horizonZenith;
    }
    else
    {
        float const angleFraction = unnormalized_v * unnormalized_v;
        viewZenith = (PI - horizonZenith) * angleFraction + horizonZenith;
    }
    float const elevation = -(viewZenith - PI / 2.0f);

    // skyview_LUT.comp:118-119
    float const ce = szg_cosf(elevation);
    direction = normalize(mk3(szg_sinf(azimuth) * ce, szg_sinf(elevation), szg_cosf(azimuth) * ce));
}

// camera.comp:320-328 with the froxel centre as the (continuous) pixel coordinate: camera position and view direction of
// column i, row j of a W x H froxel grid
SZG_DEV void aerialFroxelRay(const Atm& a, const szg_camera_packed* cam, unsigned i, unsigned j, unsigned W, unsigned H, V3& position,
                             V3& direction)
{
    position = mk3(cam->position[0], cam->position[1], cam->position[2]) / 1000000.0f;
    position.y *= -1.0f;
    position.y += a.planetRadius;
    float const clipx = (((float)i + 0.5f) / (float)W - 0.5f) * 2.0f;
    float const clipy = (((float)j + 0.5f) / (float)H - 0.5f) * 2.0f;
    V4 const dvs = mul(load_m4(cam->inverseProjection), clipx, clipy, 1.0f, 1.0f);
    V4 const rot = mul(load_m4(cam->rotation), dvs.x, dvs.y, dvs.z, dvs.w);
    direction = normalize(mk3(rot.x, rot.y, rot.z));
    direction.y *= -1.0f;
}
} // namespace szg
