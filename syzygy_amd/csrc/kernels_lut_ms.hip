// kernels_lut_ms.hip — the sky-view LUT and the aerial-perspective LUT with the multi-scattering term of
// include/szg/multiscatter_sky.h in their marches, for gfx950.
//
//   k_skyview_ms<MS, STAGED>  : k_skyview (kernels_lut.hip) with marchLoop<.., MS>
//   k_aerial_lut_ms<MS>       : k_aerial_lut with the same
//
// MS is SZG_MULTISCATTER_ADD or SZG_MULTISCATTER_ONLY; mode OFF launches the kernels of kernels_lut.hip, which this unit
// does not touch. The texel-to-ray code is shared with them (szg_lut_rays.hpp), the march is szg_march.hpp's.

#include "szg/fpmath.h"
#include "szg/multiscatter_sky.h"
#include "szg_atmosphere.hpp"
#include "szg_launch.hpp"
#include "szg_lean.hpp"
#include "szg_lut_rays.hpp"
#include "szg_march.hpp"
#include "szg_vec.hpp"

// Where k_skyview_ms takes the 32 x 32 multi-scattering texels from: 1 = staged once per workgroup in LDS (16 KiB), 0 = from
// global memory through the vector cache, which the transmittance taps already use. Both were timed
// (profiles/multiscatter_sky.md); the other one builds as `make libszg_hip_msalt.so`.
#ifndef SZG_MS_STAGE_LDS
#define SZG_MS_STAGE_LDS 0
#endif

namespace szg
{
constexpr unsigned MS_TEXELS = SZG_MULTISCATTER_DIM * SZG_MULTISCATTER_DIM;

// The workgroup shape, the reuse exit, the texel store and the status dword are k_skyview's.
template <int MS, bool STAGED>
__global__ __launch_bounds__(256) void k_skyview_ms(const szg_atmosphere_packed* __restrict__ atmospheres, unsigned atmosphereIndex,
                                                    const szg_camera_packed* __restrict__ cameras, unsigned cameraIndex,
                                                    const float4* __restrict__ tlut, int tW, int tH,
                                                    const float4* __restrict__ psi, float4* __restrict__ lut, int W, int H,
                                                    int rowBegin, int rowEnd, const unsigned* __restrict__ dirty,
                                                    const FramePrep* __restrict__ prep)
{
    __shared__ float4 s_psi[STAGED ? MS_TEXELS : 1u];
    if (dirty != nullptr && dirty[0] == 0u) // LUT reuse: inputs unchanged since these texels were computed (the whole grid leaves)
    {
        return;
    }
    unsigned const tid = threadIdx.x;
    if (STAGED)
    {
#pragma unroll
        for (unsigned k = 0; k < MS_TEXELS / 256u; k++)
        {
            s_psi[k * 256u + tid] = psi[k * 256u + tid];
        }
        __syncthreads(); // in front of the per-lane exit below: every lane of the workgroup arrives
    }
    unsigned const wave = tid >> 6, lane = tid & 63u;
    int const x = (int)(blockIdx.x * 32u + wave * 8u + (lane & 7u));
    int const y = rowBegin + (int)(blockIdx.y * 8u + (lane >> 3));
    if (x >= W || y >= rowEnd)
    {
        return;
    }
    Atm const a = load_atm(*prep);
    TLut const L = make_tlut(tlut, tW, tH, *prep);
    V3 origin, direction;
    skyviewTexelRay(a, cameras + cameraIndex, x, y, W, H, origin, direction);

    float const distance = raycastAtmosphere(a, origin, direction);
    V3 const luminance = scatteringIntegral<MS>(L, a, origin, direction, distance, STAGED ? s_psi : psi);
    lut[y * W + x] = make_float4(luminance.x, luminance.y, luminance.z, 1.0f);
    if (!slutTexelFinite(luminance.x, luminance.y, luminance.z)) // status dword behind the texels, as k_skyview keeps it
    {
        atomicOr(reinterpret_cast<unsigned*>(lut + (size_t)W * (size_t)H), 1u);
    }
}

// One froxel per lane, as k_aerial_lut; the transmittance volume is the same in every mode.
template <int MS>
__global__ __launch_bounds__(256) void k_aerial_lut_ms(const szg_atmosphere_packed* __restrict__ atmospheres, unsigned atmosphereIndex,
                                                       const szg_camera_packed* __restrict__ cameras, unsigned cameraIndex,
                                                       const float4* __restrict__ tlut, int tW, int tH,
                                                       const float4* __restrict__ psi, float4* __restrict__ luminance,
                                                       float4* __restrict__ transmittance, unsigned W, unsigned H, unsigned D,
                                                       float maxDistance)
{
    unsigned const id = blockIdx.x * 256u + threadIdx.x;
    if (id >= W * H * D)
    {
        return;
    }
    unsigned const i = id % W, j = (id / W) % H, k = id / (W * H);
    Atm const a = load_atm(atmospheres + atmosphereIndex);
    TLut const L = make_tlut(tlut, tW, tH);
    V3 position, direction;
    aerialFroxelRay(a, cameras + cameraIndex, i, j, W, H, position, direction);

    float const d = (((float)k + 0.5f) / (float)D) * maxDistance;
    V3 const lum = scatteringIntegral<MS>(L, a, position, direction, d, psi);
    V3 const T = sampleT_Segment(L, a, position, position + d * direction);
    luminance[id] = make_float4(lum.x, lum.y, lum.z, 1.0f);
    transmittance[id] = make_float4(T.x, T.y, T.z, 1.0f);
}

template <int MS>
static hipError_t skyview_ms(hipStream_t s, const szg_atmosphere_packed* d_atm, unsigned atmIndex, const szg_camera_packed* d_cam,
                             unsigned camIndex, const float* tlut, unsigned tW, unsigned tH, const float* psi, float* lut, unsigned W,
                             unsigned H, unsigned rowBegin, unsigned rowEnd, const unsigned* d_dirty, const void* d_prep)
{
    dim3 const grid((W + 31u) / 32u, (rowEnd - rowBegin + 7u) / 8u);
    hipLaunchKernelGGL((k_skyview_ms<MS, SZG_MS_STAGE_LDS != 0>), grid, dim3(256), 0, s, d_atm, atmIndex, d_cam, camIndex,
                       reinterpret_cast<const float4*>(tlut), (int)tW, (int)tH, reinterpret_cast<const float4*>(psi),
                       reinterpret_cast<float4*>(lut), (int)W, (int)H, (int)rowBegin, (int)rowEnd, d_dirty,
                       static_cast<const FramePrep*>(d_prep));
    return hipGetLastError();
}

hipError_t launch_skyview_ms(hipStream_t s, unsigned mode, const szg_atmosphere_packed* d_atm, unsigned atmIndex,
                             const szg_camera_packed* d_cam, unsigned camIndex, const float* tlut, unsigned tW, unsigned tH,
                             const float* psi, float* lut, unsigned W, unsigned H, unsigned rowBegin, unsigned rowEnd,
                             const unsigned* d_dirty, const void* d_prep)
{
    if (mode != SZG_MULTISCATTER_ADD && mode != SZG_MULTISCATTER_ONLY)
    {
        return hipErrorInvalidValue; // (mode OFF is launch_skyview's)
    }
    if (rowEnd > H)
    {
        rowEnd = H;
    }
    if (rowBegin >= rowEnd || W == 0u)
    {
        return hipSuccess;
    }
    if (d_dirty == nullptr) // the status dword starts clear and the kernel sets it (launch_skyview)
    {
        hipError_t const e = hipMemsetAsync(lut + (size_t)W * H * 4u, 0, 4, s);
        if (e != hipSuccess)
        {
            return e;
        }
    }
    return mode == SZG_MULTISCATTER_ADD
               ? skyview_ms<1>(s, d_atm, atmIndex, d_cam, camIndex, tlut, tW, tH, psi, lut, W, H, rowBegin, rowEnd, d_dirty, d_prep)
               : skyview_ms<2>(s, d_atm, atmIndex, d_cam, camIndex, tlut, tW, tH, psi, lut, W, H, rowBegin, rowEnd, d_dirty, d_prep);
}

hipError_t launch_aerial_lut_ms(hipStream_t s, unsigned mode, const szg_atmosphere_packed* d_atm, unsigned atmIndex,
                                const szg_camera_packed* d_cam, unsigned camIndex, const float* tlut, unsigned tW, unsigned tH,
                                const float* psi, float* luminance, float* transmittance, unsigned W, unsigned H, unsigned D,
                                float maxDistance)
{
    if (mode != SZG_MULTISCATTER_ADD && mode != SZG_MULTISCATTER_ONLY)
    {
        return hipErrorInvalidValue;
    }
    unsigned const n = W * H * D;
    dim3 const grid((n + 255u) / 256u);
    if (mode == SZG_MULTISCATTER_ADD)
    {
        hipLaunchKernelGGL(k_aerial_lut_ms<1>, grid, dim3(256), 0, s, d_atm, atmIndex, d_cam, camIndex,
                           reinterpret_cast<const float4*>(tlut), (int)tW, (int)tH, reinterpret_cast<const float4*>(psi),
                           reinterpret_cast<float4*>(luminance), reinterpret_cast<float4*>(transmittance), W, H, D, maxDistance);
    }
    else
    {
        hipLaunchKernelGGL(k_aerial_lut_ms<2>, grid, dim3(256), 0, s, d_atm, atmIndex, d_cam, camIndex,
                           reinterpret_cast<const float4*>(tlut), (int)tW, (int)tH, reinterpret_cast<const float4*>(psi),
                           reinterpret_cast<float4*>(luminance), reinterpret_cast<float4*>(transmittance), W, H, D, maxDistance);
    }
    return hipGetLastError();
}
} // namespace szg
