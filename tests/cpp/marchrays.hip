// marchrays.hip — test infrastructure: scatteringIntegral / marchLoop of syzygy_amd/csrc/szg_march.hpp called RAY BY RAY on
// the GPU, one thread per ray, so that a test decides which rays share a wave (tests/march_rays.py lays the waves out,
// tests/test_gpu_march_rays.py compares every lane with the oracle's scalar march bit for bit). Built with the product's
// HIPFLAGS (tests/Makefile; the flag line is checked by tests/test_device_arith_build.py).
//
// The product's own kernels_lut.hip is part of this translation unit: the FramePrep block of the `prepped` configuration
// comes from its k_frame_prep and the LUT's status dword from its k_lut_range, through its launch functions; nothing of
// either is restated here.
//
// A ray is 8 dwords: origin.xyz, direction.xyz, sample distance, flag word (bit 0: HOLE). Wave w of the launch holds rays
// 64 w .. 64 w + 63. A hole does not call scatteringIntegral at all - the divergent call of k_composite's phase B
// (kernels_composite.hip: `if (flags >> k & 1) { ... scatteringIntegral(...) }`) - and lanes at or past n have left the
// kernel; their output slots keep the sentinel the buffer was filled with.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_lut.hip" // (found on the include path, like the szg_*.hpp device headers it includes)

namespace
{
using namespace szg;

struct MrFlags
{
    uint32_t lean, signClearCoefficients, zeroAbsorptionRayleigh, zeroScatteringOzone, extModerate, moderate, rowsInterior;
    float innerCeil2, leanFloor2, extFloor2, extCeil2;
};

template <bool PREPPED>
SZG_DEV void loadBlocks(const szg_atmosphere_packed* atm, const float4* tlut, int tW, int tH, const FramePrep* prep, Atm& a, TLut& L)
{
    if (PREPPED)
    {
        a = load_atm(*prep);
        L = make_tlut(tlut, tW, tH, *prep);
    }
    else
    {
        a = load_atm(atm);
        L = make_tlut(tlut, tW, tH);
    }
}

template <bool PREPPED>
__global__ __launch_bounds__(256) void k_march_rays(const szg_atmosphere_packed* __restrict__ atm, const float4* __restrict__ tlut, int tW,
                                                    int tH, const FramePrep* __restrict__ prep, const uint4* __restrict__ rays, unsigned n,
                                                    float* __restrict__ out)
{
    unsigned const id = blockIdx.x * 256u + threadIdx.x;
    if (id >= n)
    {
        return;
    }
    Atm a;
    TLut L;
    loadBlocks<PREPPED>(atm, tlut, tW, tH, prep, a, L);
    uint4 const r0 = rays[2u * id], r1 = rays[2u * id + 1u];
    V3 const origin = mk3(__builtin_bit_cast(float, r0.x), __builtin_bit_cast(float, r0.y), __builtin_bit_cast(float, r0.z));
    V3 const direction = mk3(__builtin_bit_cast(float, r0.w), __builtin_bit_cast(float, r1.x), __builtin_bit_cast(float, r1.y));
    float const sampleDistance = __builtin_bit_cast(float, r1.z);
    bool const hole = (r1.w & 1u) != 0u;
    if (!hole)
    {
        V3 const l = scatteringIntegral(L, a, origin, direction, sampleDistance);
        out[3u * id] = l.x;
        out[3u * id + 1u] = l.y;
        out[3u * id + 2u] = l.z;
    }
}

template <bool PREPPED>
__global__ __launch_bounds__(64) void k_march_flags(const szg_atmosphere_packed* __restrict__ atm, const float4* __restrict__ tlut, int tW,
                                                    int tH, const FramePrep* __restrict__ prep, MrFlags* __restrict__ flags)
{
    if (threadIdx.x != 0u)
    {
        return;
    }
    Atm a;
    TLut L;
    loadBlocks<PREPPED>(atm, tlut, tW, tH, prep, a, L);
    MrFlags f;
    f.lean = a.lean ? 1u : 0u;
    f.signClearCoefficients = a.signClearCoefficients ? 1u : 0u;
    f.zeroAbsorptionRayleigh = a.zeroAbsorptionRayleigh ? 1u : 0u;
    f.zeroScatteringOzone = a.zeroScatteringOzone ? 1u : 0u;
    f.extModerate = a.extModerate ? 1u : 0u;
    f.moderate = L.moderate ? 1u : 0u;
    f.rowsInterior = L.rowsInterior ? 1u : 0u;
    f.innerCeil2 = a.innerCeil2;
    f.leanFloor2 = a.leanFloor2;
    f.extFloor2 = a.extFloor2;
    f.extCeil2 = a.extCeil2;
    *flags = f;
}

// device buffers of one call, freed on every path
struct Buffers
{
    void* p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Buffers()
    {
        for (void* q : p)
        {
            (void)hipFree(q);
        }
    }
};
} // namespace

extern "C" {
// The march of `n` rays (host array of 8 n dwords) in the atmosphere `atm` with the transmittance LUT `texels` (host RGBA32F,
// tW x tH), configuration `prepped` (0: load_atm(block) / make_tlut(t, w, h); 1: the FramePrep forms). `out` (host) receives
// 3 * 256 * ceil(n / 256) floats: the launch's whole output buffer, every float of it set to the bit pattern `sentinel`
// before the launch. `flags` receives what the kernel's Atm / TLut read. Returns 0 or the HIP error code.
int szg_mr_run(const szg_atmosphere_packed* atm, const float* texels, unsigned tW, unsigned tH, int prepped, const uint32_t* rays,
               unsigned n, uint32_t sentinel, float* out, MrFlags* flags)
{
    Buffers b;
    size_t const lutBytes = (size_t)tW * tH * 16u + 16u; // texels and the status dword's 16 bytes (szg_launch.hpp)
    unsigned const groups = (n + 255u) / 256u;
    size_t const outFloats = (size_t)groups * 256u * 3u;
    hipError_t st = hipMalloc(&b.p[0], sizeof(szg_atmosphere_packed));
    st = st == hipSuccess ? hipMalloc(&b.p[1], lutBytes) : st;
    st = st == hipSuccess ? hipMalloc(&b.p[2], frame_prep_bytes()) : st;
    st = st == hipSuccess ? hipMalloc(&b.p[3], (size_t)(n ? n : 1u) * 32u) : st;
    st = st == hipSuccess ? hipMalloc(&b.p[4], (outFloats ? outFloats : 1u) * 4u) : st;
    st = st == hipSuccess ? hipMalloc(&b.p[5], sizeof(MrFlags)) : st;
    st = st == hipSuccess ? hipMemcpy(b.p[0], atm, sizeof(szg_atmosphere_packed), hipMemcpyHostToDevice) : st;
    st = st == hipSuccess ? hipMemset(b.p[1], 0, lutBytes) : st;
    st = st == hipSuccess ? hipMemcpy(b.p[1], texels, (size_t)tW * tH * 16u, hipMemcpyHostToDevice) : st;
    st = st == hipSuccess && n ? hipMemcpy(b.p[3], rays, (size_t)n * 32u, hipMemcpyHostToDevice) : st;
    st = st == hipSuccess && outFloats ? hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b.p[4]), (int)sentinel, outFloats) : st;
    if (st != hipSuccess)
    {
        return (int)st;
    }
    auto* const dAtm = static_cast<const szg_atmosphere_packed*>(b.p[0]);
    auto* const dLut = static_cast<float*>(b.p[1]);
    auto* const dPrep = static_cast<FramePrep*>(b.p[2]);
    st = launch_lut_range(nullptr, dLut, tW, tH);
    st = st == hipSuccess ? launch_frame_prep(nullptr, dAtm, 0u, tW, tH, dPrep, nullptr) : st;
    if (st != hipSuccess)
    {
        return (int)st;
    }
    auto* const t4 = reinterpret_cast<const float4*>(dLut);
    auto* const dRays = static_cast<const uint4*>(b.p[3]);
    auto* const dOut = static_cast<float*>(b.p[4]);
    auto* const dFlags = static_cast<MrFlags*>(b.p[5]);
    if (prepped)
    {
        k_march_flags<true><<<1, 64>>>(dAtm, t4, (int)tW, (int)tH, dPrep, dFlags);
        if (groups)
        {
            k_march_rays<true><<<groups, 256>>>(dAtm, t4, (int)tW, (int)tH, dPrep, dRays, n, dOut);
        }
    }
    else
    {
        k_march_flags<false><<<1, 64>>>(dAtm, t4, (int)tW, (int)tH, dPrep, dFlags);
        if (groups)
        {
            k_march_rays<false><<<groups, 256>>>(dAtm, t4, (int)tW, (int)tH, dPrep, dRays, n, dOut);
        }
    }
    st = hipGetLastError();
    st = st == hipSuccess ? hipDeviceSynchronize() : st;
    st = st == hipSuccess && outFloats ? hipMemcpy(out, dOut, outFloats * 4u, hipMemcpyDeviceToHost) : st;
    st = st == hipSuccess ? hipMemcpy(flags, dFlags, sizeof(MrFlags), hipMemcpyDeviceToHost) : st;
    return (int)st;
}
} // extern "C"
