// szg_vec.hpp — the vector and matrix types of the device code and their operators, with the contraction rule
// (SZG_CON, include/szg/contraction.h) at the closed list of places where a * b + c is fused.
#pragma once

#include <hip/hip_runtime.h>

#include "szg/abi.h"

#define SZG_DEV __device__ __forceinline__

namespace szg
{
struct V2
{
    float x, y;
};
struct V3
{
    float x, y, z;
};
struct V4
{
    float x, y, z, w;
};

SZG_DEV V3 mk3(float a, float b, float c) { return V3{a, b, c}; }
SZG_DEV V3 splat(float a) { return V3{a, a, a}; }
SZG_DEV V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
SZG_DEV V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
SZG_DEV V3 operator-(V3 a) { return V3{-a.x, -a.y, -a.z}; }
SZG_DEV V3 operator*(V3 a, V3 b) { return V3{a.x * b.x, a.y * b.y, a.z * b.z}; }
SZG_DEV V3 operator/(V3 a, V3 b) { return V3{a.x / b.x, a.y / b.y, a.z / b.z}; }
SZG_DEV V3 operator*(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
SZG_DEV V3 operator*(float s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
SZG_DEV V3 operator/(V3 a, float s) { return V3{a.x / s, a.y / s, a.z / s}; }
// Contraction rule (include/szg/contraction.h): a * b + c is fused only at a closed list of places, by site class, explicitly
// and at the same places as the oracle; the compiler itself contracts nothing (-ffp-contract=off). -DSZG_LITERAL builds
// libszg_hip_literal.so (SZG_CONTRACT = 0: two roundings everywhere), i.e. kernels that execute the shaders' SPIR-V
// literally; tests/test_gpu_spirv_pin.py compares that build, bit for bit and on the GPU, with the vectors an interpreter
// recorded from the reference's committed .spv (tests/golden/spirv_vectors.npz), and holds the product to 1e-4 / 1 LSB of
// them. The fused multiply-adds INSIDE the exact operators of szg_lean.hpp (rcpN, divR, sqrtN, exp / log polynomials) are not part of
// the rule: they are how those operators reach their correctly rounded results, and stay.
#ifdef SZG_LITERAL
#define SZG_CONTRACT SZG_CONTRACT_NONE
#endif
} // namespace szg
#include "szg/contraction.h"
namespace szg
{
// shading geometry (SZG_C_DOT) ...
SZG_DEV float dot(V3 a, V3 b) { return SZG_CON(SZG_C_DOT, a.z, b.z, SZG_CON(SZG_C_DOT, a.y, b.y, a.x * b.x)); }
SZG_DEV float dot(V2 a, V2 b) { return SZG_CON(SZG_C_DOT, a.y, b.y, a.x * b.x); }
// ... and the atmosphere geometry of common.glinl (SZG_C_ATMODOT: raySphere, the LUT samplers, the march)
SZG_DEV float dotA(V3 a, V3 b) { return SZG_CON(SZG_C_ATMODOT, a.z, b.z, SZG_CON(SZG_C_ATMODOT, a.y, b.y, a.x * b.x)); }
// pbrFunctions.glinl (SZG_C_PBRDOT) and lights.comp (SZG_C_LDOT)
SZG_DEV float dotP(V3 a, V3 b) { return SZG_CON(SZG_C_PBRDOT, a.z, b.z, SZG_CON(SZG_C_PBRDOT, a.y, b.y, a.x * b.x)); }
SZG_DEV float dotL(V3 a, V3 b) { return SZG_CON(SZG_C_LDOT, a.z, b.z, SZG_CON(SZG_C_LDOT, a.y, b.y, a.x * b.x)); }
// length(position) in the 500-step loop of transmittance_LUT.comp (SZG_C_TMAIN)
SZG_DEV float dotT(V3 a, V3 b) { return SZG_CON(SZG_C_TMAIN, a.z, b.z, SZG_CON(SZG_C_TMAIN, a.y, b.y, a.x * b.x)); }
// the march's accumulations (SZG_C_ACCUM) and sample points (SZG_C_POINT)
SZG_DEV V3 fma3(V3 a, float s, V3 c) { return V3{SZG_CON(SZG_C_ACCUM, a.x, s, c.x), SZG_CON(SZG_C_ACCUM, a.y, s, c.y), SZG_CON(SZG_C_ACCUM, a.z, s, c.z)}; }
SZG_DEV V3 fma3(V3 a, V3 b, V3 c) { return V3{SZG_CON(SZG_C_ACCUM, a.x, b.x, c.x), SZG_CON(SZG_C_ACCUM, a.y, b.y, c.y), SZG_CON(SZG_C_ACCUM, a.z, b.z, c.z)}; }
SZG_DEV V3 fnma(float t, V3 d, V3 c) { return V3{SZG_CON(SZG_C_POINT, -t, d.x, c.x), SZG_CON(SZG_C_POINT, -t, d.y, c.y), SZG_CON(SZG_C_POINT, -t, d.z, c.z)}; }
SZG_DEV float length(V3 a) { return sqrtf(dot(a, a)); }
SZG_DEV V3 normalize(V3 v)
{
    float const s = 1.0f / sqrtf(dot(v, v));
    return v * s;
}
SZG_DEV V2 normalize(V2 v)
{
    float const s = 1.0f / sqrtf(dot(v, v));
    return V2{v.x * s, v.y * s};
}
SZG_DEV V3 normalizeP(V3 v)
{
    float const s = 1.0f / sqrtf(dotP(v, v));
    return v * s;
}
SZG_DEV V3 normalizeL(V3 v)
{
    float const s = 1.0f / sqrtf(dotL(v, v));
    return v * s;
}
SZG_DEV float lengthA(V3 a) { return sqrtf(dotA(a, a)); }
SZG_DEV V3 normalizeA(V3 v)
{
    float const s = 1.0f / sqrtf(dotA(v, v));
    return v * s;
}
SZG_DEV float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
SZG_DEV V3 clamp01(V3 v) { return V3{clampf(v.x, 0.0f, 1.0f), clampf(v.y, 0.0f, 1.0f), clampf(v.z, 0.0f, 1.0f)}; }
SZG_DEV V3 mix(V3 a, V3 b, V3 w)
{
    return V3{SZG_CON(SZG_C_MIX, b.x, w.x, a.x * (1.0f - w.x)), SZG_CON(SZG_C_MIX, b.y, w.y, a.y * (1.0f - w.y)),
              SZG_CON(SZG_C_MIX, b.z, w.z, a.z * (1.0f - w.z))};
}
SZG_DEV float smoothstep(float e0, float e1, float x)
{
    float const t = clampf((x - e0) / (e1 - e0), 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}
SZG_DEV float safeSqrt(float v) { return sqrtf(fmaxf(v, 0.0f)); } // atmosphere/common.glinl:23-26

// column-major 4x4 times (x, y, z, w), rows summed left to right
struct M4
{
    float m[16];
};
SZG_DEV V4 mul(const M4& a, float x, float y, float z, float w)
{
    V4 r;
    r.x = SZG_CON(SZG_C_MATVEC, a.m[12], w, SZG_CON(SZG_C_MATVEC, a.m[8], z, SZG_CON(SZG_C_MATVEC, a.m[4], y, a.m[0] * x)));
    r.y = SZG_CON(SZG_C_MATVEC, a.m[13], w, SZG_CON(SZG_C_MATVEC, a.m[9], z, SZG_CON(SZG_C_MATVEC, a.m[5], y, a.m[1] * x)));
    r.z = SZG_CON(SZG_C_MATVEC, a.m[14], w, SZG_CON(SZG_C_MATVEC, a.m[10], z, SZG_CON(SZG_C_MATVEC, a.m[6], y, a.m[2] * x)));
    r.w = SZG_CON(SZG_C_MATVEC, a.m[15], w, SZG_CON(SZG_C_MATVEC, a.m[11], z, SZG_CON(SZG_C_MATVEC, a.m[7], y, a.m[3] * x)));
    return r;
}
SZG_DEV M4 mul(const M4& a, const M4& b)
{
    M4 r;
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
        V4 const c = mul(a, b.m[j * 4 + 0], b.m[j * 4 + 1], b.m[j * 4 + 2], b.m[j * 4 + 3]);
        r.m[j * 4 + 0] = c.x;
        r.m[j * 4 + 1] = c.y;
        r.m[j * 4 + 2] = c.z;
        r.m[j * 4 + 3] = c.w;
    }
    return r;
}
// glm's mat4 * mat4 as the reference's HOST code evaluates it (one rounding per operation, columns combined left to right:
// host_scene.cpp szg_mat4_mul): for matrices the reference computes on the CPU and hands to a shader - the per-light
// projView of the shadow passes (shadowpass.cpp:188-248) - as opposed to products written in a shader (mul above).
SZG_DEV M4 mulGlm(const M4& a, const M4& b)
{
    M4 r;
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            r.m[j * 4 + i] = a.m[i] * b.m[j * 4 + 0] + a.m[4 + i] * b.m[j * 4 + 1] + a.m[8 + i] * b.m[j * 4 + 2] + a.m[12 + i] * b.m[j * 4 + 3];
        }
    }
    return r;
}
// glm::inverse(mat4) (cofactor expansion, glm/detail/func_matrix.inl), same operation order as host_scene.cpp
SZG_DEV M4 inverse4(const M4& m)
{
    auto M = [&](int c, int r) { return m.m[c * 4 + r]; };
    float const C00 = M(2, 2) * M(3, 3) - M(3, 2) * M(2, 3), C02 = M(1, 2) * M(3, 3) - M(3, 2) * M(1, 3),
                C03 = M(1, 2) * M(2, 3) - M(2, 2) * M(1, 3), C04 = M(2, 1) * M(3, 3) - M(3, 1) * M(2, 3),
                C06 = M(1, 1) * M(3, 3) - M(3, 1) * M(1, 3), C07 = M(1, 1) * M(2, 3) - M(2, 1) * M(1, 3),
                C08 = M(2, 1) * M(3, 2) - M(3, 1) * M(2, 2), C10 = M(1, 1) * M(3, 2) - M(3, 1) * M(1, 2),
                C11 = M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2), C12 = M(2, 0) * M(3, 3) - M(3, 0) * M(2, 3),
                C14 = M(1, 0) * M(3, 3) - M(3, 0) * M(1, 3), C15 = M(1, 0) * M(2, 3) - M(2, 0) * M(1, 3),
                C16 = M(2, 0) * M(3, 2) - M(3, 0) * M(2, 2), C18 = M(1, 0) * M(3, 2) - M(3, 0) * M(1, 2),
                C19 = M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2), C20 = M(2, 0) * M(3, 1) - M(3, 0) * M(2, 1),
                C22 = M(1, 0) * M(3, 1) - M(3, 0) * M(1, 1), C23 = M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1);
    float const F0[4] = {C00, C00, C02, C03}, F1[4] = {C04, C04, C06, C07}, F2[4] = {C08, C08, C10, C11},
                F3[4] = {C12, C12, C14, C15}, F4[4] = {C16, C16, C18, C19}, F5[4] = {C20, C20, C22, C23};
    float const V0[4] = {M(1, 0), M(0, 0), M(0, 0), M(0, 0)}, V1[4] = {M(1, 1), M(0, 1), M(0, 1), M(0, 1)},
                V2[4] = {M(1, 2), M(0, 2), M(0, 2), M(0, 2)}, V3_[4] = {M(1, 3), M(0, 3), M(0, 3), M(0, 3)};
    float const SA[4] = {1.0f, -1.0f, 1.0f, -1.0f}, SB[4] = {-1.0f, 1.0f, -1.0f, 1.0f};
    M4 inv;
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
        inv.m[0 * 4 + i] = (V1[i] * F0[i] - V2[i] * F1[i] + V3_[i] * F2[i]) * SA[i];
        inv.m[1 * 4 + i] = (V0[i] * F0[i] - V2[i] * F3[i] + V3_[i] * F4[i]) * SB[i];
        inv.m[2 * 4 + i] = (V0[i] * F1[i] - V1[i] * F3[i] + V3_[i] * F5[i]) * SA[i];
        inv.m[3 * 4 + i] = (V0[i] * F2[i] - V1[i] * F4[i] + V2[i] * F5[i]) * SB[i];
    }
    float const det = (M(0, 0) * inv.m[0] + M(0, 1) * inv.m[4]) + (M(0, 2) * inv.m[8] + M(0, 3) * inv.m[12]);
    float const ood = 1.0f / det;
#pragma unroll
    for (int i = 0; i < 16; i++)
    {
        inv.m[i] = inv.m[i] * ood;
    }
    return inv;
}
SZG_DEV M4 load_m4(const szg_mat4& s)
{
    M4 r;
#pragma unroll
    for (int i = 0; i < 16; i++)
    {
        r.m[i] = s.m[i];
    }
    return r;
}

} // namespace szg
