// szg_lean.hpp — the lean exact operators (division, square root, exp, pow) and the gates of their operand domains.
#pragma once

#include "szg/fpmath.h"
#include "szg_vec.hpp"

namespace szg
{
// ---------------------------------------------------------------------------
// Lean exact division and square root.
//
// hipcc's correctly rounded `/` and sqrtf() cost ~47 and ~64 cycles per wave64 operation
// on gfx950 (an fma costs ~2.3): every call carries the denormal/overflow scaling and the
// special-case fix-up. The sequences below are the SAME algorithms without the scaling
// (v_rcp_f32 / v_rsq_f32 seed, Newton, exact fma residual corrections). They return the
// IEEE-754 correctly rounded result — bit-identical to `/` and sqrtf() — whenever their
// operand preconditions hold, and cost ~6 / ~6 instructions; a division whose denominator's
// reciprocal is shared costs 3. Checked on MI355X by tests/test_gpu_device_arith.py against
// float64 references: sqrtN and rcpN for ALL binary32 inputs in their domains; divN on every
// numerator significand for the all-ones and 64 random denominators and on 2^30 pairs of each
// family of tools/verify_div.hip (the longer sweeps; history in DESIGN.md "lean exact ops").
// They are used only under a wave-uniform `lean` flag that the kernels derive from the
// atmosphere block and the ray (see leanAtmosphere / leanRay); otherwise the generic
// operators are used, so results never depend on the flag.
// ---------------------------------------------------------------------------
// Correctly rounded reciprocal: rcpN(b) == RN(1 / b) for EVERY binary32 b with |b| in [2^-60, 2^60]
// (tests/test_gpu_device_arith.py and tools/verify_div.hip, exhaustive on MI355X): v_rcp_f32 and one Newton step.
SZG_DEV float rcpN(float b)
{
    float const y = __builtin_amdgcn_rcpf(b);
    float const e = __builtin_fmaf(-b, y, 1.0f);
    return __builtin_fmaf(e, y, y);
}
// a / b given y = rcpN(b); a == +-0 or |a| in [2^-60, 2^60]. Markstein's theorem: with y the correctly rounded
// reciprocal, q0 = RN(a * y) and the exact residual r = a - b * q0 (one fma), RN(q0 + r * y) is the correctly rounded
// quotient, the only candidates for an exception being denominators whose significand is all ones — and those are
// checked exhaustively against RN(a / b) together with the premise (tests/test_gpu_device_arith.py: every numerator
// significand for the 120 all-ones denominators of the domain and for 64 random ones, 5.4e9 random and structured pairs;
// tools/verify_div.hip: 4096 random denominators and 6.4e10 pairs).
SZG_DEV float divR(float a, float b, float y)
{
    float const q0 = a * y;
    float const r = __builtin_fmaf(-b, q0, a);
    float const q = __builtin_fmaf(r, y, q0);
    return __builtin_copysignf(q, q0); // a zero quotient keeps the sign IEEE division gives it
}
SZG_DEV float divN(float a, float b) { return divR(a, b, rcpN(b)); }
// divR without the sign fix of a zero quotient (one v_bfi less). Used where a quotient of zero is consumed sign-blind or
// cannot be negative — every divRX site: exp(+-0) = 1 (densities), 1 - (+-0) (ozone tent), bias + q * scale with bias > 0
// (both LUT coordinates), mu only as -r*mu + sqrt(...) >= 0 and mu*mu (LUT tap), (mu_sun - c) - e0 with e0 != 0 (sun
// smoothstep), non-negative numerators over positive denominators (rho / H, Rp / r, distance * (i + .5) / 500), whose zero
// quotient comes out +0 on its own.
SZG_DEV float divR0(float a, float b, float y)
{
    float const q0 = a * y;
    float const r = __builtin_fmaf(-b, q0, a);
    return __builtin_fmaf(r, y, q0);
}
// sqrt(x) for x == 0 or x in [2^-96, FLT_MAX] (NaN -> NaN): v_rsq_f32 seed, one Newton step on the exact fma residual.
// Bit-identical to sqrtf for EVERY binary32 value of that domain (tests/test_gpu_device_arith.py and tools/verify_sqrt.hip,
// exhaustive on MI355X against RN(sqrt x) in float64).
// The max() only matters for x == 0: rsq stays finite, so 0 * y = 0 and the correction is fma(0, h, 0) = 0.
SZG_DEV float sqrtN(float x)
{
    float const y = __builtin_amdgcn_rsqf(fmaxf(x, 0x1p-126f));
    float const s = x * y;
    float const h = 0.5f * y;
    float const r = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(r, h, s);
}
// sqrtN for x in [2^-96, FLT_MAX] (not 0): without the max()
SZG_DEV float sqrtP(float x)
{
    float const y = __builtin_amdgcn_rsqf(x);
    float const s = x * y;
    float const h = 0.5f * y;
    float const r = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(r, h, s);
}
template <bool LEAN> SZG_DEV float sqrtX(float x) { return LEAN ? sqrtN(x) : sqrtf(x); }
// square root of a squared radius / squared length that a lean path knows to be positive (>= the squared lean floor)
template <bool LEAN> SZG_DEV float sqrtPX(float x) { return LEAN ? sqrtP(x) : sqrtf(x); }
template <bool LEAN> SZG_DEV float safeSqrtX(float v) { return sqrtX<LEAN>(fmaxf(v, 0.0f)); }
// exp of a value that is never NaN on a lean path (finite coefficients, radii above the lean floor)
template <bool LEAN> SZG_DEV float expX(float x) { return LEAN ? szg_expf_notnan(x) : szg_expf(x); }
// szg_expf (szg/fpmath.h) for x in [-86, 87], not NaN: the same reduction and polynomial, value for value. In that range the
// clamp of the argument to [-104, 89] is the identity, q = rint(x log2 e) lies in [-125, 126] and u in (0.5, 2), so
// u * 2^(q >> 1) and its product with 2^(q - (q >> 1)) are exact (no underflow, no overflow): (u * 2^q1) * 2^(q - q1) is
// u * 2^q, which is what v_ldexp_f32 returns for a normal result. 9 instructions less than szg_expf_notnan. Equal to it for
// every x of the range (tests/test_gpu_device_arith.py).
SZG_DEV float expInner(float x)
{
    float const q = __builtin_rintf(x * 1.442695040888963407359924681001892137426645954152985934135449406931f);
    float s = __builtin_fmaf(q, -0.693145751953125f, x);
    s = __builtin_fmaf(q, -1.428606765330187045e-06f, s);
    float u = 0.000198527617612853646278381f;
    u = __builtin_fmaf(u, s, 0.00139304355252534151077271f);
    u = __builtin_fmaf(u, s, 0.00833336077630519866943359f);
    u = __builtin_fmaf(u, s, 0.0416664853692054748535156f);
    u = __builtin_fmaf(u, s, 0.166666671633720397949219f);
    u = __builtin_fmaf(u, s, 0.5f);
    u = __builtin_fmaf(s * s, u, s) + 1.0f;
    return __builtin_ldexpf(u, (int)q);
}
// (quotients of the divX sites — the two segment cosines and the smoothstep argument — are consumed sign-blind too)
template <bool LEAN> SZG_DEV float divX(float a, float b) { return LEAN ? divR0(a, b, rcpN(b)) : a / b; }
template <bool LEAN> SZG_DEV float divRX(float a, float b, float y) { return LEAN ? divR0(a, b, y) : a / b; }
SZG_DEV float xorSign(float x, unsigned signMask)
{
    return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) ^ signMask);
}
SZG_DEV bool inRange(float x, float lo, float hi) { return x >= lo && x <= hi; } // false for NaN
SZG_DEV float divN0(float a, float b) { return divR0(a, b, rcpN(b)); }
// a numerator divR / divR0 accept: +-0, or a magnitude in [2^-60, 2^60] (false for NaN)
SZG_DEV bool leanQuotientOperand(float a) { return a == 0.0f || inRange(fabsf(a), 0x1p-60f, 0x1p60f); }
// true when `c` holds on every active lane: one compare into a lane mask and one scalar test (HIP's __all() builds two
// ballots from an int predicate, ~15 instructions per use). Lanes switched off by divergence - a call under a divergent `if`,
// lanes that have left the kernel - do not take part: the ballot has 0 for them, so their values can neither open nor close a
// gate (tests/test_gpu_march_rays.py runs the march with every third lane, and with all lanes but one, switched off).
SZG_DEV bool waveAll(bool c) { return __builtin_amdgcn_ballot_w64(!c) == 0ull; }

// szg_powf(x, y) (szg/fpmath.h: exp(y * log x) with GLSL's special cases) for a base that is a positive NORMAL number
// (2^-126 <= x < inf) and an exponent that is a finite number other than 0 - the same operations value for value, without
// the selects that cannot fire there: log's denormal pre-scaling (x >= 2^-126) and its x == inf / x == 0 / x < 0 / NaN
// cases, exp's NaN pass-through (the argument y * log x is a finite product), pow's x == 0 and y == 0 cases. The clamp of
// exp's argument stays: x^160 underflows for most bases. Equal to szg_powf on every base of [2^-20, 2) for the path's
// exponents and on 2^28 random pairs of the precondition (tests/test_gpu_device_arith.py).
SZG_DEV float powLean(float x, float y)
{
    int const bits = szg_float_to_bits(x * 1.3333333333333333333333333333333333333f);
    int const e = ((bits >> 23) & 0xFF) - 127;
    float const m = szg_bits_to_float(szg_float_to_bits(x) - (e << 23));
    float const t = szg_div_moderate(m - 1.0f, m + 1.0f);
    float const t2 = t * t;
    float p = 0.2392828464508056640625f;
    p = __builtin_fmaf(p, t2, 0.28518211841583251953125f);
    p = __builtin_fmaf(p, t2, 0.400005877017974853515625f);
    p = __builtin_fmaf(p, t2, 0.666666686534881591796875f);
    p = __builtin_fmaf(p, t2, 2.0f);
    float const fe = (float)e;
    float const lg = __builtin_fmaf(t, p, 0.693147180559945286226764f * fe);
    return szg_expf_notnan(y * lg);
}
// wave-uniform precondition of powLean
SZG_DEV bool powLeanOK(float x, float y)
{
    return x >= 1.17549435e-38f && x <= 0x1p127f && fabsf(y) >= 0x1p-100f && fabsf(y) <= 0x1p20f;
}

} // namespace szg
