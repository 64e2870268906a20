/*
 * szg/exact_sign.h — exact signs of the rasteriser's determinants (raster.h "coverage").
 *
 * The fp32 edge function decides almost every pixel; where its magnitude is inside its own rounding budget the sign is
 * taken (after a second filter in plain fp64) from the EXACT value of det[h_j; h_k; (px, py, 1)] of the fp32 h values instead. Every fp32 value is a dyadic
 * rational, a product of two of them is exact in fp64 (48 bits), and the product of that with a third factor is the
 * error-free pair (p, fma(a, b, -p)). The determinant is therefore a sum of at most 12 doubles, whose sign is the sign
 * of the largest non-zero component of the non-overlapping expansion that Shewchuk's Grow-Expansion builds from them
 * ("Adaptive Precision Floating-Point Arithmetic and Fast Robust Geometric Predicates", 1997, theorem 10: exact under
 * round-to-nearest-even). Straight-line code: no data-dependent loop.
 *
 * Domain: finite fp32 inputs (the callers test that first). Magnitudes: a triple product of fp32 values lies between
 * 2^-447 and 2^384, its low half 53 bits below: far inside the fp64 exponent range, so nothing overflows or underflows.
 * Only IEEE fp64 +, -, *, fma: the same bits on x86-64 and gfx950. The compiler must not re-associate (the builds use
 * -fno-fast-math); fma() is called explicitly, which -ffp-contract=off does not forbid.
 */
#ifndef SZG_EXACT_SIGN_H
#define SZG_EXACT_SIGN_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SZG_EX_FN __host__ __device__ __forceinline__
#else
#define SZG_EX_FN static inline
#endif
#if defined(__clang__)
#define SZG_EX_UNROLL _Pragma("unroll")
#else
#define SZG_EX_UNROLL
#endif

/* s + e == a + b exactly (Knuth) */
SZG_EX_FN void szg_two_sum(double a, double b, double& s, double& e)
{
    s = a + b;
    double const bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
/* p + e == a * b exactly */
SZG_EX_FN void szg_two_prod(double a, double b, double& p, double& e)
{
    p = a * b;
    e = __builtin_fma(a, b, -p);
}

/* Sign (-1, 0, +1) of t[0] + ... + t[N-1], exactly. Overwrites t with the expansion. */
template <int N> SZG_EX_FN int szg_sum_sign(double (&t)[N])
{
SZG_EX_UNROLL
    for (int m = 1; m < N; m++)
    {
        double q = t[m];
SZG_EX_UNROLL
        for (int i = 0; i < m; i++)
        {
            double s, e;
            szg_two_sum(q, t[i], s, e);
            t[i] = e;
            q = s;
        }
        t[m] = q;
    }
    int sign = 0;
SZG_EX_UNROLL
    for (int i = 0; i < N; i++) /* components grow in magnitude: the last non-zero one decides */
    {
        sign = t[i] > 0.0 ? 1 : (t[i] < 0.0 ? -1 : sign);
    }
    return sign;
}

/* sign of a * b - c * d for fp32 values: two exact fp64 products */
SZG_EX_FN int szg_diff_of_products_sign(float a, float b, float c, float d)
{
    double const p = (double)a * (double)b, q = (double)c * (double)d;
    return p > q ? 1 : (p < q ? -1 : 0);
}

/* Sign of the edge function through vertices j and k at the pixel centre (px, py):
 * E = px (hy_j hw_k - hy_k hw_j) + py (hx_k hw_j - hx_j hw_k) + (hx_j hy_k - hx_k hy_j).
 * Second filter stage before the expansion: the same expression in plain fp64. Its six products are exact, the three
 * differences and the four operations of the evaluation round once each, so its error is below
 * 2^-51 (A px + B py + C) with A, B, C the sums of the magnitudes of the products; `bound64` is the caller's upper bound
 * of that (2^-50 times the same sum). Outside it the fp64 sign stands. */
SZG_EX_FN int szg_edge_sign(float hxj, float hyj, float hwj, float hxk, float hyk, float hwk, float px, float py, double bound64)
{
    double const p0 = (double)hyj * (double)hwk, p1 = (double)hyk * (double)hwj;
    double const p2 = (double)hxk * (double)hwj, p3 = (double)hxj * (double)hwk;
    double const p4 = (double)hxj * (double)hyk, p5 = (double)hxk * (double)hyj;
    double const E = ((p0 - p1) * (double)px + (p2 - p3) * (double)py) + (p4 - p5);
    if (E > bound64)
    {
        return 1;
    }
    if (E < -bound64)
    {
        return -1;
    }
    double t[10];
    szg_two_prod(p0, (double)px, t[0], t[1]);
    szg_two_prod(-p1, (double)px, t[2], t[3]);
    szg_two_prod(p2, (double)py, t[4], t[5]);
    szg_two_prod(-p3, (double)py, t[6], t[7]);
    t[8] = p4;
    t[9] = -p5;
    return szg_sum_sign(t);
}

/* Sign of det[h_0; h_1; h_2] = hx_0 a_0 + hy_0 b_0 + hw_0 c_0 (raster.h "facing"). */
SZG_EX_FN int szg_facing_sign(const float hx[3], const float hy[3], const float hw[3])
{
    double t[12];
    szg_two_prod((double)hy[1] * (double)hw[2], (double)hx[0], t[0], t[1]);
    szg_two_prod(-((double)hy[2] * (double)hw[1]), (double)hx[0], t[2], t[3]);
    szg_two_prod((double)hx[2] * (double)hw[1], (double)hy[0], t[4], t[5]);
    szg_two_prod(-((double)hx[1] * (double)hw[2]), (double)hy[0], t[6], t[7]);
    szg_two_prod((double)hx[1] * (double)hy[2], (double)hw[0], t[8], t[9]);
    szg_two_prod(-((double)hx[2] * (double)hy[1]), (double)hw[0], t[10], t[11]);
    return szg_sum_sign(t);
}

#endif /* SZG_EXACT_SIGN_H */
