// devarith.hip — test infrastructure: the device arithmetic of include/szg/fpmath.h (its __HIP_DEVICE_COMPILE__ branches)
// and syzygy_amd/csrc/szg_device.hpp (the lean operators, the store formats), evaluated ON THE GPU over whole domains and
// compared with references computed on the GPU in float64. Built with the product's HIPFLAGS (tests/Makefile; the flag
// line is checked by tests/test_device_arith_build.py) so that it measures the code the kernels run. Driven through ctypes by
// tests/test_gpu_device_arith.py.
//
// szg_da_sweep(name, first, count, params, bound, result) runs one sweep: indices [first, first + count) of a FAMILY (index ->
// operands, __host__ __device__ so that the host can name the operands of the largest error) through an OP (value got, value
// wanted, comparison), in launches of at most 2^30 indices, the status checked after each one.
// szg_da_eval / szg_da_pack_half_range evaluate a function on given inputs and hand the values back to the host.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "szg_device.hpp"

namespace
{
constexpr int kList = 16;
constexpr unsigned kMaxLaunch = 1u << 30;
constexpr int kDenominators = 128;

struct DaParams
{
    uint32_t lo;      // first bit pattern of a bits range
    uint32_t family;  // sub-family of the seeded division pairs (0..4)
    uint64_t seed;
    uint32_t n_list;  // entries of `list` in use
    float list[kDenominators]; // denominators / exponents of a grid
};

struct DaResult
{
    uint64_t count;      // values evaluated
    uint64_t mismatches; // values outside the comparison
    double max_err;      // largest error (ULP of the reference's binade, or absolute for the ABS comparison)
    uint32_t max_a, max_b; // operand bits where it occurs
    uint32_t n_list;     // mismatches recorded below (the first ones to arrive, at most 16)
    uint32_t list_a[kList], list_b[kList], list_got[kList], list_want[kList];
};

struct DaAcc
{
    unsigned long long count, mismatches, max_bits, max_key; // max_key: high word of the error, low word the launch-local index
    unsigned n_list;
    unsigned list_a[kList], list_b[kList], list_got[kList], list_want[kList];
};

__host__ __device__ inline uint32_t f2u(float x) { return __builtin_bit_cast(uint32_t, x); }
__host__ __device__ inline float u2f(uint32_t x) { return __builtin_bit_cast(float, x); }
__host__ __device__ inline uint64_t d2u(double x) { return __builtin_bit_cast(uint64_t, x); }
__host__ __device__ inline double u2d(uint64_t x) { return __builtin_bit_cast(double, x); }

// counter-based generator: the k-th 64-bit draw of a stream depends on (seed, index, k) only, on host and device alike
__host__ __device__ inline uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
struct Rng
{
    uint64_t s;
    __host__ __device__ Rng(uint64_t seed, uint64_t index) : s(mix64(seed * 0x9E3779B97F4A7C15ull + index)) {}
    __host__ __device__ uint32_t next()
    {
        s += 0x9E3779B97F4A7C15ull;
        return (uint32_t)(mix64(s) >> 32);
    }
};
// a float with exponent in [emin, emax] (unbiased), a random significand and a random sign
__host__ __device__ inline float randomFloat(Rng& r, int emin, int emax)
{
    uint32_t const m = r.next(), e = r.next();
    int const ex = emin + (int)(e % (uint32_t)(emax - emin + 1));
    return u2f((m & 0x807FFFFFu) | ((uint32_t)(ex + 127) << 23));
}
__host__ __device__ inline bool inLeanDomain(float x) // +-0 excluded: |x| in [2^-60, 2^60]
{
    float const a = __builtin_fabsf(x);
    return a >= 0x1p-60f && a <= 0x1p60f;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Families: index -> operands (a, b); false = the index names no operand of the domain (not evaluated, not counted)
// ---------------------------------------------------------------------------------------------------------------------------
// every bit pattern lo + i (the sweep's [first, first + count) must stay inside 32 bits)
struct FamBits
{
    __host__ __device__ static bool at(const DaParams& p, uint64_t i, float& a, float& b)
    {
        a = u2f(p.lo + (uint32_t)i);
        b = 0.0f;
        return true;
    }
};
// every numerator significand (both signs) x 5 numerator exponents around the denominator's x each of list[0 .. n_list)
struct FamSignificands
{
    __host__ __device__ static bool at(const DaParams& p, uint64_t i, float& a, float& b)
    {
        uint32_t const k = (uint32_t)(i & 0xFFFFFFu);
        uint64_t const r = i >> 24;
        int const de = (int)(r % 5u) - 2;
        b = p.list[(r / 5u) % p.n_list];
        int const eb = (int)((f2u(b) >> 23) & 0xFFu);
        a = u2f(((k >> 23) << 31) | ((uint32_t)(eb + de) << 23) | (k & 0x7FFFFFu));
        return inLeanDomain(a);
    }
};
// the five families of seeded pairs of tools/verify_div.hip, exponents in [-60, 59]
struct FamDivPairs
{
    __host__ __device__ static bool at(const DaParams& p, uint64_t i, float& a, float& b)
    {
        Rng r(p.seed + p.family, i);
        a = randomFloat(r, -60, 59);
        b = randomFloat(r, -60, 59);
        switch (p.family)
        {
        case 1: // quotient next to +-1: a = b +- k ulp
        {
            int const k = (int)(r.next() % 65u) - 32;
            a = u2f((uint32_t)((int)(f2u(b) & 0x7FFFFFFFu) + k) | (r.next() & 0x80000000u));
            break;
        }
        case 2: // denominator significand tails all ones / all zeros
        {
            uint32_t const mask = (1u << (r.next() % 23u + 1u)) - 1u;
            b = u2f((r.next() & 1u) ? (f2u(b) | mask) : (f2u(b) & ~mask));
            break;
        }
        case 3: // exact multiples of the denominator
            a = b * (float)(r.next() % 4096u + 1u);
            break;
        case 4: // zero numerators of both signs
            a = (r.next() & 1u) ? 0.0f : -0.0f;
            return inLeanDomain(b);
        default:
            break;
        }
        return inLeanDomain(a) && inLeanDomain(b);
    }
};
// szg_div_moderate's declared domain: n = +0 or |n| in [2^-60, 0.5), d in [1.75, 2.5] (every bit pattern equally likely).
// Not -0: the sequence returns +0 for it where `/` returns -0 (log's m - 1 is never -0).
struct FamModerate
{
    __host__ __device__ static bool at(const DaParams& p, uint64_t i, float& a, float& b)
    {
        Rng r(p.seed, i);
        a = randomFloat(r, -60, -2);
        a = (r.next() % 64u == 0u) ? 0.0f : a;
        uint32_t const lo = f2u(1.75f), hi = f2u(2.5f);
        b = u2f(lo + r.next() % (hi - lo + 1u));
        return true;
    }
};
// every significand of the binades 2^-20 .. 2^0 x each exponent y in list[0 .. n_list)
struct FamPowGrid
{
    __host__ __device__ static bool at(const DaParams& p, uint64_t i, float& a, float& b)
    {
        uint64_t const r = i >> 23;
        a = u2f((uint32_t)((int)(r % 21u) - 20 + 127) << 23 | (uint32_t)(i & 0x7FFFFFu));
        b = p.list[(r / 21u) % p.n_list];
        return true;
    }
};
// seeded pairs of powLean's domain: x a positive normal number below 2^127, |y| in [2^-100, 2^20], both signs
struct FamPowPairs
{
    __host__ __device__ static bool at(const DaParams& p, uint64_t i, float& a, float& b)
    {
        Rng r(p.seed, i);
        uint32_t const xlo = f2u(0x1p-126f), xhi = f2u(0x1p127f), ylo = f2u(0x1p-100f), yhi = f2u(0x1p20f);
        a = u2f(xlo + r.next() % (xhi - xlo + 1u));
        b = u2f((ylo + r.next() % (yhi - ylo + 1u)) | (r.next() & 0x80000000u));
        return true;
    }
};

// ---------------------------------------------------------------------------------------------------------------------------
// Comparisons
// ---------------------------------------------------------------------------------------------------------------------------
struct Outcome
{
    float got;
    double want;
    double err;
    bool bad;
};
// THE error rule of the suite (tests/test_fpmath.py ulp_error): |got - want| in units of the last place of the binary32
// binade that holds the float64 value `want`, the binade taken no lower than 2^-126 - so a denormal or zero result is measured
// in units of 2^-149. A reference that is infinite or NaN in binary32 must be met exactly (any NaN for a NaN); a got that
// is NaN or infinite where the reference is finite is an infinite error.
__device__ inline Outcome ulpCompare(float got, double want, double bound)
{
    float const wf = (float)want;
    if (want != want || __builtin_isinf(wf))
    {
        bool const ok = (want != want) ? (got != got) : (f2u(got) == f2u(wf));
        return Outcome{got, want, ok ? 0.0 : __builtin_inf(), !ok};
    }
    double const w = __builtin_fabs(want) > 0x1p-126 ? __builtin_fabs(want) : 0x1p-126;
    int const e = (int)((d2u(w) >> 52) & 0x7FFu) - 1023;
    double const d = __builtin_fabs((double)got - want);
    double const err = (d == d) ? d * u2d((uint64_t)(1023 + 23 - e) << 52) : __builtin_inf();
    return Outcome{got, want, err, !(err <= bound)};
}
// absolute error |got - want| (NaN got: infinite)
__device__ inline Outcome absCompare(float got, double want, double bound)
{
    double const d = __builtin_fabs((double)got - want);
    double const err = (d == d) ? d : __builtin_inf();
    return Outcome{got, want, err, !(err <= bound)};
}
// bit-exact against the binary32 value `want` (RN of the float64 reference); the reported error is the ULP distance
__device__ inline Outcome exactCompare(float got, float want)
{
    Outcome o = ulpCompare(got, (double)want, 0.0);
    o.bad = f2u(got) != f2u(want);
    return o;
}
// bit-exact, any NaN equal to any NaN
__device__ inline Outcome exactNanCompare(float got, float want)
{
    Outcome o = exactCompare(got, want);
    o.bad = o.bad && !(got != got && want != want);
    return o;
}
// bit-exact except the sign of a zero
__device__ inline Outcome zeroSignCompare(float got, float want)
{
    Outcome o = exactCompare(got, want);
    o.bad = o.bad && !(got == 0.0f && want == 0.0f);
    return o;
}
__device__ inline float rnDiv(float a, float b) { return (float)((double)a / (double)b); } // correctly rounded: 53 >= 2*24 + 2
__device__ inline float rnSqrt(float x) { return (float)__builtin_sqrt((double)x); }

// ---------------------------------------------------------------------------------------------------------------------------
// Operations: operands -> outcome
// ---------------------------------------------------------------------------------------------------------------------------
struct OpRcpN
{
    __device__ static Outcome run(float a, float, double) { return exactCompare(szg::rcpN(a), rnDiv(1.0f, a)); }
};
struct OpSqrtN // NaN -> NaN
{
    __device__ static Outcome run(float a, float, double) { return exactNanCompare(szg::sqrtN(a), rnSqrt(a)); }
};
struct OpSqrtP
{
    __device__ static Outcome run(float a, float, double) { return exactCompare(szg::sqrtP(a), rnSqrt(a)); }
};
// divN == RN(a / b) bit for bit; divN0 == RN(a / b) but for the sign of a zero; divR(a, b, rcpN(b)) == divN
struct OpDiv
{
    __device__ static Outcome run(float a, float b, double)
    {
        float const want = rnDiv(a, b);
        float const y = szg::rcpN(b);
        Outcome const n = exactCompare(szg::divN(a, b), want);
        Outcome const n0 = zeroSignCompare(szg::divN0(a, b), want);
        Outcome const r = exactCompare(szg::divR(a, b, y), n.got);
        return n.bad ? n : n0.bad ? n0 : r.bad ? r : n;
    }
};
// szg_div_moderate as log uses it: n = m - 1, d = m + 1 for the operand m
struct OpModerateLog
{
    __device__ static Outcome run(float m, float, double)
    {
        float const n = m - 1.0f, d = m + 1.0f;
        return exactCompare(szg_div_moderate(n, d), rnDiv(n, d));
    }
};
struct OpModerate
{
    __device__ static Outcome run(float n, float d, double) { return exactCompare(szg_div_moderate(n, d), rnDiv(n, d)); }
};
struct OpExpInner
{
    __device__ static Outcome run(float a, float, double) { return exactCompare(szg::expInner(a), szg_expf_notnan(a)); }
};
// where powLeanOK(x, y) holds (elsewhere: nothing to compare, counted as agreeing)
struct OpPowLean
{
    __device__ static Outcome run(float a, float b, double)
    {
        if (!szg::powLeanOK(a, b))
        {
            return Outcome{0.0f, 0.0, 0.0, false};
        }
        return exactCompare(szg::powLean(a, b), szg_powf(a, b));
    }
};
// the fpmath.h functions (device build) against OCML's float64 functions
template <int F> __device__ inline float fpmath(float x)
{
    switch (F)
    {
    case 0: return szg_expf(x);
    case 2: return szg_sinf(x);
    case 3: return szg_cosf(x);
    case 4: return szg_asinf(x);
    case 5: return szg_acosf(x);
    default: return szg_logf(x);
    }
}
template <int F> __device__ inline double reference(double x)
{
    switch (F)
    {
    case 0: return exp(x);
    case 2: return sin(x);
    case 3: return cos(x);
    case 4: return asin(x);
    case 5: return acos(x);
    default: return log(x);
    }
}
template <int F> struct OpUlp
{
    __device__ static Outcome run(float a, float, double bound) { return ulpCompare(fpmath<F>(a), reference<F>((double)a), bound); }
};
template <int F> struct OpAbs
{
    __device__ static Outcome run(float a, float, double bound) { return absCompare(fpmath<F>(a), reference<F>((double)a), bound); }
};
// UNORM16 store: NaN, negatives -> 0, above 1 -> 65535, on [0, 1] within `bound` of x * 65535 (exact in float64)
struct OpUnorm16
{
    __device__ static Outcome run(float a, float, double bound)
    {
        double const want = !(a > 0.0f) ? 0.0 : a >= 1.0f ? 65535.0 : (double)a * 65535.0;
        return absCompare((float)szg::unorm16(a), want, bound);
    }
};
// monotonic codes: for x >= 0, unorm16(next float above x) >= unorm16(x)
struct OpUnorm16Step
{
    __device__ static Outcome run(float a, float, double)
    {
        unsigned const c0 = szg::unorm16(a), c1 = szg::unorm16(u2f(f2u(a) + 1u));
        return exactCompare(c1 < c0 ? 1.0f : 0.0f, 0.0f);
    }
};

// ---------------------------------------------------------------------------------------------------------------------------
// The sweep kernel and its host loop
// ---------------------------------------------------------------------------------------------------------------------------
template <class Fam, class Op>
__global__ void __launch_bounds__(256) sweepKernel(DaParams p, double bound, unsigned long long first, unsigned n, DaAcc* acc)
{
    unsigned long long cnt = 0, bad = 0, maxBits = 0, maxKey = 0;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        float a, b;
        if (!Fam::at(p, first + i, a, b))
        {
            continue;
        }
        cnt++;
        Outcome const o = Op::run(a, b, bound);
        unsigned long long const eb = d2u(o.err); // a non-negative double: its bits order like its value
        if (eb > maxBits)
        {
            maxBits = eb;
        }
        unsigned long long const key = ((eb >> 32) << 32) | i;
        if (key > maxKey)
        {
            maxKey = key;
        }
        if (o.bad)
        {
            bad++;
            if (__hip_atomic_load(&acc->n_list, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)kList)
            {
                unsigned const slot = atomicAdd(&acc->n_list, 1u);
                if (slot < (unsigned)kList)
                {
                    acc->list_a[slot] = f2u(a);
                    acc->list_b[slot] = f2u(b);
                    acc->list_got[slot] = f2u(o.got);
                    acc->list_want[slot] = f2u((float)o.want);
                }
            }
        }
    }
    atomicAdd(&acc->count, cnt);
    if (bad)
    {
        atomicAdd(&acc->mismatches, bad);
    }
    atomicMax(&acc->max_bits, maxBits);
    atomicMax(&acc->max_key, maxKey);
}

template <class Fam, class Op>
int runSweep(uint64_t first, uint64_t count, const DaParams& p, double bound, DaResult* out)
{
    std::memset(out, 0, sizeof(*out));
    DaAcc* d = nullptr;
    hipError_t st = hipMalloc(&d, sizeof(DaAcc));
    if (st != hipSuccess)
    {
        return (int)st;
    }
    DaAcc h;
    bool located = false;
    for (uint64_t done = 0; done < count && st == hipSuccess;)
    {
        unsigned const n = (unsigned)((count - done) < kMaxLaunch ? (count - done) : kMaxLaunch);
        st = hipMemset(d, 0, sizeof(DaAcc));
        if (st != hipSuccess)
        {
            break;
        }
        sweepKernel<Fam, Op><<<2048, 256>>>(p, bound, first + done, n, d);
        st = hipGetLastError();
        if (st == hipSuccess)
        {
            st = hipDeviceSynchronize();
        }
        if (st == hipSuccess)
        {
            st = hipMemcpy(&h, d, sizeof(DaAcc), hipMemcpyDeviceToHost);
        }
        if (st != hipSuccess)
        {
            break;
        }
        out->count += h.count;
        out->mismatches += h.mismatches;
        double const e = u2d(h.max_bits);
        if (h.count != 0 && (!located || e > out->max_err))
        {
            located = true;
            float a = 0.0f, b = 0.0f;
            Fam::at(p, first + done + (h.max_key & 0xFFFFFFFFull), a, b);
            out->max_err = e;
            out->max_a = f2u(a);
            out->max_b = f2u(b);
        }
        for (unsigned k = 0; k < h.n_list && k < (unsigned)kList && out->n_list < (unsigned)kList; k++, out->n_list++)
        {
            out->list_a[out->n_list] = h.list_a[k];
            out->list_b[out->n_list] = h.list_b[k];
            out->list_got[out->n_list] = h.list_got[k];
            out->list_want[out->n_list] = h.list_want[k];
        }
        done += n;
    }
    (void)hipFree(d);
    return (int)st;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Evaluation on given inputs (function numbers of oracle_builtin_eval, plus 7 = powLean)
// ---------------------------------------------------------------------------------------------------------------------------
template <int F> __global__ void __launch_bounds__(256) evalKernel(const float* x, const float* y, float* out, unsigned n)
{
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        out[i] = F == 1 ? szg_powf(x[i], y[i]) : F == 7 ? szg::powLean(x[i], y[i]) : fpmath<F>(x[i]);
    }
}
// unpack_half4 of the codes 4g .. 4g+3 (low halves first) -> out[4g .. 4g+3]
__global__ void __launch_bounds__(256) unpackHalfKernel(const uint32_t* codes, float* out, unsigned groups)
{
    for (unsigned g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x)
    {
        uint2 const v = make_uint2((codes[4 * g] & 0xFFFFu) | (codes[4 * g + 1] << 16), (codes[4 * g + 2] & 0xFFFFu) | (codes[4 * g + 3] << 16));
        szg::V4 const r = szg::unpack_half4(v);
        out[4 * g] = r.x;
        out[4 * g + 1] = r.y;
        out[4 * g + 2] = r.z;
        out[4 * g + 3] = r.w;
    }
}
// pack_half4(x[2g] * y[2g], 0, x[2g+1] * y[2g+1], 1) -> out[2g], out[2g+1]: fp32 products formed in the kernel feed the
// conversion, next to constants - the shape in which, without the guard in pack_half4, hipcc folds product and conversion into
// one v_fma_mixlo_f16 (one rounding of the exact product)
__global__ void __launch_bounds__(256) packHalfMulKernel(const float* x, const float* y, uint2* out, unsigned pairs)
{
    for (unsigned g = blockIdx.x * blockDim.x + threadIdx.x; g < pairs; g += gridDim.x * blockDim.x)
    {
        out[g] = szg::pack_half4(x[2 * g] * y[2 * g], 0.0f, x[2 * g + 1] * y[2 * g + 1], 1.0f);
    }
}
// pack_half4 of the bit patterns lo + 4g .. lo + 4g + 3
__global__ void __launch_bounds__(256) packHalfRangeKernel(uint32_t lo, uint16_t* out, unsigned groups)
{
    for (unsigned g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x)
    {
        uint32_t const b = lo + 4u * g;
        uint2 const o = szg::pack_half4(u2f(b), u2f(b + 1u), u2f(b + 2u), u2f(b + 3u));
        out[4 * g] = (uint16_t)o.x;
        out[4 * g + 1] = (uint16_t)(o.x >> 16);
        out[4 * g + 2] = (uint16_t)o.y;
        out[4 * g + 3] = (uint16_t)(o.y >> 16);
    }
}

// device buffers of one evaluation call, freed on every path
struct Buffers
{
    void* p[3] = {nullptr, nullptr, nullptr};
    ~Buffers()
    {
        for (void* q : p)
        {
            (void)hipFree(q);
        }
    }
};
int finish(hipError_t st)
{
    if (st == hipSuccess)
    {
        st = hipGetLastError();
    }
    if (st == hipSuccess)
    {
        st = hipDeviceSynchronize();
    }
    return (int)st;
}
} // namespace

extern "C" {
// One sweep (see the top of the file); returns 0 or the HIP error code, -1 for an unknown name.
int szg_da_sweep(const char* name, uint64_t first, uint64_t count, const DaParams* p, double bound, DaResult* out)
{
    struct Entry
    {
        const char* name;
        int (*run)(uint64_t, uint64_t, const DaParams&, double, DaResult*);
    };
    static const Entry table[] = {
        {"rcpN", runSweep<FamBits, OpRcpN>},
        {"sqrtN", runSweep<FamBits, OpSqrtN>},
        {"sqrtP", runSweep<FamBits, OpSqrtP>},
        {"div_significands", runSweep<FamSignificands, OpDiv>},
        {"div_pairs", runSweep<FamDivPairs, OpDiv>},
        {"moderate_log", runSweep<FamBits, OpModerateLog>},
        {"moderate_pairs", runSweep<FamModerate, OpModerate>},
        {"expInner", runSweep<FamBits, OpExpInner>},
        {"powLean_grid", runSweep<FamPowGrid, OpPowLean>},
        {"powLean_pairs", runSweep<FamPowPairs, OpPowLean>},
        {"expf", runSweep<FamBits, OpUlp<0>>},
        {"sinf", runSweep<FamBits, OpUlp<2>>},
        {"cosf", runSweep<FamBits, OpUlp<3>>},
        {"asinf", runSweep<FamBits, OpUlp<4>>},
        {"acosf", runSweep<FamBits, OpUlp<5>>},
        {"logf", runSweep<FamBits, OpUlp<6>>},
        {"sinf_abs", runSweep<FamBits, OpAbs<2>>},
        {"cosf_abs", runSweep<FamBits, OpAbs<3>>},
        {"unorm16", runSweep<FamBits, OpUnorm16>},
        {"unorm16_step", runSweep<FamBits, OpUnorm16Step>},
    };
    for (const Entry& e : table)
    {
        if (std::strcmp(e.name, name) == 0)
        {
            return e.run(first, count, *p, bound, out);
        }
    }
    return -1;
}

// out[i] = function fn (oracle_builtin_eval's numbers; 7 = szg::powLean) of x[i] (, y[i]) on the GPU; host arrays
int szg_da_eval(int fn, const float* x, const float* y, float* out, unsigned n)
{
    Buffers b;
    size_t const bytes = (size_t)n * sizeof(float);
    hipError_t st = hipMalloc(&b.p[0], bytes);
    st = st == hipSuccess ? hipMalloc(&b.p[1], bytes) : st;
    st = st == hipSuccess ? hipMalloc(&b.p[2], bytes) : st;
    st = st == hipSuccess ? hipMemcpy(b.p[0], x, bytes, hipMemcpyHostToDevice) : st;
    st = st == hipSuccess ? hipMemcpy(b.p[1], y, bytes, hipMemcpyHostToDevice) : st;
    if (st != hipSuccess)
    {
        return (int)st;
    }
    const float* dx = (const float*)b.p[0];
    const float* dy = (const float*)b.p[1];
    float* dout = (float*)b.p[2];
    switch (fn)
    {
    case 0: evalKernel<0><<<2048, 256>>>(dx, dy, dout, n); break;
    case 1: evalKernel<1><<<2048, 256>>>(dx, dy, dout, n); break;
    case 2: evalKernel<2><<<2048, 256>>>(dx, dy, dout, n); break;
    case 3: evalKernel<3><<<2048, 256>>>(dx, dy, dout, n); break;
    case 4: evalKernel<4><<<2048, 256>>>(dx, dy, dout, n); break;
    case 5: evalKernel<5><<<2048, 256>>>(dx, dy, dout, n); break;
    case 6: evalKernel<6><<<2048, 256>>>(dx, dy, dout, n); break;
    case 7: evalKernel<7><<<2048, 256>>>(dx, dy, dout, n); break;
    default: return -1;
    }
    st = (hipError_t)finish(hipSuccess);
    return (int)(st == hipSuccess ? hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost) : st);
}

// out[i] = unpack_half4 of the 16-bit codes[i], four codes per call (n a multiple of 4); host arrays
int szg_da_unpack_half4(const uint32_t* codes, float* out, unsigned n)
{
    if (n % 4u != 0u)
    {
        return -1;
    }
    Buffers b;
    hipError_t st = hipMalloc(&b.p[0], (size_t)n * 4u);
    st = st == hipSuccess ? hipMalloc(&b.p[1], (size_t)n * 4u) : st;
    st = st == hipSuccess ? hipMemcpy(b.p[0], codes, (size_t)n * 4u, hipMemcpyHostToDevice) : st;
    if (st != hipSuccess)
    {
        return (int)st;
    }
    unpackHalfKernel<<<256, 256>>>((const uint32_t*)b.p[0], (float*)b.p[1], n / 4u);
    st = (hipError_t)finish(hipSuccess);
    return (int)(st == hipSuccess ? hipMemcpy(out, b.p[1], (size_t)n * 4u, hipMemcpyDeviceToHost) : st);
}

// out[i/2] = the two words pack_half4 stores for the fp32 products x[i] * y[i] and x[i+1] * y[i+1] (lanes 0 and 2; lanes 1 and
// 3 hold 0 and 1), formed in the kernel (n even)
int szg_da_pack_half4_mul(const float* x, const float* y, uint32_t* out, unsigned n)
{
    if (n % 2u != 0u)
    {
        return -1;
    }
    Buffers b;
    hipError_t st = hipMalloc(&b.p[0], (size_t)n * 4u);
    st = st == hipSuccess ? hipMalloc(&b.p[1], (size_t)n * 4u) : st;
    st = st == hipSuccess ? hipMalloc(&b.p[2], (size_t)n * 4u) : st;
    st = st == hipSuccess ? hipMemcpy(b.p[0], x, (size_t)n * 4u, hipMemcpyHostToDevice) : st;
    st = st == hipSuccess ? hipMemcpy(b.p[1], y, (size_t)n * 4u, hipMemcpyHostToDevice) : st;
    if (st != hipSuccess)
    {
        return (int)st;
    }
    packHalfMulKernel<<<256, 256>>>((const float*)b.p[0], (const float*)b.p[1], (uint2*)b.p[2], n / 2u);
    st = (hipError_t)finish(hipSuccess);
    return (int)(st == hipSuccess ? hipMemcpy(out, b.p[2], (size_t)n * 4u, hipMemcpyDeviceToHost) : st);
}

// out[i] = the fp16 code pack_half4 stores for the fp32 bit pattern lo + i, i < n (n a multiple of 4, lo + n <= 2^32)
int szg_da_pack_half_range(uint32_t lo, uint32_t n, uint16_t* out)
{
    if (n % 4u != 0u || (uint64_t)lo + n > (1ull << 32))
    {
        return -1;
    }
    Buffers b;
    hipError_t st = hipMalloc(&b.p[0], (size_t)n * 2u);
    if (st != hipSuccess)
    {
        return (int)st;
    }
    packHalfRangeKernel<<<2048, 256>>>(lo, (uint16_t*)b.p[0], n / 4u);
    st = (hipError_t)finish(hipSuccess);
    return (int)(st == hipSuccess ? hipMemcpy(out, b.p[0], (size_t)n * 2u, hipMemcpyDeviceToHost) : st);
}
} // extern "C"
