"""The device arithmetic itself, on the GPU, over whole domains (tests/cpp/devarith.hip, built with the product's HIPFLAGS).

The parity tests compare kernels with the oracle bit for bit, but both share include/szg/fpmath.h, and the kernels take the
lean operators of szg_device.hpp only on operands the test scenes produce. Here every claim those files make is checked
directly against float64 references computed on the GPU: the lean operators (rcpN, divN / divN0 / divR, sqrtN / sqrtP,
szg_div_moderate's device branch, expInner, powLean) exhaustively or on structured and seeded operand families, the fpmath.h
functions on every binary32 input of their documented ranges (the ULP rule of tests/test_fpmath.py), the device build against
the host build on a stratified sample, and the store formats (UNORM16, fp16) on every input. Each sweep prints what it
evaluated, its mismatches, its largest error with the operands where it occurs, and its seconds."""
import ctypes as C
import time

import numpy as np
import pytest

from oracle import binding as ob
from tests import native
from tests.test_fpmath import check_special_values, ulp_error

pytestmark = pytest.mark.gpu
LAUNCH = 1 << 30  # one launch of the library covers at most this many indices; a sweep loops over launches

PI = float(np.float32(np.pi))
PI_2 = float(np.float32(np.pi / 2))
PI3_2 = float(np.float32(3 * np.pi / 2))


class Params(C.Structure):
    _fields_ = [("lo", C.c_uint32), ("family", C.c_uint32), ("seed", C.c_uint64), ("n_list", C.c_uint32), ("list", C.c_float * 128)]


class Result(C.Structure):
    _fields_ = [("count", C.c_uint64), ("mismatches", C.c_uint64), ("max_err", C.c_double), ("max_a", C.c_uint32),
                ("max_b", C.c_uint32), ("n_list", C.c_uint32), ("list_a", C.c_uint32 * 16), ("list_b", C.c_uint32 * 16),
                ("list_got", C.c_uint32 * 16), ("list_want", C.c_uint32 * 16)]


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        h = C.CDLL(native.build("cpp/libszg_devarith.so"))
        h.szg_da_sweep.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(Params), C.c_double, C.POINTER(Result)]
        h.szg_da_eval.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
        h.szg_da_unpack_half4.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
        h.szg_da_pack_half4_mul.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
        h.szg_da_pack_half_range.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        _LIB = h
    return _LIB


def bits(x):
    return int(np.array(x, np.float32).view(np.uint32))


def f(b):
    return float(np.array(b, np.uint32).view(np.float32))


def hexf(b):
    return float.hex(f(b))


def interval(lo, hi):
    """The binary32 values of [lo, hi] (both ends rounded to binary32) as bit ranges (first, count); -0 belongs to the
    negative part, +0 to the positive one."""
    lo, hi = np.float32(lo), np.float32(hi)
    parts = []
    if hi >= 0:
        start = bits(lo) if lo > 0 else 0
        parts.append((start, bits(hi) - start + 1))
    if lo < 0 or (lo == 0 and np.signbit(lo)):
        start = bits(hi) if hi < 0 else 0x80000000
        parts.append((start, bits(lo) - start + 1))
    return parts


class Sweep:
    """Totals of one or more szg_da_sweep calls."""

    def __init__(self, title):
        self.title, self.count, self.mismatches, self.max_err, self.at, self.bad, self.seconds = title, 0, 0, 0.0, None, [], 0.0

    def run(self, name, first, count, bound=0.0, lo=0, family=0, seed=0, values=()):
        p = Params(lo=lo, family=family, seed=seed, n_list=len(values))
        for i, v in enumerate(values):
            p.list[i] = v
        r = Result()
        t0 = time.perf_counter()
        status = lib().szg_da_sweep(name.encode(), first, count, C.byref(p), bound, C.byref(r))
        self.seconds += time.perf_counter() - t0
        assert status == 0, f"{name}: HIP status {status}"
        self.count += r.count
        self.mismatches += r.mismatches
        if self.at is None or r.max_err > self.max_err:
            self.max_err, self.at = r.max_err, (r.max_a, r.max_b)
        for k in range(min(r.n_list, 16)):
            self.bad.append((r.list_a[k], r.list_b[k], r.list_got[k], r.list_want[k]))
        return self

    def bits_range(self, name, lo, hi, bound=0.0):
        for first, count in interval(lo, hi):
            self.run(name, 0, count, bound, lo=first)
        return self

    def report(self):
        a, b = self.at or (0, 0)
        print(f"\n{self.title}: {self.count} values, {self.mismatches} mismatches, max error {self.max_err:.4g} at a={hexf(a)} "
              f"b={hexf(b)}, {self.seconds:.2f} s")
        for a, b, got, want in self.bad[:16]:
            print(f"    a={hexf(a)} b={hexf(b)} got {got:08x} ({hexf(got)}) want {want:08x} ({hexf(want)})")
        return self

    def exact(self):
        self.report()
        assert self.count > 0 and self.mismatches == 0
        assert self.max_err == 0.0


def evaluate(fn, x, y=None):
    """Function `fn` (oracle_builtin_eval's numbers; 7 = powLean) of x (, y) evaluated on the GPU."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(np.zeros_like(x) if y is None else y, np.float32)
    out = np.empty_like(x)
    assert lib().szg_da_eval(fn, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size) == 0
    return out


def same_bits_or_nan(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------------------
# Lean operators of szg_device.hpp
# ---------------------------------------------------------------------------------------------------------------------------
def test_rcpN_every_denominator_of_the_domain():
    """rcpN(b) == RN(1 / b) for every b with |b| in [2^-60, 2^60], both signs."""
    s = Sweep("rcpN, |b| in [2^-60, 2^60]")
    s.bits_range("rcpN", 2.0 ** -60, 2.0 ** 60).bits_range("rcpN", -(2.0 ** 60), -(2.0 ** -60))
    assert s.count == 2 * (120 * 2 ** 23 + 1)
    s.exact()


def test_sqrtN_sqrtP_every_input_of_the_domain():
    """sqrtN == RN(sqrt x) for +0 and every x in [2^-96, FLT_MAX], NaN -> NaN; sqrtP the same without 0."""
    big = float(np.finfo(np.float32).max)
    s = Sweep("sqrtN, {+0} and [2^-96, FLT_MAX]").run("sqrtN", 0, 1, lo=0).bits_range("sqrtN", 2.0 ** -96, big)
    s.exact()
    n = Sweep("sqrtN, every NaN")
    for lo in (0x7F800001, 0xFF800001):
        n.run("sqrtN", 0, 0x7FFFFF, lo=lo)
    n.report()
    assert n.count == 2 * 0x7FFFFF and n.mismatches == 0
    Sweep("sqrtP, [2^-96, FLT_MAX]").bits_range("sqrtP", 2.0 ** -96, big).exact()


ALL_ONES = [f(((e + 127) << 23) | 0x7FFFFF) for e in range(-60, 60)]


def _random_denominators(n, seed):
    rng = np.random.default_rng(seed)
    e = rng.integers(-60, 60, n)
    m = rng.integers(0, 1 << 23, n)
    s = rng.integers(0, 2, n)
    return [f((int(si) << 31) | ((int(ei) + 127) << 23) | int(mi)) for si, ei, mi in zip(s, e, m)]


@pytest.mark.parametrize("kind", ["all-ones", "random"])
def test_divN_divN0_divR_every_numerator_significand(kind):
    """divN == RN(a / b) bit for bit, divN0 but for the sign of a zero, divR(a, b, rcpN(b)) == divN: every numerator
    significand, both signs, 5 numerator exponents around the denominator's, against the 120 denominators 1.1...1 * 2^e of
    the domain (Markstein's exception class) or 64 seeded random ones."""
    dens = ALL_ONES if kind == "all-ones" else _random_denominators(64, 0xD1F)
    assert len(dens) == (120 if kind == "all-ones" else 64)
    s = Sweep(f"divN / divN0 / divR, {len(dens)} {kind} denominators x every numerator significand")
    total = (1 << 24) * 5 * len(dens)
    for first in range(0, total, LAUNCH):
        s.run("div_significands", first, min(LAUNCH, total - first), values=dens)
    s.exact()


@pytest.mark.parametrize("family,name", [(0, "random"), (1, "quotient next to +-1"), (2, "denominator tails 1..1 / 0..0"),
                                         (3, "exact multiples"), (4, "zero numerators")])
def test_divN_divN0_divR_seeded_pairs(family, name):
    """2^30 seeded pairs of each family of tools/verify_div.hip, |a|, |b| in [2^-60, 2^60] (a = +-0 in family 4)."""
    Sweep(f"divN / divN0 / divR, 2^30 pairs: {name}").run("div_pairs", 0, LAUNCH, family=family, seed=0x5EED).exact()


def test_div_moderate_device_branch():
    """szg_div_moderate (v_rcp_f32, Newton, one residual correction) == RN(n / d): every m in [0.75, 1.5) as log uses it
    (n = m - 1, d = m + 1), and 2^30 seeded pairs of the declared domain (n = +0 or |n| in [2^-60, 0.5), d in [1.75, 2.5]).
    A numerator of -0 is outside it (the quotient comes out +0; `/` gives -0): log's m - 1 is never -0."""
    lo, hi = bits(0.75), bits(1.5)
    Sweep("szg_div_moderate, m - 1 over m + 1, every m in [0.75, 1.5)").run("moderate_log", 0, hi - lo, lo=lo).exact()
    Sweep("szg_div_moderate, 2^30 pairs |n| < 0.5, d in [1.75, 2.5]").run("moderate_pairs", 0, LAUNCH, seed=0xD1A).exact()


def test_expInner_equals_szg_expf_notnan():
    """expInner == szg_expf_notnan bit for bit for every x in [-86, 87]."""
    Sweep("expInner vs szg_expf_notnan, every x in [-86, 87]").bits_range("expInner", -86.0, 87.0).exact()


POW_Y = [5.0, 1.2, 1.5, float(np.float32(1 / 2.2)), float(np.float32(1 / 2.4)), 160.0]


def test_powLean_equals_szg_powf():
    """powLean == szg_powf bit for bit where powLeanOK holds: every x significand of the binades 2^-20 .. 2^0 for each y of
    the path, 160^(1 - t) on a 4097-point grid, 2^28 seeded pairs of the whole precondition."""
    s = Sweep("powLean vs szg_powf, x in [2^-20, 2), y in {5, 1.2, 1.5, 1/2.2, 1/2.4, 160}")
    total = (1 << 23) * 21 * len(POW_Y)
    for first in range(0, total, LAUNCH):
        s.run("powLean_grid", first, min(LAUNCH, total - first), values=POW_Y)
    s.exact()
    Sweep("powLean vs szg_powf, 2^28 pairs of powLeanOK").run("powLean_pairs", 0, 1 << 28, seed=0x90E).exact()
    y = (np.float32(1) - np.arange(4097, dtype=np.float32) / np.float32(4096)).astype(np.float32)
    y = y[y != 0]  # powLeanOK needs |y| >= 2^-100
    x = np.full_like(y, 160.0)
    lean, pow_ = evaluate(7, x, y), evaluate(1, x, y)
    print(f"\npowLean vs szg_powf, 160^(1 - t): {y.size} values, {np.sum(lean.view(np.uint32) != pow_.view(np.uint32))} mismatches")
    assert np.array_equal(lean.view(np.uint32), pow_.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# fpmath.h on the device, every binary32 input, against float64
# ---------------------------------------------------------------------------------------------------------------------------
def _ulp_sweep(name, lo, hi, bound):
    s = Sweep(f"{name} on [{lo:.6g}, {hi:.6g}], bound {bound} ULP").bits_range(name, lo, hi, bound).report()
    assert s.count > 0 and s.mismatches == 0 and s.max_err <= bound
    return s


def test_expf_every_input():
    """szg_expf within 1 ULP on every non-NaN input (denormal results in units of 2^-149); where the correctly rounded
    result overflows (x above 88.72) it returns +inf, below -104 +0."""
    _ulp_sweep("expf", -np.inf, np.inf, 1.0)


def test_logf_every_input():
    _ulp_sweep("logf", 2.0 ** -149, np.inf, 2.85)


@pytest.mark.parametrize("name,lo,hi,bound", [("sinf", -PI, PI, 1.45), ("cosf", -PI, PI, 1.6), ("sinf", -PI_2, PI3_2, 5.8),
                                              ("cosf", -PI_2, PI3_2, 5.8), ("sinf", -10.0, 10.0, 5.8), ("cosf", -10.0, 10.0, 5.8)])
def test_sin_cos_every_input(name, lo, hi, bound):
    """Relative to the ULP of the result, sin and cos lose most next to their zeros (5.79 ULP at cos(0x1.2d97c8p+2) ~ 3pi/2);
    on [-pi, pi] the absolute error stays below 2^-22 (GLSL asks 2^-11)."""
    _ulp_sweep(name, lo, hi, bound)
    if (lo, hi) == (-PI, PI):
        s = Sweep(f"{name} absolute error on [-pi, pi]").bits_range(name + "_abs", lo, hi, 2.0 ** -22).report()
        assert s.mismatches == 0 and s.max_err <= 2.0 ** -22


@pytest.mark.parametrize("name,bound", [("asinf", 2.4), ("acosf", 1.3)])
def test_asin_acos_every_input(name, bound):
    _ulp_sweep(name, -1.0, 1.0, bound)


def test_special_values_on_the_device():
    check_special_values(evaluate)
    log = evaluate(6, np.array([0.0, -0.0, -1.0, np.inf, np.nan, 1.0], np.float32))
    assert log[0] == -np.inf and log[1] == -np.inf and np.isnan(log[2]) and log[3] == np.inf and np.isnan(log[4]) and log[5] == 0


def _around(x, k=1 << 16):
    b = bits(x)
    return np.arange(b - k, b + k + 1, dtype=np.int64).astype(np.uint32).view(np.float32)


def _host_sample(fn):
    """Every 256th binary32 plus the bands where the algorithms change course."""
    parts = [np.arange(0, 1 << 32, 256, dtype=np.uint64).astype(np.uint32).view(np.float32)]
    if fn == 0:
        parts += [_around(-104.0), _around(89.0), np.arange(bits(-87.0), bits(-104.0) + 1, dtype=np.uint32).view(np.float32)]
    elif fn == 6:
        parts += [np.arange(1, 1 << 23, dtype=np.uint32).view(np.float32), np.arange(bits(0.5), bits(2.0) + 1, dtype=np.uint32).view(np.float32)]
    elif fn in (2, 3):
        parts += [_around(8192.0), _around(-8192.0)] + [_around(s * k * np.pi / 2) for k in range(1, 7) for s in (1, -1)]
    else:
        parts += [_around(v) for v in (0.5, -0.5, 1.0, -1.0)]
    return np.concatenate(parts)


@pytest.mark.parametrize("fn,name", [(0, "exp"), (6, "log"), (2, "sin"), (3, "cos"), (4, "asin"), (5, "acos")])
def test_device_build_equals_host_build(fn, name):
    """The device build of fpmath.h (its __HIP_DEVICE_COMPILE__ branches: ldexp in exp, the lean quotient in log) gives the
    host build's bits, any NaN equal to any NaN, on a stratified sample of at least 2^24 inputs."""
    x = _host_sample(fn)
    t0 = time.perf_counter()
    dev, host = evaluate(fn, x), ob.builtin_eval(fn, x)
    same = same_bits_or_nan(dev, host)
    print(f"\n{name}: device vs host build, {x.size} inputs, {np.sum(~same)} differ, {time.perf_counter() - t0:.2f} s")
    assert x.size >= 1 << 24
    assert same.all(), [(float(v).hex(), float(d).hex(), float(h).hex()) for v, d, h in zip(x[~same][:8], dev[~same][:8], host[~same][:8])]


def test_powf_device_build_equals_host_build():
    """szg_powf on the device and on the host: every 256th x of the powLean grid for each y of the path, and 160^(1 - t)."""
    x = (np.arange(0, 21 << 23, 256, dtype=np.uint32) + np.uint32(107 << 23)).view(np.float32)
    xs = np.concatenate([np.tile(x, len(POW_Y)), np.full(4097, 160.0, np.float32)])
    ys = np.concatenate([np.repeat(np.array(POW_Y, np.float32), x.size),
                         (np.float32(1) - np.arange(4097, dtype=np.float32) / np.float32(4096)).astype(np.float32)])
    dev, host = evaluate(1, xs, ys), ob.builtin_eval(1, xs, ys)
    same = same_bits_or_nan(dev, host)
    print(f"\npow: device vs host build, {xs.size} pairs, {np.sum(~same)} differ")
    assert same.all()


# ---------------------------------------------------------------------------------------------------------------------------
# Store formats
# ---------------------------------------------------------------------------------------------------------------------------
def test_unorm16_every_input():
    """NaN, negatives, -inf -> 0; above 1, +inf -> 65535; on [0, 1] |code - x * 65535| <= 0.5 + 2^-8; monotonic."""
    s = Sweep("unorm16, every binary32")
    for first in range(0, 1 << 32, LAUNCH):
        s.run("unorm16", 0, LAUNCH, 0.5 + 2.0 ** -8, lo=first)
    s.report()
    assert s.count == 1 << 32 and s.mismatches == 0 and s.max_err <= 0.5 + 2.0 ** -8
    Sweep("unorm16 never decreases through the floats of [0, 1]").run("unorm16_step", 0, bits(1.0)).exact()


def test_unpack_half4_every_code():
    codes = np.arange(1 << 16, dtype=np.uint32)
    out = np.empty(codes.size, np.float32)
    assert lib().szg_da_unpack_half4(codes.ctypes.data, out.ctypes.data, codes.size) == 0
    want = codes.astype(np.uint16).view(np.float16).astype(np.float32)
    assert same_bits_or_nan(out, want).all()
    assert np.array_equal(np.isnan(out), np.isnan(want))


def _pack_range(lo, n):
    out = np.empty(n, np.uint16)
    assert lib().szg_da_pack_half_range(lo, n, out.ctypes.data) == 0
    return out


def test_pack_half4_every_input_of_the_fp16_range():
    """pack_half4 == numpy's RNE astype(float16) for every binary32 with |x| in [2^-26, 2^17), both signs, in chunks of 2^26,
    plus +-0, +-inf and NaN."""
    t0, n = time.perf_counter(), 0
    for sign in (0, 0x80000000):
        lo, hi = bits(2.0 ** -26) | sign, bits(2.0 ** 17) | sign
        for first in range(lo, hi, 1 << 26):
            count = min(1 << 26, hi - first)
            got = _pack_range(first, count)
            with np.errstate(over="ignore"):  # above 65520 the fp16 value is inf
                want = np.arange(first, first + count, dtype=np.uint32).view(np.float32).astype(np.float16).view(np.uint16)
            assert np.array_equal(got, want), hexf(first + int(np.argmax(got != want)))
            n += count
    for lo in (0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000):
        got = _pack_range(lo, 4).view(np.float16)
        want = np.arange(lo, lo + 4, dtype=np.uint32).view(np.float32).astype(np.float16)
        assert (same_bits_or_nan(got.astype(np.float32), want.astype(np.float32))).all(), hex(lo)
    print(f"\npack_half4: {n} values + 20 specials equal numpy, {time.perf_counter() - t0:.2f} s")


def _tie_pairs(n, seed=0x7E5):
    """Pairs (a, b) whose binary32 product RN32(a * b) lies exactly halfway between two fp16 values while the exact product
    does not, on the side where rounding the exact product once picks the other fp16 neighbour."""
    rng = np.random.default_rng(seed)
    found_a, found_b = [], []
    while sum(len(v) for v in found_a) < n:
        h = rng.integers(0x0001, 0x7BFF, 1 << 16).astype(np.uint16)  # finite positive fp16 codes below the largest
        lo, hi = h.view(np.float16).astype(np.float64), (h + 1).view(np.float16).astype(np.float64)
        tie = ((lo + hi) / 2).astype(np.float32)
        a = (1.0 + rng.random(h.size)).astype(np.float32)
        b = (tie.astype(np.float64) / a).astype(np.float32)
        p32 = a * b
        exact = a.astype(np.float64) * b.astype(np.float64)  # 48 bits: exact in float64
        ok = (p32 == tie) & (exact != tie.astype(np.float64))
        ok &= exact.astype(np.float16).view(np.uint16) != p32.astype(np.float16).view(np.uint16)
        sign = np.where(rng.integers(0, 2, h.size) == 1, np.float32(-1), np.float32(1))
        found_a.append(a[ok] * sign[ok])
        found_b.append(b[ok])
    return np.concatenate(found_a)[:n], np.concatenate(found_b)[:n]


def test_pack_half4_rounds_the_rounded_fp32_product():
    """pack_half4(a * b, ...) with the multiply in the kernel stores RNE16(RN32(a * b)), not the once-rounded exact product
    (the fold the asm guard in pack_half4 prevents: v_fma_mixlo_f16 rounds a * b once)."""
    a, b = _tie_pairs(1 << 14)
    words = np.empty(a.size, np.uint32)  # the two words of one pack_half4 per pair of products
    assert lib().szg_da_pack_half4_mul(a.ctypes.data, b.ctypes.data, words.ctypes.data, a.size) == 0
    got = np.empty(a.size, np.uint16)
    got[0::2], got[1::2] = (words[0::2] & 0xFFFF).astype(np.uint16), (words[1::2] & 0xFFFF).astype(np.uint16)
    twice = (a * b).astype(np.float16).view(np.uint16)
    once = (a.astype(np.float64) * b.astype(np.float64)).astype(np.float16).view(np.uint16)
    assert np.all(twice != once)  # every pair is a case where the two roundings disagree
    assert np.all((words[0::2] >> 16) == 0) and np.all((words[1::2] >> 16) == 0x3C00)
    print(f"\npack_half4 of in-kernel products at fp16 ties: {a.size} pairs, {np.sum(got != twice)} differ from RNE16(RN32(a*b))")
    assert np.array_equal(got, twice)
