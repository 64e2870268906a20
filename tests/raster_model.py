"""Exact model of the mesh rasteriser's rules (include/szg/raster.h "coverage", "facing", "depth"), written from the
header: plain Python integers and numpy, no fp32 edge function anywhere.

Every fp32 value is a dyadic rational. The model takes the three fp32 clip positions of one primitive, forms the header's
h = ((x_c + w_c) * W/2, (y_c + w_c) * H/2, w_c) with the two fp32 operations the header names, scales the nine h values by
one common power of two into Python integers, and from there everything is exact:

    a_i = hy_j hw_k - hy_k hw_j,  b_i = hx_k hw_j - hx_j hw_k,  c_i = hx_j hy_k - hx_k hy_j      (integers)
    2 E_i(x, y) = a_i (2x + 1) + b_i (2y + 1) + 2 c_i                                             (pixel centre x + .5)
    det = hx_0 a_0 + hy_0 b_0 + hw_0 c_0

Vectorisation: the integers have up to ~100 bits (more when the vertices' exponents differ), so E is first evaluated over
the grid in float64 from the correctly rounded coefficients. That value is wrong by at most 2^-51 (|a| px + |b| py + |c|)
(one rounding per coefficient, four in the evaluation; M below); where |E64| exceeds 2^-49 of that sum its sign is certain.
Only the remaining pixels — the ones on or next to an edge line — are evaluated with Python integers (object dtype).

The rule's own rounding budget (kernels_raster.hip: "|error of e_i| <= 2^-22 (A px + B py + C)", A, B, C the sums of the
magnitudes of the products the coefficients are made of) labels every pixel surely in / surely out / undecided: a test that
compares fp32 coverage with this model may only insist where the exact value is outside the budget.

Two cameras make the clip coordinates of ANY finite fp32 vertex exactly known, so no vertex stage is imitated:
    exact_perspective_camera(): projection [[1,0,0,0],[0,1,0,0],[0,0,0,1/4],[0,0,1,0]], identity view / model:
        clip = (x, y, 1/4, z) — every product is by 0, 1 or 1/4 and every sum adds zeros; depth clip means z >= 1/4;
    the identity matrix (shadow pass light matrix, or the G-buffer pass with w = 1): clip = (x, y, z, 1).
"""
from fractions import Fraction

import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------
# cameras with exactly known clip coordinates
# ---------------------------------------------------------------------------
EXACT_PROJECTION = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0.25], [0, 0, 1, 0]], np.float32)  # row-major, as written


def clip_exact_perspective(positions):
    """[N, 3] fp32 positions -> [N, 4] clip coordinates under EXACT_PROJECTION with identity view and model."""
    p = np.asarray(positions, np.float32).reshape(-1, 3)
    out = np.empty((len(p), 4), np.float32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = p[:, 0], p[:, 1], F32(0.25), p[:, 2]
    return out


def clip_identity(positions):
    p = np.asarray(positions, np.float32).reshape(-1, 3)
    out = np.ones((len(p), 4), np.float32)
    out[:, :3] = p
    return out


# ---------------------------------------------------------------------------
# exact integers
# ---------------------------------------------------------------------------
def _to_ints(values):
    """fp32 array -> (list of Python ints n_i, exponent e) with value_i = n_i * 2^e exactly."""
    v = np.asarray(values, np.float64).reshape(-1)
    assert np.isfinite(v).all()
    m, ex = np.frexp(v)  # v = m * 2^ex, |m| in [.5, 1)
    mant = [int(np.ldexp(mi, 24)) for mi in m]  # fp32: 24 bits
    exps = [int(e) - 24 for e in ex]
    nz = [e for n, e in zip(mant, exps) if n != 0]
    e0 = min(nz) if nz else 0
    return [n << (e - e0) if n != 0 else 0 for n, e in zip(mant, exps)], e0


def _sign(n):
    return (n > 0) - (n < 0)


class Primitive:
    """One assembled primitive under the header's rules, exact. `clip`: [3, 4] fp32."""

    def __init__(self, clip, W, H):
        clip = np.asarray(clip, np.float32).reshape(3, 4)
        self.W, self.H = int(W), int(H)
        self.clip = clip
        with np.errstate(all="ignore"):
            hx = (clip[:, 0] + clip[:, 3]) * (F32(W) * F32(0.5))
            hy = (clip[:, 1] + clip[:, 3]) * (F32(H) * F32(0.5))
        hw = clip[:, 3].copy()
        self.h = np.stack([hx, hy, hw], 1).astype(np.float32)  # [vertex, (x, y, w)]
        ints, self.h_exp = _to_ints(self.h)
        X, Y, Wc = ints[0::3], ints[1::3], ints[2::3]
        self.a, self.b, self.c, self.A, self.B, self.C = [], [], [], [], [], []
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            self.a.append(Y[j] * Wc[k] - Y[k] * Wc[j])
            self.b.append(X[k] * Wc[j] - X[j] * Wc[k])
            self.c.append(X[j] * Y[k] - X[k] * Y[j])
            self.A.append(abs(Y[j] * Wc[k]) + abs(Y[k] * Wc[j]))
            self.B.append(abs(X[k] * Wc[j]) + abs(X[j] * Wc[k]))
            self.C.append(abs(X[j] * Y[k]) + abs(X[k] * Y[j]))
        self.det = X[0] * self.a[0] + Y[0] * self.b[0] + Wc[0] * self.c[0]
        # budget of the fp32 determinant, same accounting as for the edges: 5 roundings on every product of three
        self.det_budget = Fraction(abs(X[0]) * self.A[0] + abs(Y[0]) * self.B[0] + abs(Wc[0]) * self.C[0], 1 << 22)
        self.facing = _sign(self.det)  # +1: clockwise in framebuffer space = front (raster.h "facing")
        # clip z, w as integers on one scale of their own
        zw, self.zw_exp = _to_ints(np.concatenate([clip[:, 2], clip[:, 3]]))
        self.z, self.w = zw[:3], zw[3:]

    # -- per-pixel quantities over the grid xs x ys (integer pixel indices) --------------------------------------
    def edge_signs(self, xs=None, ys=None):
        """int8 [3, len(ys), len(xs)]: the exact sign of facing * E_i at every pixel centre."""
        xs = np.arange(self.W) if xs is None else np.asarray(xs)
        ys = np.arange(self.H) if ys is None else np.asarray(ys)
        px = (2 * xs + 1).astype(np.float64)[None, :]
        py = (2 * ys + 1).astype(np.float64)[:, None]
        out = np.empty((3, len(ys), len(xs)), np.int8)
        for i in range(3):
            a, b, c2 = self.a[i], self.b[i], 2 * self.c[i]
            with np.errstate(over="raise"):
                E = (float(a) * px + float(b) * py) + float(c2)
                M = (abs(float(a)) * px + abs(float(b)) * py) + abs(float(c2))
            s = np.sign(E).astype(np.int8)
            unsure = ~(np.abs(E) > M * 2.0 ** -49)
            if unsure.any():
                iy, ix = np.nonzero(unsure)
                ex = a * (2 * xs[ix].astype(object) + 1) + b * (2 * ys[iy].astype(object) + 1) + c2
                s[iy, ix] = [_sign(int(v)) for v in ex]
            out[i] = s * self.facing
        return out

    def tie_break(self):
        """Per edge: does a pixel centre exactly ON the edge belong to this primitive? Left edge (s a_i > 0), else top edge
        (a_i == 0 and s b_i > 0) — the header's top-left rule, with the exact signs of a_i and b_i."""
        return [self.facing * _sign(self.a[i]) > 0 or (self.a[i] == 0 and self.facing * _sign(self.b[i]) > 0) for i in range(3)]

    def inside(self, xs=None, ys=None):
        """bool [len(ys), len(xs)]: the header's coverage rule, exact (no depth clip)."""
        if self.facing == 0:
            xs = np.arange(self.W) if xs is None else xs
            ys = np.arange(self.H) if ys is None else ys
            return np.zeros((len(ys), len(xs)), bool)
        s = self.edge_signs(xs, ys)
        owns = self.tie_break()
        ok = np.ones(s.shape[1:], bool)
        for i in range(3):
            ok &= (s[i] > 0) | ((s[i] == 0) & owns[i])
        return ok

    def _grid_f64(self, xs, ys):
        xs = np.arange(self.W) if xs is None else np.asarray(xs)
        ys = np.arange(self.H) if ys is None else np.asarray(ys)
        return (2 * xs + 1).astype(np.float64)[None, :], (2 * ys + 1).astype(np.float64)[:, None]

    def edges_f64(self, xs=None, ys=None):
        """float64 [3, h, w]: facing * 2 E_i in units of 2^(2 h_exp) (relative error <= 2^-49 of `magnitudes`), and the
        rule's rounding budget 2 * 2^-22 (A px + B py + C) in the same units."""
        px, py = self._grid_f64(xs, ys)
        E = np.stack([(float(self.a[i]) * px + float(self.b[i]) * py) + float(2 * self.c[i]) for i in range(3)]) * self.facing
        budget = np.stack([(float(self.A[i]) * px + float(self.B[i]) * py) + float(2 * self.C[i]) for i in range(3)]) * 2.0 ** -22
        return E, budget

    def classify(self, xs=None, ys=None):
        """(surely_in, surely_out, undecided) bool [h, w] for COVERAGE: every |E_i| compared with its budget. The float64
        values carry a relative error of 2^-49 of the budget's own sum, 2^-27 of the budget: the comparison uses a margin
        of 2^-20 of the budget on the safe side (a pixel that close to the band's border is called undecided)."""
        E, budget = self.edges_f64(xs, ys)
        if self.facing == 0:
            z = np.zeros(E.shape[1:], bool)
            return z, z.copy(), ~z
        hi = budget * (1.0 + 2.0 ** -20)
        surely_in = (E > hi).all(0)
        surely_out = (E < -hi).any(0)
        return surely_in, surely_out, ~(surely_in | surely_out)

    def depth_clip(self, xs=None, ys=None):
        """(inside_volume, clearly) bool [h, w]: 0 <= z <= w with z = sum E_i z_i, w = sum E_i w_i (signs by facing, so the
        sums are positive inside), in float64; `clearly` = by more than the fp32 evaluation can lose: the edge budgets
        carried through the sums plus three roundings of 2^-24 on every term."""
        E, budget = self.edges_f64(xs, ys)
        z = [float(v) for v in self.z]
        w = [float(v) for v in self.w]
        zc = sum(E[i] * z[i] for i in range(3))
        wc = sum(E[i] * w[i] for i in range(3))
        slack_z = sum((budget[i] + np.abs(E[i]) * 2.0 ** -22) * abs(z[i]) for i in range(3))
        slack_w = sum((budget[i] + np.abs(E[i]) * 2.0 ** -22) * abs(w[i]) for i in range(3))
        ok = (zc >= 0) & (zc <= wc) & (wc > 0)
        clearly = (zc > slack_z) & (wc - zc > slack_z + slack_w) & (wc > slack_w)
        clearly_not = (zc < -slack_z) | (zc - wc > slack_z + slack_w) | (wc < -slack_w)
        return ok, clearly, clearly_not

    def depth_with_bound(self, xs=None, ys=None):
        """(depth, bound) float64 [h, w]: the exact quotient sum E_i z_i / sum E_i w_i and how far the header's fp32 evaluation
        order can be from it, derived term by term: |e_i - E_i| <= budget_i carried through both sums; every product and each of
        the two additions of a sum rounds by 2^-24 of its result (3 * 2^-24 of the sum of magnitudes); the quotient of two
        uncertain numbers n +- dn, d +- dd lies within (dn |d| + dd |n|) / (|d| (|d| - dd)); the division rounds by 2^-24 of the
        quotient (+ 2^-149 in the denormal range). inf where the denominator's uncertainty reaches the denominator. The float64
        evaluation of these formulas is itself good to 2^-45: the bound is widened by that much of the depth."""
        E, budget = self.edges_f64(xs, ys)
        z = [float(v) for v in self.z]
        w = [float(v) for v in self.w]
        u = 2.0 ** -24
        mag = np.abs(E) + budget
        n = sum(E[i] * z[i] for i in range(3))
        d = sum(E[i] * w[i] for i in range(3))
        dn = sum(budget[i] * abs(z[i]) for i in range(3)) + 3 * u * sum(mag[i] * abs(z[i]) for i in range(3))
        dd = sum(budget[i] * abs(w[i]) for i in range(3)) + 3 * u * sum(mag[i] * abs(w[i]) for i in range(3))
        with np.errstate(all="ignore"):
            q = n / d
            bound = (dn * np.abs(d) + dd * np.abs(n)) / (np.abs(d) * (np.abs(d) - dd))
            bound = bound + u * (np.abs(q) + bound) + 2.0 ** -149 + 2.0 ** -45 * np.abs(q)
            bound = np.where(np.abs(d) > dd, bound, np.inf)
        return q, bound

    def attribute_with_bound(self, values, xs=None, ys=None):
        """(value, bound) for the header's attribute formula sum (e_i / S) v_i, S = (e_0 + e_1) + e_2, against the exact
        sum E_i v_i / sum E_i: S is off by the three budgets and two roundings, each weight by the quotient rule above and its
        own rounding, the three products and two additions by 3 * 2^-24 of the sum of magnitudes."""
        E, budget = self.edges_f64(xs, ys)
        v = [float(x) for x in values]
        u = 2.0 ** -24
        mag = np.abs(E) + budget
        S = E[0] + E[1] + E[2]
        dS = budget.sum(0) + 2 * u * mag.sum(0)
        with np.errstate(all="ignore"):
            exact = sum(E[i] * v[i] for i in range(3)) / S
            bound = np.zeros_like(S)
            lsum = np.zeros_like(S)
            for i in range(3):
                li = np.abs(E[i] / S)
                dl = (budget[i] * np.abs(S) + dS * np.abs(E[i])) / (np.abs(S) * (np.abs(S) - dS))
                dl = dl + u * (li + dl)
                bound += dl * abs(v[i])
                lsum += (li + dl) * abs(v[i])
            bound = bound + 3 * u * lsum + 2.0 ** -45 * np.abs(exact)
            bound = np.where(np.abs(S) > dS, bound, np.inf)
        return exact, bound

    def fits_fp32_everywhere(self, x, y):
        """True when every intermediate of the header's fp32 evaluation of e_i, sum e_i z_i and sum e_i w_i at pixel (x, y) is
        exactly representable (24 significant bits; the lattice scenes stay far from the exponent limits), so that the depth
        is ONE correctly rounded division of exact operands."""
        def fits(n):
            n = abs(int(n))
            return n == 0 or (n // (n & -n)).bit_length() <= 24

        ok = True
        zs, ws = [], []
        for i in range(3):
            t0, t1, c2 = self.a[i] * (2 * x + 1), self.b[i] * (2 * y + 1), 2 * self.c[i]
            e = t0 + t1 + c2
            ok = ok and all(fits(n) for n in (self.a[i], self.b[i], self.c[i], t0, t1, t0 + t1, e, e * self.z[i], e * self.w[i]))
            zs.append(e * self.z[i])
            ws.append(e * self.w[i])
        return ok and all(fits(n) for n in (zs[0] + zs[1], sum(zs), ws[0] + ws[1], sum(ws)))

    def depth_f64(self, xs=None, ys=None):
        """sum E_i z_i / sum E_i w_i in float64 (exact up to ~2^-48 relative where no cancellation occurs)."""
        E, _ = self.edges_f64(xs, ys)
        with np.errstate(all="ignore"):
            return sum(E[i] * float(self.z[i]) for i in range(3)) / sum(E[i] * float(self.w[i]) for i in range(3))

    def depth_exact(self, x, y):
        """The exact quotient at one pixel, a Fraction."""
        e = [self.a[i] * (2 * x + 1) + self.b[i] * (2 * y + 1) + 2 * self.c[i] for i in range(3)]
        num = sum(e[i] * self.z[i] for i in range(3))
        den = sum(e[i] * self.w[i] for i in range(3))
        return Fraction(num, den)

    def attribute_exact(self, x, y, values):
        """Perspective-correct attribute sum E_i v_i / sum E_i at one pixel, a Fraction (`values`: three fp32)."""
        e = [self.a[i] * (2 * x + 1) + self.b[i] * (2 * y + 1) + 2 * self.c[i] for i in range(3)]
        return sum(e[i] * Fraction(float(values[i])) for i in range(3)) / sum(e)


def round_to_f32(q):
    """Correctly rounded (nearest even) fp32 of a Fraction in the normal range."""
    if q == 0:
        return F32(0.0)
    s = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    scaled = q / Fraction(2) ** (e - 23)  # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    r = scaled - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and (n & 1)):
        n += 1
    return F32(s * float(n) * 2.0 ** (e - 23))


def triangles_of(clip, indices, W, H):
    """Primitives of an indexed triangle list over [N, 4] clip positions."""
    idx = np.asarray(indices).reshape(-1, 3)
    return [Primitive(clip[t], W, H) for t in idx]
