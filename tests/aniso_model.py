"""CPU model of include/szg/anisotropy.h "SAMPLER" in numpy float32, one rounding per operation as the header states them, on
top of tests/mipmap_model.py (bilinear, the level shapes, szg_logf on the host).

Shared by tests/test_aniso_model.py (CPU) and the GPU tests, which demand the kernel's bits to equal these."""
import numpy as np

from tests import mipmap_model as mm
from tests.mipmap_model import _log, bilinear, level_shapes  # noqa: F401  (level_shapes: for the callers)

F = np.float32
MAX_ANISOTROPY_REFERENCE = 1.0
MAX_ANISOTROPY_LIMIT = 16.0
LOG2E = F(1.44269504)


def footprint(w, h, duvdx, duvdy):
    """px2, py2, r2, s2 of the header: [n] float32 each."""
    duvdx, duvdy = np.asarray(duvdx, F), np.asarray(duvdy, F)
    with np.errstate(all="ignore"):
        mux, mvx = duvdx[:, 0] * F(w), duvdx[:, 1] * F(h)
        muy, mvy = duvdy[:, 0] * F(w), duvdy[:, 1] * F(h)
        px2 = (mux * mux + mvx * mvx).astype(F)
        py2 = (muy * muy + mvy * mvy).astype(F)
        return px2, py2, np.fmax(px2, py2).astype(F), np.fmin(px2, py2).astype(F)


def tap_count(w, h, duvdx, duvdy, max_anisotropy):
    """(N [n] int, eta [n] float32): N == 1 wherever the SAMPLER rule of mipmaps.h applies unchanged."""
    px2, py2, r2, s2 = footprint(w, h, duvdx, duvdy)
    A = F(max_anisotropy)
    with np.errstate(all="ignore"):
        spread = (A != F(1.0)) & (r2 > 0) & (r2 != F(np.inf))
        eta = np.where(spread, np.fmin(np.sqrt((r2 / s2).astype(F)).astype(F), A), F(1.0)).astype(F)
    return np.ceil(eta).astype(np.int64), eta


def sample(levels, srgb, st, duvdx, duvdy, max_lod, max_anisotropy, level_count_registered=None, return_detail=False):
    """The anisotropic sampler: `levels` = [level0, level1, ...], of which the first `level_count_registered` are registered
    (default: all). Returns [n, 3] float32; with return_detail also a dict of N, eta, lam (clamped), d and f per sample."""
    L = len(levels) if level_count_registered is None else level_count_registered
    st = np.asarray(st, F)
    duvdx, duvdy = np.asarray(duvdx, F), np.asarray(duvdy, F)
    n = st.shape[0]
    out = mm.sample(levels, srgb, st, duvdx, duvdy, max_lod, level_count_registered)  # N == 1, and every map without a chain
    detail = {"N": np.ones(n, np.int64), "eta": np.ones(n, F)}
    if L <= 1:
        return (out, detail) if return_detail else out
    h, w = levels[0].shape[:2]
    N, eta = tap_count(w, h, duvdx, duvdy, max_anisotropy)
    detail["N"], detail["eta"] = N, eta
    px2, py2, r2, _ = footprint(w, h, duvdx, duvdy)
    many = N > 1
    with np.errstate(all="ignore"):
        safe_r2 = np.where(many, r2, F(1.0)).astype(F)
        lam = (F(0.5) * (_log(safe_r2) * LOG2E)).astype(F) - (_log(eta) * LOG2E).astype(F)
        lam = np.fmin(np.fmax(lam.astype(F), F(0.0)), np.fmin(F(max_lod), F(L - 1))).astype(F)
    d = np.floor(lam).astype(np.int64)
    f = (lam - d.astype(F)).astype(F)
    detail["lam"], detail["d"], detail["f"] = lam, d, f
    major = np.where((px2 >= py2)[:, None], duvdx, duvdy).astype(F)
    for count in np.unique(N[many]):
        rows = np.nonzero(N == count)[0]
        acc = None
        for i in range(1, int(count) + 1):
            t = F(F(i) / F(count + 1)) - F(0.5)
            with np.errstate(all="ignore"):
                st_i = (st[rows] + (t * major[rows]).astype(F)).astype(F)
            tap = np.zeros((rows.size, 3), F)
            for k in np.unique(d[rows]):
                lo = d[rows] == k
                tap[lo] = bilinear(levels[k], srgb, st_i[lo])
                hi = lo & (f[rows] != 0)
                if hi.any():
                    fk = f[rows][hi][:, None]
                    tap[hi] = (F(1.0) - fk) * tap[hi] + fk * bilinear(levels[k + 1], srgb, st_i[hi])
            acc = tap if acc is None else (acc + tap).astype(F)
        out[rows] = (acc / F(count)).astype(F)
    return (out, detail) if return_detail else out
