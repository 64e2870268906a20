"""CPU model of include/szg/mipmaps.h: the chain generation rule in integers and numpy float32, and the trilinear sampler in
numpy float32, one rounding per operation as the header states them. szg_logf and szg_powf are include/szg/fpmath.h on the
host (oracle.binding.builtin_eval fn 6 and fn 1), the functions the kernels evaluate on the device.

Shared by tests/test_mipmap_model.py (CPU) and the GPU tests, which demand the kernels' bytes and bits to equal these."""
import numpy as np

from oracle import binding as ob
from syzygy_amd import abi

F = np.float32
MAX_LOD_REFERENCE = 1.0
MAX_LOD_NONE = 1000.0
FN_POW, FN_LOG = 1, 6


def level_count(w, h):
    return 0 if w == 0 or h == 0 else int(max(w, h)).bit_length()


def level_shapes(w, h):
    """[(w_k, h_k)] for every level of a full chain."""
    return [(max(1, w >> k), max(1, h >> k)) for k in range(level_count(w, h))]


def chain_bytes(w, h):
    return sum(wk * hk * 4 for wk, hk in level_shapes(w, h)[1:])


def _pow(x, y):
    x = np.ascontiguousarray(x, F)
    return ob.builtin_eval(FN_POW, x.reshape(-1), np.full(x.size, y, F)).reshape(x.shape)


def _log(x):
    x = np.ascontiguousarray(x, F)
    return ob.builtin_eval(FN_LOG, x.reshape(-1)).reshape(x.shape)


def decode_table(srgb):
    """decode8 of every code: c = float(code) / 255; sRGB: c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4)."""
    c = np.arange(256, dtype=F) / F(255.0)
    if not srgb:
        return c
    return np.where(c <= F(0.04045), c / F(12.92), _pow((c + F(0.055)) / F(1.055), F(2.4))).astype(F)


def encode_srgb(linear):
    """SZG_OETF_SRGB of szg_record_oetf: l <= 0.0031308 ? 12.92 l : pow(l, (float)(1 / 2.4)) * 1.055 - 0.055."""
    linear = np.asarray(linear, F)
    higher = _pow(linear, F(1.0 / 2.4)) * F(1.055) - F(0.055)
    return np.where(linear <= F(0.0031308), F(12.92) * linear, higher).astype(F)


def downsample(level, srgb):
    """One level [h, w, 4] uint8 -> the next (mipmaps.h "GENERATION")."""
    h, w = level.shape[:2]
    dw, dh = max(1, w >> 1), max(1, h >> 1)
    x = np.arange(dw)
    y = np.arange(dh)
    x0, x1 = np.minimum(2 * x, w - 1), np.minimum(2 * x + 1, w - 1)
    y0, y1 = np.minimum(2 * y, h - 1), np.minimum(2 * y + 1, h - 1)
    t00, t10 = level[y0][:, x0], level[y0][:, x1]
    t01, t11 = level[y1][:, x0], level[y1][:, x1]
    out = ((t00.astype(np.uint32) + t10 + t01 + t11 + 2) >> 2).astype(np.uint8)
    if srgb:
        table = decode_table(True)
        lin = ((table[t00[..., :3]] + table[t10[..., :3]]) + (table[t01[..., :3]] + table[t11[..., :3]])) * F(0.25)
        q = np.floor(encode_srgb(lin) * F(255.0) + F(0.5)).astype(np.int64)
        out[..., :3] = np.clip(q, 0, 255).astype(np.uint8)
    return out


def build_chain(level0, srgb):
    """[level0, level1, ...] down to 1 x 1."""
    levels = [np.ascontiguousarray(level0)]
    while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
        levels.append(downsample(levels[-1], srgb))
    return levels


def pack_chain(levels):
    """Levels 1.. back to back (mipmaps.h "CHAIN LAYOUT")."""
    if len(levels) <= 1:
        return np.zeros(0, np.uint8)
    return np.concatenate([np.ascontiguousarray(lv).reshape(-1) for lv in levels[1:]])


def _wrap_index(f, n):
    fn = F(n)
    with np.errstate(all="ignore"):
        m = f - fn * np.floor(f / fn)
    ok = np.isfinite(m) & (np.abs(m) < F(2.0**31))
    i = np.where(ok, np.trunc(np.where(ok, m, F(0))), 0).astype(np.int64)
    return np.where((i >= n) | (i < 0), 0, i)


def bilinear(level, srgb, st):
    """raster.h "textures" on one level: st [n, 2] float32 -> [n, 3] float32."""
    st = np.asarray(st, F)
    h, w = level.shape[:2]
    table = decode_table(srgb)
    u = st[:, 0] * F(w) - F(0.5)
    v = st[:, 1] * F(h) - F(0.5)
    fu, fv = np.floor(u), np.floor(v)
    a, b = (u - fu).astype(F), (v - fv).astype(F)
    i0, j0 = _wrap_index(fu, w), _wrap_index(fv, h)
    i1 = np.where(i0 + 1 == w, 0, i0 + 1)
    j1 = np.where(j0 + 1 == h, 0, j0 + 1)
    one = F(1.0)
    w00, w10, w01, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    t00, t10, t01, t11 = (table[level[j, i, :3]] for j, i in ((j0, i0), (j0, i1), (j1, i0), (j1, i1)))
    r = ((w00[:, None] * t00 + w10[:, None] * t10) + w01[:, None] * t01) + w11[:, None] * t11
    return r.astype(F)


def mip_lambda(w, h, levels, max_lod, duvdx, duvdy):
    """lambda of mipmaps.h "SAMPLER", clamped: duvdx, duvdy [n, 2] float32 -> [n] float32."""
    duvdx, duvdy = np.asarray(duvdx, F), np.asarray(duvdy, F)
    with np.errstate(all="ignore"):
        mux, mvx = duvdx[:, 0] * F(w), duvdx[:, 1] * F(h)
        muy, mvy = duvdy[:, 0] * F(w), duvdy[:, 1] * F(h)
        r2 = np.fmax(mux * mux + mvx * mvx, muy * muy + mvy * mvy).astype(F)
        positive = r2 > 0
        lam = np.where(positive, F(0.5) * (_log(np.where(positive, r2, F(1.0))) * F(1.44269504)), F(0.0)).astype(F)
        return np.fmin(np.fmax(lam, F(0.0)), np.fmin(F(max_lod), F(levels - 1))).astype(F)


def sample(levels, srgb, st, duvdx, duvdy, max_lod, level_count_registered=None, return_levels=False):
    """The trilinear sampler: `levels` = [level0, level1, ...] arrays, of which the first `level_count_registered` are
    registered (default: all). Returns [n, 3] float32, and with return_levels also the boolean matrix [n, len(levels)] of
    the levels each sample fetched."""
    L = len(levels) if level_count_registered is None else level_count_registered
    st = np.asarray(st, F)
    n = st.shape[0]
    h, w = levels[0].shape[:2]
    lam = mip_lambda(w, h, L, max_lod, duvdx, duvdy) if L > 1 else np.zeros(n, F)
    d = np.floor(lam).astype(np.int64)
    f = (lam - d.astype(F)).astype(F)
    out = np.zeros((n, 3), F)
    read = np.zeros((n, len(levels)), bool)
    for k in range(L):
        lo = d == k
        if lo.any():
            out[lo] = bilinear(levels[k], srgb, st[lo])
            read[lo, k] = True
        hi = lo & (f != 0)
        if hi.any():
            fk = f[hi][:, None]
            out[hi] = (F(1.0) - fk) * out[hi] + fk * bilinear(levels[k + 1], srgb, st[hi])
            read[hi, k + 1] = True
    return (out, read) if return_levels else out


def generate_refusals(data, chain):
    """(name, Texture or None, chain address, chain_bytes, text) of every refusal of szg_record_generate_mipmaps for an image
    at address `data` (tests/test_mipmap_model.py passes made-up addresses, tests/test_gpu_mipmaps.py real device buffers)."""
    need = chain_bytes(37, 19)
    return [
        ("null level0", None, chain, need, b"NULL level0"),
        ("null data", abi.Texture(None, 37, 19, 148, 0), chain, need, b"NULL level0"),
        ("zero width", abi.Texture(data, 0, 19, 148, 0), chain, need, b"extent"),
        ("zero height", abi.Texture(data, 37, 0, 148, 0), chain, need, b"extent"),
        ("too wide", abi.Texture(data, 32769, 1, 32769 * 4, 0), chain, 1 << 20, b"extent"),
        ("short pitch", abi.Texture(data, 37, 19, 144, 0), chain, need, b"pitch"),
        ("odd pitch", abi.Texture(data, 37, 19, 150, 0), chain, need, b"pitch"),
        ("chain_bytes too small", abi.Texture(data, 37, 19, 148, 0), chain, need - 1, b"chain_bytes"),
        ("chain_bytes zero", abi.Texture(data, 37, 19, 148, 1), chain, 0, b"chain_bytes"),
        ("null chain", abi.Texture(data, 37, 19, 148, 0), None, need, b"NULL d_chain"),
        ("misaligned data", abi.Texture(data + 2, 37, 19, 148, 0), chain, need, b"aligned"),
        ("misaligned chain", abi.Texture(data, 37, 19, 148, 0), chain + 1, need + 8, b"aligned"),
    ]
