"""include/szg/jpeg.h on the CPU: the numpy model of tests/jpeg_model.py against values computed by hand (or, for the wrap rule,
once in Python integers). The host code and the kernels are compared with this model in test_jpeg_host.py and test_gpu_jpeg.py."""
import numpy as np

from tests import jpeg_model as jm


def test_constants_are_the_integers_of_the_header():
    assert [jm.IDCT_CONSTANTS[c] for c in (0.5411961, -1.847759065, 0.765366865, 1.175875602, 0.298631336, 2.053119869,
                                           3.072711026, 1.501321110, -0.899976223, -2.562915447, -1.961570560, -0.390180644)] == \
        [2217, -7567, 3135, 4816, 1223, 8410, 12586, 6149, -3685, -10497, -8034, -1597]
    # f(x) = ((int)(x * 4096.0f + 0.5f)) << 8
    assert jm.color_fixed(1.40200) == 5743 << 8 == 1470208
    assert jm.color_fixed(0.71414) == 2925 << 8 == 748800
    assert jm.color_fixed(0.34414) == 1410 << 8 == 360960
    assert jm.color_fixed(1.77200) == 7258 << 8 == 1858048


def test_dc_only_block_is_uniform():
    # column pass 4 dc, row pass ((4 dc) * 4096 + 65536 + (128 << 17)) >> 17 = 128 + ((dc + 4) >> 3)
    dcs = np.array([-32768, -2000, -1025, -1024, -1021, -12, -5, -4, -1, 0, 3, 4, 11, 12, 1000, 1015, 1016, 1020, 2047, 32767])
    blocks = np.zeros((len(dcs), 8, 8), np.int16)
    blocks[:, 0, 0] = dcs
    got = jm.idct_blocks(blocks)
    for dc, block in zip(dcs.tolist(), got):
        want = min(max(128 + ((dc + 4) >> 3), 0), 255)
        assert (block == want).all(), (dc, want, block[0, 0])


def _idct_python(block, wrap=True):
    """rule 3 on Python integers with explicit 32-bit wrapping (or, wrap=False, on unbounded integers), one block [8][8]"""
    M = 0xFFFFFFFF
    K = jm.IDCT_CONSTANTS

    def s32(v):
        if not wrap:
            return v
        v &= M
        return v - (1 << 32) if v & 0x80000000 else v

    def one(s, bias):
        c = lambda x: K[x]  # noqa: E731
        p2, p3 = s[2], s[6]
        p1 = s32((p2 + p3) * c(0.5411961))
        t2 = s32(p1 + p3 * c(-1.847759065))
        t3 = s32(p1 + p2 * c(0.765366865))
        p2, p3 = s[0], s[4]
        t0 = s32((p2 + p3) * 4096)
        t1 = s32((p2 - p3) * 4096)
        x0, x3, x1, x2 = s32(t0 + t3 + bias), s32(t0 - t3 + bias), s32(t1 + t2 + bias), s32(t1 - t2 + bias)
        t0, t1, t2, t3 = s[7], s[5], s[3], s[1]
        p3, p4, p1, p2 = s32(t0 + t2), s32(t1 + t3), s32(t0 + t3), s32(t1 + t2)
        p5 = s32((p3 + p4) * c(1.175875602))
        t0, t1, t2, t3 = s32(t0 * c(0.298631336)), s32(t1 * c(2.053119869)), s32(t2 * c(3.072711026)), s32(t3 * c(1.501321110))
        p1 = s32(p5 + p1 * c(-0.899976223))
        p2 = s32(p5 + p2 * c(-2.562915447))
        p3 = s32(p3 * c(-1.961570560))
        p4 = s32(p4 * c(-0.390180644))
        t3, t2, t1, t0 = s32(t3 + p1 + p4), s32(t2 + p2 + p3), s32(t1 + p2 + p4), s32(t0 + p1 + p3)
        return [s32(v) for v in (x0 + t3, x1 + t2, x2 + t1, x3 + t0, x3 - t0, x2 - t1, x1 - t2, x0 - t3)]

    mid = [[0] * 8 for _ in range(8)]
    for col in range(8):
        out = one([block[r][col] for r in range(8)], 512)
        for r in range(8):
            mid[r][col] = out[r] >> 10
    return [[min(max(v >> 17, 0), 255) for v in one(mid[r], 65536 + (128 << 17))] for r in range(8)]


def test_extreme_block_wraps_as_32_bit_twos_complement():
    rng = np.random.default_rng(7)
    extreme = np.where(rng.integers(0, 2, (8, 8)) == 1, 32767, -32768).astype(np.int16)
    full = rng.integers(-32768, 32768, (8, 8)).astype(np.int16)
    for block in (extreme, full, np.full((8, 8), 32767, np.int16), np.full((8, 8), -32768, np.int16)):
        want = np.array(_idct_python(block.astype(int).tolist()), np.uint8)
        assert (jm.idct_blocks(block) == want).all()
    # the wrap is real: on unbounded integers the extreme blocks give another picture
    for block in (extreme, full):
        unbounded = np.array(_idct_python(block.astype(int).tolist(), wrap=False), np.uint8)
        assert (jm.idct_blocks(block) != unbounded).any()


def test_h2v1_last_pair_quirk_on_a_three_sample_row():
    n = np.array([10, 50, 200], np.uint8)
    samples = np.zeros((8, 8), np.uint8)
    samples[0, :3] = n
    # component with h = 1 in a frame whose h_max is 2: hs = 2, vs = 1, W = 6 -> wl = 3
    out = jm.upsample(samples, 6, 1, 1, 1, 2, 1)[0]
    # out[4] = (3 * in[1] + in[2] + 2) >> 2 = 88: sample wl - 2 carries the weight 3 (an unquirked filter would give 163)
    assert out.tolist() == [10, (3 * 10 + 50 + 2) >> 2, (3 * 50 + 10 + 2) >> 2, (3 * 50 + 200 + 2) >> 2, (3 * 50 + 200 + 2) >> 2, 200]
    assert out.tolist() == [10, 20, 40, 88, 88, 200]
    # W = 5 reads the same samples (wl = 3) and drops the last output
    assert jm.upsample(samples, 5, 1, 1, 1, 2, 1)[0].tolist() == [10, 20, 40, 88, 88]
    # wl == 1: both outputs are the sample
    assert jm.upsample(samples, 2, 1, 1, 1, 2, 1)[0].tolist() == [10, 10]


def test_upsampling_clamps_to_the_samples_that_exist_not_to_the_padding():
    samples = np.full((16, 16), 255, np.uint8)  # the MCU padding is 255 everywhere
    samples[:2, :2] = [[0, 40], [80, 120]]      # H = 3, W = 3 with 2 x 2 subsampling: ch = 2, wl = 2
    out = jm.upsample(samples, 3, 3, 1, 1, 2, 2)
    # row 0: near = far = row 0 -> t = 4 * in; row 1: near 0, far 1; row 2: near 1, far 0
    t0 = [0, 160]
    t1 = [3 * 0 + 80, 3 * 40 + 120]
    t2 = [3 * 80 + 0, 3 * 120 + 40]
    for row, t in zip(out, (t0, t1, t2)):
        assert row.tolist() == [(t[0] + 2) >> 2, (3 * t[0] + t[1] + 8) >> 4, (3 * t[1] + t[0] + 8) >> 4]
    # (1, 2), (4, 1) and (1, 4)
    col = jm.upsample(samples, 1, 3, 1, 1, 1, 2)[:, 0]
    assert col.tolist() == [0, (3 * 0 + 80 + 2) >> 2, (3 * 80 + 0 + 2) >> 2]
    assert jm.upsample(samples, 7, 1, 1, 1, 4, 1)[0].tolist() == [0, 0, 0, 0, 40, 40, 40]
    assert jm.upsample(samples, 1, 7, 1, 1, 1, 4)[:, 0].tolist() == [0, 0, 0, 0, 80, 80, 80]


def test_colour_conversion_by_hand():
    y = np.array([0, 255, 128, 76, 255], np.uint8)
    cb = np.array([128, 128, 0, 85, 255], np.uint8)
    cr = np.array([128, 128, 255, 255, 0], np.uint8)
    r, g, b = jm.ycbcr_to_rgb(y, cb, cr)

    def by_hand(Y, Cb, Cr):
        yf = (Y << 20) + (1 << 19)
        cbs, crs = Cb - 128, Cr - 128
        rr = yf + crs * 1470208
        gg = yf - crs * 748800 + (((-cbs * 360960) & 0xFFFFFFFF) & 0xFFFF0000)
        gg = ((gg + (1 << 31)) % (1 << 32)) - (1 << 31)
        bb = yf + cbs * 1858048
        return tuple(min(max(v >> 20, 0), 255) for v in (rr, gg, bb))

    for k in range(len(y)):
        assert (int(r[k]), int(g[k]), int(b[k])) == by_hand(int(y[k]), int(cb[k]), int(cr[k]))
    assert (int(r[0]), int(g[0]), int(b[0])) == (0, 0, 0) and (int(r[1]), int(g[1]), int(b[1])) == (255, 255, 255)


def test_masks_and_grey_and_rgb_frames():
    rng = np.random.default_rng(3)
    planes = [(1, 1, rng.integers(-200, 200, (1, 1, 8, 8)).astype(np.int16)) for _ in range(3)]
    grey = jm.reconstruct({"width": 8, "height": 8, "color": "grey", "planes": planes[:1]})
    assert (grey[..., 0] == grey[..., 1]).all() and (grey[..., 0] == grey[..., 2]).all() and (grey[..., 3] == 255).all()
    assert (grey[..., 0] == jm.sample_plane(planes[0][2])).all()
    rgb = jm.reconstruct({"width": 8, "height": 8, "color": "rgb", "planes": planes})
    for c in range(3):
        assert (rgb[..., c] == jm.sample_plane(planes[c][2])).all()
    red = jm.reconstruct({"width": 8, "height": 8, "color": "rgb", "planes": planes}, 0xFFFFFFFF, 0x000000FF)
    assert (red[..., 0] == 255).all() and (red[..., 1:] == rgb[..., 1:]).all()
    occ = jm.reconstruct({"width": 8, "height": 8, "color": "rgb", "planes": planes}, 0xFF0000FF, 0)
    assert (occ[..., 1:3] == 0).all() and (occ[..., 0] == rgb[..., 0]).all() and (occ[..., 3] == 255).all()
