"""GPU: multiple scattering in the sky-view LUT and the aerial LUT (include/szg/multiscatter_sky.h; k_skyview_ms and
k_aerial_lut_ms of syzygy_amd/csrc/kernels_lut_ms.hip) through the C-ABI.

Shapes: sky-view LUT 64 x 32, transmittance LUT 512 x 128 uploaded from the oracle, multi-scattering LUT 32 x 32, aerial volume
32^3. Cameras at 2 m, 2500 m, 30 000 m and 200 000 m: the LEAN + INNER body of the march, LEAN, the generic body, and rays that
miss the atmosphere. Suns at 35 and -3 degrees. The oracle's sky-view LUT is finite at every texel of these cases.

What holds the new kernels to what:
  zero LUT      mode ADD with an all-zero multi-scattering LUT is the oracle's single scattering, bit for bit
  additivity    ADD == float32(OFF + ONLY) per channel, bit for bit
  linearity     ONLY doubles exactly when the LUT doubles
  composition   row slices == the whole LUT, bit for bit
  model         ONLY against the float64 model (tests/multiscatter_sky_model.py) within 2 * D0, D0 the model's own distance from
                the oracle as the CPU test measured it
  status dword  0 after a finite launch, 1 after a texel that is not finite, as k_skyview keeps it
  frame, host state, the C++ mirror
"""
import functools
import subprocess

import numpy as np
import pytest

from tests import multiscatter_sky_model as model
from tests import native
from tests import util
from tests.test_gpu_parity import gpu, staged  # noqa: F401  (gpu is a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32
TLUT, SLUT = (512, 128), (64, 32)
CAMERAS = [2.0, 2500.0, 30000.0, 200000.0]
SUNS = [35.0, -3.0]
CASES = [(c, s) for c in CAMERAS for s in SUNS]
AERIAL_MAX_DISTANCE = 0.05  # Mm


def inputs(altitude_m, elevation, W=64, H=64):
    from syzygy_amd import scene

    cam = scene.default_camera()
    cam.cameraPosition[:] = [0.0, -float(altitude_m), 0.0]  # y points down
    return util.Inputs(W, H, elevation_degrees=elevation, camera=cam)


@functools.lru_cache(maxsize=None)
def oracle_tlut():
    from oracle import binding as ob

    t = ob.transmittance_lut(inputs(2500.0, 35.0).atm, TLUT[0], TLUT[1], threads=8)  # (it sees neither the sun nor the camera)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def oracle_skyview(altitude_m, elevation):
    from oracle import binding as ob

    inp = inputs(altitude_m, elevation)
    s = ob.skyview_lut(inp.atm, inp.cam, oracle_tlut(), SLUT[0], SLUT[1], threads=8)
    s.setflags(write=False)
    return s


def same_bits(got, want, what):
    """Bit for bit, NaN compared by position."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), f"{what}: NaN pattern differs at {int((np.isnan(got) != nan).sum())} values"
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} values differ in their bits; first at {tuple(bad[0])}: " \
                          f"{got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}"


class Sky:
    """A sky-view pipeline on the oracle's transmittance LUT, with the staged blocks of one case."""

    def __init__(self, gpu, inp):
        self.gpu, self.inp = gpu, inp
        self.cameras, self.atmospheres, self.lights = staged(gpu, inp)
        self.sky = gpu.pl.SkyViewComputePipeline.create(transmittance_extent=TLUT, skyview_extent=SLUT)
        assert self.sky is not None
        self.sky.upload_lut(self.sky.transmittanceLUT(), oracle_tlut().copy())

    def kernel_psi(self):
        """The multi-scattering LUT as k_multiscatter computes it (its own test: test_multiscatter_lut_matches_its_oracle)."""
        self.sky.recordMultiScatterLUT(None, 0, self.atmospheres)
        torch.cuda.synchronize()
        return self.sky.download_lut(self.sky.multiScatterLUT())

    def upload_psi(self, psi):
        self.sky.upload_lut(self.sky.multiScatterLUT(), psi)

    def skyview(self, mode, rows=None):
        self.sky.setMultiScattering(mode)
        if rows is None:
            self.sky.recordSkyViewLUT(None, 0, self.atmospheres, 0, self.cameras)
        else:
            for b, e in rows:
                self.sky.recordSkyViewLUTRows(None, 0, self.atmospheres, 0, self.cameras, b, e)
        torch.cuda.synchronize()
        return self.sky.download_lut(self.sky.skyviewLUT())

    def aerial(self, mode):
        self.sky.setMultiScattering(mode)
        self.sky.recordAerialLUT(None, 0, self.atmospheres, 0, self.cameras, AERIAL_MAX_DISTANCE)
        torch.cuda.synchronize()
        lum, tr = self.sky.aerialLUT()
        return self.sky.download_lut(lum), self.sky.download_lut(tr)

    def destroy(self):
        self.sky.destroy()


def synthetic_psi(seed=11):
    """Texels in [2^-6, 2^-2]."""
    psi = np.ones((32, 32, 4), F)
    psi[..., :3] = np.exp2(np.random.default_rng(seed).uniform(-6.0, -2.0, (32, 32, 3))).astype(F)
    assert psi[..., :3].min() >= 2.0 ** -6 and psi[..., :3].max() <= 2.0 ** -2
    return psi


# ---------------------------------------------------------------------------
# 1. zero LUT: the single-scattering accumulator inside the new kernels is the oracle's, at every gate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("altitude_m,elevation", CASES)
def test_zero_lut_is_the_oracles_single_scattering(gpu, altitude_m, elevation):
    s = Sky(gpu, inputs(altitude_m, elevation))
    s.upload_psi(np.zeros((32, 32, 4), F))
    want = oracle_skyview(altitude_m, elevation)
    assert np.isfinite(want).all()
    same_bits(s.skyview(gpu.abi.SZG_MULTISCATTER_ADD), want, f"sky-view, zero LUT, {altitude_m} m, sun {elevation}")
    got_lum, got_tr = s.aerial(gpu.abi.SZG_MULTISCATTER_ADD)
    want_lum, want_tr = gpu.ob.aerial_lut(s.inp.atm, s.inp.cam, oracle_tlut(), AERIAL_MAX_DISTANCE, threads=8)
    same_bits(got_lum, want_lum, f"aerial luminance, zero LUT, {altitude_m} m, sun {elevation}")
    same_bits(got_tr, want_tr, f"aerial transmittance, zero LUT, {altitude_m} m, sun {elevation}")
    s.destroy()


# ---------------------------------------------------------------------------
# 2. additivity with the kernel's own LUT
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("altitude_m,elevation", CASES)
def test_add_is_off_plus_only(gpu, altitude_m, elevation):
    A = gpu.abi
    s = Sky(gpu, inputs(altitude_m, elevation))
    psi = s.kernel_psi()
    assert np.isfinite(psi).all() and (psi[..., :3] >= 0).all() and (psi[..., :3] > 0).any()  # (0 where the sun is far below the horizon)
    off, only, add = (s.skyview(m) for m in (A.SZG_MULTISCATTER_OFF, A.SZG_MULTISCATTER_ONLY, A.SZG_MULTISCATTER_ADD))
    same_bits(off, oracle_skyview(altitude_m, elevation), "mode OFF is the oracle's LUT")
    same_bits(add[..., :3], off[..., :3] + only[..., :3], f"sky-view ADD == OFF + ONLY, {altitude_m} m, sun {elevation}")
    assert (add[..., 3] == 1.0).all() and (only[..., 3] == 1.0).all()
    assert (only[..., :3] >= 0).all() and (only[..., :3] > 0).any()  # the term is there ...
    if altitude_m < 100000.0 and elevation > 0.0:
        assert (only[..., :3] > 0).all()  # ... at every texel while the sun is up along every ray
    (a_off, t_off), (a_only, t_only), (a_add, t_add) = (s.aerial(m) for m in (A.SZG_MULTISCATTER_OFF, A.SZG_MULTISCATTER_ONLY, A.SZG_MULTISCATTER_ADD))
    with np.errstate(invalid="ignore"):
        same_bits(a_add[..., :3], a_off[..., :3] + a_only[..., :3], f"aerial ADD == OFF + ONLY, {altitude_m} m, sun {elevation}")
    same_bits(t_only, t_off, "the transmittance volume does not see the mode")
    same_bits(t_add, t_off, "the transmittance volume does not see the mode")
    s.destroy()


# ---------------------------------------------------------------------------
# 3. linearity in the LUT
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("altitude_m", [2.0, 2500.0, 30000.0])
def test_only_doubles_exactly_with_the_lut(gpu, altitude_m):
    s = Sky(gpu, inputs(altitude_m, 35.0))
    psi = synthetic_psi()
    s.upload_psi(psi)
    one = s.skyview(gpu.abi.SZG_MULTISCATTER_ONLY)
    double = psi.copy()
    double[..., :3] *= F(2.0)
    s.upload_psi(double)
    two = s.skyview(gpu.abi.SZG_MULTISCATTER_ONLY)
    # far above the denormal range and far below overflow: a factor of 2 is exact in every product, sum and fused sum
    print(f"{altitude_m} m: ONLY texels in [{one[..., :3].min():.3e}, {one[..., :3].max():.3e}]")
    assert np.isfinite(one).all() and one[..., :3].min() > 2.0 ** -100 and one[..., :3].max() < 2.0 ** 100
    same_bits(two[..., :3], one[..., :3] * F(2.0), f"ONLY with 2 Psi, {altitude_m} m")
    s.destroy()


# ---------------------------------------------------------------------------
# 4. wave composition: the 8 x 8 wave patches fall differently in the slice launches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("altitude_m", [2.0, 30000.0])
def test_row_slices_equal_the_whole_lut(gpu, altitude_m):
    s = Sky(gpu, inputs(altitude_m, 35.0))
    s.kernel_psi()
    for mode in (gpu.abi.SZG_MULTISCATTER_ADD, gpu.abi.SZG_MULTISCATTER_ONLY):
        whole = s.skyview(mode)
        s.sky.skyviewLUT_tensor().fill_(-1.0)
        sliced = s.skyview(mode, rows=[(10, 32), (0, 3), (3, 10)])
        same_bits(sliced, whole, f"mode {mode}: rows [0,3) [3,10) [10,32) against the whole LUT, {altitude_m} m")
    s.destroy()


def test_status_dword_is_kept_as_k_skyview_keeps_it(gpu):
    """The dword behind the sky-view texels: 0 after a launch whose texels are all finite, 1 after one that stored a texel that
    is not, cleared again by the next launch (the composite reads it before it leaves a sample of this LUT unevaluated)."""
    A = gpu.abi
    s = Sky(gpu, inputs(2500.0, 35.0))

    def dword():
        im = s.sky.skyviewLUT()
        n = im.width * im.height * 4
        return int(gpu.pl._alias_tensor(im.data, (n + 4,))[n:n + 1].view(torch.int32).item())

    s.kernel_psi()
    assert np.isfinite(s.skyview(A.SZG_MULTISCATTER_ADD)).all() and dword() == 0
    poisoned = np.ones((32, 32, 4), F)
    poisoned[..., :3] = np.inf
    s.upload_psi(poisoned)
    assert not np.isfinite(s.skyview(A.SZG_MULTISCATTER_ADD)[..., :3]).any() and dword() == 1
    assert not np.isfinite(s.skyview(A.SZG_MULTISCATTER_ONLY, rows=[(8, 16)])[8:16, :, :3]).any() and dword() == 1
    assert np.isfinite(s.skyview(A.SZG_MULTISCATTER_OFF)).all() and dword() == 0  # (mode OFF does not read the LUT)
    s.upload_psi(synthetic_psi())
    assert np.isfinite(s.skyview(A.SZG_MULTISCATTER_ONLY)).all() and dword() == 0
    s.destroy()


# ---------------------------------------------------------------------------
# 5. the float64 model's multi-scattering part
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("altitude_m", [2500.0, 30000.0])
def test_only_against_the_model(gpu, altitude_m):
    """Tolerance 2 * D0, D0 = the model's distance from the ORACLE's single scattering on these cases (CPU test; 6.6e-4). The
    new term shares every ill-conditioned factor (T_begin, integral) with the single-scattering term and adds a tap of a smooth
    32 x 32 LUT and products."""
    worst = 0.0
    for elevation in (70.0, 35.0, 5.0, -3.0):
        s = Sky(gpu, inputs(altitude_m, elevation))
        psi = s.kernel_psi()
        got = s.skyview(gpu.abi.SZG_MULTISCATTER_ONLY)[..., :3]
        _, want = model.skyview(s.inp.atm, s.inp.cam, oracle_tlut(), SLUT[0], SLUT[1], psi)
        d = model.metric(got, want)
        print(f"camera {altitude_m:.0f} m, sun {elevation:+.0f} deg: d = {d.max():.3e} (tolerance {2 * model.D0:.3e}) "
              f"at texel {np.unravel_index(d.argmax(), d.shape)[:2]}")
        worst = max(worst, float(d.max()))
        s.destroy()
    assert worst <= 2.0 * model.D0, (worst, 2.0 * model.D0)


# ---------------------------------------------------------------------------
# 6. a frame through szg_skyview_record_draw_commands
# ---------------------------------------------------------------------------
def test_frame_in_mode_add(gpu):
    W, H = 160, 90
    inp = util.Inputs(W, H, elevation_degrees=35.0, spots=4)
    cameras, atmospheres, lights = staged(gpu, inp)

    def lit_frame():
        frame = gpu.ob.HostFrame(W, H)
        gpu.ob.gbuffer_fill(frame, inp.rect, None, inp.cam, inp.synthetic.fill, threads=8)
        gpu.ob.lights(frame, inp.rect, None, None, inp.cam, inp.dirs, 2, 1, inp.spots, 4, threads=8)
        return frame

    frame = lit_frame()
    prior = frame.color.copy()
    target = gpu.pl.SceneTexture(W, H, debug=True)
    deferred = gpu.pl.DeferredShadingPipeline((W, H), max_spot_lights=1, max_shadow_maps=1)
    deferred.upload_gbuffer(frame.planes())

    def prime():
        target.color.copy_(torch.from_numpy(prior.view(np.int16)))
        target.depth.copy_(torch.from_numpy(frame.depth))

    def draw(mode):
        sky = gpu.pl.SkyViewComputePipeline.create(transmittance_extent=TLUT, skyview_extent=SLUT)
        sky.setMultiScattering(mode)
        prime()
        sky.recordDrawCommands(None, target, inp.rect, deferred.gbuffer(), deferred.shadowMaps(), 0, atmospheres, 0, cameras, 0, lights)
        torch.cuda.synchronize()
        return sky, target.debug.cpu().numpy(), target.color_numpy()

    sky_off, debug_off, _ = draw(gpu.abi.SZG_MULTISCATTER_OFF)
    sky, debug_add, color_add = draw(gpu.abi.SZG_MULTISCATTER_ADD)
    tlut, slut = sky.download_lut(sky.transmittanceLUT()), sky.download_lut(sky.skyviewLUT())
    same_bits(tlut, oracle_tlut(), "the frame's transmittance LUT")
    # the frame recorded the multi-scattering LUT itself, from this transmittance LUT, and the sky-view LUT read it
    same_bits(sky.download_lut(sky.multiScatterLUT()), gpu.ob.multiscatter_lut(inp.atm, tlut)[0], "the frame's multi-scattering LUT")
    slut_off = sky_off.download_lut(sky_off.skyviewLUT())
    assert (slut[..., :3] > slut_off[..., :3]).all()
    # the composite did not change: the oracle's, fed with the LUT the GPU computed
    gpu.ob.composite(frame, inp.rect, None, None, inp.atm, inp.cam, inp.dirs, 0, tlut, slut, threads=8)
    same_bits(debug_add, frame.debug, "composite of the mode-ADD sky-view LUT")
    assert (color_add == frame.color).all()
    # taps, sum and the final pow are monotone: no sky pixel gets darker
    sky_pixels = ~(frame.depth > 0)
    assert sky_pixels.any() and (~sky_pixels).any()
    assert np.isfinite(debug_add[sky_pixels]).all()
    assert (debug_add[sky_pixels][:, :3] >= debug_off[sky_pixels][:, :3]).all()
    assert (debug_add[sky_pixels][:, :3] > debug_off[sky_pixels][:, :3]).any()

    # the fast composite reads the mode-ADD aerial volume unchanged
    max_distance = 10.0e-3
    sky.recordAerialLUT(None, 0, atmospheres, 0, cameras, max_distance)
    torch.cuda.synchronize()
    volume = sky.download_lut(sky.aerialLUT()[0])
    sky_off.recordAerialLUT(None, 0, atmospheres, 0, cameras, max_distance)
    torch.cuda.synchronize()
    assert (volume.view(np.uint32) != sky_off.download_lut(sky_off.aerialLUT()[0]).view(np.uint32)).any()
    fast = lit_frame()
    gpu.ob.composite(fast, inp.rect, None, None, inp.atm, inp.cam, inp.dirs, 0, tlut, slut, threads=8, aerial=(volume, max_distance))
    prime()
    sky.recordCompositeFast(None, target, inp.rect, deferred.gbuffer(), deferred.shadowMaps(), 0, atmospheres, 0, cameras, 0, lights)
    torch.cuda.synchronize()
    same_bits(target.debug.cpu().numpy(), fast.debug, "fast composite of the mode-ADD aerial volume")
    assert (target.color_numpy() == fast.color).all()
    deferred.cleanup()
    sky.destroy()
    sky_off.destroy()


# ---------------------------------------------------------------------------
# 7. host state
# ---------------------------------------------------------------------------
def test_refusals_and_lut_reuse(gpu):
    from syzygy_amd import SzgError

    A = gpu.abi
    altitude_m, elevation = 2500.0, 35.0
    s = Sky(gpu, inputs(altitude_m, elevation))
    sky = s.sky
    alias = sky.skyviewLUT_tensor()  # taken once: later writes through it are behind the library's back, as a sentinel must be
    SENTINEL = 12345.0

    def frame():
        sky.recordTransmittance(None, 0, s.atmospheres)
        sky.recordSkyViewLUT(None, 0, s.atmospheres, 0, s.cameras)
        torch.cuda.synchronize()
        return alias.cpu().numpy()

    def recomputed():
        """Plant a sentinel, record a frame: was the sky-view LUT computed again?"""
        alias[0, 0, 0] = SENTINEL
        return float(frame()[0, 0, 0]) != SENTINEL

    # refusals: no multi-scattering LUT on this pipeline yet; a mode above 2
    assert sky.multiScattering() == A.SZG_MULTISCATTER_OFF
    sky.setMultiScattering(A.SZG_MULTISCATTER_ADD)
    for call in (lambda: sky.recordSkyViewLUT(None, 0, s.atmospheres, 0, s.cameras),
                 lambda: sky.recordSkyViewLUTRows(None, 0, s.atmospheres, 0, s.cameras, 0, 8),
                 lambda: sky.recordAerialLUT(None, 0, s.atmospheres, 0, s.cameras, AERIAL_MAX_DISTANCE)):
        with pytest.raises(SzgError) as e:
            call()
        assert e.value.code == A.SZG_ERR_INVALID_ARGUMENT and "szg_skyview_record_multiscatter_lut" in str(e.value)
    with pytest.raises(SzgError):
        sky.setMultiScattering(3)
    assert sky.multiScattering() == A.SZG_MULTISCATTER_ADD
    sky.setMultiScattering(A.SZG_MULTISCATTER_OFF)

    # LUT reuse on; the same atmosphere and camera in every frame
    sky.recordTransmittance(None, 0, s.atmospheres)  # (the library's own transmittance LUT from here on: the same bits)
    sky.setLUTReuse(True)
    want_off = oracle_skyview(altitude_m, elevation)
    same_bits(frame(), want_off, "mode OFF")
    assert not recomputed(), "with reuse on, an unchanged frame keeps the LUT: the sentinel method works"
    sky.recordMultiScatterLUT(None, 0, s.atmospheres)
    assert not recomputed(), "mode OFF reads no multi-scattering LUT"
    sky.setMultiScattering(A.SZG_MULTISCATTER_ADD)
    assert recomputed(), "a change of mode"
    add = frame().copy()
    assert (add[..., :3] > want_off[..., :3]).all()
    sky.setMultiScattering(A.SZG_MULTISCATTER_ADD)
    assert not recomputed(), "setting the mode it has"
    sky.recordMultiScatterLUT(None, 0, s.atmospheres)
    assert not recomputed(), "szg_skyview_record_multiscatter_lut alone: its texels are a function of what the key covers"
    sky.multiScatterLUT()
    assert recomputed(), "the accessor hands out writable texels while a mode is set"
    same_bits(frame(), add, "mode ADD again")
    sky.setMultiScattering(A.SZG_MULTISCATTER_ONLY)
    assert recomputed(), "a change of mode"
    same_bits(add[..., :3], want_off[..., :3] + frame()[..., :3], "ADD == OFF + ONLY through the reuse path")
    sky.setMultiScattering(A.SZG_MULTISCATTER_OFF)
    assert recomputed(), "a change of mode"
    same_bits(frame(), want_off, "mode OFF after ADD restores the oracle's bits")
    s.destroy()


# ---------------------------------------------------------------------------
# 8. the C++ mirror
# ---------------------------------------------------------------------------
def test_cpp_set_multi_scattering_equals_the_python_path(gpu, tmp_path):
    from syzygy_amd import lib

    lib()  # built and loadable
    exe = native.build("multiscatter_sky/skyview_multiscatter")
    prefix = str(tmp_path / "cpp")
    done = subprocess.run([exe, str(gpu.abi.SZG_MULTISCATTER_ADD), prefix], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip().endswith("ok mode 1"), done.stdout + done.stderr
    got = np.fromfile(prefix + ".skyview", F).reshape(SLUT[1], SLUT[0], 4)
    atm = gpu.abi.AtmospherePacked.from_buffer_copy(open(prefix + ".atmosphere", "rb").read())
    cam = gpu.abi.CameraPacked.from_buffer_copy(open(prefix + ".camera", "rb").read())
    cameras, atmospheres = gpu.pl.TStagedBuffer(gpu.abi.CameraPacked, 1), gpu.pl.TStagedBuffer(gpu.abi.AtmospherePacked, 1)
    cameras.push(cam)
    atmospheres.push(atm)
    cameras.recordCopyToDevice()
    atmospheres.recordCopyToDevice()
    sky = gpu.pl.SkyViewComputePipeline.create(transmittance_extent=TLUT, skyview_extent=SLUT)
    sky.setMultiScattering(gpu.abi.SZG_MULTISCATTER_ADD)
    sky.recordTransmittance(None, 0, atmospheres)
    sky.recordMultiScatterLUT(None, 0, atmospheres)
    sky.recordSkyViewLUT(None, 0, atmospheres, 0, cameras)
    torch.cuda.synchronize()
    want = sky.download_lut(sky.skyviewLUT())
    same_bits(got, want, "the C++ caller's sky-view LUT against the Python path's")
    off = gpu.ob.skyview_lut(atm, cam, sky.download_lut(sky.transmittanceLUT()), SLUT[0], SLUT[1], threads=8)
    assert np.isfinite(got).all() and (got[..., :3] > off[..., :3]).all()  # ... and it is not the single-scattering LUT
    sky.destroy()
