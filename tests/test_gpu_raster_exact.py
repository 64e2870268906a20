"""The scenes of tests/test_raster_exact.py through the HIP rasteriser (recordGBufferRaster, the shadow raster): the kernel
output is compared with the exact model DIRECTLY (tests/raster_model.py through tests/raster_scenes.py), and with the oracle
bit for bit on every single raster call. Ordinary bounded launches; run with -m gpu."""
import numpy as np
import pytest

from oracle import binding as ob
from syzygy_amd import abi
from tests import raster_scenes as rs
from tests import test_raster_exact as cpu

pytestmark = pytest.mark.gpu


class KernelBackend:
    """Pipelines and targets are kept per extent: the per-primitive checks make thousands of small raster calls."""

    def __init__(self):
        import torch

        if not torch.cuda.is_available():
            pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
        from syzygy_amd import pipelines

        self.torch, self.pl = torch, pipelines
        self.oracle = cpu.OracleBackend()
        self._gb, self._sh = {}, {}
        self.calls = 0

    def _cameras(self, cam):
        cameras = self.pl.TStagedBuffer(abi.CameraPacked, 1)
        cameras.push(cam)
        cameras.recordCopyToDevice()
        return cameras

    def gbuffer(self, W, H, cam, ms, tile=None, planes=False):
        rows = H if tile is None else tile.local_rows
        if (W, rows) not in self._gb:
            if len(self._gb) > 6:
                self.close_gbuffers()
            self._gb[(W, rows)] = (self.pl.SceneTexture(W, rows), self.pl.DeferredShadingPipeline((W, rows), max_spot_lights=1, max_shadow_maps=0))
        target, deferred = self._gb[(W, rows)]
        deferred.recordGBufferRaster(None, abi.Rect(0, 0, W, H), target, 0, self._cameras(cam), ms, tile=tile)
        self.torch.cuda.synchronize()
        depth = target.depth.cpu().numpy()
        got = deferred.download_gbuffer(W, rows) if planes else None
        want_depth, want = self.oracle.gbuffer(W, H, cam, ms, tile=tile, planes=True)
        assert (depth.view(np.uint32) == want_depth.view(np.uint32)).all(), "kernel depth differs from the oracle"
        if planes:
            for name, a in got.items():
                b = want[name]
                bits = np.uint16 if a.dtype == np.float16 else np.uint32
                same = (a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))
                assert same.all(), f"{name}: kernel differs from the oracle at {(~same).sum()} values"
        self.calls += 1
        return depth, got

    def shadow(self, dim, ms, bias_constant=0.0, bias_slope=0.0):
        if dim not in self._sh:
            for _, d in self._sh.values():
                d.cleanup()
            self._sh.clear()
            lights = self.pl.TStagedBuffer(abi.DirectionalLightPacked, 1)
            light = abi.DirectionalLightPacked()
            eye = abi.Mat4.from_numpy(np.eye(4, dtype=np.float32))
            light.projection, light.view = eye, eye
            lights.push([light])
            lights.recordCopyToDevice()
            self._sh[dim] = (lights, self.pl.DeferredShadingPipeline((8, 8), max_spot_lights=1, max_shadow_maps=1, shadow_map_dim=dim))
        lights, deferred = self._sh[dim]
        deferred.setConfiguration(abi.DeferredConfiguration(bias_constant, bias_slope))
        deferred.recordShadowRaster(None, lights, None, ms)
        self.torch.cuda.synchronize()
        sm = deferred.shadowMaps()
        got = self.pl._memcpy2d_from(sm.maps[0], dim * 4, dim).cpu().numpy().view(np.float32).reshape(dim, dim)
        want = self.oracle.shadow(dim, ms, bias_constant, bias_slope)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), "kernel shadow map differs from the oracle"
        self.calls += 1
        return got

    def close_gbuffers(self):
        for _, d in self._gb.values():
            d.cleanup()
        self._gb.clear()

    def close(self):
        self.close_gbuffers()
        for _, d in self._sh.values():
            d.cleanup()
        self._sh.clear()


@pytest.fixture(scope="module")
def backend():
    b = KernelBackend()
    yield b
    print(f"{b.calls} raster calls, each bit-identical to the oracle")
    b.close()


@pytest.mark.parametrize("W,H,seed,count", cpu.SOUP_CASES)
def test_gpu_soup_coverage_agrees_with_exact_arithmetic_outside_the_rounding_band(backend, W, H, seed, count):
    cpu.test_soup_coverage_agrees_with_exact_arithmetic_outside_the_rounding_band(backend, W, H, seed, count)


def test_gpu_orthographic_fans_at_2048_own_their_centre_pixel_once(backend):
    cpu.test_orthographic_fans_at_2048_own_their_centre_pixel_once(backend)


@pytest.mark.parametrize("W,H,step", cpu.PERSPECTIVE_LATTICES)
def test_gpu_perspective_lattice_hits_every_pixel_once(backend, W, H, step):
    cpu.test_perspective_lattice_hits_every_pixel_once(backend, W, H, step)


@pytest.mark.parametrize("cam_name", ["w1", "perspective"])
@pytest.mark.parametrize("ulps", [0, 1, -1])
@pytest.mark.parametrize("W,H,step", cpu.SMALL_LATTICES)
def test_gpu_lattices_on_and_one_ulp_off_pixel_centres_are_watertight(backend, W, H, step, ulps, cam_name):
    cpu.test_lattices_on_and_one_ulp_off_pixel_centres_are_watertight(backend, W, H, step, ulps, cam_name)


@pytest.mark.parametrize("W,H,rows", cpu.LARGE_LATTICES)
@pytest.mark.parametrize("cam_name", ["w1", "perspective"])
def test_gpu_lattice_at_large_extents_is_watertight(backend, W, H, rows, cam_name):
    cpu.test_lattice_at_large_extents_is_watertight(backend, W, H, rows, cam_name)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("W,H", [(97, 61), (64, 48)])
def test_gpu_closed_convex_mesh_in_perspective_is_watertight(backend, W, H, seed):
    cpu.test_closed_convex_mesh_in_perspective_is_watertight(backend, W, H, seed)


@pytest.mark.parametrize("dim", cpu.SHADOW_DIMS)
def test_gpu_shadow_pass_fans_are_watertight_at_every_map_size(backend, dim):
    cpu.test_shadow_pass_fans_are_watertight_at_every_map_size(backend, dim)


@pytest.mark.parametrize("layers,quads", cpu.TIE_CASES)
def test_gpu_depth_ties_go_to_the_first_submitted_primitive(backend, layers, quads):
    cpu.test_depth_ties_go_to_the_first_submitted_primitive(backend, layers, quads)


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("tw,th", cpu.TEXTURE_SIZES)
def test_gpu_texture_rule_at_texel_centres_and_midpoints(backend, tw, th, srgb):
    cpu.test_texture_rule_at_texel_centres_and_midpoints(backend, tw, th, srgb)


@pytest.mark.parametrize("W,H,step", [(64, 32, 4), (32, 32, 2)])
def test_gpu_lattice_depth_equals_the_correctly_rounded_exact_quotient(backend, W, H, step):
    cpu.test_lattice_depth_equals_the_correctly_rounded_exact_quotient(backend, W, H, step)


@pytest.mark.parametrize("W,H", cpu.NORMAL_EXTENTS)
def test_gpu_perturbed_normal_equals_the_float64_cotangent_frame(backend, W, H):
    cpu.test_perturbed_normal_equals_the_float64_cotangent_frame(backend, W, H)


@pytest.mark.parametrize("dim,constant,slope", cpu.BIAS_CASES)
def test_gpu_shadow_depth_bias_slope_term_against_the_exact_depth_slope(backend, dim, constant, slope):
    cpu.test_shadow_depth_bias_slope_term_against_the_exact_depth_slope(backend, dim, constant, slope)
