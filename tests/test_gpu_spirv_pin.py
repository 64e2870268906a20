"""The HIP kernels against the reference's own shader binaries, on the GPU.

tests/golden/spirv_vectors.npz holds what the reference's committed SPIR-V computes when it is executed literally
(tests/test_spirv_pin.py, tests/golden/spirv_interp.py). libszg_hip_literal.so is the product's kernels with the contraction
rule switched off (-DSZG_LITERAL: two roundings at the closed list of places where the product fuses, szg_device.hpp) - the
kernels' own literal execution of the same shaders. A child process renders the vectors' inputs through the C-ABI with that
library: all four passes must reproduce every recorded value BIT FOR BIT (fp32 and UNORM16), and the 512 x 128 transmittance
LUT as a whole (SHA-256). The product library fuses at a measured subset of those places (include/szg/contraction.h) and is held to
the same vectors within north_star's bar: 1e-4 relative, one UNORM16 step.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _child(library):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product path has no CPU fallback")
    env = dict(os.environ)
    if library:
        env["SZG_HIP_LIBRARY"] = os.path.join(ROOT, "syzygy_amd", "csrc", library)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_spirv_pin_child.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().split("\n")[-1])


def test_literal_kernels_reproduce_the_reference_spirv_bit_for_bit():
    out = _child("libszg_hip_literal.so")
    assert out["library"] == "libszg_hip_literal.so" and out["values"] >= 5000
    assert out["transmittance_mismatches"] == 0, out
    assert out["skyview_mismatches"] == 0, out
    assert out["lights_mismatches"] == 0 and out["lights_unorm_mismatches"] == 0, out
    assert out["camera_mismatches"] == 0 and out["camera_unorm_mismatches"] == 0, out
    assert out["transmittance_lut_sha256_equal"], out


def test_product_kernels_stay_within_1e4_and_one_unorm16_step_of_the_reference_spirv():
    """The product library on the same inputs. It fuses a * b + c only at the site classes of include/szg/contraction.h that
    were measured, alone and together, to leave EVERY recorded value within north_star's 1e-4 relative and one UNORM16 step
    (profiles/r03_contraction_classes.md; round 2 fused everywhere and was 2.3e-3 / 7 steps away). These vectors are a sample
    (84 sky-view texels, none next to the horizon): tests/test_gpu_contraction_whole_images.py holds the rule to the same bar
    on whole LUTs and frames. The bounds are the bar itself, not a multiple of the measurement."""
    out = _child(None)
    assert out["library"] == "libszg_hip.so"
    assert 0 < out["camera_mismatches"] + out["lights_mismatches"]  # the two builds are different programs
    for shader in ("transmittance", "skyview", "lights", "camera"):
        assert out[shader + "_rel_max"] <= 1e-4, (shader, out)
    assert out["lights_unorm_max_step"] <= 1 and out["camera_unorm_max_step"] <= 1, out
    assert out["transmittance_lut_sha256_equal"], out  # no fused class reaches transmittance_LUT.comp's arithmetic
