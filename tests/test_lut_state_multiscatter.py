"""The events include/szg/multiscatter_sky.h adds to the LUT bookkeeping of the sky-view pipeline
(syzygy_amd/csrc/lut_state.hpp: a change of mode, the multi-scattering LUT recorded, the multi-scattering LUT handed out),
walked on the CPU by tests/multiscatter_sky/lut_state_multiscatter.cpp. tests/test_gpu_multiscatter_sky.py sees the same rules
through the sentinel of its host-state test."""
import subprocess

from tests import native


def test_multiscatter_events_of_the_lut_state():
    out = subprocess.run([native.build("multiscatter_sky/lut_state_multiscatter")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "lut_state_multiscatter ok" in out.stdout, out.stdout + out.stderr
