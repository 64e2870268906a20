"""The LUT bookkeeping of the sky-view pipeline (syzygy_amd/csrc/lut_state.hpp) is plain C++ with no HIP in it:
tests/cpp/lut_state.cpp walks its event table and four sequences on the CPU. The GPU tests of tests/test_gpu_parity.py
(LUT reuse, row slices, the all-gather, texels written through a kept pointer) hold the same behaviour end to end."""
import subprocess

from tests import native


def test_lut_state_table_and_sequences():
    out = subprocess.run([native.build("cpp/lut_state")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "lut_state ok" in out.stdout, out.stdout + out.stderr
