"""The JPEG host code under AddressSanitizer + UBSan: tests/jpeg/fuzz_jpeg.cpp, a stand-alone CPU program built over
syzygy_amd/csrc/host_jpeg.cpp, decodes fixtures of every layout and entropy mode and corrupted variants of them (flipped bits,
truncations, marker lengths, Huffman tables with over-long codes, huge dimensions, restart markers out of order). Any
out-of-bounds access, signed overflow or leak aborts it."""
import os
import subprocess

from tests import jpeg_fixtures as jf
from tests import native

SEEDS = ["444_17x9_base_q92", "422_33x31_prog_q92", "420_33x31_rst_q92", "420_9x17_prog_q12", "grey_7x5_rst_q12",
         "h1v2_17x17_base_q85", "h4v1_33x16_base_q85", "h1v4_15x31_base_q85", "rgbids_17x9_base_q85", "adobe0_17x9_base_q85",
         "444_130x70_rst_q12", "refused_cmyk_17x9"]
MUTANTS = 1500


def test_jpeg_host_code_survives_corrupted_input_under_sanitizers():
    exe = native.build("jpeg/fuzz_jpeg")
    files = [os.path.join(jf.FOLDER, name + ".jpg") for name in SEEDS]
    out = subprocess.run([exe, str(MUTANTS)] + files, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=1:max_allocation_size_mb=4096"))
    assert out.returncode == 0, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    inputs, decoded = int(lines[0].split()[0]), int(lines[0].split()[2])
    assert inputs == len(SEEDS) * (MUTANTS + 1) and len(SEEDS) - 1 <= decoded < inputs
    per_seed = {os.path.basename(line.split()[0])[:-4]: int(line.split()[1]) for line in lines[1:]}
    assert sorted(per_seed) == sorted(SEEDS)
    for name, count in per_seed.items():
        if name.startswith("refused_"):
            continue  # 4 components: refused by rule 1, whatever else a mutation changes
        # at least one mutant of every seed still decodes, and the mutations do bite
        assert 0 < count < MUTANTS, (name, count)
