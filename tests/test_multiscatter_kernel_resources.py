"""What the compiler reports for the multi-scattering twins of the two LUT kernels (`make ms-resource-usage` in
syzygy_amd/csrc: the library's flags and the scheduler options of the LUT unit, -Rpass-analysis=kernel-resource-usage):
k_skyview_ms and k_aerial_lut_ms, one instance per mode, none of them with scratch. Their occupancy is not pinned
(DESIGN.md §16 states it). Only the remark lines are read."""
import pytest

from tests import native

FIELDS = {"VGPRs": r"\bVGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "occupancy": r"Occupancy \[waves/SIMD\]: (\d+)",
          "lds": r"LDS Size \[bytes/block\]: (\d+)", "spill": r"VGPRs Spill: (\d+)"}


@pytest.fixture(scope="module")
def remarks():
    return native.resource_remarks("ms-resource-usage", FIELDS)


# (Itanium mangling: k_skyview_ms<1, false> is ...12k_skyview_msILi1ELb0EEE..., k_aerial_lut_ms<2> ...15k_aerial_lut_msILi2EEE...)
@pytest.mark.parametrize("fragment", ["12k_skyview_msILi1E", "12k_skyview_msILi2E", "15k_aerial_lut_msILi1E", "15k_aerial_lut_msILi2E"])
def test_no_instance_has_scratch(remarks, fragment):
    found = [(n, r) for n, r in remarks.items() if fragment in n]
    assert len(found) == 1, (fragment, sorted(remarks))
    r = found[0][1]
    print(found[0][0], r)
    assert set(r) == set(FIELDS), r
    assert r["scratch"] == 0 and r["spill"] == 0 and r["occupancy"] >= 2 and r["lds"] <= 16384, r


def test_the_unit_holds_these_kernels_and_no_others(remarks):
    assert len(remarks) == 4 and all("k_skyview_ms" in n or "k_aerial_lut_ms" in n for n in remarks), sorted(remarks)
