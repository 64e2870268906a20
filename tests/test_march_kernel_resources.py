"""What the compiler reports for the kernels that hold the march (`make march-resource-usage` in syzygy_amd/csrc: the library's
flags and per-unit scheduler options, -Rpass-analysis=kernel-resource-usage). k_composite runs four waves per SIMD without
scratch and with an LDS queue small enough for four workgroups per CU (4 x 40 960 B = 160 KiB); k_skyview likewise without
scratch. Only the remark lines are read."""
import pytest

from tests import native

FIELDS = {"VGPRs": r"\bVGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "occupancy": r"Occupancy \[waves/SIMD\]: (\d+)",
          "lds": r"LDS Size \[bytes/block\]: (\d+)"}


@pytest.fixture(scope="module")
def remarks():
    return native.resource_remarks("march-resource-usage", FIELDS)


def one(remarks, fragment):
    found = [(n, r) for n, r in remarks.items() if fragment in n]
    assert len(found) == 1, (fragment, [n for n, _ in found])
    assert set(found[0][1]) == set(FIELDS), found[0]
    return found[0][1]


# (Itanium mangling: k_composite<true> is ...k_compositeILb1EEE..., k_composite<false> ...ILb0EEE...)
@pytest.mark.parametrize("fragment", ["11k_compositeILb0EE", "11k_compositeILb1EE"])
def test_composite_has_no_scratch_at_four_waves(remarks, fragment):
    r = one(remarks, fragment)
    print(fragment, r)
    assert r["scratch"] == 0 and r["VGPRs"] <= 128 and r["occupancy"] == 4 and r["lds"] <= 40960, r


def test_skyview_has_no_scratch_at_four_waves(remarks):
    r = one(remarks, "9k_skyviewE")
    print(r)
    assert r["scratch"] == 0 and r["occupancy"] == 4, r
