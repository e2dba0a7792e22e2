"""The resources of the two kernels that match descriptors, read off the gfx950 code objects (no GPU needed: hipcc
cross-compiles).

stereo_curve_cost_kernel and motion_stereo_kernel run one depth pixel per lane through the descriptor DP of
vg_stereo_device.hpp, with the DP's rows in registers and its ring, thresholds and descriptor in the block's LDS (DESIGN.md
sections 5.10 and 5.11).  That holds only while a lane needs no scratch, two waves fit a SIMD's 512 registers (VGPRs + AGPRs
<= 256) and two 256-lane blocks fit the CU's 160 KiB of LDS (<= 81 920 bytes each).  Both kernels declare the one LDS struct,
so they report the same size.  These are conditions from the hardware, not measurements."""
import pytest

from tests import isa

KERNELS = {"vg_stereo_tu.hip": "stereo_curve_cost_kernel", "vg_motion_tu.hip": "motion_stereo_kernel"}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    hipcc = isa.hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = {}
    for unit, kernel in KERNELS.items():
        text = isa.device_asm(hipcc, unit, str(tmp_path_factory.mktemp("isa") / (unit + ".s")))
        found = [v for k, v in isa.kernel_metadata(text).items() if kernel in k]
        assert len(found) == 1, (unit, kernel)
        out[kernel] = found[0]
    return out


@pytest.mark.parametrize("kernel", sorted(KERNELS.values()))
def test_matching_kernel_keeps_two_waves_two_blocks_and_no_scratch(meta, kernel):
    m = meta[kernel]
    print(kernel, {k: m.get(k) for k in (".vgpr_count", ".agpr_count", ".group_segment_fixed_size",
                                         ".private_segment_fixed_size", ".vgpr_spill_count")})
    assert int(m[".private_segment_fixed_size"]) == 0
    assert int(m.get(".vgpr_spill_count", 0)) == 0
    assert int(m[".vgpr_count"]) + int(m.get(".agpr_count", 0)) <= 256
    assert 0 < int(m[".group_segment_fixed_size"]) <= 81920


def test_matching_kernels_share_one_lds_layout(meta):
    sizes = {k: int(m[".group_segment_fixed_size"]) for k, m in meta.items()}
    assert len(set(sizes.values())) == 1, sizes
