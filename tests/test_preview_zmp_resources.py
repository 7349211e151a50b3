"""The kernels of csrc/preview_zmp.h against what they were built for, read from the compiler's
kernel-resource remarks as tests/test_kernel_resources.py does: no scratch, the knot kernel's two suffix tables in LDS,
and the resident wavefronts per SIMD of each bucket of the sampled kernel."""
import pytest

from test_kernel_resources import _usage

EXPECT = {"ccc_amd::pvz_knots_kernel": (4, 8216), "void ccc_amd::pvz_sampled_kernel<2>": (4, 0),
          "void ccc_amd::pvz_sampled_kernel<4>": (4, 0), "void ccc_amd::pvz_sampled_kernel<8>": (3, 0),
          "void ccc_amd::pvz_sampled_kernel<16>": (2, 0)}  # kernel -> (min waves per SIMD, LDS bytes)


@pytest.fixture(scope="module")
def usage():
    return _usage("preview_zmp")


@pytest.mark.parametrize("kernel", sorted(EXPECT))
def test_preview_zmp_kernel_resources(usage, kernel):
    u = usage[kernel]
    assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["LDS Size"] == EXPECT[kernel][1], u
    assert u["Occupancy"] >= EXPECT[kernel][0], u
