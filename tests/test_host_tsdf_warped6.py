"""kfusion::cuda::TsdfVolume::integrateWarped6 and DynFusion's canonical volume in north-star mode
(DynFuParams::north_star_fuse_canonical) through the C++ host adaptor (tests/cpp/test_host_tsdf_warped6.cpp): the C call's
bits, the occupancy map, the switches' rules, a four-frame north-star sequence with the switch off and on."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_host_integrate_warped6_and_canonical_volume():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_tsdf_warped6"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "3 tests, 0 failed" in r.stdout
