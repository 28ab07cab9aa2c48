"""kfusion::cuda::TsdfVolume::fetchCloud / fetchNormals through the C++ host adaptor (tests/cpp/test_host_extract.cpp):
the reference's buffer behaviour and pose handling, the C entry points' bits, a PCD file of the cloud."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_host_tsdf_volume_fetch_cloud_and_normals():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_extract"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "5 tests, 0 failed" in r.stdout
