"""kfusion::cuda::rasterizeMesh and DynFusion's view of the warped canonical model (DynFuParams::model_view,
renderWarpedModel) through the C++ host adaptor (tests/cpp/test_host_mesh_view.cpp): the wrapper against the C call, image
sizes per flag, the view against warpToLive -> dfa_mesh_rasterize -> shade byte for byte, the throws, and frames that are
bit-identical with the view on and off, in both solve modes."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_host_mesh_view():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_mesh_view"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 tests, 0 failed" in r.stdout
