"""kfusion::cuda::MarchingCubes::runIndexed / dfa::convertToIndexedMesh through the C++ host adaptor
(tests/cpp/test_host_mc_indexed.cpp): the indexed mesh against run()'s soup, the winding, the VTK text read back."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_host_marching_cubes_indexed_mesh():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_mc_indexed"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "5 tests, 0 failed" in r.stdout
