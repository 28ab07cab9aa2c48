"""kfusion::cuda::visibleVertices, NorthStarSolver::setVertexMask and DynFuParams::north_star_visible_only through the C++
host adaptor (tests/cpp/test_host_visible_term.cpp): the wrapper on the two-plane case, the constructor's throws, three frames
of the synthetic sphere that are bit-identical with the switch on and off, and the frame's count against the rule stated on
the device's dumped model map."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_host_visible_term():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_visible_term"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 tests, 0 failed" in r.stdout
