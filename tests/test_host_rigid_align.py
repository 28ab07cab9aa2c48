"""The rigid pre-alignment of north-star mode (DynFuParams::north_star_rigid_prealign) through the C++ host adaptor
(tests/cpp/test_host_rigid_align.cpp): Warpfield::composeRigid against the statement's known answers, and four-frame north-star
sequences under a planted camera motion — the estimate is its inverse, the solve starts from a lower energy, zero iterations
change no bit, an empty depth frame skips the step, the other switches run with it, the switch's rule."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_host_rigid_pre_alignment():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_rigid_align"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 tests, 0 failed" in r.stdout
