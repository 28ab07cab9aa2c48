"""The rigid pre-alignment of north-star mode with its whole Gauss-Newton loop on the device (DynFuParams::rigid_prealign_device)
through the C++ host adaptor (tests/cpp/test_host_rigid_loop.cpp), on the four-frame planted-motion sequence of
test_host_rigid_align.cpp: ten iterations at full resolution are the host loop's pose to 0.1 mm and 1e-4 rad, the default
schedule recovers the planted motion, starts the solve lower and stops early, an empty depth frame is a skipped frame, the
switch's rule, and no bit changes with the switch off."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_host_rigid_pre_alignment_on_the_device():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_rigid_loop"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "5 tests, 0 failed" in r.stdout
