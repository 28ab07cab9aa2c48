"""The growing canonical model (DynFuParams::north_star_regrow_canonical, canonical_min_weight, fuse_unsupported_rigid)
through the C++ host adaptor (tests/cpp/test_host_regrow.cpp): a four-frame north-star sequence whose frame 0 sees half the
sphere — the cloud is the canonical volume's surface at the weight floor by the public calls' bits, it and the nodes grow,
each switch's own effect, the model view on the regrown mesh, the switches' rules."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_host_regrown_canonical_model():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_regrow"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "5 tests, 0 failed" in r.stdout
