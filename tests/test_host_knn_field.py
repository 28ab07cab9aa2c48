"""The k-NN field through the C++ host adaptors (tests/cpp/test_host_knn_field.cpp): TsdfVolume::buildKnnField /
appendKnnField, and DynFusion sequences with DynFuParams::fuse_knn_field off and on — reference mode and north-star mode —
whose canonical volumes are equal byte for byte after every frame, over frames that insert nodes."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_host_knn_field_and_cached_canonical_fusion():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_knn_field"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "5 tests, 0 failed" in r.stdout
