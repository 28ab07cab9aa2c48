"""The regularisation hierarchy through the C++ host adaptor (tests/cpp/test_host_reg_hierarchy.cpp):
DynFuParams::north_star_reg_hierarchy / reg_level_slots and the L, beta, epsilon it reads — the switch's rules; on the
half-sphere north-star sequence the levels are dfa_node_levels' on the field's nodes, old nodes keep theirs as the field
grows and the frames solve; switched off, a sequence keeps its bits, also on plans a hierarchical run has used."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_host_reg_hierarchy():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_reg_hierarchy"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "3 tests, 0 failed" in r.stdout
