"""Colour in the C++ host adaptor (tests/cpp/test_host_color.cpp): TsdfVolume::integrateWarped6Color against the C call's bits,
the rules of DynFuParams::north_star_fuse_color and the two overloads of DynFusion::operator(), and a four-frame static
north-star sequence before a colour ramp — geometry bit for bit that of north_star_fuse_canonical alone, canonicalColors() the
ramp at every vertex's own projection within 1 + slope * trunc * f / z_min."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    from dynfu_amd import build as B
    return B.build_cpp_tests()["test_host_color"]


def _run(exe, name):
    r = subprocess.run([exe, "HostColorTest." + name], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "1 tests, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_integrate_warped6_color_matches_the_c_call(exe):
    _run(exe, "IntegrateWarped6ColorMatchesTheCCall")


def test_switch_rules(exe):
    _run(exe, "SwitchRules")


def test_static_sequence_before_a_colour_ramp(exe):
    _run(exe, "StaticSequenceBeforeAColourRamp")


def test_every_projecting_vertex_has_a_colour(exe):
    """a = 255 on at least the share of vertices that project inside the image onto non-zero depth: every one of them, the
    vertices of the closing walls at the scene's depth edges included (the model's vertices are sampled on their lattice edge)."""
    _run(exe, "EveryProjectingVertexHasAColour")
