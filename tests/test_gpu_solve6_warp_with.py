"""-m gpu: dfa_solver6_warp_with, the north-star blend of a plan's vertices under transforms the caller gives — what carries
the canonical mesh of DynFusion's model view through the deformation a north-star solve found.

It is the kernel of dfa_solver6_warp with another source of transforms, so the two must agree bit for bit wherever both are
defined: after a solve, with the solved transforms; and a second plan that has never solved, over the same nodes and the
same vertices, must give those bits too.  Identity transforms leave the cloud where it is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dynfu_amd import synth  # noqa: E402
from gpu_util import bits, dev, host  # noqa: E402


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


@pytest.fixture(scope="module")
def solved(A):
    cfg = synth.CONFIGS["T0"]
    c, intr = synth.canonical(cfg), synth.intrinsics(cfg)
    P, Nm = A.compute_points_normals(dev(synth.depth_frame(cfg, 4)), *intr)
    s = A.Solver6(cfg["D"], len(c["verts"]), cfg["k"])
    keep = [dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(c["verts"]), dev(c["normals"])]
    s.set_problem(*keep)
    s.solve(P, Nm, *intr, A.Solve6Params(num_iter=1, gn_iter=2, linear_iter=40, lambda_=200.0))
    dq = s.node_dq()
    assert not np.array_equal(host(dq), c["node_dq"])  # the solve moved something
    return cfg, c, keep, s, dq, [host(t) for t in s.warp()]


def test_equals_the_plans_own_warp_after_a_solve(solved):
    _, _, _, s, dq, (wv, wn) = solved
    v, n = s.warp_with(dq)
    assert np.array_equal(bits(host(v)), bits(wv)) and np.array_equal(bits(host(n)), bits(wn))


def test_a_plan_that_never_solved_gives_the_same_bits(A, solved):
    cfg, c, keep, _, dq, (wv, wn) = solved
    s2 = A.Solver6(cfg["D"], len(c["verts"]), cfg["k"])
    s2.set_problem(*keep)
    v, n = s2.warp_with(dq)
    assert np.array_equal(bits(host(v)), bits(wv)) and np.array_equal(bits(host(n)), bits(wn))
    v, _ = s2.warp_with(dq, want_normals=False)
    assert np.array_equal(bits(host(v)), bits(wv))


def test_identity_transforms_leave_the_cloud_in_place(A, solved):
    cfg, c, keep, s, _, _ = solved
    ident = np.zeros((cfg["D"], 8), np.float32)
    ident[:, 0] = 1.0
    v, n = s.warp_with(dev(ident))
    # the blended real part is (W, 0, 0, 0) with W the sum of the normalised weights, the dual part zero, and the point
    # fl(fl(fl(W p) W) fl(1 / fl(W W))): five roundings of 2^-24 each, relative to the largest coordinate
    eps = 5 * 2.0 ** -24
    assert np.abs(host(v) - c["verts"]).max() <= eps * np.abs(c["verts"]).max()
    assert np.abs(host(n) - c["normals"]).max() <= eps * np.abs(c["normals"]).max()


def test_invalid_arguments(A, solved):
    cfg, c, _, s, dq, _ = solved
    L = A._lib
    lib = L.load()
    out = dev(np.zeros((len(c["verts"]), 3), np.float32))
    assert lib.dfa_solver6_warp_with(s._h, None, L._dev(out), None, None) == 1  # DFA_ERR_INVALID
    assert lib.dfa_solver6_warp_with(s._h, L._dev(dq), None, None, None) == 1
    fresh = A.Solver6(cfg["D"], len(c["verts"]), cfg["k"])  # no problem set
    assert lib.dfa_solver6_warp_with(fresh._h, L._dev(dq), L._dev(out), None, None) == 1
