"""The statements of the rigid pre-alignment (tests/rigid_align_statement.py) on the CPU: the hand-made answers of
tests/rigid_align_cases.py hold in both statements, no shape case has a knife-edge vertex or passes on empty sums, the
constants recorded in rigid_align_cases.py are the measured ones, and the north-star blend is left-invariant."""
import numpy as np
import pytest

import icp_cases as K
import img_statement as St
import rigid_align_cases as C
import rigid_align_statement as RS
from solve6_statement import dq_point as _dq_point


def dq_point(dq, c):
    """T(c) of dual quaternions whose real part is a unit quaternion only to float32 rounding: divided by |r|^2, as the
    blend divides by |a|^2"""
    return _dq_point(dq, c) / (dq[..., :4] ** 2).sum(-1)[..., None]


def _edge(normals):
    v, n, want, want_no_n = C.edge_values_vertices()
    vs, ns = C.edge_values_maps()
    cols = C.EV["cols"]
    gates = (C.EV["dist_thresh"], C.EV["cos_thresh"])
    return v, (n if normals else None), (want if normals else want_no_n), vs[:, :cols], ns[:, :cols], gates


@pytest.mark.parametrize("normals", [True, False])
def test_every_hand_made_answer_holds_in_both_statements(normals):
    v, n, want, vmap, nmap, gates = _edge(normals)
    sums, ok, rows, sum64, abs64, _ = RS.rigid_sums64(v, n, C.IDENT, vmap, nmap, C.EV["intr"], *gates)
    assert np.array_equal(ok.astype(np.int64), want), np.argwhere(ok != want.astype(bool))
    assert not rows[~ok].any()
    for i in range(len(v)):  # vertex by vertex: one row, nothing to round between the two statements but the row itself
        s1, ok1, _, s64, a64, _ = RS.rigid_sums64(v[i:i + 1], None if n is None else n[i:i + 1], C.IDENT, vmap, nmap, C.EV["intr"], *gates)
        assert int(ok1.sum()) == want[i], i
        assert C.within_bar(s1, s64, a64, 4), i  # s = c exactly at the identity; products of a few digits
    assert want.sum() > 0 and C.within_bar(sums, sum64, abs64, 8)
    # the rows of the matched vertices, by hand for two of them
    assert np.array_equal(rows[0], np.array([0 * -1 - 1 * 0, 1 * 0 - (-0.125) * -1, 0, 0, 0, -1, 0], np.float32))  # L - s = (-0.125, 0, 0)
    assert np.array_equal(rows[11], np.array([0.25 * -1, 0, 0, 0, 0, -1, -0.25], np.float32))                      # L - s = (0, 0, 0.25)


def test_the_padding_of_the_edge_maps_is_poison():
    """read as pixels, the padding columns would match every vertex that projects there"""
    v, n, _, _ = C.edge_values_vertices()
    vs, ns = C.edge_values_maps()
    pad = slice(C.EV["cols"], None)
    assert np.isfinite(vs[:, pad]).all() and np.isfinite(ns[:, pad]).all()
    _, ok, *_ = RS.rigid_sums64(np.array([[0, 0, 1]], np.float32), None, C.IDENT, vs[:, pad], ns[:, pad], (4.0, 4.0, 1.0, 2.0), 0.25, 0.5)
    assert ok.all()


@pytest.mark.parametrize("name", list(C.CASES))
def test_no_shape_case_has_a_knife_edge_vertex_or_passes_on_empty_sums(name):
    c = C.inputs(name)
    _, ok, _, sum64, abs64, knife = C.stated(name)
    N = len(c["vertices"])
    assert knife == 0
    assert N == (C.CASES[name][1] if C.CASES[name][1] is not None else N)
    if N >= 63:
        assert ok.sum() >= 0.3 * N, (int(ok.sum()), N)  # icp_cases' floor
    if N == 0:
        assert not sum64.any() and not abs64.any()


def test_variants_of_one_case_state_the_same_sums():
    """stride 4 (the 4th float NaN) and padded maps are storage only"""
    a, b = C.stated("80x60 NEAR"), C.stated("80x60 stride 4")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = C.stated("53x37 NEAR"), C.stated("53x37 padded")
    assert np.array_equal(a[0], b[0])
    assert C.stated("80x60 no normals")[1].sum() > C.stated("80x60 NEAR")[1].sum()  # the cosine gate does reject


def test_the_constants_of_the_per_sum_bar_are_four_times_the_measured_deviations():
    """c of |got[q] - sum64[q]| <= c 2^-24 abs64[q]: the largest deviation of the float32 statement (rounded to float32, as
    the kernel delivers its sums) from sum64 over the cases, in units of 2^-24 abs64[q]; c is 4 times that, rounded up to a
    power of two.  The nearly converged cases have a constant of their own, as in icp_cases."""
    worst = {False: 0.0, True: 0.0}
    for name in C.CASES:
        sums, ok, _, sum64, abs64, _ = C.stated(name)
        u = float(St.per_sum_units(sums.astype(np.float32), sum64, abs64).max())
        print("%-32s matched %5d units %9.1f" % (name, ok.sum(), u))
        conv = name in C.CONVERGED_CASES
        worst[conv] = max(worst[conv], u)
    print("largest deviations in units of 2^-24 abs64:", worst)
    assert worst[False] == pytest.approx(C.MEASURED_UNITS, rel=5e-3)
    assert worst[True] == pytest.approx(C.MEASURED_UNITS_CONVERGED, rel=5e-3)
    assert C.C_BAR == 2 ** int(np.ceil(np.log2(4 * worst[False])))
    assert C.C_BAR_CONVERGED == 2 ** int(np.ceil(np.log2(4 * worst[True])))


def test_pose_bar_is_four_times_the_float32_to_fp64_trajectory_gap():
    """10 iterations from the identity at 80 x 60, once driven by the float32 statement's sums rounded to float32 and once by
    sum64, both through icp_update.  The largest pose-entry difference is the measured reference of the GPU-driven
    trajectory's bar, C.POSE_BAR = icp_cases.pose_bar(gap).  Both recover motion() within tests/cpp/test_host_icp.cpp's bars."""
    a, b = C.trajectory(C.sums32), C.trajectory(C.sums64)
    gap = C.pose_gap(a, b)
    print("gap", gap, "bar", K.pose_bar(gap))
    assert gap == pytest.approx(C.MEASURED_POSE_GAP, rel=0.25)
    assert C.POSE_BAR == K.pose_bar(C.MEASURED_POSE_GAP)
    R, t = K.motion()
    for traj in (a, b):
        final = traj[-1].astype(np.float64)
        assert np.abs(final[:9].reshape(3, 3) - R).max() <= 3e-3 and np.abs(final[9:] - t).max() <= 5e-3


def test_compose_rigid_is_the_composition():
    P = C.invariance_problem()
    dq = P["node_dq"].astype(np.float64)
    g = P["node_pos"].astype(np.float64)
    for T in (C.T_SMALL, C.T_40):
        out = RS.compose_rigid(dq, T)
        assert np.abs(dq_point(out, g) - RS.apply_rigid(T, dq_point(dq, g))).max() <= 1e-12
        assert np.abs((out[:, :4] ** 2).sum(1) - (dq[:, :4] ** 2).sum(1)).max() <= 1e-12
    ident = RS.compose_rigid(dq, C.IDENT)
    assert np.array_equal(ident, dq)


def test_the_north_star_blend_is_left_invariant():
    """For random nodes and two rigid T (0.6 degrees and 40 degrees), in float64: the blend of compose_rigid(dq, T) is T
    applied to the blend of dq, and every regulariser residual T_n g_m - T_m g_m keeps its norm.  The same difference with
    the blends evaluated in float32 is the measured reference of the GPU check of dfa_solver6_warp_with:
    C.INVARIANCE_BAR = 4 x C.MEASURED_INVARIANCE_GAP."""
    P = C.invariance_problem()
    dq, idx, wn, c, g = P["node_dq"], P["idx"], P["wn"], P["canon"], P["node_pos"].astype(np.float64)
    gap32 = 0.0
    for T in (C.T_SMALL, C.T_40):
        moved = RS.compose_rigid(dq, T)
        p0, p1 = RS.blend_points(dq, idx, wn, c), RS.blend_points(moved, idx, wn, c)
        assert np.abs(p1 - RS.apply_rigid(T, p0)).max() <= 1e-12
        assert np.abs(p0 - c).max() > 1e-3  # the field does move the cloud
        n, m = np.meshgrid(np.arange(len(g)), np.arange(len(g)), indexing="ij")
        e0 = dq_point(dq.astype(np.float64)[n], g[m]) - dq_point(dq.astype(np.float64)[m], g[m])
        e1 = dq_point(moved[n], g[m]) - dq_point(moved[m], g[m])
        assert np.abs(np.linalg.norm(e1, axis=-1) - np.linalg.norm(e0, axis=-1)).max() <= 1e-12
        assert np.linalg.norm(e0, axis=-1).max() > 1e-2
        q0 = RS.blend_points(dq, idx, wn.astype(np.float32), c, np.float32)
        q1 = RS.blend_points(moved.astype(np.float32), idx, wn.astype(np.float32), c, np.float32)
        gap32 = max(gap32, float(np.abs(q1.astype(np.float64) - RS.apply_rigid(T, q0)).max()))
    print("float32 gap", gap32)
    assert gap32 == pytest.approx(C.MEASURED_INVARIANCE_GAP, rel=0.25)
    assert C.INVARIANCE_BAR == pytest.approx(4 * C.MEASURED_INVARIANCE_GAP, rel=1e-12)
