"""The statement of dfa_rigid_align_cloud (tests/rigid_loop_statement.py) on the schedules of tests/rigid_loop_cases.py, on the
CPU: it measures the constants the GPU test's bars come from and checks that the decisions the GPU test compares exactly —
refused or not, stopped or not — are nowhere near a knife edge in the statement."""
import numpy as np
import pytest

import icp_cases as K
import rigid_align_cases as C
import rigid_loop_cases as L
import rigid_loop_statement as LS


@pytest.mark.parametrize("name", list(L.SCHEDULES))
def test_pose_bar_is_four_times_the_float32_to_fp64_gap_and_no_update_is_refused(name):
    a, b = L.stated(name), L.stated(name, True)
    assert a["status"] == 0 and b["status"] == 0
    assert a["iters_run"] == b["iters_run"]
    for r in (r for r in a["rows"] + b["rows"] if r is not None):
        assert abs(r["det"]) > 100 * LS.DET_GATE  # two decades clear of the determinant gate (the smallest is 1.2)
    gap = L.pose_gap(a, b)
    print(name, "iterations", a["iters_run"], "gap", gap, "bar", K.pose_bar(gap))
    assert gap == pytest.approx(L.MEASURED_POSE_GAP[name], rel=0.25)
    assert L.POSE_BAR[name] == K.pose_bar(L.MEASURED_POSE_GAP[name])
    if L.inputs(name)[3] == 0.0:
        assert a["iters_run"] == list(L.inputs(name)[2])  # thresholds of 0 never stop
        assert all(r is not None for r in a["rows"])


def test_the_full_resolution_schedule_is_the_trajectory_of_rigid_align_cases():
    a = L.stated("full 1x10")
    want = C.trajectory(C.sums32)
    assert len(a["poses"]) == C.ITERS and all(np.array_equal(x, y) for x, y in zip(a["poses"], want))
    R, t = K.motion()
    final = a["aff"].astype(np.float64)
    assert np.abs(final[:9].reshape(3, 3) - R).max() <= 3e-3 and np.abs(final[9:] - t).max() <= 5e-3


def test_no_step_norm_of_the_stop_schedule_is_within_a_factor_two_of_its_threshold():
    _, steps, iters, stop_rot, stop_trans = L.inputs(L.STOP)
    a = L.stated(L.STOP)
    assert a["iters_run"] == L.STOP_ITERS_RUN and a["iters_run"] == L.stated(L.STOP, True)["iters_run"]
    nearest = []
    for r in (r for r in a["rows"] if r is not None):
        for norm, th in ((r["rot"], stop_rot), (r["trans"], stop_trans)):
            assert not (th / 2 <= norm <= 2 * th), (r["level"], norm, th)
            nearest.append(norm)
    above, below = min(n for n in nearest if n > stop_rot), max(n for n in nearest if n < stop_rot)
    print("nearest above", above, "below", below)
    assert above == pytest.approx(4.4e-5, rel=0.05) and below == pytest.approx(6.3e-6, rel=0.05)
    # rows of the launches behind a stop did not run; the level after a stop starts from the pose reached
    sched = [l for l, n in enumerate(iters) for _ in range(n)]
    assert [r is not None for r in a["rows"]] == [k < 4 or 4 <= k < 6 or 9 <= k < 13 for k in range(len(sched))]
    assert np.array_equal(a["rows"][9]["pose"], a["poses"][5])


def test_a_stop_threshold_above_every_norm_runs_one_iteration_per_level():
    c, steps, iters, _, _ = L.inputs("4-2-1")
    a = LS.run(c["vertices"], c["normals"], L.IDENT, c["vmap"], c["nmap"], c["intr"], L.GATES, steps, iters, 1e30, 1e30)
    assert a["status"] == 0 and a["iters_run"] == [1, 1, 1]


@pytest.mark.parametrize("name", list(L.SINGULAR))
def test_a_level_of_one_vertex_is_refused_far_below_the_gate(name):
    a = L.stated(name)
    ran = [r for r in a["rows"] if r is not None]
    assert a["status"] == 1 and len(ran) == 1 and ran[0]["matched"] == 1 and abs(ran[0]["det"]) < 1e-10 * LS.DET_GATE
    assert a["iters_run"][0] == 1 and sum(a["iters_run"]) == 1 and np.array_equal(a["aff"], L.IDENT)


def test_an_empty_cloud_and_maps_without_a_pixel_are_singular():
    c = C.inputs("80x60 NEAR")
    none = np.empty((0, 3), np.float32)
    a = LS.run(none, none, L.IDENT, c["vmap"], c["nmap"], c["intr"], L.GATES, (4, 1), (2, 3))
    assert a["status"] == 1 and a["iters_run"] == [1, 0] and a["matched_first"] == 0 and np.array_equal(a["aff"], L.IDENT)
    nan = np.full_like(c["vmap"], np.nan)
    a = LS.run(c["vertices"], c["normals"], L.IDENT, nan, nan, c["intr"], L.GATES, (4, 1), (2, 3))
    assert a["status"] == 1 and a["iters_run"] == [1, 0] and a["matched_first"] == 0
