"""-m gpu tests of dfa_rigid_align_cloud (dynfu_amd/csrc/icp.hip: rigid_loop_rows_kernel, rigid_loop_step_kernel; the step
itself is csrc/rigid_step.hpp) on the schedules of tests/rigid_loop_cases.py.  With the trace of a call, iteration by
iteration: the 27 sums and the matched count are, bit for bit, dfa_rigid_sums_cloud's at the traced pose over a contiguous
copy of the level's vertices; the next pose is img_statement.icp_update's of those sums within 2 float32 ulps or 1e-7 (the
bar of the host step's known answers); the iterations per level are the statement's exactly (the CPU test keeps every
decision off its knife edge); rows that did not run stay NaN; the final pose is within the recorded bar of the fp64-driven
loop."""
import ctypes as C_

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import icp_cases as K  # noqa: E402
import img_statement as St  # noqa: E402
import rigid_align_cases as C  # noqa: E402
import rigid_loop_cases as L  # noqa: E402
import rigid_loop_statement as LS  # noqa: E402
from gpu_util import bits, dev, host  # noqa: E402

NAN_BITS = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _maps(c):
    """the case's maps on the device, pitched when the case says so (the padding finite: a point and a normal that would match)"""
    if not c["pad"]:
        return dev(c["vmap"]), dev(c["nmap"])
    cols = c["vmap"].shape[1]
    wide_v, _ = C.pitched(c["vmap"], c["pad"], (0.0, 0.0, 1.5, 0.0))
    wide_n, _ = C.pitched(c["nmap"], c["pad"], (0.0, 0.0, -1.0, 0.0))
    v, n = dev(wide_v)[:, :cols], dev(wide_n)[:, :cols]
    assert not v.is_contiguous() and v.stride(0) == (cols + c["pad"]) * 4
    return v, n


def _run(A, name, maps=None, stream=None, trace=True, aff0=None, **kw):
    c, steps, iters, stop_rot, stop_trans = L.inputs(name)
    v, n = maps or _maps(c)
    a = dict(level_step=steps, level_iters=iters, stop_rot=stop_rot, stop_trans=stop_trans)
    a.update(kw)
    return A.rigid_align_cloud(dev(c["vertices"]), None if c["normals"] is None else dev(c["normals"]),
                               L.IDENT if aff0 is None else aff0, v, n, c["intr"], trace=trace, stream=stream, **L.GATES, **a)


def _within_step_bar(got, want):
    """2 float32 ulps of the entry's magnitude or 1e-7, per entry (tests/cpp/test_host_icp.cpp's bar)"""
    want = want.astype(np.float64)
    mag = np.where(want != 0, np.abs(want), 1e-30)
    tol = np.maximum(2.0 * 2.0 ** (np.floor(np.log2(mag)) - 23), 1e-7)
    return bool((np.abs(got.astype(np.float64) - want) <= tol).all())


def _check_trace(A, name, out):
    """the per-iteration checks of the module docstring; -> the traced rows that ran, as (level, sums, matched, pose)"""
    c, steps, iters, _, _ = L.inputs(name)
    maps = _maps(c)
    tr = host(out["trace"])
    sched = [l for l, k in enumerate(iters) for _ in range(k)]
    assert tr.shape == (len(sched), 40)
    level_cloud = {}
    ran = []
    for g, l in enumerate(sched):
        row = tr[g]
        if (bits(row) == NAN_BITS).all():
            continue
        if l not in level_cloud:
            v = dev(np.ascontiguousarray(c["vertices"][::steps[l]]))
            n = None if c["normals"] is None else dev(np.ascontiguousarray(c["normals"][::steps[l]]))
            level_cloud[l] = (v, n)
        v, n = level_cloud[l]
        pose, matched = row[28:40].copy(), int(row[27:28].view(np.uint32)[0])
        sums, m = A.rigid_sums_cloud(v, n, pose, maps[0], maps[1], c["intr"], **L.GATES)
        assert np.array_equal(bits(host(sums)), bits(row[:27])), (name, g)
        assert m == matched, (name, g, m, matched)
        ran.append((g, l, row[:27].copy(), matched, pose))
    for k, (g, l, sums, matched, pose) in enumerate(ran):
        ok, want = St.icp_update(sums.astype(np.float64), pose)
        if k + 1 < len(ran):
            assert ok and _within_step_bar(ran[k + 1][4], want), (name, g)
        elif out["status"] == 0:
            assert ok and _within_step_bar(out["aff"], want), (name, g)
        else:
            assert not ok, (name, g)
    assert ran and out["matched_first"] == ran[0][3] and out["matched_last"] == ran[-1][3]
    assert [sum(1 for r in ran if r[1] == l) for l in range(len(steps))] == out["iters_run"]
    return ran


@pytest.mark.parametrize("name", list(L.SCHEDULES))
def test_every_traced_iteration_is_the_one_linearisation_and_the_host_step(A, name):
    out = _run(A, name)
    want, want64 = L.stated(name), L.stated(name, True)
    ran = _check_trace(A, name, out)
    assert out["status"] == 0 and out["iters_run"] == want["iters_run"]
    assert [g for g, *_ in ran] == [g for g, r in enumerate(want["rows"]) if r is not None]  # the other rows are NaN
    assert np.array_equal(ran[0][4], L.IDENT)
    gap = float(np.abs(out["aff"].astype(np.float64) - want64["aff"]).max())
    print(name, "iterations", out["iters_run"], "gap to the fp64-driven loop", gap, "bar", L.POSE_BAR[name])
    assert gap <= L.POSE_BAR[name]
    # the last accepted twist's norms: the statement's of the last traced sums (both solve in double; float32 on the way out)
    _, x = LS.twist(ran[-1][2].astype(np.float64))
    assert out["last_rot"] == pytest.approx(np.linalg.norm(x[:3]), rel=1e-5)
    assert out["last_trans"] == pytest.approx(np.linalg.norm(x[3:]), rel=1e-5)
    if name == L.STOP:
        assert out["iters_run"] == L.STOP_ITERS_RUN


def test_ten_iterations_at_full_resolution_reproduce_the_trajectory_driven_through_rigid_sums_cloud(A):
    c = C.inputs("80x60 NEAR")
    maps = _maps(c)
    v, n = dev(c["vertices"]), dev(c["normals"])

    def kernel_sums(case, aff):
        return host(A.rigid_sums_cloud(v, n, aff, maps[0], maps[1], case["intr"], **C.GATES)[0]).astype(np.float64)
    want = C.trajectory(kernel_sums)
    out = _run(A, "full 1x10", maps=maps)
    tr = host(out["trace"])
    got = [tr[g, 28:40] for g in range(1, C.ITERS)] + [out["aff"]]
    gap = C.pose_gap(got, [w.astype(np.float64) for w in want])
    print("gap", gap, "bar", C.POSE_BAR)
    assert gap <= C.POSE_BAR
    R, t = K.motion()
    final = out["aff"].astype(np.float64)
    assert np.abs(final[:9].reshape(3, 3) - R).max() <= 3e-3 and np.abs(final[9:] - t).max() <= 5e-3
    assert out["matched_last"] >= out["matched_first"] > 0


def test_thresholds_above_every_norm_run_one_iteration_per_level(A):
    out = _run(A, "4-2-1", stop_rot=1e30, stop_trans=1e30)
    assert out["status"] == 0 and out["iters_run"] == [1, 1, 1]
    ran = _check_trace(A, "4-2-1", out)
    assert [g for g, *_ in ran] == [0, 4, 9]
    # one threshold alone does not stop
    out = _run(A, "4-2-1", stop_rot=1e30, stop_trans=0.0, trace=False)
    assert out["iters_run"] == [4, 5, 10] and out["trace"] is None


@pytest.mark.parametrize("name", list(L.SINGULAR))
def test_a_level_of_one_vertex_is_singular(A, name):
    aff0 = C.inputs("80x60 NEAR")["aff"]
    out = _run(A, name, aff0=aff0)
    iters = L.inputs(name)[2]
    assert out["status"] == 1 and out["iters_run"] == [1] + [0] * (len(iters) - 1)
    assert np.array_equal(bits(out["aff"]), bits(aff0))
    tr = host(out["trace"])
    assert not (bits(tr[0]) == NAN_BITS).any() and (bits(tr[1:]) == NAN_BITS).all()
    assert np.array_equal(bits(tr[0, 28:40]), bits(aff0)) and out["matched_first"] == out["matched_last"] == int(tr[0, 27:28].view(np.uint32)[0])


def test_no_vertices_and_maps_of_nan_are_singular(A):
    import torch
    c = C.inputs("80x60 NEAR")
    aff0 = c["aff"]
    v, n = _maps(c)
    kw = dict(level_step=(4, 1), level_iters=(2, 3), trace=True, **L.GATES)
    none = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    nan = torch.full_like(v, float("nan"))
    for out in (A.rigid_align_cloud(none, none, aff0, v, n, c["intr"], **kw),
                A.rigid_align_cloud(none, None, aff0, v, n, c["intr"], **kw),
                A.rigid_align_cloud(dev(c["vertices"]), dev(c["normals"]), aff0, nan, nan, c["intr"], **kw)):
        assert out["status"] == 1 and out["iters_run"] == [1, 0] and np.array_equal(bits(out["aff"]), bits(aff0))
        assert out["matched_first"] == out["matched_last"] == 0
        tr = host(out["trace"])
        assert not tr[0, :27].any() and np.array_equal(bits(tr[0, 28:40]), bits(aff0)) and (bits(tr[1:]) == NAN_BITS).all()
    # no iterations at all: the report alone, the pose aff0
    out = A.rigid_align_cloud(dev(c["vertices"]), dev(c["normals"]), aff0, v, n, c["intr"], level_step=(4, 1), level_iters=(0, 0),
                              trace=True, **L.GATES)
    assert out["status"] == 0 and out["iters_run"] == [0, 0] and np.array_equal(bits(out["aff"]), bits(aff0))
    assert out["trace"].shape == (0, 40) and out["matched_first"] == 0


def test_two_calls_and_two_streams_give_the_same_bits(A):
    import torch
    names = ["16-4-1 stop 2e-5", "padded maps"]
    maps = [_maps(L.inputs(nm)[0]) for nm in names]
    alone = [_run(A, nm, maps=mp) for nm, mp in zip(names, maps)]
    again = [_run(A, nm, maps=mp) for nm, mp in zip(names, maps)]

    def same(a, b):
        return (np.array_equal(bits(a["aff"]), bits(b["aff"])) and np.array_equal(bits(host(a["trace"])), bits(host(b["trace"])))
                and a["iters_run"] == b["iters_run"] and a["matched_last"] == b["matched_last"]
                and a["last_rot"] == b["last_rot"] and a["last_trans"] == b["last_trans"])
    for a, b in zip(alone, again):
        assert a["status"] == 0 and same(a, b)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(3):
        for k in (0, 1):  # each (device, stream) has its own state and partial sums
            assert same(_run(A, names[k], maps=maps[k], stream=streams[k]), alone[k])


def test_a_bad_schedule_is_refused_without_a_launch(A):
    import torch
    from dynfu_amd import _lib
    c = C.inputs("80x60 N=65")
    v, n = _maps(c)
    cloud, normals = dev(c["vertices"]), dev(c["normals"])
    report = torch.full((C_.sizeof(_lib.RigidAlignReport),), 7, dtype=torch.uint8, device="cuda")
    trace = torch.full((64, 40), 7.0, dtype=torch.float32, device="cuda")

    def call(steps, iters, levels=None, stop_rot=0.0, stop_trans=0.0):
        arr = lambda a: None if a is None else (C_.c_int * max(len(a), 1))(*a)  # noqa: E731
        return _lib.load().dfa_rigid_align_cloud(
            C_.c_void_p(cloud.data_ptr()), C_.c_void_p(normals.data_ptr()), 3, 65, _lib._aff12(L.IDENT), C_.c_void_p(v.data_ptr()),
            v.stride(0) * 4, C_.c_void_p(n.data_ptr()), n.stride(0) * 4, v.shape[1], v.shape[0], *[float(x) for x in c["intr"]], 0.1, 0.5,
            arr(steps), arr(iters), len(steps) if levels is None else levels, stop_rot, stop_trans,
            C_.c_void_p(report.data_ptr()), C_.c_void_p(trace.data_ptr()), _lib._stream())
    INVALID = 1  # DFA_ERR_INVALID
    bad = [dict(steps=(1,), iters=(1,), levels=0), dict(steps=(1,) * 5, iters=(1,) * 5), dict(steps=(0,), iters=(1,)),
           dict(steps=(4, -1), iters=(1, 1)), dict(steps=(1,), iters=(-1,)), dict(steps=(1,), iters=(65,)),
           dict(steps=(4, 2, 1), iters=(30, 30, 5)), dict(steps=None, iters=(1,), levels=1), dict(steps=(1,), iters=None, levels=1),
           dict(steps=(1,), iters=(1,), stop_rot=-1.0), dict(steps=(1,), iters=(1,), stop_trans=float("nan"))]
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert b"dfa_rigid_align_cloud" in _lib.load().dfa_last_error()
    torch.cuda.synchronize()
    assert (host(report) == 7).all() and (host(trace) == 7.0).all()  # nothing was enqueued
    assert call((4, 2, 1), (30, 30, 4)) == 0  # 64 iterations in all
    torch.cuda.synchronize()
    r = _lib.RigidAlignReport.from_buffer_copy(host(report).tobytes())
    assert r.status in (0, 1) and r.iters_run[0] >= 1 and r.iters_run[3] == 0  # (17 vertices in the first level: either)
    with pytest.raises(A.DynfuAmdError):
        A.rigid_align_cloud(cloud, normals, L.IDENT, v, n, c["intr"], 0.1, 0.5, (4, 1), (1,))
    with pytest.raises(A.DynfuAmdError):
        A.rigid_align_cloud(cloud, normals, L.IDENT, v, n, c["intr"], 0.1, 0.5, (), ())
