"""-m gpu tests of dfa_rigid_sums_cloud (dynfu_amd/csrc/icp.hip, rigid_rows_cloud_kernel) against the statements of
tests/rigid_align_statement.py on the cases of tests/rigid_align_cases.py: every sum within the recorded per-sum bar of the
fp64 statement (c measured on the CPU by tests/test_rigid_align_statement_cpu.py), the matched count exact (no case has a
knife-edge vertex, checked there), the hand-made edge values vertex by vertex and as a whole, the same bits on every call
and on two streams, the GPU-driven trajectory within the recorded pose bar of the fp64-driven one, and the left-invariance
of the north-star blend on the device (dfa_solver6_warp_with)."""
import ctypes as C_

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import icp_cases as K  # noqa: E402
import img_statement as St  # noqa: E402
import rigid_align_cases as C  # noqa: E402
import rigid_align_statement as RS  # noqa: E402
from gpu_util import bits, dev, host  # noqa: E402


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


def _gpu(A, c, aff=None, maps=None, stream=None):
    v, n = maps or _maps(c)
    sums, m = A.rigid_sums_cloud(dev(c["vertices"]), None if c["normals"] is None else dev(c["normals"]),
                                 c["aff"] if aff is None else aff, v, n, c["intr"], stream=stream, **C.GATES)
    return host(sums), m


@pytest.mark.parametrize("name", list(C.CASES))
def test_sums_within_the_per_sum_bar_and_matched_exact(A, name):
    c = C.inputs(name)
    want, ok, _, sum64, abs64, knife = C.stated(name)
    got, m = _gpu(A, c)
    print(name, "matched", m, "units", St.per_sum_units(got, sum64, abs64).max(), "bar", C.c_of(name))
    assert knife == 0 and m == int(ok.sum())
    assert C.within_bar(got, sum64, abs64, C.c_of(name))
    if len(ok) == 0:
        assert not got.any()


def _edge(normals):
    v, n, want, want_no_n = C.edge_values_vertices()
    vs, ns = C.edge_values_maps()
    cols = C.EV["cols"]
    return v, (n if normals else None), (want if normals else want_no_n), vs, ns, cols


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("normals", [True, False])
def test_edge_values_vertex_by_vertex_and_as_a_whole(A, normals, stride):
    v, n, want, vs, ns, cols = _edge(normals)
    dv, dn = dev(vs)[:, :cols], dev(ns)[:, :cols]  # 3 padding columns of poison
    gates = dict(dist_thresh=C.EV["dist_thresh"], cos_thresh=C.EV["cos_thresh"])

    def run(sl):
        vv = dev(C.with_stride(v[sl], stride))
        nn = None if n is None else dev(C.with_stride(n[sl], stride))
        sums, m = A.rigid_sums_cloud(vv, nn, C.IDENT, dv, dn, C.EV["intr"], **gates)
        s32, ok, _, sum64, abs64, _ = RS.rigid_sums64(v[sl], None if n is None else n[sl], C.IDENT, vs[:, :cols], ns[:, :cols],
                                                      C.EV["intr"], gates["dist_thresh"], gates["cos_thresh"])
        return host(sums), m, s32, ok, sum64, abs64
    for i in range(len(v)):
        got, m, s32, ok, sum64, abs64 = run(slice(i, i + 1))
        assert m == want[i] == int(ok.sum()), i
        assert np.array_equal(got.astype(np.float64), s32), i  # one vertex: float32 products, nothing to add
    got, m, s32, ok, sum64, abs64 = run(slice(None))
    assert m == int(want.sum()) == int(ok.sum())
    assert C.within_bar(got, sum64, abs64, C.C_BAR)


def test_two_calls_and_two_streams_give_the_same_bits(A):
    import torch
    cases = [C.inputs("80x60 NEAR"), C.inputs("53x37 padded")]
    maps = [_maps(c) for c in cases]
    alone = [_gpu(A, c, maps=mp) for c, mp in zip(cases, maps)]
    again = [_gpu(A, c, maps=mp) for c, mp in zip(cases, maps)]
    for (s0, m0), (s1, m1) in zip(alone, again):
        assert m0 == m1 > 0 and np.array_equal(bits(s0), bits(s1))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(3):
        for k in (0, 1):  # each (device, stream) has its own partial-sum scratch
            s, m = _gpu(A, cases[k], maps=maps[k], stream=streams[k])
            assert m == alone[k][1] and np.array_equal(bits(s), bits(alone[k][0]))


def test_no_vertices_give_zeros(A):
    import torch
    c = C.inputs("80x60 N=0")
    got, m = _gpu(A, c)
    assert m == 0 and got.shape == (27,) and not got.any() and not np.signbit(got).any()
    # through the C ABI with NULL clouds and a sums buffer full of NaN
    from dynfu_amd import _lib
    v, n = _maps(c)
    sums = torch.full((27,), float("nan"), dtype=torch.float32, device="cuda")
    rc = _lib.load().dfa_rigid_sums_cloud(None, None, 3, 0, _lib._aff12(C.IDENT), C_.c_void_p(v.data_ptr()), v.stride(0) * 4,
                                          C_.c_void_p(n.data_ptr()), n.stride(0) * 4, v.shape[1], v.shape[0], *[float(x) for x in c["intr"]],
                                          0.1, 0.5, C_.c_void_p(sums.data_ptr()), None, _lib._stream())
    torch.cuda.synchronize()
    assert rc == 0 and not host(sums).any()


def test_bad_arguments_are_refused_without_a_launch(A):
    import torch
    from dynfu_amd import _lib
    c = C.inputs("80x60 N=65")
    v, n = _maps(c)
    cloud, normals = dev(c["vertices"]), dev(c["normals"])
    sums = torch.full((27,), 7.0, dtype=torch.float32, device="cuda")
    matched = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    good = dict(vertices=cloud.data_ptr(), normals=normals.data_ptr(), stride=3, N=65, vmap=v.data_ptr(), vstep=v.stride(0) * 4,
                nmap=n.data_ptr(), nstep=n.stride(0) * 4, cols=v.shape[1], rows=v.shape[0], fx=c["intr"][0], fy=c["intr"][1],
                dist=0.1)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        p = lambda x: C_.c_void_p(x) if x else None  # noqa: E731
        return _lib.load().dfa_rigid_sums_cloud(p(a["vertices"]), p(a["normals"]), a["stride"], a["N"], _lib._aff12(c["aff"]), p(a["vmap"]),
                                                a["vstep"], p(a["nmap"]), a["nstep"], a["cols"], a["rows"], float(a["fx"]), float(a["fy"]),
                                                float(c["intr"][2]), float(c["intr"][3]), float(a["dist"]), 0.5,
                                                C_.c_void_p(sums.data_ptr()), C_.c_void_p(matched.data_ptr()), _lib._stream())
    INVALID = 1  # DFA_ERR_INVALID
    bad = [dict(stride=2), dict(stride=5), dict(N=-1), dict(vertices=0), dict(vmap=0), dict(nmap=0), dict(cols=0), dict(rows=-3),
           dict(vstep=good["cols"] * 16 - 16), dict(nstep=good["cols"] * 16 - 16), dict(vstep=good["vstep"] + 4),
           dict(nstep=good["nstep"] + 8), dict(vmap=good["vmap"] + 4), dict(nmap=good["nmap"] + 8), dict(dist=-0.1),
           dict(dist=float("nan")), dict(fx=0.0), dict(fy=0.0)]
    for kw in bad:
        assert call(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert (host(sums) == 7.0).all() and int(host(matched)[0]) == 7  # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    assert int(host(matched)[0]) == int(C.stated("80x60 N=65")[1].sum())
    with pytest.raises(A.DynfuAmdError):
        A.rigid_sums_cloud(cloud, normals, C.IDENT, v, n, (0.0, 1.0, 0.0, 0.0), 0.1, 0.5)


def test_the_gpu_driven_trajectory_follows_the_fp64_one(A):
    """10 iterations from the identity at 80 x 60: the kernel's sums and the statement's sum64 each drive St.icp_update.  After
    every iteration the two poses agree to C.POSE_BAR, 4 times the float32-to-fp64 gap measured on the CPU, the kernel's
    matched count is the statement's at the same pose (or within its knife-edge count there), and the final pose recovers
    motion() to 3e-3 / 5e-3."""
    c = C.inputs("80x60 NEAR")
    maps = _maps(c)
    counts = []

    def kernel_sums(case, aff):
        got, m = _gpu(A, case, aff=aff, maps=maps)
        _, ok, _, _, _, knife = RS.rigid_sums64(case["vertices"], case["normals"], aff, case["vmap"], case["nmap"], case["intr"], **C.GATES)
        counts.append((m, int(ok.sum()), knife))
        return got.astype(np.float64)
    got, want = C.trajectory(kernel_sums), C.trajectory(C.sums64)
    for it, (m, n, knife) in enumerate(counts):
        assert abs(m - n) <= knife, (it, m, n, knife)
    gap = C.pose_gap(got, want)
    print("gap", gap, "bar", C.POSE_BAR)
    assert gap <= C.POSE_BAR
    R, t = K.motion()
    final = got[-1].astype(np.float64)
    assert np.abs(final[:9].reshape(3, 3) - R).max() <= 3e-3 and np.abs(final[9:] - t).max() <= 5e-3
    assert counts[-1][0] >= counts[0][0]


def test_warp_with_of_the_composed_transforms_is_the_rigid_motion_of_the_warp(A):
    """left-invariance on the device: a plan of D = 37 nodes, N = 1031 vertices, k = 8; dfa_solver6_warp_with of
    compose_rigid(dq, T) equals T applied to warp_with(dq) within C.INVARIANCE_BAR (4 x the float32 difference measured on the
    CPU), for a small T and one of 40 degrees; the normals rotate with it."""
    P = C.invariance_problem()
    plan = A.Solver6(C.INV_D, C.INV_N, C.INV_K)
    plan.set_problem(dev(P["node_pos"]), dev(P["node_dq"]), dev(P["node_w"]), dev(P["canon"]), dev(P["canon_n"]))
    v0, n0 = (host(x).astype(np.float64) for x in plan.warp_with(dev(P["node_dq"])))
    assert np.abs(v0 - P["canon"]).max() > 1e-3
    for T in (C.T_SMALL, C.T_40):
        moved = RS.compose_rigid(P["node_dq"], T).astype(np.float32)
        v1, n1 = (host(x).astype(np.float64) for x in plan.warp_with(dev(moved)))
        gap = np.abs(v1 - RS.apply_rigid(T, v0)).max()
        print("gap", gap, "bar", C.INVARIANCE_BAR)
        assert gap <= C.INVARIANCE_BAR
        assert np.abs(n1 - n0 @ T[:9].reshape(3, 3).T).max() <= C.INVARIANCE_BAR
    plan.close()
