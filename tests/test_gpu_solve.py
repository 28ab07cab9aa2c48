"""-m gpu parity tests of the solver seam vs the CPU oracle and the reference's OptTest scenes.

Tolerances (float32 PCG on the GPU vs float64 oracle):
  * OptTest scenes: the reference's own bar, |warp(src) - target| <= 1e-3 per axis
    (test/opt_optimisation_test.cpp:94) — rank-deficient systems, so warped vertices are
    compared, not node translations (SURVEY.md §7 "Under-determined solves");
  * well-posed problems (lambda > 0, N >> D): node translations within 2e-5 m of the float64
    oracle (|t| ~ 1e-2 m, i.e. 2e-3 relative) and final cost within 1e-3 relative.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import dev, host  # noqa: E402
from opt_scene_runner import SCN, run_scene, scene_ids  # noqa: E402


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _params(A, **kw):
    d = dict(num_iter=1, nonlinear_iter=1, linear_iter=256, tukey_offset=4.652, psi_data=0.01, lambda_=0.0,
             psi_reg=1e-4, pcg_tol=0.0, gn_tol=0.0)
    d.update(kw)
    return A.SolveParams(**d)


def _hip_solve(A, prm):
    def solve(node_pos, node_dq, node_w, k, canon, live):
        s = A.Solver(len(node_pos), len(canon), k)
        s.set_problem(dev(node_pos), dev(node_dq), dev(node_w), dev(canon), dev(live))
        s.solve(prm)
        out = host(s.node_dq())
        st = s.stats()
        assert st["final_cost"] <= st["initial_cost"] * (1 + 1e-6) + 1e-12
        s.close()
        return out

    return solve


def _hip_warp(A):
    def warp(node_pos, node_dq, node_w, k, verts):
        return host(A.warp_to_live(dev(node_pos), dev(node_dq), dev(node_w), k, dev(verts))[0])

    return warp


@pytest.mark.parametrize("scene", SCN["scenes"], ids=scene_ids())
def test_reference_opttest_scenes(A, scene):
    P = SCN["params"]
    prm = _params(A, num_iter=P["numIter"], nonlinear_iter=P["nonLinearIter"], linear_iter=P["linearIter"],
                  tukey_offset=SCN["tukeyOffset"], psi_data=SCN["psi_data"], lambda_=SCN["lambda_"],
                  psi_reg=SCN["psi_reg"])
    worst, log = run_scene(scene, _hip_solve(A, prm), _hip_warp(A))
    assert worst <= SCN["tol"], log


def _problem(name, frame=3, n_verts=None):
    cfg = synth.CONFIGS[name]
    c = synth.canonical(cfg)
    k = cfg["k"]
    verts = c["verts"] if n_verts is None else c["verts"][:n_verts]
    idx = O.knn(c["node_pos"], verts, k, threads=8)
    w = np.zeros(idx.shape, np.float32)
    for v in range(len(verts)):
        for j in range(k):
            w[v, j] = O.transformation_weight(c["node_pos"][idx[v, j]], float(c["node_w"][idx[v, j]]), verts[v])
    t_true = synth.true_translations(c["node_pos"], frame, cfg["k"])
    live = synth.live_vertices(verts, idx, w, t_true)
    return cfg, c, verts, live, t_true


@pytest.mark.parametrize("name,lam", [("T0", 200.0), ("T1", 200.0), ("T0", 0.5)])
def test_translations_match_oracle_well_posed(A, name, lam):
    cfg, c, verts, live, t_true = _problem(name)
    k = cfg["k"]
    kw = dict(num_iter=3, nonlinear_iter=2, linear_iter=256, lambda_=lam)
    t_ref, dq_ref, st_ref = O.solve_ref(c["node_pos"], c["node_dq"], c["node_w"], k, verts, live, use_double=True,
                                        threads=8, **kw)
    s = A.Solver(cfg["D"], len(verts), k)
    s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
    s.solve(_params(A, **kw))
    t = host(s.translations())
    st = s.stats()
    assert np.array_equal(host(s.data_graph()), O.knn(c["node_pos"], verts, k, threads=8))
    assert np.array_equal(host(s.reg_graph()), O.knn(c["node_pos"], c["node_pos"], k))
    assert np.abs(t - t_ref).max() <= 2e-5, (np.abs(t - t_ref).max(), np.abs(t_ref).max())
    np.testing.assert_allclose(st["initial_cost"], st_ref["initial_cost"], rtol=1e-4)
    np.testing.assert_allclose(st["final_cost"], st_ref["final_cost"], rtol=1e-3, atol=1e-9)
    np.testing.assert_allclose(host(s.node_dq()), dq_ref, atol=2e-5)
    assert st["gn_iters"] == st_ref["gn_iters"]
    # the regulariser barely bends a smooth field: the ground truth is recovered
    if lam <= 1.0:
        assert np.abs(t - t_true).max() < 2e-3
    # the post-solve warpToLive through the plan's graph == the stand-alone entry point, bit for bit
    wv, wn = s.warp_to_live(dev(c["normals"]))
    rv, rn = A.warp_to_live(dev(c["node_pos"]), s.node_dq(), dev(c["node_w"]), k, dev(verts), dev(c["normals"]))
    assert np.array_equal(host(wv), host(rv)) and np.array_equal(host(wn), host(rn))
    s.close()


def test_tukey_and_huber_weights_match_oracle(A):
    cfg, c, verts, live, _ = _problem("T0")
    k = cfg["k"]
    rng = np.random.default_rng(2)
    live = live + rng.normal(0, 0.02, live.shape).astype(np.float32)  # some vertices beyond the cut-off
    dq = np.stack([O.dq_from_euler(0, 0, 0, *rng.uniform(-0.01, 0.01, 3)) for _ in range(cfg["D"])])
    s = A.Solver(cfg["D"], len(verts), k)
    s.set_problem(dev(c["node_pos"]), dev(dq), dev(c["node_w"]), dev(verts), dev(live))
    s.solve(_params(A, num_iter=1, nonlinear_iter=0, lambda_=200.0))  # weights only, no GN step
    tk = host(s.tukey_weights())
    ref = O.tukey_weights(c["node_pos"], dq, c["node_w"], k, verts, live, 4.652, 0.01, threads=8)
    assert 0.02 < (ref == 0).mean() < 0.98
    np.testing.assert_allclose(tk, ref, atol=3e-5)
    np.testing.assert_allclose(host(s.huber_weights()), O.huber_weights(c["node_pos"], dq, c["node_w"], k, 1e-4),
                               rtol=2e-3, atol=1e-6)
    assert np.all(host(s.translations()) == 0)
    s.close()


def test_early_exit_tolerances_reach_same_solution(A):
    cfg, c, verts, live, _ = _problem("T0")
    k = cfg["k"]
    out = []
    for kw in (dict(pcg_tol=0.0, gn_tol=0.0), dict(pcg_tol=1e-5, gn_tol=1e-7)):
        s = A.Solver(cfg["D"], len(verts), k)
        s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
        s.solve(_params(A, num_iter=2, nonlinear_iter=3, lambda_=200.0, **kw))
        out.append((host(s.translations()), s.stats()))
        s.close()
    assert np.abs(out[0][0] - out[1][0]).max() < 2e-6
    # a looser PCG tolerance leaves work for the next linearisation, so only the GN count and the
    # iteration budget are comparable
    assert out[1][1]["gn_iters"] <= out[0][1]["gn_iters"]
    assert out[1][1]["pcg_iters"] < 2 * 3 * 256 and out[0][1]["pcg_iters"] < 2 * 3 * 256


@pytest.mark.parametrize("name", ["C1", "C3", "C4"])
def test_large_configs_recover_the_ground_truth_field(A, name):
    """BASELINE configs C1 (512 nodes, k = 8), C3 (4096 nodes, k = 8, 524288 vertices) and C4 (8192 nodes, k = 8,
    1048576 vertices): the register-resident (C1) and the many-workgroup (C3, C4) PCG kernels recover the synthetic node
    translations; the graph equals the exhaustive-search graph on a sample of the vertices."""
    import torch
    cfg = synth.CONFIGS[name]
    c = synth.canonical(cfg)
    k, D = cfg["k"], cfg["D"]
    nodes, node_w, node_dq, verts = (dev(c[n]) for n in ("node_pos", "node_w", "node_dq", "verts"))
    idx, w = A.knn(nodes, node_w, verts, k)
    sample = np.arange(0, len(c["verts"]), 997)
    assert np.array_equal(host(idx)[sample], O.knn(c["node_pos"], c["verts"][sample], k, threads=8))
    t_true = synth.true_translations(c["node_pos"], 5, cfg["k"])
    live = dev(synth.live_vertices(c["verts"], host(idx), host(w), t_true))
    s = A.Solver(D, len(c["verts"]), k)
    s.set_problem(nodes, node_dq, node_w, verts, live)
    s.solve(_params(A, num_iter=3, nonlinear_iter=1, lambda_=1.0, pcg_tol=1e-6))
    st = s.stats()
    assert st["final_cost"] < 1e-4 * st["initial_cost"]
    warped, _ = A.warp_to_live(nodes, s.node_dq(), node_w, k, verts)
    assert float((warped - live).abs().max()) < 2e-4
    assert st["max_row_nnz"] <= 256
    s.close()


def test_degenerate_problems(A):
    """no vertices (regulariser only), a single node, fewer nodes than k, k = 1"""
    import torch
    z = lambda *sh: torch.zeros(sh, device="cuda")
    ident = lambda D: torch.tensor([[1.0, 0, 0, 0, 0, 0, 0, 0]] * D, device="cuda")
    nodes = torch.rand((16, 3), device="cuda")
    s = A.Solver(16, 0, 4)
    s.set_problem(nodes, ident(16), torch.full((16,), 0.3, device="cuda"), z(0, 3), z(0, 3))
    s.solve(_params(A, num_iter=2, nonlinear_iter=2, lambda_=10.0))
    assert float(s.translations().abs().max()) == 0.0  # nothing pulls the nodes
    s.close()
    for D, k in ((1, 4), (3, 8), (5, 1)):
        nodes = torch.rand((D, 3), device="cuda")
        verts = torch.rand((50, 3), device="cuda")
        live = verts + 0.01
        s = A.Solver(D, 50, k)
        s.set_problem(nodes, ident(D), torch.full((D,), 2.0, device="cuda"), verts, live)
        s.solve(_params(A, num_iter=2, nonlinear_iter=2, lambda_=0.0))
        st = s.stats()
        assert np.isfinite(st["final_cost"]) and st["final_cost"] <= st["initial_cost"] * (1 + 1e-6)
        g = host(s.data_graph())
        assert g.shape == (50, k) and (g[:, : min(k, D)] >= 0).all() and (g[:, min(k, D):] == -1).all()
        s.close()


def test_plan_capacity_and_argument_errors(A):
    import torch
    s = A.Solver(16, 100, 4)
    z = lambda *sh: torch.zeros(sh, device="cuda")
    with pytest.raises(A.DynfuAmdError):  # more nodes than the plan
        s.set_problem(z(17, 3), z(17, 8), z(17), z(10, 3), z(10, 3))
    with pytest.raises(A.DynfuAmdError):  # solve before set_problem
        s.solve(_params(A))
    with pytest.raises(A.DynfuAmdError):
        A.Solver(10, 10, 0)
    s.close()


def test_config_c2_full_size_properties(A):
    """BASELINE config C2 (2048 nodes, k = 4, 262144 vertices): properties that need no oracle
    run — every solve lowers its own cost, more re-weighted outer iterations fit the live
    vertices at least as well (the Tukey-weighted cost itself is not comparable across
    re-weightings), the recovered field reproduces the live vertices (linearity of the
    reference model), and the solve is invariant to the order of the vertices."""
    import torch
    cfg = synth.CONFIGS["C2"]
    c = synth.canonical(cfg)
    k, D = cfg["k"], cfg["D"]
    nodes, node_w, node_dq, verts = (dev(c[n]) for n in ("node_pos", "node_w", "node_dq", "verts"))
    idx, w = A.knn(nodes, node_w, verts, k)
    t_true = synth.true_translations(c["node_pos"], 11, cfg["k"])
    live_np = synth.live_vertices(c["verts"], host(idx), host(w), t_true)
    live = dev(live_np)
    s = A.Solver(D, len(c["verts"]), k)
    res = []
    for perm in (None, torch.randperm(len(c["verts"]), device="cuda", generator=torch.Generator("cuda").manual_seed(1))):
        v, l = (verts, live) if perm is None else (verts[perm].contiguous(), live[perm].contiguous())
        s.set_problem(nodes, node_dq, node_w, v, l)
        fit = []
        for it in (1, 2, 5):
            s.solve(_params(A, num_iter=it, nonlinear_iter=1, lambda_=200.0, pcg_tol=1e-6))
            st = s.stats()
            assert st["final_cost"] < st["initial_cost"]
            warped, _ = A.warp_to_live(nodes, s.node_dq(), node_w, k, v)
            fit.append(float((warped - l).norm()))
        assert fit[1] <= fit[0] * 1.001 and fit[2] <= fit[1] * 1.001, fit
        res.append(host(s.translations()))
        assert float((warped - l).abs().max()) < 1.5e-3  # lambda = 200 smooths ~1 mm
    assert np.abs(res[0] - res[1]).max() < 1e-5
    assert s.stats()["max_row_nnz"] <= 256
    s.close()


def test_multi_workgroup_pcg_matches_the_oracle_and_the_single_workgroup_kernels(A, devlib, monkeypatch):
    """DFA_PCG_VARIANT=3 forces the many-workgroup PCG (the path of plans above 2048 nodes) on a small problem, =1 the
    register-resident kernel with the three coordinates in ONE workgroup (shared CG scalars, as the oracle);
    the default solves the coordinates in three workgroups."""
    cfg, c, verts, live, t_true = _problem("T1")
    k = cfg["k"]
    kw = dict(num_iter=3, nonlinear_iter=2, linear_iter=200, lambda_=200.0, pcg_tol=1e-6)
    t_ref, dq_ref, st_ref = O.solve_ref(c["node_pos"], c["node_dq"], c["node_w"], k, verts, live, use_double=True,
                                        threads=8, **kw)
    out, short = {}, {}
    for variant in ("default", "1", "3"):
        if variant != "default":
            monkeypatch.setenv("DFA_PCG_VARIANT", variant)
        s = A.Solver(cfg["D"], len(verts), k)
        s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
        s.solve(_params(A, **kw))
        out[variant] = (host(s.translations()), s.stats())
        # two iterations only: far from the round-off floor, where whether a linearisation is still worth solving is
        # decided by noise (and costs ~100 PCG iterations either way)
        s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
        s.solve(_params(A, **dict(kw, num_iter=2, nonlinear_iter=1)))
        short[variant] = s.stats()
        s.close()
    monkeypatch.delenv("DFA_PCG_VARIANT", raising=False)
    t3, st3 = out["3"]
    t1, st1 = out["1"]
    td, std = out["default"]
    for t in (t3, t1, td):
        assert np.abs(t - t_ref).max() <= 2e-5
    assert st3["gn_iters"] == st1["gn_iters"] == std["gn_iters"] == st_ref["gn_iters"]
    for st in (st3, st1, std):
        np.testing.assert_allclose(st["final_cost"], st_ref["final_cost"], rtol=1e-3, atol=1e-9)
    # same algorithm in the two joint kernels: the counts agree up to round-off at the stopping threshold
    assert abs(short["3"]["pcg_iters"] - short["1"]["pcg_iters"]) <= 0.1 * short["1"]["pcg_iters"] + 3
    # per-coordinate CG: every coordinate is at least as well conditioned as the joint system
    assert 0 < short["default"]["pcg_iters"] <= 1.1 * short["1"]["pcg_iters"] + 3
    for v in ("default", "3"):
        np.testing.assert_allclose(short[v]["final_cost"], short["1"]["final_cost"], rtol=1e-3)


@pytest.mark.parametrize("D,k", [(9216, 4), (12288, 4), (12288, 8)])
def test_more_than_8192_nodes(A, D, k):
    """9 216 / 12 288 nodes: beyond the single-workgroup PCG (the team PCG: 288 / 384 rows per member, three / two threads per
    row); the ground-truth field is recovered.  k = 8 at 12 288 nodes: rows of the normal matrix may be longer than the 2 x 20
    register slots two threads hold — then the teams give up before they have written anything, the guard launch solves the
    system, the plan goes on with a launch per iteration: the answer is the same either way."""
    cfg = dict(synth.CONFIGS["T1"], D=D, k=k)
    c = synth.canonical(cfg)
    k = cfg["k"]
    verts = c["verts"][::8].copy()  # 16 vertices per node
    idx = O.knn(c["node_pos"], verts, k, threads=8)
    d2 = ((verts[:, None, :].astype(np.float64) - c["node_pos"][idx].astype(np.float64)) ** 2).sum(-1)
    w = np.exp(-d2 / (2 * float(c["node_w"][0]) ** 2)).astype(np.float32)
    t_true = synth.true_translations(c["node_pos"], 3, k)
    live = synth.live_vertices(verts, idx, w, t_true)
    s = A.Solver(cfg["D"], len(verts), k)
    s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
    s.solve(_params(A, num_iter=2, nonlinear_iter=1, linear_iter=150, lambda_=200.0, pcg_tol=1e-6))
    st = s.stats()
    t = host(s.translations())
    assert st["gn_iters"] == 2 and st["pcg_iters"] > 10 and np.isfinite(t).all()
    assert st["final_cost"] < 1e-2 * st["initial_cost"]
    t_ref, _, st_ref = O.solve_ref(c["node_pos"], c["node_dq"], c["node_w"], k, verts, live, num_iter=2, nonlinear_iter=1,
                                   linear_iter=150, lambda_=200.0, pcg_tol=1e-6, use_double=True, threads=8,
                                   tukey_offset=synth.SOLVER["tukey_offset"], psi_data=synth.SOLVER["psi_data"],
                                   psi_reg=synth.SOLVER["psi_reg"])
    assert np.abs(t - t_ref).max() <= 5e-5
    info = s.team_pcg_info()  # (98 KB of (m, t) pairs per member: the team PCG, 384 rows per member, two threads per row)
    rows = (D + 31) // 32
    if st["max_row_nnz"] <= (1024 // rows) * 20:
        assert info["launches"] >= 2 and info["aborts"] == 0 and not info["disabled"], info
    else:  # a row too long for the slots: every team said so, the guard launch solved, the host has seen it
        assert info["launches"] >= 1 and info["aborts"] >= 1, (info, st["max_row_nnz"])
    s.close()


@pytest.mark.parametrize("variant", [None, "1", "3"])
def test_iterations_behind_a_converged_one_are_no_ops(A, devlib, monkeypatch, variant):
    """Once a linearisation's gradient is at the round-off floor the unknown can no longer change: the remaining
    Gauss-Newton iterations return at entry (gn_noop) — same iteration count, same translations and cost as a solve
    that stops right there.  All three PCG paths (per-coordinate, joint, many-workgroup with its host-side
    stop)."""
    if variant is not None:
        monkeypatch.setenv("DFA_PCG_VARIANT", variant)
    cfg, c, verts, live, t_true = _problem("T1")
    k = cfg["k"]
    s = A.Solver(cfg["D"], len(verts), k)
    out = {}
    for n in (2, 4, 12):
        s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
        s.solve(_params(A, num_iter=n, nonlinear_iter=1, linear_iter=256, lambda_=200.0, pcg_tol=1e-6))
        out[n] = (host(s.translations()).copy(), s.stats())
    s.close()
    st12 = out[12][1]
    assert st12["gn_iters"] == 12 and out[4][1]["gn_iters"] == 4
    assert st12["gn_noop"] >= 6, st12                  # converges within a handful of iterations
    first_noop = 12 - st12["gn_noop"]                  # iterations 0 .. first_noop-1 ran (the last of them was skipped
    assert out[2][1]["gn_noop"] == 0                   # by the floor test itself)
    if first_noop <= 4:  # (two solves are not bit-reproducible: the assembly's LDS atomics arrive in any order)
        assert np.abs(out[4][0] - out[12][0]).max() < 1e-6
        np.testing.assert_allclose(out[4][1]["final_cost"], st12["final_cost"], rtol=1e-5)
    assert np.abs(out[12][0] - t_true).max() < 1e-4  # the regulariser (lambda = 200) moves the optimum by 5e-5


@pytest.mark.parametrize("variant", [None, "3"])
def test_inner_iterations_behind_a_gradient_at_the_floor_are_no_ops(A, devlib, monkeypatch, variant):
    """Budgets shaped like the reference's (dyn_fusion.cpp:183-189: outer x 16 inner iterations): while the robust weights
    are frozen the energy is linear least squares, so once an inner iteration finds its gradient at the round-off floor
    the rest of that outer iteration returns at entry; the next outer iteration re-weights and runs again.  Same
    translations and cost as a solve whose inner budget ends right there, and as the oracle's."""
    if variant is not None:
        monkeypatch.setenv("DFA_PCG_VARIANT", variant)
    cfg, c, verts, live, t_true = _problem("T1")
    k = cfg["k"]
    s = A.Solver(cfg["D"], len(verts), k)
    out = {}
    for outer, inner in ((2, 3), (2, 12), (1, 16)):
        s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
        s.solve(_params(A, num_iter=outer, nonlinear_iter=inner, linear_iter=256, lambda_=200.0, pcg_tol=1e-6))
        out[(outer, inner)] = (host(s.translations()).copy(), s.stats())
    s.close()
    st = out[(2, 12)][1]
    assert st["gn_iters"] == 24 and out[(1, 16)][1]["gn_iters"] == 16
    # each outer iteration: one step that solves, at most two more until the gradient is at the floor, the rest no-ops
    assert st["gn_noop"] >= 2 * 9, st
    assert out[(1, 16)][1]["gn_noop"] >= 13
    # the second outer iteration did run (re-weighted): same result as the (2, 3) budget, which has no room for no-ops
    assert np.abs(out[(2, 12)][0] - out[(2, 3)][0]).max() < 2e-6
    np.testing.assert_allclose(out[(2, 3)][1]["final_cost"], st["final_cost"], rtol=1e-4)
    t_ref, _, st_ref = O.solve_ref(c["node_pos"], c["node_dq"], c["node_w"], k, verts, live, num_iter=2, nonlinear_iter=12,
                                   linear_iter=256, lambda_=200.0, pcg_tol=1e-6, use_double=True, threads=8,
                                   tukey_offset=synth.SOLVER["tukey_offset"], psi_data=synth.SOLVER["psi_data"],
                                   psi_reg=synth.SOLVER["psi_reg"])
    assert np.abs(out[(2, 12)][0] - t_ref).max() <= 2e-5


@pytest.mark.parametrize("name,variant", [("T1", None), ("T1", "3"), ("C1", None)])
def test_inner_iterations_restart_on_the_true_residual_of_the_same_matrix(A, devlib, monkeypatch, name, variant):
    """While the robust weights are frozen the matrix of an outer iteration's first linearisation holds for its inner
    iterations, whose right-hand side is g_base - A (t - t_base): same translations and final cost as re-linearising and
    re-assembling every inner iteration (DFA_NO_REGRADIENT=1), and as the oracle, which does exactly that."""
    if variant is not None:
        monkeypatch.setenv("DFA_PCG_VARIANT", variant)
    cfg, c, verts, live, t_true = _problem(name)
    k = cfg["k"]
    s = A.Solver(cfg["D"], len(verts), k)
    out = {}
    for long_way in (False, True):
        if long_way:
            monkeypatch.setenv("DFA_NO_REGRADIENT", "1")
        s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
        s.solve(_params(A, num_iter=2, nonlinear_iter=4, linear_iter=40, lambda_=200.0, pcg_tol=1e-3))  # inexact inner solves
        out[long_way] = (host(s.translations()).copy(), s.stats())
    s.close()
    assert out[False][1]["gn_iters"] == out[True][1]["gn_iters"] == 8
    assert np.abs(out[False][0] - out[True][0]).max() < 5e-6
    np.testing.assert_allclose(out[False][1]["final_cost"], out[True][1]["final_cost"], rtol=2e-4)
    np.testing.assert_allclose(out[False][1]["initial_cost"], out[True][1]["initial_cost"], rtol=1e-6)
    assert np.abs(out[False][0] - t_true).max() < 2e-4


def test_solver_timing_accumulates_pauses_and_resumes(A):
    """dfa_solver_enable_timing: 1 starts a measurement, 0 pauses it, 2 resumes; dfa_solver_get_timing returns the
    sums over the measured solves (bench.py brackets every 8th frame this way)"""
    cfg, c, verts, live, t_true = _problem("T0")
    k = cfg["k"]
    s = A.Solver(cfg["D"], len(verts), k)
    args = (dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
    prm = _params(A, num_iter=2, nonlinear_iter=1, linear_iter=64, lambda_=200.0)
    per_solve = []
    for mode in (1, 0, 2, 2, 0):
        s.enable_timing(mode)
        s.set_problem(*args)
        s.solve(prm)
        per_solve.append(s.stats()["pcg_iters"])
    tm = s.timing()
    assert tm["solves"] == 3 and tm["pcg_launches"] == 3 * 2 and tm["assemble_launches"] == 3 * 2
    assert tm["pcg_iters"] == per_solve[0] + per_solve[2] + per_solve[3]
    assert tm["pcg_ms"] > 0 and tm["assemble_ms"] > 0 and tm["matrix_nnz"] > 0
    s.enable_timing(1)  # a new measurement forgets the old one
    s.set_problem(*args)
    s.solve(prm)
    tm = s.timing()
    assert tm["solves"] == 1 and tm["pcg_launches"] == 2
    s.close()


@pytest.mark.parametrize("D,k", [(1500, 8), (2048, 8), (700, 16)])
def test_rows_wider_than_the_register_slots(A, D, k):
    """k = 8 / 16 above 1024 (512) nodes: row pairs exceed the 32 (64) register slots of the register-resident PCG —
    the entries that do not fit are streamed; same translations as the fp64 oracle"""
    cfg = dict(synth.CONFIGS["T1"], D=D, k=k)
    c = synth.canonical(cfg)
    verts = c["verts"][::4].copy()
    idx = O.knn(c["node_pos"], verts, k, threads=8)
    d2 = ((verts[:, None, :].astype(np.float64) - c["node_pos"][idx].astype(np.float64)) ** 2).sum(-1)
    w = np.exp(-d2 / (2 * float(c["node_w"][0]) ** 2)).astype(np.float32)
    t_true = synth.true_translations(c["node_pos"], 3, k)
    live = synth.live_vertices(verts, idx, w, t_true)
    kw = dict(num_iter=2, nonlinear_iter=1, linear_iter=200, lambda_=200.0, pcg_tol=1e-6)
    s = A.Solver(D, len(verts), k)
    s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
    s.solve(_params(A, **kw))
    st, t = s.stats(), host(s.translations())
    s.close()
    assert st["max_row_nnz"] > (16 if D > 1024 else 32), st  # some pair cannot fit
    t_ref, _, st_ref = O.solve_ref(c["node_pos"], c["node_dq"], c["node_w"], k, verts, live, use_double=True, threads=8,
                                   tukey_offset=synth.SOLVER["tukey_offset"], psi_data=synth.SOLVER["psi_data"],
                                   psi_reg=synth.SOLVER["psi_reg"], **kw)
    assert st["gn_iters"] == 2 and st["pcg_iters"] > 10
    assert np.abs(t - t_ref).max() <= 3e-5
    np.testing.assert_allclose(st["final_cost"], st_ref["final_cost"], rtol=2e-3, atol=1e-9)


def test_pipelined_sequence_gives_the_same_translations(A):
    """bench.py --pipeline builds the graphs of frame f+1 on a third stream, into a second plan, while frame f is
    solved: the node translations of every frame must be those of the frame-by-frame schedule (to the solve's own
    run-to-run noise: the assembly adds with LDS float atomics, whose order is not fixed; |t| ~ 5e-3 m)."""
    import sys, torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    dev0 = torch.device("cuda", 0)
    ref = []
    seq = bench.Sequence("T1", dev0)
    for f in range(6):
        seq.frame(f)
        torch.cuda.synchronize()
        ref.append(seq.solver.translations().clone())
    seq2 = bench.Sequence("T1", dev0)
    seq2.enable_pipeline()
    for f in range(6):
        seq2.frame(f)  # no synchronisation between frames: the streams' events order them
        got = seq2.solver.translations().clone()
        torch.cuda.synchronize()
        assert float((got - ref[f]).abs().max()) <= 5e-7, "frame %d: %g" % (f, float((got - ref[f]).abs().max()))
    assert float(ref[0].abs().max()) > 1e-3  # the frames do move


def test_overlap_callback_runs_once_per_solve_and_changes_nothing(A):
    """dfa_solver_set_overlap_callback: called on the calling thread behind the assembly launch of every Gauss-Newton
    iteration of every solve (once with -1 when no iteration runs); work it enqueues on another stream runs beside the PCG; exceptions it raises surface
    from solve(); the solution is that of a solve without it."""
    import torch
    cfg, c, verts, live, _ = _problem("T1")
    k = cfg["k"]
    args = (dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
    prm = _params(A, num_iter=3, lambda_=200.0, pcg_tol=1e-6)
    s = A.Solver(cfg["D"], len(verts), k)
    s.set_problem(*args)
    s.solve(prm)
    t_ref = host(s.translations())

    side = torch.cuda.Stream()
    calls, seen, ev = [], [], torch.cuda.Event()
    vol = torch.empty((64, 64, 64), dtype=torch.int32, device="cuda")

    def cb(gn_iteration):
        seen.append(gn_iteration)
        if gn_iteration > 0:
            return
        calls.append(torch.cuda.current_stream().cuda_stream)
        ev.record()
        side.wait_event(ev)
        with torch.cuda.stream(side):
            A.tsdf_clear(vol)  # any independent work

    s.set_overlap_callback(cb)
    for _ in range(3):
        s.set_problem(*args)
        s.solve(prm)
    torch.cuda.synchronize()
    assert len(calls) == 3 and int(vol.abs().max()) == 0
    assert seen == [0, 1, 2] * 3  # behind the assembly of every Gauss-Newton iteration (num_iter = 3)
    assert np.abs(host(s.translations()) - t_ref).max() <= 5e-7
    s.set_problem(*args)
    s.solve(_params(A, num_iter=0))  # nothing to iterate: still called, once, with -1
    assert len(calls) == 4 and seen[-1] == -1

    def boom(gn_iteration):
        raise RuntimeError("from the callback")

    s.set_overlap_callback(boom)
    s.set_problem(*args)
    with pytest.raises(RuntimeError, match="from the callback"):
        s.solve(prm)
    s.set_overlap_callback(None)
    s.set_problem(*args)
    s.solve(prm)
    assert len(calls) == 4 and np.abs(host(s.translations()) - t_ref).max() <= 5e-7
    s.close()


def _noisy_problem(name, seed=5):
    """ground-truth targets plus millimetre noise: a residual that never vanishes, so every iteration of the budget works"""
    import torch
    cfg = synth.CONFIGS[name]
    c = synth.canonical(cfg)
    k = cfg["k"]
    nodes, node_w, node_dq, verts = (dev(c[n]) for n in ("node_pos", "node_w", "node_dq", "verts"))
    return cfg, c, nodes, node_w, node_dq, verts


@pytest.mark.parametrize("name", ["T1", "C2", "C3"])
def test_deterministic_variant_is_bit_reproducible(A, name):
    """dfa_solver_set_deterministic (DFA_ASSEMBLE_DETERMINISTIC=1): the same inputs give the same bits
    — translations, matrix-dependent statistics — run after run and plan after plan, on the register-resident (T1, C2) and
    the many-workgroup (C3) PCG paths, with the robust weights re-evaluated and the inner iterations restarted; the
    result agrees with the default path's to its run-to-run scatter."""
    import torch
    cfg, c, nodes, node_w, node_dq, verts = _noisy_problem(name)
    k, D = cfg["k"], cfg["D"]
    idx, w = A.knn(nodes, node_w, verts, k)
    t_true = synth.true_translations(c["node_pos"], 7, k)
    live_np = synth.live_vertices(c["verts"], host(idx), host(w), t_true)
    live_np = live_np + np.random.default_rng(3).normal(0, 1e-3, live_np.shape).astype(np.float32)
    live = dev(live_np)
    prm = _params(A, num_iter=3, nonlinear_iter=2, lambda_=200.0, pcg_tol=1e-6)

    def run(det):
        s = A.Solver(D, len(c["verts"]), k)
        s.set_deterministic(det)
        outs = []
        for _ in range(3):
            s.set_problem(nodes, node_dq, node_w, verts, live)
            s.solve(prm)
            ent, cnt, g = (host(x) for x in s.matrix())
            used = np.arange(256)[:, None] < cnt[None, :]  # slots beyond a row's length hold whatever was there
            outs.append((host(s.translations()).copy(), s.stats(), np.where(used[..., None], ent, 0).view(np.uint32), cnt, g))
        s.close()
        return outs

    det = run(True) + run(True)  # two plans, three solves each
    t0, st0, m0, cnt0, g0 = det[0]
    assert np.isfinite(t0).all() and st0["final_cost"] < st0["initial_cost"]
    for t, st, m, cnt, g in det[1:]:
        assert np.array_equal(t, t0)
        assert st["final_cost"] == st0["final_cost"] and st["pcg_iters"] == st0["pcg_iters"]
        assert np.array_equal(cnt, cnt0) and np.array_equal(m, m0) and np.array_equal(g, g0)  # the normal equations, bit for bit
    # rows of the matrix are sorted by column in this variant
    cols = m0[..., 1].view(np.int32)
    for a in range(0, D, max(1, D // 64)):
        assert (np.diff(cols[: cnt0[a], a]) > 0).all()
    ref = run(False)
    assert np.abs(ref[0][0] - t0).max() < 5e-5  # the same solution up to the default path's own scatter
    assert np.abs(t0 - t_true).max() < 2e-3


def test_a_node_with_more_than_four_million_rows(A):
    """the assembly's fixed-point sums (64-bit, 2^40 per unit of the addends' bound) hold up to 2^22 rows per node at full
    resolution; a longer list gives up a bit of the grid per doubling instead of overflowing: 3 nodes, 4.6 M vertices
    (1.5 M or more rows each, one of them > 2^22 with k = 3), translations against the float64 oracle"""
    rng = np.random.default_rng(11)
    D, k, N = 3, 3, 4_600_000
    node_pos = np.array([[0.0, 0.0, 1.5], [0.06, 0.0, 1.5], [0.0, 0.07, 1.52]], np.float32)
    node_w = np.full(D, 0.2, np.float32)
    node_dq = np.zeros((D, 8), np.float32)
    node_dq[:, 0] = 1.0
    verts = (node_pos[rng.integers(0, D, N)] + rng.normal(0, 0.03, (N, 3))).astype(np.float32)
    idx = O.knn(node_pos, verts, k, threads=8)
    d2 = ((verts[:, None, :].astype(np.float64) - node_pos[idx].astype(np.float64)) ** 2).sum(-1)
    w = np.exp(-d2 / (2 * 0.2 ** 2)).astype(np.float32)
    t_true = np.array([[0.004, -0.002, 0.001], [-0.003, 0.002, 0.002], [0.001, 0.003, -0.002]], np.float32)
    live = synth.live_vertices(verts, idx, w, t_true)
    s = A.Solver(D, N, k)
    keep = [dev(node_pos), dev(node_dq), dev(node_w), dev(verts), dev(live)]
    s.set_problem(*keep)
    s.solve(_params(A, num_iter=2, nonlinear_iter=1, linear_iter=60, lambda_=200.0, pcg_tol=1e-6))
    t, st = host(s.translations()), s.stats()
    t_ref, _, st_ref = O.solve_ref(node_pos, node_dq, node_w, k, verts, live, num_iter=2, nonlinear_iter=1, linear_iter=60,
                                   lambda_=200.0, pcg_tol=1e-6, use_double=True, threads=8, tukey_offset=synth.SOLVER["tukey_offset"],
                                   psi_data=synth.SOLVER["psi_data"], psi_reg=synth.SOLVER["psi_reg"])
    assert np.isfinite(t).all() and np.abs(t - t_ref).max() <= 2e-5
    np.testing.assert_allclose(st["final_cost"], st_ref["final_cost"], rtol=2e-3, atol=1e-9)
    s.close()


def _threads():
    return max(1, min(16, os.cpu_count() or 1))


@pytest.mark.parametrize("name,noise", [("C2", 0.0), ("C2", 1e-3), ("C3", 0.0), ("C3", 1e-3), ("C4", 0.0)])
def test_translations_match_oracle_at_baseline_sizes(A, name, noise):
    """One frame of BASELINE config C2 (2 048 nodes, k = 4, 262 144 vertices: the headline's own kernel instantiation,
    pcg_paired_kernel<1024,32,1>), of C3 (4 096 nodes, k = 8, 524 288 vertices) and of C4 (8 192 nodes, 1 048 576
    vertices: both the team PCG, pcg_team_kernel — three teams of persistent workgroups, a coordinate per XCD) with
    bench.py's parameters — 5 / 10 outer iterations, PCG <= 256 at 1e-6, lambda = 200 — HIP against the fp64 statement
    (O.solve_ref(use_double=True): energy.t:50-55, opt_solver.cpp:204-231): node translations within 2e-5 m, energies
    within 1e-3.  noise = 0: SURVEY 8(d)'s index-aligned targets; noise = 1 mm on the live vertices: a fit with a residual."""
    cfg = synth.CONFIGS[name]
    c = synth.canonical(cfg)
    k, D = cfg["k"], cfg["D"]
    nodes, node_w, node_dq, verts = (dev(c[n]) for n in ("node_pos", "node_w", "node_dq", "verts"))
    idx, w = A.knn(nodes, node_w, verts, k)
    t_true = synth.true_translations(c["node_pos"], 7, k)
    live_np = synth.live_vertices(c["verts"], host(idx), host(w), t_true)
    if noise:
        live_np = (live_np + np.random.default_rng(11).normal(0, noise, live_np.shape)).astype(np.float32)
    kw = dict(num_iter=cfg["gn_iters"], nonlinear_iter=1, linear_iter=256, pcg_tol=1e-6, **synth.SOLVER)
    t_ref, dq_ref, st_ref = O.solve_ref(c["node_pos"], c["node_dq"], c["node_w"], k, c["verts"], live_np, use_double=True,
                                        threads=_threads(), **kw)
    s = A.Solver(D, len(c["verts"]), k)
    s.set_problem(nodes, node_dq, node_w, verts, dev(live_np))
    s.solve(_params(A, **kw))
    t, st = host(s.translations()), s.stats()
    assert st["max_row_nnz"] <= 256 and st["gn_iters"] == st_ref["gn_iters"] == cfg["gn_iters"]
    assert np.abs(t - t_ref).max() <= 2e-5, (np.abs(t - t_ref).max(), np.abs(t_ref).max())
    np.testing.assert_allclose(st["initial_cost"], st_ref["initial_cost"], rtol=1e-4)
    # (noise = 0 is not a zero-energy fit either: lambda = 200 bends the field, the final energy is ~1e-5 of the first)
    np.testing.assert_allclose(st["final_cost"], st_ref["final_cost"], rtol=1e-3)
    assert noise or st["final_cost"] < 1e-4 * st["initial_cost"]
    np.testing.assert_allclose(host(s.node_dq()), dq_ref, atol=2e-5)
    info = s.team_pcg_info()
    if D > 2048:  # the team form ran every PCG, no team gave up, the plan has not gone back to a launch per iteration
        assert info["launches"] >= st["gn_iters"] - st["gn_noop"] and info["aborts"] == 0 and not info["disabled"], info
    else:
        assert info["launches"] == 0
    s.close()


def _c3_problem(A, frame=7):
    cfg = synth.CONFIGS["C3"]
    c = synth.canonical(cfg)
    k = cfg["k"]
    nodes, node_w, node_dq, verts = (dev(c[n]) for n in ("node_pos", "node_w", "node_dq", "verts"))
    idx, w = A.knn(nodes, node_w, verts, k)
    live = dev(synth.live_vertices(c["verts"], host(idx), host(w), synth.true_translations(c["node_pos"], frame, k)))
    kw = dict(num_iter=cfg["gn_iters"], nonlinear_iter=1, linear_iter=256, pcg_tol=1e-6, **synth.SOLVER)
    return cfg, (nodes, node_dq, node_w, verts, live), kw


@pytest.mark.parametrize("pair_form", [False, True])
def test_team_pcg_against_a_launch_per_iteration(A, devlib, monkeypatch, pair_form):
    """The team PCG (pcg_team_kernel: no kernel boundary per iteration) against the launched form it replaces
    (pcg_mb_step_kernel, DFA_MB_TEAM=0 in the development library) on a C3 frame with the bench's parameters: the same
    Gauss-Newton iterations, PCG iteration counts within 10 % (per-coordinate stopping instead of the joint one), node
    translations within 1e-6 m; then 200 solves in a row without a team giving up (every spin is bounded: a hang would show
    as aborts and a plan that went back to launches)."""
    cfg, prob, kw = _c3_problem(A)
    res = {}
    # two forms of the team PCG: t's replica in registers and m alone exchanged (rows that fit 16 slots per thread: this
    # problem), or (m, t) pairs exchanged (longer rows; DFA_MB_TEAM_ABORT=16 selects it at any row length)
    if pair_form:
        monkeypatch.setenv("DFA_MB_TEAM_ABORT", "16")
    for form in ("0", "1"):
        monkeypatch.setenv("DFA_MB_TEAM", form)
        s = A.Solver(cfg["D"], prob[3].shape[0], cfg["k"])
        s.set_problem(*prob)
        s.solve(_params(A, **kw))
        res[form] = (host(s.translations()), s.stats(), s.team_pcg_info())
        if form == "1":
            for _ in range(200):
                s.solve(_params(A, **kw))
            t200, info200 = host(s.translations()), s.team_pcg_info()
        s.close()
    monkeypatch.delenv("DFA_MB_TEAM")
    monkeypatch.delenv("DFA_MB_TEAM_ABORT", raising=False)
    (t0, st0, i0), (t1, st1, i1) = res["0"], res["1"]
    assert i0["launches"] == 0 and i1["launches"] > 0 and i1["aborts"] == 0
    assert st0["gn_iters"] == st1["gn_iters"] and st0["gn_noop"] == st1["gn_noop"]
    assert abs(st1["pcg_iters"] - st0["pcg_iters"]) <= 0.1 * st0["pcg_iters"] + 3, (st0["pcg_iters"], st1["pcg_iters"])
    assert np.abs(t1 - t0).max() <= 1e-6
    np.testing.assert_allclose(st1["final_cost"], st0["final_cost"], rtol=1e-3)
    assert info200["aborts"] == 0 and not info200["disabled"] and info200["launches"] >= 200
    assert np.array_equal(t200, t1)  # the same solve, the same bits: sums in a fixed order, no atomics on data


def test_team_pcg_of_two_plans_on_two_streams(A):
    """Two plans above 2 048 nodes solved on two HIP streams at once: each team launch wants every CU of XCDs 0-2, and two
    half-assembled teams would wait for each other until they time out — the launches take turns instead (an event behind
    every team launch, waited for by the next one on another stream).  No team gives up, both answers are those of the plans
    solved alone."""
    import torch
    cfg, prob, kw = _c3_problem(A, frame=5)
    cfg2, prob2, _ = _c3_problem(A, frame=9)
    alone = []
    for pr in (prob, prob2):
        s = A.Solver(cfg["D"], pr[3].shape[0], cfg["k"])
        s.set_problem(*pr)
        s.solve(_params(A, **kw))
        alone.append(host(s.translations()))
        s.close()
    plans = [A.Solver(cfg["D"], prob[3].shape[0], cfg["k"]) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(6):
        for s, st, pr in zip(plans, streams, (prob, prob2)):
            with torch.cuda.stream(st):
                s.set_problem(*pr)
                s.solve(_params(A, **kw))
    torch.cuda.synchronize()
    for s, st, want in zip(plans, streams, alone):
        with torch.cuda.stream(st):
            info = s.team_pcg_info()
            assert info["aborts"] == 0 and not info["disabled"] and info["launches"] >= 6, info
            # (to round-off: the order inside a chunk of the node -> rows transposition is not fixed across launches)
            assert np.abs(host(s.translations()) - want).max() <= 1e-6
        s.close()


@pytest.mark.parametrize("mask", [2, 7, 8 + 4, 8 + 7, 32 + 2, 32 + 7])
def test_team_pcg_guard_solves_what_a_team_gave_up(A, devlib, monkeypatch, mask):
    """DFA_MB_TEAM_ABORT (development builds) makes the teams of the masked coordinates give up at entry, as a team does
    that cannot assemble on its XCD or meets a row too long for its register slots — with 8 added they leave without a word,
    as on a device where no workgroup ever lands on that team's XCD (another partition mode, other XCC_IDs); with 32 added
    one member gives up late, behind the barrier of the round where its team converges, while the other 31 finish (a
    member whose wait timed out on a stall): the guard launch behind solves every coordinate its team did not complete
    (same recurrence, one workgroup) on a t no member has touched, the answer is the team's, the event is counted in pinned
    memory and the plan takes a launch per iteration from its next solve on — and still gives the same answer."""
    cfg, prob, kw = _c3_problem(A, frame=4)
    s = A.Solver(cfg["D"], prob[3].shape[0], cfg["k"])
    s.set_problem(*prob)
    s.solve(_params(A, **kw))
    t_team, st_team = host(s.translations()), s.stats()
    s.close()
    monkeypatch.setenv("DFA_MB_TEAM_ABORT", str(mask))
    s = A.Solver(cfg["D"], prob[3].shape[0], cfg["k"])
    s.set_problem(*prob)
    s.solve(_params(A, **kw))
    t_guard, st_guard, info = host(s.translations()), s.stats(), s.team_pcg_info()
    assert info["aborts"] >= 1 and info["launches"] >= 1
    assert np.abs(t_guard - t_team).max() <= 1e-6 and st_guard["gn_iters"] == st_team["gn_iters"]
    assert abs(st_guard["pcg_iters"] - st_team["pcg_iters"]) <= 0.1 * st_team["pcg_iters"] + 3
    monkeypatch.delenv("DFA_MB_TEAM_ABORT")
    launches = info["launches"]
    s.solve(_params(A, **kw))  # the host has seen the abort count: this solve is launched iteration by iteration
    info = s.team_pcg_info()
    assert info["disabled"] and info["launches"] == launches
    assert np.abs(host(s.translations()) - t_team).max() <= 1e-6
    s.close()


def test_team_pcg_rounds_that_wrap_around_32_bits(A, devlib, monkeypatch):
    """The barrier rounds of the team PCG are 32-bit tags that grow from launch to launch.  DFA_MB_TEAM_EPOCH (development
    builds) starts a plan's rounds just below 2^32: the launch whose rounds would wrap clears the plan's flag words and
    starts again at 1.  Every solve of that plan, before and after the wrap, gives the bits of a plan started at 1, and no
    team gives up (a stale or zero round tag would let a team pass a barrier early, or wait until it times out)."""
    cfg, prob, kw = _c3_problem(A, frame=6)
    span = kw["linear_iter"] + 8  # rounds a launch takes
    start = 2**32 - 3 * span - 100  # the fourth launch wraps
    plans = []
    for epoch in (None, start):
        if epoch is not None:
            monkeypatch.setenv("DFA_MB_TEAM_EPOCH", str(epoch))
        s = A.Solver(cfg["D"], prob[3].shape[0], cfg["k"])
        monkeypatch.delenv("DFA_MB_TEAM_EPOCH", raising=False)
        s.set_deterministic(True)  # (the same bits from the same inputs in two plans)
        s.set_problem(*prob)
        plans.append(s)
    for _ in range(3):
        t = []
        for s in plans:
            s.solve(_params(A, **kw))
            t.append(host(s.translations()))
        assert np.array_equal(t[0], t[1])
    for s in plans:
        info = s.team_pcg_info()
        assert info["aborts"] == 0 and not info["disabled"], info
        s.close()
    assert info["launches"] * span > 2**32 - start  # (the second plan's rounds did wrap)


@pytest.mark.parametrize("name,k", [("T0", 4), ("T1", 4), ("T1", 8)])
def test_team_pcg_on_small_problems_matches_the_oracle(A, devlib, monkeypatch, name, k):
    """DFA_MB_TEAM=2 (development builds) routes plans of any size to the team PCG: 64 and 512 nodes — fewer rows than a
    team has members' threads, members without a row — against the fp64 statement, 2e-5 m"""
    cfg, c, verts, live, t_true = _problem(name)
    if k != cfg["k"]:
        cfg = dict(cfg, k=k)
        idx = O.knn(c["node_pos"], verts, k, threads=8)
        d2 = ((verts[:, None, :].astype(np.float64) - c["node_pos"][idx].astype(np.float64)) ** 2).sum(-1)
        w = np.exp(-d2 / (2 * float(c["node_w"][0]) ** 2)).astype(np.float32)
        live = synth.live_vertices(verts, idx, w, t_true)
    kw = dict(num_iter=3, nonlinear_iter=2, linear_iter=200, lambda_=200.0, pcg_tol=1e-6)
    t_ref, _, st_ref = O.solve_ref(c["node_pos"], c["node_dq"], c["node_w"], k, verts, live, use_double=True, threads=8, **kw)
    monkeypatch.setenv("DFA_MB_TEAM", "2")
    s = A.Solver(cfg["D"], len(verts), k)
    s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
    s.solve(_params(A, **kw))
    t, st, info = host(s.translations()), s.stats(), s.team_pcg_info()
    s.close()
    monkeypatch.delenv("DFA_MB_TEAM")
    assert info["launches"] > 0 and info["aborts"] == 0
    assert np.abs(t - t_ref).max() <= 2e-5 and st["gn_iters"] == st_ref["gn_iters"]
    np.testing.assert_allclose(st["final_cost"], st_ref["final_cost"], rtol=1e-3, atol=1e-9)


def test_every_row_rejected_and_no_regulariser_leaves_the_nodes_alone(A):
    """lambda = 0 and live vertices a metre away: every Tukey weight is 0, no row adds anything to the normal matrix, the
    largest addend the re-weighting linearisation finds (SolveState::amax) is 0 — the assembly's fixed-point grid then comes
    from the bound every addend obeys instead of from a grid for addends of 1e-30: finite energies, t = 0."""
    cfg, c, verts, live, _ = _problem("T1")
    far = (live + np.float32(1.0)).astype(np.float32)
    s = A.Solver(cfg["D"], len(verts), cfg["k"])
    s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(far))
    s.solve(_params(A, num_iter=2, nonlinear_iter=2, linear_iter=50, lambda_=0.0))
    st = s.stats()
    assert float(s.tukey_weights().abs().max()) == 0.0
    assert np.isfinite(st["final_cost"]) and float(s.translations().abs().max()) == 0.0
    # the same plan, a well-posed problem next: the scale is found again
    s.set_problem(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), dev(verts), dev(live))
    s.solve(_params(A, num_iter=2, nonlinear_iter=2, linear_iter=200, lambda_=200.0, pcg_tol=1e-6))
    assert s.stats()["final_cost"] < 1e-3 * s.stats()["initial_cost"]
    s.close()


@pytest.mark.parametrize("offset", [0.31, 0.4])
def test_normal_matrix_sums_follow_the_scale_of_the_problem(A, offset):
    """The assembly adds tau w_a w_b as 64-bit fixed point (LDS float adds run a lane at a time on gfx950).  Its grid comes
    from the largest addend of the PROBLEM (SolveState::amax, found by the re-weighting linearisation) — not from a fixed
    bound of 1: the T1 nodes pushed `offset` metres off the surface see every vertex at an RBF weight below 4e-4 / 2e-6,
    every product w_a w_b is below 2e-7 / 4e-12 (the fixed grid of round 4 had a quantum of 9e-13), lambda = 0 leaves no
    regulariser to set the scale — and the translations still agree with the fp64 statement to 2e-3 of their size, as the
    float sums this replaced did (the fp32 CPU statement: 5e-4)."""
    cfg = synth.CONFIGS["T1"]
    c = synth.canonical(cfg)
    k = cfg["k"]
    node_pos = (c["node_pos"].astype(np.float64) + offset * c["normals"][::synth.VERTS_PER_NODE].astype(np.float64)).astype(np.float32)
    idx, w = A.knn(dev(node_pos), dev(c["node_w"]), dev(c["verts"]), k)
    w_np = host(w)
    assert (w_np.max(1) ** 2).max() < 2e-7 and w_np.max() > 0
    t_true = synth.true_translations(node_pos, 3, k) / w_np.max()  # vertices still move by centimetres
    live = synth.live_vertices(c["verts"], host(idx), w_np, t_true)
    kw = dict(num_iter=3, nonlinear_iter=2, linear_iter=256, lambda_=0.0)
    t_ref, _, st_ref = O.solve_ref(node_pos, c["node_dq"], c["node_w"], k, c["verts"], live, use_double=True, threads=8, **kw)
    s = A.Solver(cfg["D"], len(c["verts"]), k)
    s.set_problem(dev(node_pos), dev(c["node_dq"]), dev(c["node_w"]), dev(c["verts"]), dev(live))
    s.solve(_params(A, **kw))
    t, st = host(s.translations()), s.stats()
    scale = np.abs(t_ref).max()
    assert scale > 5.0 and np.abs(t - t_ref).max() <= 2e-3 * scale, (np.abs(t - t_ref).max(), scale)
    assert st["final_cost"] < 1e-6 * st["initial_cost"]
    # a huge lambda sets the scale from the other side: the sums neither overflow nor lose the data term's share
    kw = dict(kw, lambda_=1e12)
    t_ref, _, _ = O.solve_ref(node_pos, c["node_dq"], c["node_w"], k, c["verts"], live, use_double=True, threads=8, **kw)
    s.solve(_params(A, **kw))
    assert np.isfinite(host(s.translations())).all() and np.isfinite(s.stats()["final_cost"])
    with pytest.raises(A.DynfuAmdError):
        s.solve(_params(A, **dict(kw, lambda_=float("inf"))))
    s.close()
