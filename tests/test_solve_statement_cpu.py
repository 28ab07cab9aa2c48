"""The float64 statement of one linearisation (tests/solve_statement.py) on hand-computed problems and against the CPU
oracle's float64 Gauss-Newton step.  No GPU."""
import numpy as np
import pytest

import oracle as O
from dynfu_amd import synth
from solve_statement import Statement, knn_graph, rbf_weights


def _dense(S):
    return S.dense()


def test_one_vertex_on_two_nodes_is_tau_w_wT():
    node_pos = np.array([[0.0, 0.0, 1.0], [0.05, 0.0, 1.0]], np.float32)
    node_w = np.array([0.1, 0.2], np.float32)
    canon = np.array([[0.01, 0.02, 1.0]], np.float32)
    live = canon + np.array([[0.003, -0.001, 0.002]], np.float32)
    idx = np.array([[0, 1]], np.int32)
    tau = np.array([0.7])
    S = Statement(node_pos, node_w, 2, canon, live, idx, tau, lam=0.0)
    d0 = ((canon[0].astype(np.float64) - node_pos[0]) ** 2).sum()
    d1 = ((canon[0].astype(np.float64) - node_pos[1]) ** 2).sum()
    w0, w1 = np.float64(np.float32(0.1)), np.float64(np.float32(0.2))  # the nodes' radii as given (float32)
    w = np.array([np.exp(-d0 / (2 * w0 ** 2)), np.exp(-d1 / (2 * w1 ** 2))])
    np.testing.assert_allclose(_dense(S), 0.7 * np.outer(w, w), rtol=1e-14)
    b = live[0].astype(np.float64) - canon[0]
    np.testing.assert_allclose(S.g, 0.7 * w[:, None] * b[None, :], rtol=1e-14)
    assert list(S.row_lengths()) == [2, 2] and list(S.columns(0)) == [0, 1]
    assert list(S.n_add) == [1, 1, 1, 1]
    # one GN step from t = 0 zeroes the residual of a rank-one least-squares problem along w
    x = np.linalg.lstsq(_dense(S), S.g, rcond=None)[0]
    np.testing.assert_allclose(w @ x, b, rtol=1e-12)


def test_regulariser_only_is_a_graph_laplacian_times_w_reg_squared():
    rng = np.random.default_rng(1)
    D, k, lam = 6, 3, 50.0
    node_pos = rng.uniform(-0.1, 0.1, (D, 3)).astype(np.float32)
    canon = node_pos[:2] + 0.01
    idx = np.array([[0, 1, 2], [1, 0, 2]], np.int32)
    S = Statement(node_pos, np.full(D, 0.1, np.float32), k, canon, canon, idx, np.zeros(2), lam)
    reg = knn_graph(node_pos, node_pos, k)
    assert (reg[:, 0] == np.arange(D)).all()  # itself first: the self edge, empty
    L = np.zeros((D, D))
    for n in range(D):
        for m in reg[n, 1:]:
            L[n, n] += 1
            L[m, m] += 1
            L[n, m] -= 1
            L[m, n] -= 1
    np.testing.assert_allclose(_dense(S), lam / (D * k) * L, rtol=1e-14)
    assert (S.g == 0).all() and S.cost == 0.0  # t = 0: the regulariser has no residual
    # away from t = 0: g = -w_reg^2 L t
    t = rng.normal(0, 0.01, (D, 3))
    St = Statement(node_pos, np.full(D, 0.1, np.float32), k, canon, canon, idx, np.zeros(2), lam, t=t)
    np.testing.assert_allclose(St.g, -lam / (D * k) * L @ t, rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(St.cost, lam / (D * k) * np.einsum("ic,ij,jc->", t, L, t), rtol=1e-12)


def test_fewer_nodes_than_k_leaves_empty_slots():
    node_pos = np.array([[0.0, 0.0, 1.0], [0.04, 0.0, 1.0]], np.float32)
    node_w = np.full(2, 0.1, np.float32)
    canon = np.array([[0.01, 0.0, 1.0], [0.03, 0.01, 1.0]], np.float32)
    live = canon + 0.001
    tau = np.array([1.0, 0.5])
    lam = 8.0
    idx4 = knn_graph(node_pos, canon, 4)
    assert (idx4[:, 2:] == -1).all() and (idx4[:, :2] >= 0).all()
    S4 = Statement(node_pos, node_w, 4, canon, live, idx4, tau, lam)
    # the same rows as k = 2 with the regulariser's weight of k = 4: w_reg^2 = lambda / (D k)
    S2 = Statement(node_pos, node_w, 2, canon, live, idx4[:, :2], tau, lam * 2 / 4)
    np.testing.assert_allclose(_dense(S4), _dense(S2), rtol=1e-14)
    np.testing.assert_allclose(S4.g, S2.g, rtol=1e-14)
    w = rbf_weights(node_pos, node_w, canon, idx4)
    assert (w[:, 2:] == 0).all()
    data = np.zeros((2, 2))
    for v in range(2):
        data[np.ix_(idx4[v, :2], idx4[v, :2])] += tau[v] * np.outer(w[v, :2], w[v, :2])
    wr = lam / (2 * 4)
    np.testing.assert_allclose(_dense(S4), data + wr * 2 * np.array([[1, -1], [-1, 1]]), rtol=1e-14)


def test_k_equal_one_has_no_regularisation_rows():
    rng = np.random.default_rng(4)
    node_pos = rng.uniform(-0.1, 0.1, (5, 3)).astype(np.float32)
    canon = rng.uniform(-0.1, 0.1, (40, 3)).astype(np.float32)
    idx = knn_graph(node_pos, canon, 1)
    tau = rng.uniform(0, 1, 40)
    S = Statement(node_pos, np.full(5, 0.05, np.float32), 1, canon, canon, idx, tau, lam=200.0)
    w = rbf_weights(node_pos, np.full(5, 0.05, np.float32), canon, idx)[:, 0]
    expect = np.bincount(idx[:, 0], tau * w * w, minlength=5)
    np.testing.assert_allclose(_dense(S), np.diag(expect), rtol=1e-13)
    assert (S.rows == S.cols).all() and (S.reg_add == 0).all()


def test_rows_with_zero_tau_and_untouched_nodes_contribute_nothing():
    node_pos = np.array([[0.0, 0.0, 1.0], [0.05, 0.0, 1.0], [0.0, 0.05, 1.0], [0.5, 0.5, 1.0]], np.float32)
    node_w = np.full(4, 0.1, np.float32)
    canon = np.array([[0.01, 0.0, 1.0], [0.0, 0.04, 1.0]], np.float32)
    live = canon + 0.002
    idx = np.array([[0, 1], [2, 0]], np.int32)
    S = Statement(node_pos, node_w, 2, canon, live, idx, np.array([1.0, 0.0]), lam=0.0)
    # vertex 1 (tau = 0) would have coupled nodes 2 and 0: no column (2, 0) or (0, 2), no diagonal of node 2
    assert list(S.row_lengths()) == [2, 2, 0, 0]
    assert list(S.columns(0)) == [0, 1]
    assert (S.g[2:] == 0).all()
    # (the lists still name every row, whatever its tau: data rows plus the regularisation rows n -> m, m != n)
    reg = knn_graph(node_pos, node_pos, 2)
    reg_rows = np.bincount(np.r_[np.arange(4), reg[:, 1]], minlength=4)
    assert list(S.list_len) == list(np.array([2, 1, 1, 0]) + reg_rows)
    # with the regulariser on, node 3 is still reached by regularisation rows only
    S2 = Statement(node_pos, node_w, 2, canon, live, idx, np.array([1.0, 0.0]), lam=1.0)
    assert S2.row_lengths()[3] >= 2
    # a row whose weights underflow keeps its off-diagonal columns (tau != 0) but a zero diagonal is no entry
    far = np.array([[5.0, 5.0, 5.0]], np.float32)
    S3 = Statement(node_pos[:2], node_w[:2], 2, far, far, np.array([[0, 1]]), np.array([1.0]), lam=0.0)
    assert list(S3.rows) == [0, 1] and list(S3.cols) == [1, 0] and (S3.vals == 0).all()


def test_fixed_point_quantum_follows_amax_and_long_lists():
    node_pos = np.array([[0.0, 0.0, 1.0], [0.05, 0.0, 1.0]], np.float32)
    canon = np.array([[0.0, 0.0, 1.0]], np.float32)
    S = Statement(node_pos, np.full(2, 0.1, np.float32), 2, canon, canon, np.array([[0, 1]]), np.array([0.75]), lam=0.0)
    assert S.amax == np.float32(0.75)  # w = 1 at the node itself
    np.testing.assert_array_equal(S.fixed_quantum(), [2.0 ** (0 - 40)] * 2)  # 0.75 < 2^0
    S.list_len = np.array([(1 << 22) - 1, 1 << 22])
    np.testing.assert_array_equal(S.fixed_quantum(), [2.0 ** -40, 2.0 ** -39])
    S.list_len = np.array([1 << 23, (1 << 24) + 5])
    np.testing.assert_array_equal(S.fixed_quantum(), [2.0 ** -38, 2.0 ** -37])


def _oracle_problem(name, lam):
    cfg = synth.CONFIGS[name]
    c = synth.canonical(cfg)
    k = cfg["k"]
    verts = c["verts"]
    idx = O.knn(c["node_pos"], verts, k, threads=8)
    w = np.array([[O.transformation_weight(c["node_pos"][idx[v, j]], float(c["node_w"][idx[v, j]]), verts[v]) for j in range(k)]
                  for v in range(len(verts))], np.float32)
    t_true = synth.true_translations(c["node_pos"], 3, k)
    live = synth.live_vertices(verts, idx, w, t_true)
    return cfg, c, verts, live, idx, w


@pytest.mark.parametrize("name", ["T0", "T1"])
def test_one_gauss_newton_step_equals_the_float64_oracle(name):
    lam = 200.0
    cfg, c, verts, live, idx, w = _oracle_problem(name, lam)
    k, D = cfg["k"], cfg["D"]
    P = synth.SOLVER
    tau = O.tukey_weights(c["node_pos"], c["node_dq"], c["node_w"], k, verts, live, P["tukey_offset"], P["psi_data"], threads=8)
    reg = O.knn(c["node_pos"], c["node_pos"], k)
    assert np.array_equal(reg, knn_graph(c["node_pos"], c["node_pos"], k))
    S = Statement(c["node_pos"], c["node_w"], k, verts, live, idx, tau, lam, rbf=w, reg_idx=reg)
    x = S.solve()
    t_ref, _, st = O.solve_ref(c["node_pos"], c["node_dq"], c["node_w"], k, verts, live, num_iter=1, nonlinear_iter=1,
                               linear_iter=5000, pcg_tol=1e-30, lambda_=lam, tukey_offset=P["tukey_offset"],
                               psi_data=P["psi_data"], psi_reg=P["psi_reg"], use_double=True, threads=8)
    # (the oracle hands its float64 answer back as float32: that rounding is the comparison's floor)
    err = np.abs(t_ref - x).max() / np.abs(x).max()
    assert err <= 1e-7 and np.abs(t_ref - x.astype(np.float32)).max() <= 2 * np.spacing(np.float32(np.abs(x).max())), err
    np.testing.assert_allclose(S.cost, st["initial_cost"], rtol=1e-9)
    # the statement's own matrix: symmetric, positive definite at lambda > 0, A x = g to float64 round-off
    M = S.dense()
    assert np.abs(M - M.T).max() <= 1e-15 * np.abs(M).max() and S.lambda_min() > 0
    assert np.abs(M @ x - S.g).max() <= 1e-12 * np.abs(S.g).max()
