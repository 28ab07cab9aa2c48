"""-m gpu: the reference-parity solve's normal equations and one PCG step, entry by entry, against the independent float64
statement of one linearisation (tests/solve_statement.py).

The device's A (the ELL rows of Solver.matrix()), its row lengths and its right-hand side g are compared with the
statement fed the device's own Tukey weights (already checked against the oracle by test_gpu_solve.py) and RBF weights
(A.knn, the same launch_knn that builds the plan's data graph).  |A_dev - A| <= budget per entry, where the budget is the
arithmetic's (Statement.budget): 2 u per float32 addend fl(fl(tau w_a) w_b) (+3 u for w_reg^2), one grid quantum
2^(e - 40 + extra) per off-diagonal addend (amax < 2^e, `extra` bits for lists past 2^22 rows), a float32 register sum for
the diagonal (gamma_(ceil(n/256) + 8) sum|addend|, plus 4 quanta on the default path), and u |A| for the final rounding.

PCG: the true preconditioned residual of the device's t on the device's own system, in float64 with the ELL's diagonal,
meets the stop rule r.z <= max(tol^2, 1e-12) r0.z0 (joint form; the per-coordinate forms stop each coordinate at a third
of it, which implies it) up to the drift of the float32 recurrence, bounded per node by
delta_i = u (n_i + 4) (iters + 1) ((|A| |t|)_i + |g_i|): every one of the iters + 1 updates of t and r rounds an
n_i-term row product and at most 4 vector operations.  That worst case is 200-800 times sqrt(target) at these sizes,
while the measured true r.z stays below the target itself (0.67-0.98 of it for every form at T1 ... C3: the true and the
recurred residual agree to a few per cent after ~60-130 iterations), so the test also asserts r.z <= 4 target — a
factor 2 on the residual's norm for the recurrence's drift; a PCG stopped at tol instead of tol^2 misses it by 1e6.  Then |t - x*| <= (|g - g_dev| + |r_true| + |A_dev - A|_F |t|) /
lambda_min(A) per coordinate, x* the statement's float64 solution.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import dev, host  # noqa: E402
from solve_statement import U32, Statement  # noqa: E402

ELL = 256


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _params(A, **kw):
    d = dict(num_iter=1, nonlinear_iter=1, linear_iter=256, lambda_=200.0, pcg_tol=1e-6, gn_tol=0.0, **{
        k: v for k, v in synth.SOLVER.items() if k != "lambda_"})
    d.update(kw)
    return A.SolveParams(**d)


def _problem(A, name="T1", k=None, D=None, noise=0.0, offset=0.0, every=1, frame=7):
    """(node_pos, node_dq, node_w, verts, live) as numpy, and the device's RBF weights; `offset` pushes the nodes off the
    surface along its normals (tiny weights), `every` thins the vertices"""
    cfg = dict(synth.CONFIGS[name])
    if D is not None and D > cfg["D"]:
        cfg["D"] = D
    c = synth.canonical(cfg)
    k = k or cfg["k"]
    node_pos, node_dq, node_w = c["node_pos"], c["node_dq"], c["node_w"]
    if offset:
        node_pos = (node_pos.astype(np.float64) + offset * c["normals"][::synth.VERTS_PER_NODE][:len(node_pos)]).astype(np.float32)
    if D is not None and D < len(node_pos):
        node_pos, node_dq, node_w = node_pos[:D], node_dq[:D], node_w[:D]
    verts = np.ascontiguousarray(c["verts"][::every])
    idx, w = A.knn(dev(node_pos), dev(node_w), dev(verts), k)
    idx, w = host(idx), host(w)
    t_true = synth.true_translations(node_pos, frame, k)
    if offset:
        t_true = t_true / max(w.max(), 1e-30)
    live = synth.live_vertices(verts, idx, w, t_true)
    if noise:
        live = (live + np.random.default_rng(3).normal(0, noise, live.shape)).astype(np.float32)
    return (node_pos, node_dq, node_w, verts, live), k, idx, w


def _solve(A, prob, k, det=False, stats=True, **kw):
    node_pos, node_dq, node_w, verts, live = prob
    s = A.Solver(len(node_pos), len(verts), k)
    s.set_deterministic(det)
    s.set_problem(*(dev(x) for x in prob))
    s.solve(_params(A, **kw))
    ent, cnt, g = (host(x).copy() for x in s.matrix())
    out = dict(ent=ent, cnt=cnt, g=g, tau=host(s.tukey_weights()).copy(), dg=host(s.data_graph()).copy(),
               rg=host(s.reg_graph()).copy(), t=host(s.translations()).copy(), info=s.team_pcg_info())
    out["st"] = s.stats() if stats else None
    s.close()
    return out


def _statement(prob, k, out, idx, w, lam, t=None):
    node_pos, _, node_w, verts, live = prob
    assert np.array_equal(out["dg"], idx)  # the weights fed to the statement belong to the plan's graph
    assert np.array_equal(out["rg"], O.knn(node_pos, node_pos, k))
    return Statement(node_pos, node_w, k, verts, live, out["dg"], out["tau"], lam, t=t, rbf=w, reg_idx=out["rg"])


def _device_coo(ent, cnt):
    c = np.minimum(cnt, ELL)
    used = (np.arange(ELL)[:, None] < c[None, :]).T
    vals = np.ascontiguousarray(ent[..., 0].T)[used].astype(np.float64)
    cols = np.ascontiguousarray(ent[..., 1].T).view(np.int32)[used]
    return np.repeat(np.arange(len(cnt)), c), cols, vals


def _check_matrix(S, out, det, assert_values=True):
    """column sets, row lengths, ascending order, |A_dev - A| <= budget, |g_dev - g| <= budget; returns the worst
    ratios (entry error / budget, g error / budget) and the budget relative to the entries above 1e-6 max|A|"""
    rows, cols, vals = _device_coo(out["ent"], out["cnt"])
    lens = S.row_lengths()
    assert np.array_equal(out["cnt"], np.minimum(lens, ELL))
    if out["st"] is not None:
        assert out["st"]["max_row_nnz"] == lens.max()
    same_row = np.diff(rows) == 0
    assert (np.diff(cols)[same_row] > 0).all()  # ascending columns
    assert np.array_equal(rows, S.rows) and np.array_equal(cols, S.cols)
    bud = S.budget(deterministic=det)
    err = np.abs(vals - S.vals)
    gb = S.g_budget()
    gerr = np.abs(out["g"].astype(np.float64) - S.g)
    if assert_values:
        bad = np.flatnonzero(err > bud)
        assert bad.size == 0, [(int(S.rows[i]), int(S.cols[i]), vals[i], S.vals[i], bud[i]) for i in bad[:5]]
        assert (gerr <= gb).all(), np.abs(gerr / gb).max()
    big = np.abs(S.vals) > 1e-6 * np.abs(S.vals).max()
    rel = (bud / np.maximum(np.abs(S.vals), 1e-300))[big].max()
    grid = (S.grid_share(det) / np.maximum(np.abs(S.vals), 1e-300))[big].max()
    return (err / bud).max(), (gerr / np.maximum(gb, 1e-300)).max(), rel, grid


# ---------------------------------------------------------------------------------------------- (a) A, lengths and g
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8, 9, 12, 16])
@pytest.mark.parametrize("det", [False, True])
def test_matrix_and_gradient_equal_the_statement_for_every_record_layout(A, k, det):
    """32-bit ids (k = 4), 16-bit ids (k = 8, 16), the scalar record path for every other k, through K = 4, 8, 16; both
    assemblies; T1 geometry with 2 cm noise so that some Tukey weights are 0"""
    prob, k, idx, w = _problem(A, "T1", k=k, noise=2e-2, every=2)
    out = _solve(A, prob, k, det=det, lambda_=200.0)
    assert (out["tau"] == 0).any() and (out["tau"] > 0).any()
    S = _statement(prob, k, out, idx, w, 200.0)
    r, gr, rel, grid = _check_matrix(S, out, det)
    print(f"k={k} det={det}: max |dA|/budget {r:.3g}, |dg|/budget {gr:.3g}, budget/entry {rel:.3g}, grid/entry {grid:.3g}")
    assert grid <= 1e-5


@pytest.mark.parametrize("name", ["T0", "T1", "C1", "C2", "C3"])
@pytest.mark.parametrize("lam", [0.0, 200.0])
def test_matrix_at_the_project_configurations(A, name, lam):
    """at T0 ... C3 the grid's share of the budget is at most 1e-5 of every entry above 1e-6 max|A| — the fixed-point grid
    is harmless there — and the whole budget at most 1e-4 of it (the float32 rounding of the addends, 2 u each, is what is
    left where the regulariser's negative addends cancel most of an entry: 3.4e-5 at C2), so a 1 % error in any such
    entry cannot hide inside the tolerance"""
    prob, k, idx, w = _problem(A, name)
    det = name in ("T1", "C2")
    out = _solve(A, prob, k, det=det, lambda_=lam)
    S = _statement(prob, k, out, idx, w, lam)
    r, gr, rel, grid = _check_matrix(S, out, det)
    print(f"{name} lambda={lam}: max |dA|/budget {r:.3g}, |dg|/budget {gr:.3g}, budget/entry {rel:.3g}, grid/entry {grid:.3g}")
    assert grid <= 1e-5 and rel <= 1e-4


def test_fewer_nodes_than_k(A):
    """3 nodes at k = 5: slots of -1 in every data and regularisation row"""
    prob, k, idx, w = _problem(A, "T0", k=5, D=3, every=4)
    assert (idx[:, 3:] == -1).all()
    for det in (False, True):
        out = _solve(A, prob, k, det=det, lambda_=200.0)
        S = _statement(prob, k, out, idx, w, 200.0)
        _check_matrix(S, out, det)


@pytest.mark.parametrize("offset", [0.31, 0.4])
def test_tiny_weights_off_the_surface(A, offset):
    """the T1 nodes pushed off the surface (every w_a w_b < 2e-7 / 4e-12), lambda = 0: the grid follows amax"""
    prob, k, idx, w = _problem(A, "T1", offset=offset, frame=3)
    assert (w.max(1) ** 2).max() < 2e-7 and w.max() > 0
    out = _solve(A, prob, k, lambda_=0.0)
    S = _statement(prob, k, out, idx, w, 0.0)
    r, gr, rel, grid = _check_matrix(S, out, False)
    print(f"offset={offset}: max |dA|/budget {r:.3g}, |dg|/budget {gr:.3g}, budget/entry {rel:.3g}, grid/entry {grid:.3g}")


def test_huge_lambda_puts_the_data_term_below_the_grid(A):
    """lambda = 1e12: amax is w_reg^2, the data addends are partly below the grid — only the budget is asserted, and
    the budget-to-entry ratios are reported"""
    prob, k, idx, w = _problem(A, "T1", frame=3)
    out = _solve(A, prob, k, lambda_=1e12)
    S = _statement(prob, k, out, idx, w, 1e12)
    r, gr, rel, grid = _check_matrix(S, out, False)
    print(f"lambda=1e12: max |dA|/budget {r:.3g}, |dg|/budget {gr:.3g}, budget/entry {rel:.3g}, grid/entry {grid:.3g}")


def test_lists_past_four_million_rows_give_up_grid_bits(A):
    """3 nodes, k = 3, 4.6 M vertices (test_gpu_solve.py::test_a_node_with_more_than_four_million_rows): a list past
    2^22 rows uses a grid one bit coarser per doubling (fixed_scale_for_rows), within the budget that says so"""
    rng = np.random.default_rng(11)
    D, k, N = 3, 3, 4_600_000
    node_pos = np.array([[0.0, 0.0, 1.5], [0.06, 0.0, 1.5], [0.0, 0.07, 1.52]], np.float32)
    node_w = np.full(D, 0.2, np.float32)
    node_dq = np.zeros((D, 8), np.float32)
    node_dq[:, 0] = 1.0
    verts = (node_pos[rng.integers(0, D, N)] + rng.normal(0, 0.03, (N, 3))).astype(np.float32)
    idx, w = (host(x) for x in A.knn(dev(node_pos), dev(node_w), dev(verts), k))
    t_true = np.array([[0.004, -0.002, 0.001], [-0.003, 0.002, 0.002], [0.001, 0.003, -0.002]], np.float32)
    live = synth.live_vertices(verts, idx, w, t_true)
    prob = (node_pos, node_dq, node_w, verts, live)
    out = _solve(A, prob, k, lambda_=200.0, linear_iter=60)
    S = _statement(prob, k, out, idx, w, 200.0)
    assert S.list_len.max() > 1 << 22
    r, gr, rel, grid = _check_matrix(S, out, False)
    print(f"4.6M rows: max |dA|/budget {r:.3g}, |dg|/budget {gr:.3g}, budget/entry {rel:.3g}, grid/entry {grid:.3g}")


# ------------------------------------------------------------------------------- (b) the gradient away from t = 0
@pytest.mark.parametrize("name", ["T1", "C2"])
def test_gradient_and_matrix_of_the_second_linearisation(A, name):
    """order-stable plan: a solve of one outer iteration gives t1; a second plan of two leaves the matrix, the gradient
    (now with regularisation terms) and the Tukey weights re-evaluated at t1 — against the statement at t1"""
    prob, k, idx, w = _problem(A, name, noise=1e-3)
    t1 = _solve(A, prob, k, det=True)["t"]
    out = _solve(A, prob, k, det=True, num_iter=2)
    assert np.abs(t1).max() > 0
    S = _statement(prob, k, out, idx, w, 200.0, t=t1)
    reg_g = Statement(prob[0], prob[2], k, prob[3], prob[3], idx, np.zeros(len(idx)), 200.0, t=t1, rbf=w,
                      reg_idx=out["rg"]).g
    # the regulariser's share of g stands out of the budget at many nodes (T1: most, C2: a third): a gradient without it would fail
    assert (np.abs(reg_g) > S.g_budget()).mean() > 0.2
    r, gr, rel, grid = _check_matrix(S, out, True)
    print(f"{name} at t1: max |dA|/budget {r:.3g}, |dg|/budget {gr:.3g}")


# ------------------------------------------------------------------------------------------------- (c) capacity
def _hub(S_count):
    """a hub node with S_count satellites on a 5 cm sphere around it, one vertex between the hub and each satellite
    (at 2/5 of the way: hub and satellite are its two nearest nodes): the hub's row has S_count + 1 columns at k = 2"""
    i = np.arange(S_count) + 0.5
    phi = np.arccos(1 - 2 * i / S_count)
    th = np.pi * (1 + 5 ** 0.5) * i
    u = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)
    hub = np.array([0.0, 0.0, 1.5])
    node_pos = np.concatenate([hub[None], hub + 0.05 * u]).astype(np.float32)
    verts = (hub + 0.02 * u).astype(np.float32)
    D = len(node_pos)
    node_dq = np.zeros((D, 8), np.float32)
    node_dq[:, 0] = 1.0
    node_w = np.full(D, 0.05, np.float32)
    live = (verts + np.float32(0.001)).astype(np.float32)
    return node_pos, node_dq, node_w, verts, live


@pytest.mark.parametrize("sats,det", [(255, False), (255, True), (256, False), (256, True), (600, False), (600, True)])
def test_rows_at_and_past_the_ell_capacity_and_the_hash(A, sats, det):
    """256 columns: accepted and equal to the statement.  257, and more than the 512-slot hash: the solve returns, stats()
    raises DFA_ERR_CAPACITY, the row lengths are capped at 256"""
    prob = _hub(sats)
    k = 2
    idx, w = (host(x) for x in A.knn(*(dev(x) for x in (prob[0], prob[2], prob[3])), k))
    assert (np.sort(idx, 1) == np.stack([np.zeros(sats, int), np.arange(1, sats + 1)], 1)).all()
    out = _solve(A, prob, k, det=det, stats=False, lambda_=0.0, linear_iter=20)
    S = _statement(prob, k, out, idx, w, 0.0)
    assert S.row_lengths()[0] == sats + 1
    s = A.Solver(len(prob[0]), len(prob[3]), k)
    s.set_deterministic(det)
    s.set_problem(*(dev(x) for x in prob))
    s.solve(_params(A, lambda_=0.0, linear_iter=20))
    if sats + 1 <= ELL:
        out["st"] = s.stats()
        _check_matrix(S, out, det)
    else:
        with pytest.raises(A.DynfuAmdError, match="capacity"):
            s.stats()
        assert out["cnt"][0] == ELL and np.array_equal(out["cnt"][1:], S.row_lengths()[1:])
    s.close()


# ------------------------------------------------------------------------------- (d) one PCG step against x*
_LAMBDA_MIN = {}  # (the same statement for every PCG form of one problem)


def _pcg_check(S, out, tol, label):
    """(1) the true preconditioned residual of t_dev on the device's system meets the stop rule up to the recurrence's
    drift; (2) |t_dev - x*| within the bound that follows from (1), the matrix and gradient errors and lambda_min"""
    rows, cols, vals = _device_coo(out["ent"], out["cnt"])
    D = S.D
    t = out["t"].astype(np.float64)
    g = out["g"].astype(np.float64)
    diag = np.zeros(D)
    dm = rows == cols
    diag[rows[dm]] = vals[dm]
    diag = np.where(diag > 0, diag, 1.0)
    At = np.stack([np.bincount(rows, vals * t[cols, c], minlength=D) for c in range(3)], 1)
    Aabs_t = np.stack([np.bincount(rows, np.abs(vals) * np.abs(t[cols, c]), minlength=D) for c in range(3)], 1)
    r = g - At
    rz = (r * r / diag[:, None]).sum()
    r0z0 = (g * g / diag[:, None]).sum()
    iters = out["st"]["pcg_iters"]
    nrow = np.minimum(out["cnt"], ELL)[:, None]
    delta = U32 * (nrow + 4) * (iters + 1) * (Aabs_t + np.abs(g))
    drift = np.sqrt((delta * delta / diag[:, None]).sum())
    target = max(tol * tol, 1e-12) * r0z0
    assert np.sqrt(rz) <= np.sqrt(target) + drift, (rz / target, drift / np.sqrt(target))
    assert rz <= 4.0 * target, rz / target  # (the observed drift: see the module docstring)
    # (2): A (x* - t) = (g - g_dev) + r_true + (A_dev - A) t
    x = S.solve()
    dA = np.zeros((D, D))
    dA[rows, cols] += vals
    dA[S.rows, S.cols] -= S.vals
    key = (S.D, S.k, len(S.vals), float(S.vals.sum()))
    lam_min = _LAMBDA_MIN.setdefault(key, S.lambda_min())
    assert lam_min > 0
    bound = (np.linalg.norm(S.g - g, axis=0) + np.linalg.norm(r, axis=0) + np.linalg.norm(dA) * np.linalg.norm(t, axis=0)) / lam_min
    err = np.linalg.norm(t - x, axis=0)
    assert (err <= bound * (1 + 1e-9) + 1e-30).all(), (err, bound)
    print(f"{label}: rz/target {rz / target:.3g} (drift/sqrt(target) {drift / np.sqrt(target):.3g}, iters {iters}), "
          f"|t-x*| {err.max():.3g} <= {bound.max():.3g}, lambda_min {lam_min:.3g}")


FORMS = [  # (label, problem, env, det): every PCG form
    ("paired<512> T1", dict(name="T1"), {}, False),
    ("paired<512> 700 nodes k=16", dict(name="T1", D=700, k=16, every=4), {}, False),
    ("paired<1024> C2", dict(name="C2"), {}, False),
    ("paired<1024> 1500 nodes k=8 streamed", dict(name="T1", D=1500, k=8, every=4), {}, False),
    ("team register form C3", dict(name="C3"), {}, False),
    ("team pair form C3", dict(name="C3"), {"DFA_MB_TEAM": "1", "DFA_MB_TEAM_ABORT": "16"}, False),
    ("guard after a team gave up C3", dict(name="C3"), {"DFA_MB_TEAM_ABORT": "7"}, False),
    ("launched C3", dict(name="C3"), {"DFA_MB_TEAM": "0"}, False),
    ("variant 1 T1", dict(name="T1"), {"DFA_PCG_VARIANT": "1"}, False),
    ("variant 3 T1", dict(name="T1"), {"DFA_PCG_VARIANT": "3"}, False),
    ("order-stable T1", dict(name="T1"), {}, True),
    ("order-stable C3", dict(name="C3"), {}, True),
]


@pytest.mark.parametrize("tol,linear_iter", [(1e-6, 256), (0.0, 255)])
@pytest.mark.parametrize("label,pkw,env,det", FORMS, ids=[f[0] for f in FORMS])
def test_one_pcg_step_meets_its_stop_rule_and_the_float64_solution(A, devlib, monkeypatch, label, pkw, env, det, tol, linear_iter):
    prob, k, idx, w = _problem(A, noise=1e-3, **pkw)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    out = _solve(A, prob, k, det=det, pcg_tol=tol, linear_iter=linear_iter, lambda_=200.0)
    for key in env:
        monkeypatch.delenv(key)
    if env.get("DFA_MB_TEAM_ABORT") == "7":
        assert out["info"]["aborts"] >= 1  # (the guard launch solved what the teams gave up)
    elif label.startswith("team"):
        assert out["info"]["launches"] >= 1 and out["info"]["aborts"] == 0
    elif "C3" in label:  # the launched form, or the team form of the order-stable plan
        assert out["info"]["aborts"] == 0
    S = _statement(prob, k, out, idx, w, 200.0)
    _check_matrix(S, out, det)
    _pcg_check(S, out, tol, f"{label} tol={tol}")
