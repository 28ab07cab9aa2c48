"""-m gpu: the hand-off of the re-weighting linearisation's tail to the assembly launch (solve_linearise.hip,
solve_assemble.hip: the linearisation ends with its rows' partial sums, every assembly workgroup forms amax itself, one
extra assembly workgroup books the cost) leaves the bits of the linearisation's own tail — costs, amax, the stored robust
weights, every record tail, the assembled ELL rows, the gradient, the translations and the iteration counters — and, on
a default plan, the float64 statement (tests/solve_statement.py) within the budgets of
test_gpu_solve_normal_equations.py.

Runs on the development flavour of the library, where DFA_LIN_HANDOFF=0 keeps the linearisation's own tail on every path.
The plans compared bit for bit are order-stable (set_deterministic), and no node's list is longer than the 4 096 entries
such a plan sorts (DET_SORT_MAX, solve_graph.hip), so that a solve is the same from run to run whichever form runs.

Shapes: the smallest at which each thing can go wrong — one linearisation workgroup; two; exactly 1 024 without a second
trip; one row in the second trip; k = 8 (the other record layout and kernel instantiation); fewer nodes than k.  Control
paths: a solve whose gradient reaches the floor (later launches return at entry: nothing stale may be booked); inner
iterations that regradient; a cost-decrease tolerance (the linearisation keeps its tail with either setting); the closing
evaluation alone.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import dev, host  # noqa: E402
from solve_statement import Statement  # noqa: E402

CAP = 1024 * 256  # LIN_MAX_BLOCKS x threads of a workgroup
ELL = 256


class _State(C.Structure):
    """SolveState (csrc/solve.hpp)"""
    _fields_ = [("initial_cost", C.c_double), ("cost", C.c_double), ("final_cost", C.c_double), ("grad_first", C.c_double),
                ("have_initial", C.c_int), ("done", C.c_int), ("gn_iters", C.c_int), ("pcg_iters", C.c_int),
                ("max_row_nnz", C.c_int), ("overflow", C.c_int), ("pcg_fallback", C.c_int), ("split_iters", C.c_int),
                ("split_ticket", C.c_uint), ("mb_done", C.c_int), ("converged", C.c_int), ("mb_skip", C.c_int),
                ("mb_iters", C.c_int), ("weights_fresh", C.c_int), ("gn_noop", C.c_int), ("cost_stale", C.c_int),
                ("mb", C.c_float * 5), ("amax", C.c_float), ("prof", C.c_longlong * 8), ("lin_pending", C.c_int)]


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _cloud(A, D, N, k=4, noise=1e-3, far=True):
    """D nodes on a 6 cm lattice, N vertices around them, live = canonical moved by a smooth field, `noise` m of noise, a
    few far points (Tukey weight 0)"""
    rng = np.random.default_rng(7 * D + N)
    dims = (4, 4, 4) if D <= 64 else (16, 8, 8)
    g = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), -1).reshape(-1, 3)[:D]
    node_pos = (np.array([0.0, 0.0, 1.5]) + 0.06 * g).astype(np.float32)
    node_w = np.full(D, 0.06, np.float32)
    node_dq = np.zeros((D, 8), np.float32)
    node_dq[:, 0] = 1.0
    verts = (node_pos[rng.integers(0, D, N)] + 0.03 * rng.standard_normal((N, 3))).astype(np.float32)
    idx, w = (host(x) for x in A.knn(dev(node_pos), dev(node_w), dev(verts), k))
    live = synth.live_vertices(verts, idx, w, (0.004 * rng.standard_normal((D, 3))).astype(np.float32))
    if noise:
        live = (live + rng.normal(0, noise, live.shape)).astype(np.float32)
    if far:
        live = live.copy()
        live[5::41] += np.float32(0.2)
    return (node_pos, node_dq, node_w, verts, live), k, idx, w


def _params(A, **kw):
    d = dict(num_iter=2, nonlinear_iter=1, linear_iter=32, pcg_tol=1e-6, gn_tol=0.0, **synth.SOLVER)
    d.update(kw)
    return A.SolveParams(**d)


def _run(A, prob, k, params, deterministic=True):
    import torch
    D, N = len(prob[0]), len(prob[3])
    s = A.Solver(D, N, k)
    s.set_deterministic(deterministic)
    s.set_problem(*(dev(x) for x in prob))
    s.solve(params)
    st = s.stats()  # (raises where the device set `overflow`)
    torch.cuda.synchronize()
    fn = s._L.dfa_dev_solver_graph_ptrs
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_void_p)], C.c_int
    p = (C.c_void_p * 11)()
    fn(s._h, p)

    def words(ptr, n):
        class _Holder:
            __cuda_array_interface__ = dict(shape=(n,), typestr="<u4", data=(int(ptr), False), version=2)
        return torch.as_tensor(_Holder(), device="cuda").cpu().numpy().view(np.uint32).copy()

    R, rec = N + D * k, (k + k // 2 + 4 if k % 8 == 0 else 2 * k + 4)  # (solve_rec_words)
    assert int(p[10]) >= C.sizeof(_State)
    state = _State.from_buffer_copy(words(p[8], (int(p[10]) + 3) // 4).tobytes()[:C.sizeof(_State)])
    ent, cnt, g = (host(x).copy() for x in s.matrix())
    out = dict(tails=words(p[3], R * rec).reshape(R, rec)[:, rec - 4:].copy(), tau=host(s.tukey_weights()).copy(),
               t=host(s.translations()).copy(), dg=host(s.data_graph()).copy(), rg=host(s.reg_graph()).copy(), st=st,
               ent=ent, cnt=cnt, g=g, state=state)
    s.close()
    return out


def _both(A, monkeypatch, prob, k, params):
    res = {}
    for form in ("0", "1"):
        monkeypatch.setenv("DFA_LIN_HANDOFF", form)
        res[form] = _run(A, prob, k, params)
    monkeypatch.delenv("DFA_LIN_HANDOFF")
    return res["0"], res["1"]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_same_bits(old, new):
    so, sn = old["state"], new["state"]
    for f in ("initial_cost", "cost", "final_cost"):
        assert np.float64(getattr(sn, f)).view(np.uint64) == np.float64(getattr(so, f)).view(np.uint64), f
    assert np.float32(sn.amax).view(np.uint32) == np.float32(so.amax).view(np.uint32)
    for f in ("gn_iters", "gn_noop", "weights_fresh", "have_initial", "done", "converged", "cost_stale", "pcg_iters", "max_row_nnz"):
        assert getattr(sn, f) == getattr(so, f), f
    assert sn.lin_pending == 0 and so.lin_pending == 0  # every hand-off was booked; the other form never leaves one
    for f in ("initial_cost", "final_cost", "gn_iters", "gn_noop"):
        assert new["st"][f] == old["st"][f], f
    assert np.array_equal(_bits(new["tau"]), _bits(old["tau"]))
    assert np.array_equal(new["tails"], old["tails"])
    assert np.array_equal(new["cnt"], old["cnt"])
    used = np.arange(new["ent"].shape[0])[:, None] < np.minimum(new["cnt"], new["ent"].shape[0])[None, :]
    assert np.array_equal(_bits(new["ent"])[used], _bits(old["ent"])[used])  # values and columns of every stored entry
    assert np.array_equal(_bits(new["g"]), _bits(old["g"]))
    assert np.array_equal(_bits(new["t"]), _bits(old["t"]))


SHAPES = {  # D, N, k
    "one_workgroup": (4, 200, 4),                   # R = 216
    "two_workgroups": (4, 241, 4),                  # R = 257
    "exactly_1024": (1024, CAP - 4096, 4),          # R = 262 144: no second trip
    "one_row_second_trip": (1024, CAP - 4096 + 1, 4),  # R = 262 145
    "k8": (64, 3000, 8),
    "fewer_nodes_than_k": (3, 600, 4),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_hand_off_leaves_the_bits_of_the_linearisations_own_tail(A, devlib, monkeypatch, case):
    D, N, k = SHAPES[case]
    prob, k, idx, w = _cloud(A, D, N, k)
    R = N + D * k
    assert {"one_workgroup": R <= 256, "two_workgroups": R == 257, "exactly_1024": R == CAP, "one_row_second_trip": R == CAP + 1,
            "k8": True, "fewer_nodes_than_k": (idx[:, 3] == -1).all()}[case]
    assert np.bincount(idx[idx >= 0], minlength=D).max() <= 4000  # reproducible solves (module docstring)
    old, new = _both(A, monkeypatch, prob, k, _params(A))
    _assert_same_bits(old, new)
    assert new["state"].amax > 0 and new["st"]["gn_iters"] == 2 and new["state"].weights_fresh == 1
    assert (new["tau"][:N] == 0).any() and (new["tau"][:N] > 0).any()
    assert new["st"]["final_cost"] < new["st"]["initial_cost"]


def test_gradient_at_the_floor_books_nothing_stale(A, devlib, monkeypatch):
    """exact targets: the PCG finds its gradient at the floor after a few iterations, the later linearisations and
    assemblies return at entry — the booking workgroup must not book the partials of the last launch that ran again"""
    prob, k, idx, w = _cloud(A, 16, 2000, noise=0.0, far=False)
    old, new = _both(A, monkeypatch, prob, k, _params(A, num_iter=6, linear_iter=64))
    assert new["st"]["gn_noop"] > 0 and new["state"].converged == 1
    _assert_same_bits(old, new)
    assert new["st"]["final_cost"] <= new["st"]["initial_cost"]


def test_inner_iterations_that_regradient(A, devlib, monkeypatch):
    prob, k, idx, w = _cloud(A, 16, 2000)
    old, new = _both(A, monkeypatch, prob, k, _params(A, num_iter=2, nonlinear_iter=3))
    _assert_same_bits(old, new)
    assert new["st"]["gn_iters"] > 2  # (inner iterations ran: each outer iteration's first linearisation handed off)


def test_cost_decrease_tolerance_keeps_the_linearisations_own_tail(A, devlib, monkeypatch):
    prob, k, idx, w = _cloud(A, 16, 2000)
    old, new = _both(A, monkeypatch, prob, k, _params(A, num_iter=2, nonlinear_iter=3, gn_tol=1e-3))
    _assert_same_bits(old, new)


def test_closing_evaluation_alone(A, devlib, monkeypatch):
    prob, k, idx, w = _cloud(A, 16, 2000)
    old, new = _both(A, monkeypatch, prob, k, _params(A, num_iter=0))
    _assert_same_bits(old, new)
    assert new["st"]["gn_iters"] == 0 and new["st"]["initial_cost"] == new["st"]["final_cost"] > 0
    assert new["state"].amax > 0


def _coo(ent, cnt):
    c = np.minimum(cnt, ELL)
    used = (np.arange(ELL)[:, None] < c[None, :]).T
    vals = np.ascontiguousarray(ent[..., 0].T)[used]
    cols = np.ascontiguousarray(ent[..., 1].T).view(np.int32)[used]
    return np.repeat(np.arange(len(cnt)), c), cols, vals


def test_default_plan_agrees_with_the_statement_within_budget(A):
    """the product library, a default (not order-stable) plan, one Gauss-Newton iteration: the first linearisation hands
    off, the assembly forms amax and books the cost; the closing evaluation keeps its own tail.  Budgets: those of
    test_gpu_solve_normal_equations.py (Statement.budget / g_budget); costs: test_gpu_solve.py's tolerances."""
    prob, k, idx, w = _cloud(A, 64, 3000)
    node_pos, _, node_w, verts, live = prob
    s = A.Solver(len(node_pos), len(verts), k)
    s.set_problem(*(dev(x) for x in prob))
    s.solve(_params(A, num_iter=1, linear_iter=64))
    ent, cnt, g = (host(x).copy() for x in s.matrix())
    tau, t, dg, rg, st = (host(s.tukey_weights()).copy(), host(s.translations()).copy(), host(s.data_graph()).copy(),
                          host(s.reg_graph()).copy(), s.stats())
    s.close()
    assert np.array_equal(dg, idx) and np.array_equal(rg, O.knn(node_pos, node_pos, k))
    lam = synth.SOLVER["lambda_"]
    S = Statement(node_pos, node_w, k, verts, live, dg, tau, lam, rbf=w, reg_idx=rg)  # the linearisation at t = 0
    rows, cols, vals = _coo(ent, cnt)
    assert np.array_equal(cnt, np.minimum(S.row_lengths(), ELL)) and st["max_row_nnz"] == S.row_lengths().max()
    assert np.array_equal(rows, S.rows) and np.array_equal(cols, S.cols)
    err, bud = np.abs(vals.astype(np.float64) - S.vals), S.budget(deterministic=False)
    assert (err <= bud).all(), (err / np.maximum(bud, 1e-300)).max()
    gerr, gb = np.abs(g.astype(np.float64) - S.g), S.g_budget()
    assert (gerr <= gb).all(), (gerr / np.maximum(gb, 1e-300)).max()
    b = live.astype(np.float64) - verts.astype(np.float64)
    cost0 = float((tau[:len(verts)].astype(np.float64) * (b * b).sum(1)).sum())  # (t = 0: e = b, the regulariser's rows are 0)
    S1 = Statement(node_pos, node_w, k, verts, live, dg, tau, lam, t=t, rbf=w, reg_idx=rg)
    print(f"cost {st['initial_cost']:.9g} -> {st['final_cost']:.9g}; statement {cost0:.9g} -> {S1.cost:.9g}")
    np.testing.assert_allclose(st["initial_cost"], cost0, rtol=1e-4)
    np.testing.assert_allclose(st["final_cost"], S1.cost, rtol=1e-3, atol=1e-9)
    assert st["gn_iters"] == 1 and (tau == 0).any() and (tau > 0).any()
