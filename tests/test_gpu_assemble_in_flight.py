"""-m gpu: the in-flight form of assemble_kernel (solve_assemble.hip: a thread's list entries in chunks of T = 3, the chunk's
node_list entries and row records asked for together, then the hash work) against the float64 statement of one
linearisation (tests/solve_statement.py), with the budgets of test_gpu_solve_normal_equations.py, and against the plain
loop on the development flavour of the library (DFA_ASM_IN_FLIGHT=0 / 1 forces either form).

The product takes the form for k = 4 plans whose grid is resident in one round, so every plan here (at most 256 nodes)
runs it.  With D = k = 4 every data row lists all four nodes and every node is named by six regularisation entries
(three rows of its own, one of each other node; the self edge is empty), so a node's list is N + 6 entries long and N alone
sets it: the chunk is 256 x 3 = 768 entries, a trip inside it 256.  A list of 0 or 1 entries cannot have those six: those
two lengths are taken with a single node, which has no regularisation entry at all.  Every case asserts the lengths it
was built for (Statement.list_len; the development-flavour test also reads node_ptr).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import dev, host  # noqa: E402
from solve_statement import Statement  # noqa: E402

ELL = 256
LENGTHS = [0, 1, 255, 256, 257, 512, 513, 767, 768, 769, 1537]  # chunk and trip boundaries, two chunks


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _params(A, lam=200.0):
    d = dict(num_iter=1, nonlinear_iter=1, linear_iter=64, lambda_=lam, pcg_tol=1e-6, gn_tol=0.0,
             **{k: v for k, v in synth.SOLVER.items() if k != "lambda_"})
    return A.SolveParams(**d)


def _small(A, D, N, k=4, far=0, seed=0):
    """D nodes 4 cm apart, N vertices among them, live = canonical moved by a smooth field; `far` live points are pushed
    30 cm away (Tukey weight 0) at positions spread through the list"""
    rng = np.random.default_rng(100 * D + N + seed)
    corners = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1]], np.float64)[:D]
    node_pos = (np.array([0.0, 0.0, 1.5]) + 0.04 * corners).astype(np.float32)
    node_w = np.full(D, 0.05, np.float32)
    node_dq = np.zeros((D, 8), np.float32)
    node_dq[:, 0] = 1.0
    verts = (np.array([0.01, 0.01, 1.51]) + 0.02 * rng.standard_normal((N, 3))).astype(np.float32)
    if N:
        idx, w = (host(x) for x in A.knn(dev(node_pos), dev(node_w), dev(verts), k))
    else:
        idx, w = np.zeros((0, k), np.int32), np.zeros((0, k), np.float32)
    t_true = (0.003 * rng.standard_normal((D, 3))).astype(np.float32)
    live = synth.live_vertices(verts, idx, w, t_true) if N else verts.copy()
    if far:
        live = live.copy()
        live[np.linspace(3, N - 4, far).astype(int)] += np.float32(0.3)
    return (node_pos, node_dq, node_w, verts, live), k, idx, w


def _t1(A):
    """T1's geometry at k = 4 (the record layout the in-flight form serves), 2 cm noise: some Tukey weights are 0"""
    c = synth.canonical(dict(synth.CONFIGS["T1"]))
    node_pos, node_dq, node_w, k = c["node_pos"], c["node_dq"], c["node_w"], 4
    verts = np.ascontiguousarray(c["verts"])
    idx, w = (host(x) for x in A.knn(dev(node_pos), dev(node_w), dev(verts), k))
    live = synth.live_vertices(verts, idx, w, synth.true_translations(node_pos, 7, k))
    live = (live + np.random.default_rng(3).normal(0, 2e-2, live.shape)).astype(np.float32)
    return (node_pos, node_dq, node_w, verts, live), k, idx, w


def _solve(A, prob, k, lam=200.0):
    s = A.Solver(len(prob[0]), len(prob[3]), k)
    s.set_problem(*(dev(x) for x in prob))
    s.solve(_params(A, lam))
    ent, cnt, g = (host(x).copy() for x in s.matrix())
    out = dict(ent=ent, cnt=cnt, g=g, tau=host(s.tukey_weights()).copy(), dg=host(s.data_graph()).copy(),
               rg=host(s.reg_graph()).copy(), st=s.stats())  # (stats() raises where the device set `overflow`)
    return s, out


def _coo(ent, cnt):
    c = np.minimum(cnt, ELL)
    used = (np.arange(ELL)[:, None] < c[None, :]).T
    vals = np.ascontiguousarray(ent[..., 0].T)[used]
    cols = np.ascontiguousarray(ent[..., 1].T).view(np.int32)[used]
    return np.repeat(np.arange(len(cnt)), c), cols, vals


def _statement(prob, k, out, idx, w, lam=200.0):
    node_pos, _, node_w, verts, live = prob
    assert np.array_equal(out["dg"], idx)
    assert np.array_equal(out["rg"], O.knn(node_pos, node_pos, k))
    return Statement(node_pos, node_w, k, verts, live, out["dg"], out["tau"], lam, rbf=w, reg_idx=out["rg"])


def _check(S, out):
    """row lengths, max_row_nnz, ascending columns and the column sets as the statement says; every entry and the gradient
    within the statement's budgets (off-diagonal: the fixed-point sum, one grid quantum per addend)"""
    rows, cols, vals = _coo(out["ent"], out["cnt"])
    lens = S.row_lengths()
    assert np.array_equal(out["cnt"], np.minimum(lens, ELL))
    assert out["st"]["max_row_nnz"] == (lens.max() if len(lens) else 0)
    assert (np.diff(cols)[np.diff(rows) == 0] > 0).all()
    assert np.array_equal(rows, S.rows) and np.array_equal(cols, S.cols)
    err, bud = np.abs(vals.astype(np.float64) - S.vals), S.budget(deterministic=False)
    bad = np.flatnonzero(err > bud)
    assert bad.size == 0, [(int(S.rows[i]), int(S.cols[i]), vals[i], S.vals[i], bud[i]) for i in bad[:5]]
    gerr, gb = np.abs(out["g"].astype(np.float64) - S.g), S.g_budget()
    assert (gerr <= gb).all(), (gerr / np.maximum(gb, 1e-300)).max()


def _case(A, length):
    if length < 6:  # a single node: no regularisation entry, the list is the data rows
        prob, k, idx, w = _small(A, 1, length)
    else:
        prob, k, idx, w = _small(A, 4, length - 6)
    return prob, k, idx, w


@pytest.mark.parametrize("length", LENGTHS)
def test_lists_at_the_trip_and_chunk_boundaries(A, length):
    prob, k, idx, w = _case(A, length)
    s, out = _solve(A, prob, k)
    s.close()
    S = _statement(prob, k, out, idx, w)
    assert (S.list_len == length).all()
    _check(S, out)


def test_fewer_nodes_than_k_leaves_empty_slots_inside_a_chunk(A):
    prob, k, idx, w = _small(A, 3, 600)
    assert (idx[:, 3] == -1).all() and (idx[:, :3] >= 0).all()
    s, out = _solve(A, prob, k)
    s.close()
    S = _statement(prob, k, out, idx, w)
    assert (S.list_len == 600 + 4).all()  # (two rows of its own, one of each other node)
    _check(S, out)


def test_rows_of_weight_zero_in_the_middle_of_a_chunk(A):
    prob, k, idx, w = _small(A, 4, 600, far=97)
    s, out = _solve(A, prob, k)
    s.close()
    zero = np.flatnonzero(out["tau"] == 0)
    assert len(zero) >= 97 and zero.min() < 256 and zero.max() > 512 and (out["tau"] > 0).sum() > 400
    _check(_statement(prob, k, out, idx, w), out)


def test_t1_sized_plan(A):
    prob, k, idx, w = _t1(A)
    s, out = _solve(A, prob, k)
    s.close()
    assert (out["tau"] == 0).any() and (out["tau"] > 0).any()
    S = _statement(prob, k, out, idx, w)
    assert S.list_len.max() > 256  # (lists of more than one trip; their lengths differ from node to node)
    _check(S, out)


# ------------------------------------------------------------------ both forms, forced, on the development flavour
def _node_ptr(s, D):
    import torch
    torch.cuda.synchronize()
    fn = s._L.dfa_dev_solver_graph_ptrs
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_void_p)], C.c_int
    p = (C.c_void_p * 11)()
    fn(s._h, p)

    class _Holder:
        __cuda_array_interface__ = dict(shape=(D + 1,), typestr="<i4", data=(int(p[5]), False), version=2)

    return torch.as_tensor(_Holder(), device="cuda").cpu().numpy().copy()


def _off_diagonal_bits(out):
    rows, cols, vals = _coo(out["ent"], out["cnt"])
    off = rows != cols
    return rows[off], cols[off], vals[off].view(np.uint32)


FORCED = [("len%d" % n, n) for n in LENGTHS] + [("absent", "absent"), ("tau0", "tau0"), ("T1", "T1")]


@pytest.mark.parametrize("label,what", FORCED, ids=[f[0] for f in FORCED])
def test_both_forms_leave_the_same_off_diagonal_bits(A, devlib, monkeypatch, label, what):
    """the fixed-point sums do not depend on the order of the adds, so the two forms agree bit for bit off the diagonal
    (the diagonal and the gradient are float sums over a list whose order the transposition does not fix from run to run)"""
    if what == "absent":
        prob, k, idx, w = _small(A, 3, 600)
    elif what == "tau0":
        prob, k, idx, w = _small(A, 4, 600, far=97)
    elif what == "T1":
        prob, k, idx, w = _t1(A)
    else:
        prob, k, idx, w = _case(A, what)
    res = {}
    for form in ("0", "1"):
        monkeypatch.setenv("DFA_ASM_IN_FLIGHT", form)
        s, out = _solve(A, prob, k)
        ptr = _node_ptr(s, len(prob[0]))
        s.close()
        if isinstance(what, int):
            assert (np.diff(ptr) == what).all()  # the device's own list lengths
        res[form] = out
    monkeypatch.delenv("DFA_ASM_IN_FLIGHT")
    assert np.array_equal(res["0"]["cnt"], res["1"]["cnt"])
    assert res["0"]["st"]["max_row_nnz"] == res["1"]["st"]["max_row_nnz"]
    for x, y in zip(_off_diagonal_bits(res["0"]), _off_diagonal_bits(res["1"])):
        assert np.array_equal(x, y)
    r0, c0, _ = _coo(res["0"]["ent"], res["0"]["cnt"])
    r1, c1, _ = _coo(res["1"]["ent"], res["1"]["cnt"])
    assert np.array_equal(r0, r1) and np.array_equal(c0, c1)
