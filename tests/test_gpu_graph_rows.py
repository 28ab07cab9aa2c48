"""-m gpu: the fused graph build of dfa_solver_set_problem (graph_rows_kernel: both k-NN searches, the rows and the reset in
one launch) leaves, bit for bit, what the sequence it replaces leaves (knn_kernel / knn_wave_kernel, then
prepare_rows_kernel) — straight after set_problem and after one order-stable solve with the benchmark's parameters.

Runs on the development flavour of the library: DFA_GRAPH_ROWS=0 forces the old sequence there, DFA_GRAPH_GRID=1 puts the
nodes of ANY problem into the grid (the product takes the grid, and with it the fused launch, from ~1 k nodes or 4 M
node-query pairs on; the shapes here are the smallest that reach each branch of the kernel), and
dfa_dev_solver_graph_ptrs hands out the plan's graph arrays.  Every case is also compared with the product's own choice for
its size (no grid: exhaustive searches, old sequence), which must give the same bits again.

In every mode the data graph and the regularisation graph also equal warp_statement.knn, the numpy statement of the k-NN
contract: the modes are not only equal to each other.

Not readable through the C ABI and therefore compared through the development accessor: rw, rb, the record heads of re,
node_ptr, node_list (as a set per node), t, the state block and the tickets."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import warp_statement as W  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import dev, host  # noqa: E402

# (D, N, k, duplicated nodes)
CASES = {
    "partial_groups": (37, 1000, 4, 0),   # D % 4 != 0: a partial last wave group of the node search; N % 256 != 0
    "ids16": (300, 5000, 8, 0),           # the 16-bit-id record layout
    "few_vertices": (64, 40, 4, 0),       # fewer vertices than nodes
    "ties": (128, 2000, 4, 8),            # eight nodes twice: ties in (distance, index), self edges / m == n
    "tiny": (5, 300, 4, 0),               # below every threshold of the product
    "absent": (3, 50, 4, 0),              # fewer nodes than k: -1 slots in both graphs, all-empty regularisation rows
}


def _problem(D, N, k, dup, seed=0, shift=0.0):
    rng = np.random.default_rng(1000 * D + N + seed)
    nodes = np.stack([rng.uniform(-0.5, 0.5, D), rng.uniform(-0.4, 0.4, D), 2.0 + 0.1 * rng.standard_normal(D)], -1).astype(np.float32)
    if dup:
        nodes[D - dup:] = nodes[:dup]
    spacing = 0.9 / np.sqrt(D)
    node_w = np.full(D, 1.5 * spacing, np.float32)
    node_dq = np.zeros((D, 8), np.float32)
    node_dq[:, 0] = 1.0
    # vertices around the nodes (some exactly ON a node: distance 0), a few far outside their bounding box
    canon = (nodes[rng.integers(0, D, N)] + 0.5 * spacing * rng.standard_normal((N, 3))).astype(np.float32)
    canon[:: 17] = nodes[rng.integers(0, D, len(canon[:: 17]))]
    canon[5:: 97] += np.float32(3.0)
    live = (canon + np.float32(shift) + 0.004 * np.sin(7.0 * canon + seed)).astype(np.float32)
    return nodes, node_dq, node_w, canon, live


def _copy(ptr, n, dtype):
    import torch

    if n == 0:
        return np.empty(0, dtype)

    class _Holder:
        __cuda_array_interface__ = dict(shape=(n,), typestr="<u4", data=(int(ptr), False), version=2)

    return torch.as_tensor(_Holder(), device="cuda").cpu().numpy().view(np.uint32).copy()


def _graph_state(s, D, N, k):
    """every array the graph build writes, as uint32 words (node lists sorted inside each node's segment)"""
    import torch
    torch.cuda.synchronize()
    fn = s._L.dfa_dev_solver_graph_ptrs
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_void_p)], C.c_int
    p = (C.c_void_p * 11)()
    fused = fn(s._h, p)
    R = N + D * k
    words = k + k // 2 + 4 if k % 8 == 0 else 2 * k + 4  # solve_rec_words
    out = dict(ridx=_copy(p[0], R * k, np.uint32), rw=_copy(p[1], R * k, np.uint32), rb=_copy(p[2], R * 3, np.uint32),
               re_head=_copy(p[3], R * words, np.uint32).reshape(R, words)[:, : words - 4].copy(),
               reg_idx=_copy(p[4], D * k, np.uint32), node_ptr=_copy(p[5], D + 1, np.uint32), t=_copy(p[7], 3 * D, np.uint32),
               state=_copy(p[8], (p[10] or 0) // 4, np.uint32), ticket=_copy(p[9], 64, np.uint32))
    ptr = out["node_ptr"].view(np.int32)
    lst = _copy(p[6], int(ptr[D]), np.uint32)
    out["node_list"] = np.concatenate([np.sort(lst[ptr[a]: ptr[a + 1]]) for a in range(D)] + [np.empty(0, np.uint32)])
    return bool(fused), out


def _solved(A, s):
    s.solve(A.SolveParams(num_iter=5, nonlinear_iter=1, linear_iter=256, pcg_tol=1e-6, gn_tol=0.0, **synth.SOLVER))
    ent, cnt, g = s.matrix()
    return dict(entries=host(ent).view(np.uint32).copy(), row_lengths=host(cnt).copy(), gradient=host(g).view(np.uint32).copy(),
                translations=host(s.translations()).view(np.uint32).copy(), tukey=host(s.tukey_weights()).view(np.uint32).copy(),
                data_graph=host(s.data_graph()).copy(), reg_graph=host(s.reg_graph()).copy())


def _run(A, monkeypatch, prob, k, mode, plan=None):
    """mode 'fused' / 'split': the nodes in the grid, new / old launch sequence; 'product': the library's own choice"""
    for name in ("DFA_GRAPH_GRID", "DFA_GRAPH_ROWS"):
        monkeypatch.delenv(name, raising=False)
    if mode != "product":
        monkeypatch.setenv("DFA_GRAPH_GRID", "1")
    if mode == "split":
        monkeypatch.setenv("DFA_GRAPH_ROWS", "0")
    nodes, node_dq, node_w, canon, live = prob
    D, N = len(nodes), len(canon)
    s = plan or A.Solver(D, N, k)
    s.set_deterministic(True)
    s.set_problem(*(dev(x) for x in prob))
    fused, graph = _graph_state(s, D, N, k)
    # both graphs are the k-NN contract itself, whichever launch sequence built them (the modes are otherwise compared
    # with each other only)
    assert np.array_equal(host(s.data_graph()), W.knn(nodes, canon, k)), mode
    assert np.array_equal(host(s.reg_graph()), W.knn(nodes, nodes, k)), mode
    res = _solved(A, s)
    if plan is None:
        s.close()
    return fused, graph, res


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name]), "%s: %s differs" % (what, name)


@pytest.fixture
def A(devlib):
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_graph_build_leaves_the_bits_of_the_old_sequence(A, monkeypatch, case):
    D, N, k, dup = CASES[case]
    prob = _problem(D, N, k, dup)
    fused, g_new, r_new = _run(A, monkeypatch, prob, k, "fused")
    split, g_old, r_old = _run(A, monkeypatch, prob, k, "split")
    assert fused and not split
    _assert_same(g_new, g_old, "after set_problem")
    _assert_same(r_new, r_old, "after the solve")
    # the reset role: unknowns, state block and tickets are zero behind set_problem
    assert not g_new["t"].any() and not g_new["state"].any() and not g_new["ticket"].any()
    # below want_grid's threshold the product searches exhaustively and keeps the old sequence: the same bits once more
    own, g_own, r_own = _run(A, monkeypatch, prob, k, "product")
    assert not own
    _assert_same(g_own, g_old, "product's choice, after set_problem")
    _assert_same(r_own, r_old, "product's choice, after the solve")
    if case == "absent":
        assert (g_new["ridx"].view(np.int32).reshape(-1, k)[:N, D:] == -1).all() and (g_new["reg_idx"].view(np.int32).reshape(D, k)[:, D:] == -1).all()
    if case == "ties":
        reg = g_new["reg_idx"].view(np.int32).reshape(D, k)
        assert (reg[:dup, :2] == np.stack([np.arange(dup), D - dup + np.arange(dup)], -1)).all()  # (0, n) before (0, n + 120)


def test_second_problem_on_one_plan_equals_a_fresh_plan(A, monkeypatch):
    D, N, k, dup = CASES["partial_groups"]
    first, second = _problem(D, N, k, dup), _problem(D, N, k, dup, seed=3, shift=0.002)
    second = first[:4] + (second[4],)  # the same nodes and vertices, another live cloud
    for name in ("DFA_GRAPH_ROWS",):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DFA_GRAPH_GRID", "1")
    plan = A.Solver(D, N, k)
    fused, _, r1 = _run(A, monkeypatch, first, k, "fused", plan=plan)
    assert fused and r1["translations"].any()  # the first solve has left unknowns, a state block and tickets behind
    fused, g2, r2 = _run(A, monkeypatch, second, k, "fused", plan=plan)
    plan.close()
    assert fused and not g2["t"].any() and not g2["state"].any() and not g2["ticket"].any()
    _, g_fresh, r_fresh = _run(A, monkeypatch, second, k, "fused")
    _assert_same(g2, g_fresh, "second set_problem")
    _assert_same(r2, r_fresh, "second solve")
    assert not np.array_equal(r1["translations"], r2["translations"])
