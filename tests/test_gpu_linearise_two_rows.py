"""-m gpu: the two-row form of linearise_kernel (solve_linearise.hip: a thread's second row asks for its own data ahead
of the first row's arithmetic) leaves the bits of the plain loop — cost, amax, the stored robust weights and every record
tail (e, tau) — and the cost of the float64 statement (tests/solve_statement.py).

Runs on the development flavour of the library, where DFA_LIN_TWO_ROWS=0 / 1 forces either form.  The grid is capped at
1 024 workgroups x 256 threads = 262 144 threads, so R = N + D k rows decide the trips: one workgroup; exactly one trip; a
lone row of a second trip; C2 (a second trip of the 8 192 regularisation rows); a third trip (D = 16).  One solve of one
Gauss-Newton iteration runs the re-weighting linearisation (Tukey weights evaluated, mode 0) and the closing one (stored
weights, mode 2, at the solved t) on an order-stable plan, so that everything between the two launches is the same from
run to run.  That holds while no node's list is longer than 4 096 entries — longer lists keep the order the
transposition's atomics left (DET_SORT_MAX, solve_graph.hip), the gradient's float sums and with them t then differ from
run to run in the last bits, whichever form runs — so the shapes with a prescribed R take 1 024 nodes and assert their
list lengths.  The third trip's 16 nodes have lists of ~131 k entries: that case compares the forms without a PCG between
their launches (num_iter = 0: the closing linearisation evaluates the Tukey weights itself, at t = 0).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dynfu_amd import synth  # noqa: E402
from gpu_util import dev, host  # noqa: E402
from solve_statement import Statement  # noqa: E402

CAP = 1024 * 256  # LIN_MAX_BLOCKS x threads of a workgroup


class _State(C.Structure):
    """SolveState (csrc/solve.hpp) up to the field compared here"""
    _fields_ = [("initial_cost", C.c_double), ("cost", C.c_double), ("final_cost", C.c_double), ("grad_first", C.c_double),
                ("ints", C.c_int * 8), ("split_ticket", C.c_uint), ("ints2", C.c_int * 7), ("mb", C.c_float * 5), ("amax", C.c_float)]


def _cloud(A, D, N, k=4):
    """D nodes on a 6 cm lattice, N vertices around them, live = canonical moved by a smooth field, 1 mm noise, a few far points"""
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
    live = (live + rng.normal(0, 1e-3, live.shape)).astype(np.float32)  # (1 mm noise: the solved cost is not round-off)
    live[5::41] += np.float32(0.2)  # Tukey weight 0
    return (node_pos, node_dq, node_w, verts, live), k, idx, w


def _c2(A):
    c = synth.canonical(dict(synth.CONFIGS["C2"]))
    k = 4
    idx, w = (host(x) for x in A.knn(dev(c["node_pos"]), dev(c["node_w"]), dev(c["verts"]), k))
    live = synth.live_vertices(c["verts"], idx, w, synth.true_translations(c["node_pos"], 7, k))
    live = (live + np.random.default_rng(3).normal(0, 1e-3, live.shape)).astype(np.float32)
    return (c["node_pos"], c["node_dq"], c["node_w"], c["verts"], live), k, idx, w


CASES = {  # problem, Gauss-Newton iterations of the solve
    "one_block": (lambda A: _cloud(A, 4, 200), 1),                   # R = 216
    "one_trip": (lambda A: _cloud(A, 1024, CAP - 4096), 1),          # R = 262 144: no second trip
    "lone_second": (lambda A: _cloud(A, 1024, CAP - 4096 + 1), 1),   # R = 262 145: one row in the second trip
    "C2": (_c2, 1),                                                  # R = 262 144 + 8 192
    "third_trip": (lambda A: _cloud(A, 16, 2 * CAP - 64 + 37), 0),   # R = 524 325
}


def _run(A, prob, k, num_iter):
    import torch
    D, N = len(prob[0]), len(prob[3])
    s = A.Solver(D, N, k)
    s.set_deterministic(True)
    s.set_problem(*(dev(x) for x in prob))
    s.solve(A.SolveParams(num_iter=num_iter, nonlinear_iter=1, linear_iter=32, pcg_tol=1e-6, gn_tol=0.0, **synth.SOLVER))
    st = s.stats()
    torch.cuda.synchronize()
    fn = s._L.dfa_dev_solver_graph_ptrs
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_void_p)], C.c_int
    p = (C.c_void_p * 11)()
    fn(s._h, p)

    def words(ptr, n):
        class _Holder:
            __cuda_array_interface__ = dict(shape=(n,), typestr="<u4", data=(int(ptr), False), version=2)
        return torch.as_tensor(_Holder(), device="cuda").cpu().numpy().view(np.uint32).copy()

    R, rec = N + D * k, 2 * k + 4  # (k = 4: 32-bit ids, solve_rec_words)
    state = _State.from_buffer_copy(words(p[8], (int(p[10]) + 3) // 4).tobytes()[:C.sizeof(_State)])
    out = dict(tails=words(p[3], R * rec).reshape(R, rec)[:, rec - 4:].copy(), tau=host(s.tukey_weights()).copy(),
               t=host(s.translations()).copy(), dg=host(s.data_graph()).copy(), rg=host(s.reg_graph()).copy(), st=st,
               amax=np.float32(state.amax), cost=(state.initial_cost, state.cost, state.final_cost))
    s.close()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_two_row_form_leaves_the_bits_of_the_plain_loop(devlib, monkeypatch, case):
    import dynfu_amd as A
    A.load()
    build, num_iter = CASES[case]
    prob, k, idx, w = build(A)
    R = len(prob[3]) + len(prob[0]) * k
    longest = np.bincount(idx[idx >= 0], minlength=len(prob[0])).max()  # (data entries; the regulariser adds a few dozen at most)
    assert num_iter == 0 or longest <= 4000  # the solve between the two linearisations is reproducible (module docstring)
    assert {"one_block": R <= 256, "one_trip": R == CAP, "lone_second": R == CAP + 1, "C2": CAP < R <= 2 * CAP,
            "third_trip": R > 2 * CAP}[case]
    res = {}
    for form in ("0", "1"):
        monkeypatch.setenv("DFA_LIN_TWO_ROWS", form)
        res[form] = _run(A, prob, k, num_iter)
    monkeypatch.delenv("DFA_LIN_TWO_ROWS")
    old, new = res["0"], res["1"]
    assert new["cost"] == old["cost"] and new["st"]["initial_cost"] == old["st"]["initial_cost"]
    assert new["st"]["final_cost"] == old["st"]["final_cost"]
    assert new["amax"].view(np.uint32) == old["amax"].view(np.uint32) and new["amax"] > 0
    assert np.array_equal(new["tau"].view(np.uint32), old["tau"].view(np.uint32))
    assert np.array_equal(new["tails"], old["tails"])
    assert np.array_equal(new["t"].view(np.uint32), old["t"].view(np.uint32))
    assert (new["tau"] == 0).any() and (new["tau"] > 0).any()
    # the cost of the float64 statement with the device's own Tukey weights (evaluated at t = 0): at the solved t (the
    # closing linearisation: stored weights) from Statement itself, at t = 0 (the re-weighting one) from its formula there —
    # e = b, the regulariser's rows are 0 — which spares a second 2.6 s statement at the largest shape.  Tolerances: those
    # of test_gpu_solve.py's initial and final cost.
    node_pos, _, node_w, verts, live = prob
    assert np.array_equal(new["dg"], idx)
    lam = synth.SOLVER["lambda_"]
    S1 = Statement(node_pos, node_w, k, verts, live, idx, new["tau"], lam, t=new["t"], rbf=w, reg_idx=new["rg"])
    b = live.astype(np.float64) - verts.astype(np.float64)
    cost0 = float((new["tau"].astype(np.float64) * (b * b).sum(1)).sum())
    print(f"{case}: R={R} cost {new['st']['initial_cost']:.9g} -> {new['st']['final_cost']:.9g}; statement {cost0:.9g} -> {S1.cost:.9g}")
    np.testing.assert_allclose(new["st"]["initial_cost"], cost0, rtol=1e-4)
    np.testing.assert_allclose(new["st"]["final_cost"], S1.cost, rtol=1e-3, atol=1e-9)
    np.testing.assert_allclose(new["amax"], S1.amax, rtol=1e-6)  # (w_reg^2 is rounded twice on the device)
