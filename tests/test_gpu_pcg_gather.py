"""-m gpu: the gather of the register-resident PCG (pcg_paired_kernel's matvec) on the slot layouts C2 does not reach: a
two-slot remainder in row A, in row B, in both and in neither, ranges beyond 32 slots, nA + nB = E exactly, waves without
rows, and a pair that does not fit (the streaming path inside the same launch).  Every problem first ASSERTS that its
matrix has the layout it is here for — the per-wave (nA, nB) recomputed on the host by the kernel's own rule from the row
lengths of the solve's last linearisation — and then compares the solve with the float64 oracle and with itself."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import dev, host  # noqa: E402
from test_gpu_pcg_sorted_rows import _params  # noqa: E402

GN_ITERS = 3
TOL_M = 2e-5  # the tolerance of test_gpu_pcg_sorted_rows.test_c2_translations_match_the_oracle

# name -> (D, k, keep every s-th vertex)
PROBLEMS = {
    "one_wave_both_remainders": (64, 4, 16),
    "remainders_mixed": (1088, 4, 8),
    "long_ranges": (512, 8, 1),
    "unfit": (1536, 8, 8),
}


def kernel_shape(D):
    """(threads, slots per row pair) of the register-resident kernel that serves D nodes"""
    assert D <= 2048
    return (512, 64) if D <= 1024 else (1024, 32)


def wave_slots(cnt, NT, E):
    """The kernel's slot rule on the host: rows ranked by length, longest first; thread t owns ranks t ("A") and D-1-t ("B");
    nA = the wave's longest A rounded up to even, nB the same of B, limited to E - nA.
    -> (list of (nA, nB) per wave, rows owned per thread (NT,), unfit)"""
    D = len(cnt)
    ranked = np.sort(np.minimum(cnt, 256))[::-1]
    t = np.arange(NT)
    ia, ib = t, D - 1 - t
    has_a, has_b = (ia < D) & (ia <= ib), (ib >= 0) & (ib > ia)
    cnt_a = np.where(has_a, ranked[np.clip(ia, 0, D - 1)], 0)
    cnt_b = np.where(has_b, ranked[np.clip(ib, 0, D - 1)], 0)
    waves, unfit = [], False
    for w in range(NT // 64):
        sl = slice(64 * w, 64 * w + 64)
        na = (min(int(cnt_a[sl].max()), E) + 1) & ~1
        cap_b = E - na
        nb = min((int(np.minimum(cnt_b[sl], cap_b).max()) + 1) & ~1, cap_b)
        unfit |= bool((cnt_a[sl] > E).any() or (cnt_b[sl] > cap_b).any())
        waves.append((na, nb))
    return waves, has_a.astype(int) + has_b.astype(int), unfit


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


_CACHE = {}


def _problem(A, name):
    """inputs, the oracle's solve and the order-stable solve of one problem, computed once for all tests"""
    if name in _CACHE:
        return _CACHE[name]
    D, k, every = PROBLEMS[name]
    c = synth.canonical(dict(D=D))
    verts_np = np.ascontiguousarray(c["verts"][::every])
    nodes, node_w, node_dq, verts = dev(c["node_pos"]), dev(c["node_w"]), dev(c["node_dq"]), dev(verts_np)
    idx, w = A.knn(nodes, node_w, verts, k)
    t_true = synth.true_translations(c["node_pos"], 7, k)
    live_np = synth.live_vertices(verts_np, host(idx), host(w), t_true)
    live_np = (live_np + np.random.default_rng(11).normal(0, 1e-3, live_np.shape)).astype(np.float32)
    args = (nodes, node_dq, node_w, verts, dev(live_np))
    kw = dict(num_iter=GN_ITERS, nonlinear_iter=1, linear_iter=256, pcg_tol=1e-6, **synth.SOLVER)
    t_ref, _, st_ref = O.solve_ref(c["node_pos"], c["node_dq"], c["node_w"], k, verts_np, live_np, use_double=True,
                                   threads=max(1, min(16, os.cpu_count() or 1)), **kw)

    def solve(det, plan=None):
        s = plan or A.Solver(D, len(verts_np), k)
        s.set_deterministic(det)
        s.set_problem(*args)
        s.solve(_params(A, **kw))
        return s, host(s.translations()).copy(), s.stats()

    s, t_det, st_det = solve(True)
    cnt = host(s.matrix()[1]).copy()
    p = dict(D=D, k=k, args=args, solve=solve, t_ref=t_ref, st_ref=st_ref, plan=s, t_det=t_det, st_det=st_det, cnt=cnt)
    _CACHE[name] = p
    return p


def _layout(p):
    NT, E = kernel_shape(p["D"])
    waves, rows, unfit = wave_slots(p["cnt"], NT, E)
    print("D %d k %d  <%d,%d,1>  (nA, nB) per wave: %s  unfit %s" % (p["D"], p["k"], NT, E, waves, unfit))
    return NT, E, waves, rows, unfit


def _assert_layout(name, p):
    """the coverage the problem is here for"""
    NT, E, waves, rows, unfit = _layout(p)
    live = [w for w in waves if w != (0, 0)]
    if name == "unfit":
        assert (NT, E) == (1024, 32) and unfit, waves
        return
    assert not unfit, waves
    assert all(na + nb <= E and nb <= na for na, nb in waves), waves
    if name == "one_wave_both_remainders":
        # one live wave, a two-slot remainder in both rows, empty waves beside it
        assert (NT, E) == (512, 64) and len(live) == 1 and waves[0] == live[0] and len(waves) == 8, waves
        assert live[0][0] % 4 == 2 and live[0][1] % 4 == 2, waves
    elif name == "remainders_mixed":
        # A and B each with and without a remainder; a wave without rows; a wave whose threads partly own no row (D is
        # even, so a thread owns two rows or none: no rank is its own mirror)
        assert (NT, E) == (1024, 32), waves
        assert {na % 4 for na, _ in live} == {0, 2} and {nb % 4 for _, nb in live} == {0, 2}, waves
        assert (0, 0) in waves, waves
        per_wave = rows.reshape(-1, 64)
        assert any(r.min() == 0 and r.max() > 0 for r in per_wave), per_wave.sum(1)
    elif name == "long_ranges":
        # ranges beyond 32 slots, nA + nB = E exactly
        assert (NT, E) == (512, 64), waves
        assert max(na for na, _ in live) > 32, waves
        assert any(na + nb == E for na, nb in live), waves


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_translations_match_the_oracle(A, name):
    p = _problem(A, name)
    _assert_layout(name, p)
    t, st, t_ref, st_ref = p["t_det"], p["st_det"], p["t_ref"], p["st_ref"]
    err = np.abs(t - t_ref).max()
    print("order-stable |t - t_oracle| max %.3e m (|t| max %.3e), cost %.6e oracle %.6e" %
          (err, np.abs(t_ref).max(), st["final_cost"], st_ref["final_cost"]))
    assert st["gn_iters"] == st_ref["gn_iters"] == GN_ITERS
    assert err <= TOL_M, (err, np.abs(t_ref).max())
    np.testing.assert_allclose(st["final_cost"], st_ref["final_cost"], rtol=1e-3)


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_order_stable_solves_repeat_bit_for_bit(A, name):
    p = _problem(A, name)
    _assert_layout(name, p)
    _, t_again, st_again = p["solve"](True, plan=p["plan"])  # the same plan once more
    other, t_other, st_other = p["solve"](True)              # another plan of the same problem
    other.close()
    for t, st in ((t_again, st_again), (t_other, st_other)):
        assert np.array_equal(t.view(np.uint32), p["t_det"].view(np.uint32)), np.abs(t - p["t_det"]).max()
        assert st["pcg_iters"] == p["st_det"]["pcg_iters"]


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_default_mode_agrees_with_the_order_stable_mode(A, name):
    p = _problem(A, name)
    _assert_layout(name, p)
    s, t, st = p["solve"](False)
    s.close()
    err = np.abs(t - p["t_det"]).max()
    print("default against order-stable: %.3e m" % err)
    assert st["gn_iters"] == GN_ITERS
    assert err <= TOL_M, err
