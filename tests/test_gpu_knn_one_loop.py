"""-m gpu: the one-loop walk of the vertex -> node searches (csrc/knn_walk.hpp: a lane walks the nine row ranges around its
cell in one loop; knn_grid_query<K, false, true> in graph_rows_kernel and knn_kernel) against

  * warp_statement.knn, the exhaustive numpy statement of the k-NN contract ((distance, index) order, -1 for an absent
    neighbour and for a NaN query), and
  * the nine wave-wide loops it replaces, which the development flavour of the library keeps behind DFA_KNN_ONE_LOOP=0: the
    indices and weights of dfa_knn, and ridx / rw / rb / the record heads / reg_idx / the transposition of
    Solver.set_problem, bit for bit.

Shapes: 1 024 - 1 100 nodes (the product takes the grid from 1 024 nodes on), 4 133 vertices through the plan (not a
multiple of 64; the plan is the smallest solve_graph_rows_fits accepts: k itself, 16-byte aligned arrays), the same
vertices repeated to 33 064 queries through dfa_knn (one lane per query from 32 769 on; fewer take one wave per query),
k = 4, 8, 16.  One statement per node set (k = 16; a shorter list is its prefix), shared by the cases.

Node sets and what they reach:
  surface   a slab of nodes, eight of them twice (ties are decided by index); queries on nodes, around them, at the
            corners, edge midpoints and face centres of the bounding box from inside and outside (rows outside the grid are
            empty), far outside it, and one NaN
  flat      every node at one z: a grid one cell thick in z
  line      every node in one x-row of cells: eight of nine ranges empty
  placed    1 024 nodes in the unit cube (11 cells per axis) put cell by cell: wave 0 is one lane with nine full ranges
            (12 each) beside 63 lanes with one candidate each (fewer than k in the block: on to the shell loop); lane 0 of
            wave 1 has ranges of 0, 1, 3, 4, 5 and 9; a query in the last cell, whose row ends at the last element of the
            sorted array.  tools/knn_walk_count.row_lengths asserts that the ranges are the ones meant."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import warp_statement as W  # noqa: E402
from gpu_util import dev, host  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PLAN = 4133
N_KNN = 8 * N_PLAN  # 33 064 > 32 768
KMAX = 16


def _row_lengths(nodes, queries):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import knn_walk_count as T
    finally:
        sys.path.pop(0)
    return T.row_lengths(nodes, queries)


def _fill(queries, nodes, rng, n=N_PLAN):
    """the given queries first, then vertices around the nodes, up to n"""
    queries = np.asarray(queries, np.float32).reshape(-1, 3)
    spacing = np.float32(0.9 / np.sqrt(len(nodes)))
    rest = nodes[rng.integers(0, len(nodes), n - len(queries))] + 0.7 * spacing * rng.standard_normal((n - len(queries), 3))
    return np.concatenate([queries, rest.astype(np.float32)])


def _surface(rng):
    D = 1100
    nodes = np.stack([rng.uniform(-0.5, 0.5, D), rng.uniform(-0.4, 0.4, D), 2.0 + 0.1 * rng.standard_normal(D)], -1).astype(np.float32)
    nodes[D - 8:] = nodes[:8]
    lo, hi = nodes.min(0), nodes.max(0)
    mid = (lo + hi) / 2
    special = []
    for code in range(27):  # corners (no axis at the middle), edge midpoints (one), face centres (two)
        pick = [code % 3, code // 3 % 3, code // 9]
        if pick == [1, 1, 1]:
            continue
        p = np.array([(lo[c], mid[c], hi[c])[pick[c]] for c in range(3)], np.float32)
        out = np.array([(-1, 0, 1)[pick[c]] for c in range(3)], np.float32)
        special += [p - 1e-3 * out, p, p + 0.05 * out]  # just inside, on the box, outside it
    special += [nodes[i] for i in range(16)]  # exactly on nodes, the doubled ones among them
    special += [nodes[3] + np.float32(3.0), np.full(3, np.nan, np.float32), np.array([50.0, -50.0, 2.0], np.float32)]
    return nodes, _fill(special, nodes, rng)


def _flat(rng):
    D = 1024
    nodes = np.stack([rng.uniform(-0.5, 0.5, D), rng.uniform(-0.4, 0.4, D), np.full(D, 2.0)], -1).astype(np.float32)
    q = _fill(np.empty((0, 3)), nodes, rng)
    q[::5, 2] = 2.0  # in the plane of the nodes as well as off it
    return nodes, q


def _line(rng):
    D = 1024
    nodes = np.zeros((D, 3), np.float32)
    nodes[:, 0] = rng.uniform(-1, 1, D)
    nodes[:, 1], nodes[:, 2] = 0.25, 2.0
    q = nodes[rng.integers(0, D, N_PLAN)] + np.float32(0.01) * rng.standard_normal((N_PLAN, 3))
    return nodes, q.astype(np.float32)


def _placed(rng):
    D = 1024
    cs = 1.0 / D ** (1.0 / 3.0)  # the unit cube: cbrt(1 / D) = 0.0992, int(1 / cs) + 1 = 11 cells per axis
    inside = lambda cell, n: (np.asarray(cell, np.float64) + 0.5 + rng.uniform(-0.3, 0.3, (n, 3))) * cs
    nodes = [np.zeros((1, 3)), np.ones((1, 3))]  # the box; (1, 1, 1) lies in the last cell (10, 10, 10)
    for z in (1, 2, 3):  # a 3 x 3 x 3 block of cells with four nodes each: nine ranges of 12 around cell (2, 2, 2)
        for y in (1, 2, 3):
            for x in (1, 2, 3):
                nodes.append(inside((x, y, z), 4))
    for (y, z), n in {(1, 8): 1, (2, 8): 3, (3, 8): 4, (1, 9): 5, (2, 9): 9}.items():  # rows of 1, 3, 4, 5, 9 around cell (6, 2, 8)
        nodes.append(inside((6, y, z), n))
    nodes += [inside((1, 8, 9), 1), inside((9, 7, 8), 1)]  # two lonely nodes: nothing else within their blocks
    have = sum(len(a) for a in nodes)
    filler = np.stack([rng.uniform(0.02, 0.98, D - have), rng.uniform(0.02, 0.98, D - have), rng.uniform(4.1, 5.9, D - have) * cs], -1)
    nodes = np.concatenate(nodes + [filler]).astype(np.float32)
    assert len(nodes) == D
    lonely = np.concatenate([inside((1, 8, 9), 32), inside((9, 7, 8), 31)])
    wave0 = np.concatenate([inside((2, 2, 2), 1), lonely])
    wave1 = np.concatenate([inside((6, 2, 8), 1), inside((10, 10, 10), 3), np.ones((1, 3)), filler[:59] + 0.01])
    q = _fill(np.concatenate([wave0, wave1]), nodes, rng)
    L = _row_lengths(nodes, q)
    assert (L[0] == 12).all() and (L[1:64].sum(1) == 1).all(), L[:64]
    assert sorted(L[64]) == [0, 0, 0, 0, 1, 3, 4, 5, 9], L[64]
    assert L[65:69, 4].min() >= 1  # the last cell holds (1, 1, 1): its row ends with the array
    return nodes, q


_SETS = {"surface": _surface, "flat": _flat, "line": _line, "placed": _placed}
_memo = {}


def _case(name):
    """(nodes, node_w, node_dq, queries, statement for k = 16 over the plan's vertices), computed once"""
    if name not in _memo:
        rng = np.random.default_rng(sorted(_SETS).index(name) + 131)
        nodes, q = _SETS[name](rng)
        assert len(q) == N_PLAN and q.dtype == np.float32 and nodes.dtype == np.float32
        D = len(nodes)
        node_w = np.full(D, 1.5 * 0.9 / np.sqrt(D), np.float32)
        node_dq = np.zeros((D, 8), np.float32)
        node_dq[:, 0] = 1.0
        want = W.knn(nodes, q, KMAX)
        want.setflags(write=False)
        _memo[name] = (nodes, node_w, node_dq, q, want)
    return _memo[name]


@pytest.fixture
def A(devlib):
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _forms(monkeypatch, fn):
    """fn() with the one-loop walk and with the nine loops"""
    monkeypatch.delenv("DFA_KNN_ONE_LOOP", raising=False)
    new = fn()
    monkeypatch.setenv("DFA_KNN_ONE_LOOP", "0")
    old = fn()
    monkeypatch.delenv("DFA_KNN_ONE_LOOP", raising=False)
    return new, old


@pytest.mark.parametrize("k", [4, 8, 16])
@pytest.mark.parametrize("name", sorted(_SETS))
def test_dfa_knn_one_lane_per_query(A, monkeypatch, name, k):
    nodes, node_w, _, q, want = _case(name)
    rep = np.resize(np.arange(N_PLAN), N_KNN)
    d_nodes, d_w, d_q = dev(nodes), dev(node_w), dev(q[rep])

    def run():
        idx, w = A.knn(d_nodes, d_w, d_q, k)
        return host(idx).copy(), host(w).view(np.uint32).copy()

    (idx, w), (idx_old, w_old) = _forms(monkeypatch, run)
    assert np.array_equal(idx, want[rep, :k])
    assert np.array_equal(idx, idx_old) and np.array_equal(w, w_old)
    if name == "surface":
        assert (idx[np.isnan(q[rep]).any(1)] == -1).all() and np.isnan(q).any()


@pytest.mark.parametrize("k", [4, 8, 16])
@pytest.mark.parametrize("name", sorted(_SETS))
def test_plan_graph_build(A, monkeypatch, name, k):
    import test_gpu_graph_rows as G
    nodes, node_w, node_dq, q, want = _case(name)
    D = len(nodes)
    live = (q + np.float32(0.004) * np.sin(7.0 * q)).astype(np.float32)
    monkeypatch.delenv("DFA_GRAPH_GRID", raising=False)  # (>= 1 024 nodes: in the grid by the product's own rule)
    monkeypatch.delenv("DFA_GRAPH_ROWS", raising=False)

    def run():
        s = A.Solver(D, N_PLAN, k)
        s.set_deterministic(True)
        s.set_problem(dev(nodes), dev(node_dq), dev(node_w), dev(q), dev(live))
        fused, graph = G._graph_state(s, D, N_PLAN, k)
        graph["data_graph"], graph["reg_graph"] = host(s.data_graph()).copy(), host(s.reg_graph()).copy()
        s.close()
        return fused, graph

    (fused, new), (fused_old, old) = _forms(monkeypatch, run)
    assert fused and fused_old  # both through graph_rows_kernel: only the walk differs
    assert np.array_equal(new["data_graph"], want[:, :k])
    assert np.array_equal(new["reg_graph"], W.knn(nodes, nodes, k))
    G._assert_same(new, old, "%s, k = %d" % (name, k))
