"""CPU checks of the regularisation hierarchy's statement (tests/reg_hierarchy_statement.py) on the cases of
tests/reg_hierarchy_cases.py: the properties the rule promises, the flat graph as its one-level case, what the hierarchy
buys on the strip — and the argument checks of the two new entry points, which return before any HIP call."""
import ctypes

import numpy as np
import pytest

import reg_hierarchy_cases as C
import reg_hierarchy_statement as R
from solve6_statement import check_graph

SETS = C.node_sets()


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("beta", C.BETAS)
def test_levels_nest(name, beta):
    """node_levels asserts that a representative of level l + 1 represents level l; here: the levels of a shallower
    configuration are those of a deeper one, cut off"""
    pos = SETS[name]
    deep = R.node_levels(pos, C.EPS, beta, 4)
    for levels in (1, 2, 3):
        assert np.array_equal(R.node_levels(pos, C.EPS, beta, levels), np.minimum(deep, levels - 1))
    if name in ("strip", "sphere"):
        assert (np.bincount(deep, minlength=4) > 0).all(), np.bincount(deep)  # every level has nodes: nothing is vacuous


@pytest.mark.parametrize("name", ["strip", "sphere", "coincident", "nan"])
def test_append_leaves_old_levels_unchanged(name):
    pos = SETS[name]
    rng = np.random.default_rng(3)
    extra = (pos[rng.integers(0, len(pos), 16)] + rng.normal(0, 2 * C.EPS, (16, 3))).astype(np.float32)
    extra[0] = pos[0]  # one of them coincides with an old node
    grown = np.concatenate([pos, extra])
    for beta in C.BETAS:
        assert np.array_equal(R.node_levels(grown, C.EPS, beta, 4)[:len(pos)], R.node_levels(pos, C.EPS, beta, 4))


def test_special_nodes():
    two = SETS["coincident"]
    lv = R.node_levels(two, C.EPS, 4, 3)
    assert lv[0] > 0 and lv[1] == 0  # of two coincident nodes the lower index represents
    rows = R.rows(two, lv, (2, 1, 1), 4)
    assert rows[2, 0] == 0 and rows[2, 1] == 1  # ... and a tie in distance goes to the lower index
    nan = SETS["nan"]
    lv = R.node_levels(nan, C.EPS, 4, 3)
    assert lv[5] == 0
    rows = R.rows(nan, lv, (2, 1, 1), 4)
    assert (rows[5] == -1).all() and not (rows == 5).any()  # a NaN node has no neighbours and is nobody's
    far = np.float32([[0.1, 0.1, 1.0], [60000.0, 0.1, 1.0], [0.1, np.inf, 1.0]])
    assert R.cells0(far, C.EPS)[1].tolist() == [True, False, False]  # |c0| >= 2^20 and infinity represent no cell


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("k,slots", C.CONFIGS)
@pytest.mark.parametrize("beta", C.BETAS)
def test_rows_are_compact_duplicate_free_and_level_ordered(name, k, slots, beta):
    pos = SETS[name]
    for levels in ((3,) if name == "sphere" else (1, 2, 3, 4)):  # (the sphere's rows take a second per configuration)
        use = C.slots_for(slots, levels)
        lv = R.node_levels(pos, C.EPS, beta, levels)
        g = R.rows(pos, lv, use, k)
        R.check_rows(pos, lv, use, k, g)
        for n in range(len(pos)):
            row = g[n][g[n] >= 0]
            assert (g[n][len(row):] == -1).all() and len(set(row.tolist())) == len(row) and n not in row
            # level-ordered: the first slots[0] of all nodes, then of level >= 1, ...
            at = 0
            for l in range(min(int(lv[n]), len(use) - 1) + 1):
                seg = row[at:at + use[l]]
                assert (lv[seg] >= l).all()
                at += use[l]
            assert len(row) <= at


@pytest.mark.parametrize("name", ["strip", "sphere", "D1", "D2", "coincident"])
@pytest.mark.parametrize("k", [4, 8])
def test_one_level_is_the_flat_statement(name, k):
    pos = SETS[name]
    lv = R.node_levels(pos, C.EPS, 4, 1)
    assert not lv.any()
    check_graph(pos, pos, R.rows(pos, lv, (k,), k), exclude_self=True)


def strip_hops(slots, data_graph=None, reg_graph=None):
    """hops of every strip node from the nodes the masked-in vertices name, over the statement's pattern (or a device's graphs)"""
    sc = C.strip_scene()
    nodes = sc["nodes"]
    dg = C.knn_numpy(nodes, sc["verts"], 4) if data_graph is None else data_graph
    if reg_graph is None:
        reg_graph = R.rows(nodes, R.node_levels(nodes, C.EPS, 4, len(slots)), slots, 4)
    adj = R.pattern(len(nodes), dg, reg_graph)
    return R.hops(adj, np.unique(dg[sc["mask"] != 0])), adj


def test_strip_the_far_end_is_less_than_half_as_many_hops_away():
    """what the propagation test of test_gpu_solve6_reg_hierarchy.py relies on, from the statement alone: with 14 PCG
    iterations the flat graph's far end is out of reach (>= 16 hops) and the hierarchy's is well within (<= 12)"""
    flat, adj_flat = strip_hops((4,))
    hier, adj_hier = strip_hops((2, 1, 1))
    degree = lambda a: int(a.sum(1).max())  # blocks of the longest block row, the diagonal included
    print(f"\nstrip: farthest node {flat.max()} hops flat, {hier.max()} hierarchical; block-row degree {degree(adj_flat)} / {degree(adj_hier)}")
    assert flat.min() >= 0 and hier.min() >= 0
    assert flat.max() == 22 and hier.max() <= 8
    assert flat.max() > 2 * hier.max()
    assert flat.max() >= 14 + 2 and hier.max() <= 14 - 2
    assert degree(adj_hier) <= 48


def test_sphere_rows_fit_the_plan():
    pos = SETS["sphere"]
    assert len(pos) > 256
    lv = R.node_levels(pos, C.EPS, 4, 3)
    g = R.rows(pos, lv, (4, 2, 2), 8)
    indeg = np.bincount(g[g >= 0], minlength=len(pos))
    print(f"\nsphere: D {len(pos)}, level sets {np.bincount(lv).tolist()}, most arriving edges {indeg.max()}")
    assert (pos[:, 0] < 0).any() and (pos[:, 0] > 0).any() and (pos[:, 1] < 0).any() and (pos[:, 1] > 0).any()
    assert indeg.max() + 8 < 48  # arriving + leaving regularisation edges of the busiest row stay far below the row's capacity


# ------------------------------------------------------------------------------------------------ argument checks
DFA_ERR_INVALID = 1
vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
HOST = (ctypes.c_float * 4)()


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (torch's bundled HIP runtime must be the one the library binds to)
    from dynfu_amd import build as B
    L = ctypes.CDLL(B.build())
    L.dfa_last_error.restype = ctypes.c_char_p
    L.dfa_node_levels.argtypes = [vp, i, f, i, i, vp, vp]
    L.dfa_solver6_set_reg_hierarchy.argtypes = [vp, i, ctypes.POINTER(i), f, i]
    return L


@pytest.mark.parametrize("eps,beta,levels,text", [(0.05, 4, 9, b"levels"), (0.05, 4, 0, b"levels"), (0.0, 4, 3, b"epsilon"),
                                                  (-1.0, 4, 3, b"epsilon"), (float("nan"), 4, 3, b"epsilon"), (0.05, 1, 3, b"beta")])
def test_node_levels_refuses(lib, eps, beta, levels, text):
    p = ctypes.addressof(HOST)
    assert lib.dfa_node_levels(p, 1, eps, beta, levels, p, None) == DFA_ERR_INVALID
    assert text in lib.dfa_last_error()


@pytest.mark.parametrize("slots,eps,beta,text", [((0, 2, 2), 0.05, 4, b"level 0"), ((2, -1, 1), 0.05, 4, b"negative slot"),
                                                 ((2,) * 9, 0.05, 4, b"levels"), ((2, 1, 1), 0.05, 1, b"beta"),
                                                 ((2, 1, 1), 0.0, 4, b"epsilon")])
def test_set_reg_hierarchy_refuses_a_bad_configuration_before_it_looks_at_the_plan(lib, slots, eps, beta, text):
    arr = (i * len(slots))(*slots)
    assert lib.dfa_solver6_set_reg_hierarchy(None, len(slots), arr, eps, beta) == DFA_ERR_INVALID
    assert text in lib.dfa_last_error()
