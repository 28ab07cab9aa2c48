"""-m gpu: the multi-level regularisation graph (dynfu_amd/csrc/reg_hierarchy.hip) against its numpy statement
(tests/reg_hierarchy_statement.py) on the cases of tests/reg_hierarchy_cases.py: dfa_node_levels exactly, a plan's
reg_graph() by the statement's row check, an append, the one-level configuration against a plan that was never given a
hierarchy, the refused configurations, a second plan on a second stream, the row capacity on the sphere."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import reg_hierarchy_cases as C  # noqa: E402
import reg_hierarchy_statement as R  # noqa: E402
from gpu_util import dev, host  # noqa: E402

SETS = C.node_sets()
ROWB = 48


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


@functools.lru_cache(maxsize=None)
def _levels(name, beta, levels):
    return R.node_levels(SETS[name], C.EPS, beta, levels)


def _plan(A, pos, k, slots=None, beta=4):
    """a plan over `pos` (the nodes are their own vertices), its graph built"""
    D = len(pos)
    s = A.Solver6(D, D, k)
    if slots is not None:
        s.set_reg_hierarchy(list(slots), C.EPS, beta)
    dq = np.zeros((D, 8), np.float32)
    dq[:, 0] = 1
    keep = [dev(pos), dev(dq), dev(np.full(D, 3 * C.EPS, np.float32)), dev(pos)]
    s.set_problem(*keep)
    return s, keep


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("beta", C.BETAS)
def test_node_levels_is_the_statement(A, name, beta):
    pos = SETS[name]
    for levels in (1, 2, 3, 4, 8):
        got = host(A.node_levels(dev(pos), C.EPS, beta, levels))
        ref = R.node_levels(pos, C.EPS, beta, levels)
        assert got.dtype == np.int32 and np.array_equal(got, ref), (levels, np.flatnonzero(got != ref)[:8])


def test_node_levels_with_cells_of_both_signs_and_out_of_range(A):
    rng = np.random.default_rng(11)
    pos = rng.uniform(-3, 3, (5000, 3)).astype(np.float32)
    pos[7] = [60000.0, 0.0, 0.0]    # |c0| >= 2^20 at epsilon = 0.05: no cell
    pos[8] = [np.inf, 0.0, 0.0]
    pos[9] = [0.0, -np.inf, 0.0]
    pos[10] = [-52428.75, 0.1, 0.1]  # c0 = -1 048 575: the last cell in range
    for eps, beta in ((0.05, 4), (0.05, 2), (0.31, 3), (0.05, 1 << 30)):
        got = host(A.node_levels(dev(pos), eps, beta, 8))
        assert np.array_equal(got, R.node_levels(pos, eps, beta, 8)), (eps, beta)
    assert (pos < 0).any()


@pytest.mark.parametrize("name", [n for n in SETS if n != "D0"])
@pytest.mark.parametrize("k,slots", C.CONFIGS)
@pytest.mark.parametrize("beta", C.BETAS)
def test_reg_graph_passes_the_row_check(A, name, k, slots, beta):
    pos = SETS[name]
    for levels in ((3,) if name == "sphere" else (2, 3, 4)):
        use = C.slots_for(slots, levels)
        s, keep = _plan(A, pos, k, use, beta)
        lv = host(s.node_levels())
        assert np.array_equal(lv, _levels(name, beta, levels))
        segments = R.check_rows(pos, lv, use, k, host(s.graphs()[1]))
        assert segments >= len(pos)
        s.close()


def test_append_keeps_the_levels(A):
    pos = SETS["sphere"]
    rng = np.random.default_rng(3)
    extra = (pos[rng.integers(0, len(pos), 16)] + rng.normal(0, 2 * C.EPS, (16, 3))).astype(np.float32)
    extra[0] = pos[0]
    before = host(A.node_levels(dev(pos), C.EPS, 4, 4))
    after = host(A.node_levels(dev(np.concatenate([pos, extra])), C.EPS, 4, 4))
    assert np.array_equal(after[:len(pos)], before) and before.max() == 3


@pytest.mark.parametrize("name", ["strip", "sphere", "nan", "D2"])
@pytest.mark.parametrize("k", [4, 8])
def test_one_level_is_the_flat_plan_bit_for_bit(A, name, k):
    pos = SETS[name]

    def graph_and_pattern(s):
        rg = host(s.graphs()[1]).copy()
        import torch
        cols = host(s._view("matrix_columns", (s.D, ROWB), torch.int32))
        cnt = host(s._view("matrix_row_blocks", (s.D,), torch.int32))
        used = np.arange(ROWB)[None, :] < cnt[:, None]
        return rg, cnt.copy(), cols[used].copy()

    flat, keep0 = _plan(A, pos, k)
    ref = graph_and_pattern(flat)
    assert flat.node_levels() is None
    one, keep1 = _plan(A, pos, k, (k,))
    assert one.node_levels() is None  # one level: the graph is flat
    for a, b in zip(ref, graph_and_pattern(one)):
        assert np.array_equal(a, b)
    # ... and a plan that had a hierarchy and was given back the flat graph
    one.set_reg_hierarchy(C.slots_for(C.CONFIGS[0][1], 3), C.EPS, 4)
    one.set_problem(*keep1)
    assert one.node_levels() is not None
    if len(pos) > 8:
        assert not np.array_equal(ref[0], host(one.graphs()[1]))
    one.set_reg_hierarchy(None)
    one.set_problem(*keep1)
    assert one.node_levels() is None
    for a, b in zip(ref, graph_and_pattern(one)):
        assert np.array_equal(a, b)
    flat.close(), one.close()


@pytest.mark.parametrize("slots,eps,beta", [((0, 2, 2), 0.05, 4), ((2, -1, 1), 0.05, 4), ((2, 2, 1), 0.05, 4), ((1,) * 9, 0.05, 4),
                                            ((2, 1, 1), 0.05, 1), ((2, 1, 1), 0.0, 4), ((2, 1, 1), -0.05, 4)])
def test_invalid_configurations_are_refused(A, slots, eps, beta):
    s = A.Solver6(16, 16, 4)
    with pytest.raises(A.DynfuAmdError, match="error 1:"):  # DFA_ERR_INVALID
        s.set_reg_hierarchy(list(slots), eps, beta)
    s.set_reg_hierarchy([2, 1, 1], 0.05, 4)  # (and a good one is taken)
    s.close()


def test_set_node_transforms_keeps_the_graph(A):
    pos = SETS["strip"]
    s, keep = _plan(A, pos, 4, (2, 1, 1))
    rg, lv = host(s.graphs()[1]).copy(), host(s.node_levels()).copy()
    s.set_node_transforms(keep[1].clone())
    assert np.array_equal(host(s.graphs()[1]), rg) and np.array_equal(host(s.node_levels()), lv)
    s.close()


def test_a_second_plan_on_a_second_stream_gives_the_same_rows(A):
    import torch
    pos = SETS["sphere"]
    s0, keep0 = _plan(A, pos, 8, (4, 2, 2))
    rg0, lv0 = host(s0.graphs()[1]).copy(), host(s0.node_levels()).copy()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s1, keep1 = _plan(A, pos, 8, (4, 2, 2))
        lv_alone = A.node_levels(keep1[0], C.EPS, 4, 3)
        side.synchronize()
        rg1, lv1 = host(s1.graphs()[1]).copy(), host(s1.node_levels()).copy()
    assert np.array_equal(rg0, rg1) and np.array_equal(lv0, lv1) and np.array_equal(host(lv_alone), lv0)
    s0.close(), s1.close()


def test_sphere_rows_stay_within_the_plan(A):
    pos = SETS["sphere"]
    sc = C.sphere_scene()
    s = A.Solver6(len(pos), len(sc["verts"]), 8)
    s.set_reg_hierarchy([4, 2, 2], C.EPS, 4)
    keep = [dev(sc["nodes"]), dev(sc["dq"]), dev(sc["w"]), dev(sc["verts"]), dev(sc["normals"])]
    s.set_problem(*keep)
    st = s.stats()
    flat = A.Solver6(len(pos), len(sc["verts"]), 8)
    flat.set_problem(*keep)
    print(f"\nsphere: max_row_blocks {st['max_row_blocks']} (flat {flat.stats()['max_row_blocks']}), level sets "
          f"{np.bincount(host(s.node_levels())).tolist()}", end="")
    assert st["overflow"] == 0 and 0 < st["max_row_blocks"] <= ROWB
    s.close(), flat.close()
