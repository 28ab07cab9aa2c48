"""-m gpu: the north-star solve over the multi-level regularisation graph.

(a) The sphere at k = 8, slots {4, 2, 2}: normal equations, PCG step and update against the float64 statement of one
    linearisation (tests/solve6_statement.py) fed the plan's own reg_graph — the checks and tolerances of
    test_gpu_solve6_normal_equations.py, imported.
(b) Propagation on the strip at k = 4 from identity transforms: a vertex mask leaves data rows only where x < 0.2 m, the
    live maps are the surface moved 5 mm along its normal, one Gauss-Newton iteration of 14 PCG iterations at pcg_tol = 0.
    Hops are breadth-first distances over the plan's real block pattern from the nodes with a non-zero gradient.  Asserted
    first: the farthest node is at least 16 hops away in the flat plan and at most 12 in the hierarchical one (the
    statement alone gives 22 and 7: test_reg_hierarchy_statement_cpu.py).  Then: every node beyond 14 hops has a step of
    exactly 0.0 in both plans, and the farthest node's step is exactly zero flat and non-zero hierarchical."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import reg_hierarchy_cases as C  # noqa: E402
import reg_hierarchy_statement as R  # noqa: E402
from gpu_util import dev, host  # noqa: E402
from test_gpu_solve6_normal_equations import PRM, _check, _check_pcg, _check_update, _statement  # noqa: E402

ROWB = 48


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _solve(A, sc, k, slots, linear_iter, pcg_tol, mask=None):
    s = A.Solver6(len(sc["nodes"]), len(sc["verts"]), k)
    if slots is not None:
        s.set_reg_hierarchy(list(slots), C.EPS, 4)
    keep = [dev(sc["nodes"]), dev(sc["dq"]), dev(sc["w"]), dev(sc["verts"]), dev(sc["normals"])]
    s.set_problem(*keep)
    if mask is not None:
        s.set_vertex_mask(dev(mask))
    s.solve(sc["P"], sc["Nm"], *sc["intr"], A.Solve6Params(num_iter=1, gn_iter=1, linear_iter=linear_iter, pcg_tol=pcg_tol,
                                                             gn_tol=0.0, **PRM))
    blocks, cols, cnt, g = (host(x).copy() for x in s.matrix())
    dg, rg = (host(x).copy() for x in s.graphs())
    lv = s.node_levels()
    out = dict(blocks=blocks, cols=cols, cnt=cnt, g=g, x=host(s.step()).copy(), dq=host(s.node_dq()).copy(), dg=dg, rg=rg,
               st=s.stats(), prm=dict(PRM), linear_iter=linear_iter, tol=pcg_tol, levels=None if lv is None else host(lv).copy())
    s.close()
    return out


def test_normal_equations_and_pcg_step_on_the_sphere(A):
    sc = C.sphere_scene()
    sc.update(P=dev(sc["vmap"]), Nm=dev(sc["nmap"]), k=8)
    slots = (4, 2, 2)
    out = _solve(A, sc, 8, slots, 100, 1e-4)
    assert np.array_equal(out["levels"], R.node_levels(sc["nodes"], C.EPS, 4, 3)) and out["levels"].max() == 2
    R.check_rows(sc["nodes"], out["levels"], slots, 8, out["rg"])
    S = _statement(sc, out)
    assert S.valid > 0.2 * S.N  # (the half of the sphere that faces the camera)
    Hd = _check(S, out, "sphere, slots {4, 2, 2}")
    _check_pcg(S, out, Hd, "sphere, slots {4, 2, 2}")
    _check_update(S, sc, out)
    assert out["st"]["overflow"] == 0 and S.row_blocks.max() <= ROWB


LINEAR_ITER = 14


def test_a_step_reaches_the_far_end_of_the_strip_through_the_hierarchy_only(A):
    sc = C.strip_scene()
    sc.update(P=dev(sc["vmap"]), Nm=dev(sc["nmap"]))
    res = {}
    for name, slots in (("flat", None), ("hierarchical", (2, 1, 1))):
        out = _solve(A, sc, 4, slots, LINEAR_ITER, 0.0, mask=sc["mask"])
        assert out["st"]["pcg_it_hist"][0] == LINEAR_ITER and 0 < out["st"]["valid_hist"][0] <= int(sc["mask"].sum())
        sources = np.flatnonzero(np.abs(out["g"]).max(1) > 0)
        assert 0 < len(sources) < 16
        h = R.hops(R.pattern_of_plan(out["cols"], out["cnt"]), sources)
        assert h.min() >= 0 and np.isfinite(out["x"]).all()
        res[name] = (h, np.abs(out["x"]).max(1))
        print(f"\n{name}: farthest node {h.max()} hops, largest |step| there {res[name][1][h == h.max()].max():.3g}; "
              f"max row blocks {out['cnt'].max()}", end="")
    (hf, xf), (hh, xh) = res["flat"], res["hierarchical"]
    # the preconditions
    assert hf.max() >= LINEAR_ITER + 2, hf.max()
    assert hh.max() <= LINEAR_ITER - 2, hh.max()
    far = int(np.argmax(hf))
    assert hh[far] <= LINEAR_ITER - 2
    # a PCG iteration carries the step one hop
    assert (xf[hf > LINEAR_ITER] == 0.0).all() and (xh[hh > LINEAR_ITER] == 0.0).all()
    assert (hf > LINEAR_ITER).any()
    assert xf[far] == 0.0 and xh[far] != 0.0
    assert (xh[hh == hh.max()] != 0.0).all()  # the hierarchy's own far end has moved as well
