"""-m gpu: the default assembly writes every ELL row in ascending column order (the register-resident PCG's gather then
spreads its LDS reads over the banks), with the same bits as the order-stable variant, and C2 still solves to the float64
oracle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import dev, host  # noqa: E402


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _params(A, **kw):
    d = dict(num_iter=1, nonlinear_iter=1, linear_iter=256, tukey_offset=4.652, psi_data=0.01, lambda_=200.0,
             psi_reg=1e-4, pcg_tol=1e-6, gn_tol=0.0)
    d.update(kw)
    return A.SolveParams(**d)


def _inputs(A, name, noise=1e-3):
    cfg = synth.CONFIGS[name]
    c = synth.canonical(cfg)
    k = cfg["k"]
    nodes, node_w, node_dq, verts = (dev(c[n]) for n in ("node_pos", "node_w", "node_dq", "verts"))
    idx, w = A.knn(nodes, node_w, verts, k)
    t_true = synth.true_translations(c["node_pos"], 7, k)
    live_np = synth.live_vertices(c["verts"], host(idx), host(w), t_true)
    if noise:
        live_np = (live_np + np.random.default_rng(11).normal(0, noise, live_np.shape)).astype(np.float32)
    return cfg, c, (nodes, node_dq, node_w, verts, dev(live_np)), live_np


def _matrix(A, cfg, c, args, det):
    """(entries as (value bits, column), row lengths) of a one-linearisation solve: both variants assemble at the same t"""
    s = A.Solver(cfg["D"], len(c["verts"]), cfg["k"])
    s.set_deterministic(det)
    s.set_problem(*args)
    s.solve(_params(A))
    ent, cnt, _ = (host(x) for x in s.matrix())
    ent, cnt = ent.copy(), cnt.copy()
    s.close()
    return ent.view(np.uint32), cnt


@pytest.mark.parametrize("name", ["T1", "C2"])
def test_default_rows_are_sorted_and_equal_the_order_stable_rows(A, name):
    cfg, c, args, _ = _inputs(A, name)
    D = cfg["D"]
    m, cnt = _matrix(A, cfg, c, args, det=False)
    md, cntd = _matrix(A, cfg, c, args, det=True)
    assert np.array_equal(cnt, cntd)
    assert (cnt > 0).all() and cnt.max() <= 256
    cols = m[..., 1].view(np.int32)
    for a in range(D):
        n = cnt[a]
        assert (np.diff(cols[:n, a]) > 0).all(), (a, cols[:n, a])
        assert ((cols[:n, a] >= 0) & (cols[:n, a] < D)).all()
        # the off-diagonal entries are fixed-point sums in both variants: the same bits at the same places (the diagonal
        # is summed in float by the order-stable variant)
        off = cols[:n, a] != a
        assert np.array_equal(m[:n, a][off], md[:n, a][off]), a
        assert np.array_equal(md[:n, a, 1], m[:n, a, 1])


def test_c2_translations_match_the_oracle(A):
    cfg, c, args, live_np = _inputs(A, "C2")
    k, D = cfg["k"], cfg["D"]
    kw = dict(num_iter=cfg["gn_iters"], nonlinear_iter=1, linear_iter=256, pcg_tol=1e-6, **synth.SOLVER)
    t_ref, _, st_ref = O.solve_ref(c["node_pos"], c["node_dq"], c["node_w"], k, c["verts"], live_np, use_double=True,
                                   threads=max(1, min(16, os.cpu_count() or 1)), **kw)
    s = A.Solver(D, len(c["verts"]), k)
    s.set_problem(*args)
    s.solve(_params(A, **kw))
    t, st = host(s.translations()), s.stats()
    ent, cnt, _ = (host(x) for x in s.matrix())
    cols = ent.view(np.uint32)[..., 1].view(np.int32)
    assert all((np.diff(cols[: cnt[a], a]) > 0).all() for a in range(D))
    s.close()
    assert st["gn_iters"] == st_ref["gn_iters"] == cfg["gn_iters"]
    assert np.abs(t - t_ref).max() <= 2e-5, (np.abs(t - t_ref).max(), np.abs(t_ref).max())
    np.testing.assert_allclose(st["final_cost"], st_ref["final_cost"], rtol=1e-3)
