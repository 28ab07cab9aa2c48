"""CPU checks of the north-star statement (tests/solve6_statement.py): its Jacobian against central differences of its own
residual through its own apply_twist, its H and g against the fp64 oracle's dump of the same linearisation
(orc6_set_dump) for k = 1 ... 8 and lambda = 0 / 200, its solution x* against the oracle's Gauss-Newton step, and hand
cases."""
import numpy as np
import pytest

import oracle as O
from dynfu_amd import synth
from solve6_statement import Statement6, apply_twist, dq_point

PRM = dict(tukey_offset=4.652, psi_data=0.01, lambda_=200.0, psi_reg=1e-4, dist_thresh=0.1, cos_thresh=0.5, damping=1e-4)


def _scene(name, frame, k=None, rough=0.0, seed=5):
    cfg = dict(synth.CONFIGS[name])
    if k:
        cfg["k"] = k
    c = synth.canonical(cfg)
    intr = synth.intrinsics(cfg)
    P, Nm = O.points_normals(synth.depth_frame(cfg, frame), *intr)
    dq = c["node_dq"].copy()
    if rough:
        rng = np.random.default_rng(seed)
        tw = np.c_[rng.normal(0, rough, (len(dq), 3)), rng.normal(0, rough / 5, (len(dq), 3))]
        dq = apply_twist(c["node_pos"], dq, tw).astype(np.float32)
    return cfg, c, intr, P, Nm, dq


def _oracle_blocks(dump):
    row_ptr, cols, blk, g = dump
    D = len(row_ptr) - 1
    rows = np.repeat(np.arange(D), np.diff(row_ptr))
    return {(int(a), int(b)): blk[i] for i, (a, b) in enumerate(zip(rows, cols))}, g


def _compare_with_oracle(S, dump, touched=None):
    """same column sets; |H - H_orc| <= 1e-9 |J|^T W |J| per entry on blocks no ambiguous vertex touches; g likewise"""
    ob, og = _oracle_blocks(dump)
    rows, cols, blocks = S.block_coo()
    assert set(ob) == set(zip(rows.tolist(), cols.tolist()))
    worst = 0.0
    for i, (a, b) in enumerate(zip(rows.tolist(), cols.tolist())):
        if touched is not None and (touched[a] or touched[b]):
            continue
        err = np.abs(blocks[i] - ob[(a, b)])
        worst = max(worst, float((err / np.maximum(S.habs[i], 1e-300)).max()))
    assert worst <= 1e-9, worst
    gscale = np.abs(S.J.T @ (S.W * np.abs(S.r))).reshape(S.D, 6)
    ok = np.ones(S.D, bool) if touched is None else ~touched
    gerr = (np.abs(S.g - og) / np.maximum(gscale, 1e-300))[ok]
    assert gerr.max(initial=0.0) <= 1e-9, gerr.max(initial=0.0)
    return worst


def _touched(S, idx):
    t = np.zeros(S.D, bool)
    amb = idx[S.amb]
    t[amb[amb >= 0]] = True
    return t


@pytest.mark.parametrize("name,frame", [("T0", 0), ("T0", 6), ("T1", 0), ("T1", 6)])
@pytest.mark.parametrize("k", [1, 4, 6, 8])
@pytest.mark.parametrize("lam", [0.0, 200.0])
def test_normal_equations_equal_the_oracle_dump(name, frame, k, lam):
    cfg, c, intr, P, Nm, dq = _scene(name, frame, k)
    idx, wn, reg = O.graph6(c["node_pos"], c["node_w"], k, c["verts"])
    prm = dict(PRM, lambda_=lam)
    S = Statement6(c["node_pos"], dq, c["node_w"], c["verts"], c["normals"], P, Nm, intr, prm, idx, reg, wn=wn, pattern="weights")
    dump, (_, st) = O.solve6_dump(c["node_pos"], dq, c["node_w"], k, c["verts"], c["normals"], P, Nm, intr, gn=0,
                                  num_iter=1, gn_iter=1, linear_iter=1, **prm)
    assert st["valid_first"] == S.valid
    assert st["initial_cost"] == pytest.approx(S.cost, rel=1e-9)
    _compare_with_oracle(S, dump, _touched(S, idx))
    # (uniform fractional pixel coordinates put 4e-3 of the vertices within 1e-3 px of a rounding boundary in u or v)
    assert S.n_amb <= 6e-3 * len(c["verts"])


@pytest.mark.parametrize("name,k,lam,rough", [("T0", 4, 200.0, 0.0), ("T0", 3, 500.0, 0.01), ("T1", 8, 200.0, 0.0)])
def test_solution_is_the_oracle_gauss_newton_step(name, k, lam, rough):
    cfg, c, intr, P, Nm, dq = _scene(name, 6, k, rough=rough)
    idx, wn, reg = O.graph6(c["node_pos"], c["node_w"], k, c["verts"])
    prm = dict(PRM, lambda_=lam)
    S = Statement6(c["node_pos"], dq, c["node_w"], c["verts"], c["normals"], P, Nm, intr, prm, idx, reg, wn=wn, pattern="weights")
    x = S.solve()
    assert np.abs(S.H @ x.reshape(-1) - S.g.reshape(-1)).max() <= 1e-9 * np.abs(S.g).max()
    out, st = O.solve6(c["node_pos"], dq, c["node_w"], k, c["verts"], c["normals"], P, Nm, intr, num_iter=1, gn_iter=1,
                       linear_iter=3000, pcg_tol=1e-9, **prm)
    assert st["pcg_rel_hist"][0] <= 1e-9
    mine = apply_twist(c["node_pos"], dq, x)
    # (the oracle returns float32 transforms; its PCG stops at a relative residual of 1e-9)
    assert np.abs(mine - out).max() <= 2e-6, np.abs(mine - out).max()


def test_jacobian_is_the_derivative_of_the_residual():
    cfg, c, intr, P, Nm, dq = _scene("T0", 6, 4, rough=0.02)
    idx, wn, reg = O.graph6(c["node_pos"], c["node_w"], 4, c["verts"])
    S = Statement6(c["node_pos"], dq, c["node_w"], c["verts"], c["normals"], P, Nm, intr, PRM, idx, reg, wn=wn, pattern="weights")
    assert S.valid > 1000
    J = S.J.tocsc()
    dq64 = dq.astype(np.float64)
    rng = np.random.default_rng(1)
    h = 1e-6
    for i in rng.choice(S.D, 6, replace=False):
        for comp in range(6):
            tw = np.zeros((S.D, 6))
            tw[i, comp] = h
            rp = S.residuals(apply_twist(c["node_pos"], dq64, tw))
            rm = S.residuals(apply_twist(c["node_pos"], dq64, -tw))
            fd = (rp - rm) / (2 * h)
            col = J[:, 6 * i + comp].toarray().ravel()
            scale = np.abs(col).max()
            assert scale > 0
            assert np.abs(fd - col).max() <= 1e-6 * scale, (i, comp, np.abs(fd - col).max() / scale)


def _tiny_image(p, n, l_offset=0.0, size=3):
    """a size x size live map whose centre pixel holds l = p + l_offset n and normal n; intrinsics that put p there"""
    f = 100.0
    cx = cy = (size - 1) / 2
    intr = (f, f, cx - f * p[0] / p[2], cy - f * p[1] / p[2])
    vmap = np.full((size, size, 4), np.nan, np.float32)
    nmap = np.full((size, size, 4), np.nan, np.float32)
    vmap[size // 2, size // 2, :3] = p + l_offset * n
    vmap[size // 2, size // 2, 3] = 0
    nmap[size // 2, size // 2, :3] = n
    nmap[size // 2, size // 2, 3] = 0
    return vmap, nmap, intr


def test_one_vertex_one_node_by_hand():
    """k = 1: p = T(c), the row is a = ((p - g^) x n, n), H = rho a a^T + damping I, g = -rho a r"""
    g0 = np.array([[0.1, -0.05, 1.2]], np.float32)
    # a rotation of 120 degrees about (1, 1, 1) — unit in float32 — and a translation
    from solve6_statement import pure, qmul
    r = np.array([0.5, 0.5, 0.5, 0.5])
    dq = np.r_[r, 0.5 * qmul(pure(np.array([0.01, 0.02, -0.03])), r)][None].astype(np.float32)
    c0 = np.array([0.12, -0.02, 1.18])
    g0 = (g0.astype(np.float64) - 0).astype(np.float32)
    # the canonical point whose image lies in front of the camera: T^-1 of c0 (R^T (c0 - t))
    rot = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64)  # (w = x = y = z = 1/2: x -> y -> z -> x)
    c = (rot.T @ (c0 - np.array([0.01, 0.02, -0.03])))[None].astype(np.float32)
    n = np.array([0.3, -0.2, -0.9])
    n = (n / np.linalg.norm(n)).astype(np.float32)
    p = dq_point(dq.astype(np.float64), c.astype(np.float64))[0]
    vmap, nmap, intr = _tiny_image(p, n.astype(np.float64), -0.004)
    prm = dict(PRM, lambda_=0.0)
    S = Statement6(g0, dq, np.array([0.5], np.float32), c, None, vmap, nmap, intr, prm, np.zeros((1, 1), np.int32),
                   -np.ones((1, 1), np.int32))
    assert S.valid == 1 and S.assoc[0]
    l = vmap[1, 1, :3].astype(np.float64)
    nn = n.astype(np.float64)
    r = nn @ (p - l)
    assert r == pytest.approx(0.004, rel=1e-4)
    rho = (1 - (abs(r) / float(np.float32(4.652)) / float(np.float32(0.01))) ** 2) ** 2  # (float32 parameters)
    gh = dq_point(dq.astype(np.float64), g0.astype(np.float64))[0]
    a = np.r_[np.cross(p - gh, nn), nn]
    H = rho * np.outer(a, a) + float(np.float32(1e-4)) * np.eye(6)
    assert S.row_blocks.tolist() == [1] and S.cols.tolist() == [0]
    assert np.allclose(S.blocks[0], H, rtol=1e-12, atol=1e-15)
    assert np.allclose(S.g[0], -rho * a * r, rtol=1e-12, atol=1e-18)
    assert S.cost == pytest.approx(rho * r * r, rel=1e-12)


def test_two_nodes_regulariser_only_with_huber_active():
    g = np.array([[0.0, 0.0, 1.0], [0.05, 0.01, 1.02]], np.float32)
    ident = np.array([[1, 0, 0, 0, 0, 0, 0, 0]] * 2, np.float64)
    t = np.array([[0.003, 0.0, -0.001, 0, 0, 0], [0.0, -0.002, 0.001, 0, 0, 0]])
    tw = np.c_[np.zeros((2, 3)), t[:, :3]]
    dq = apply_twist(g, ident, tw).astype(np.float32)
    vmap = np.full((2, 2, 4), np.nan, np.float32)
    prm = dict(PRM, lambda_=200.0, psi_reg=1e-3)
    reg = np.array([[1], [0]], np.int32)
    S = Statement6(g, dq, np.full(2, 0.5, np.float32), np.zeros((0, 3), np.float32), None, vmap, vmap, (100, 100, 1, 1), prm,
                   np.zeros((0, 1), np.int32), reg)
    wreg2 = 200.0 / (2 * 1)
    Hd = np.zeros((12, 12))
    gd = np.zeros(12)
    cost = 0.0
    tr = dq_point(dq.astype(np.float64), np.zeros((2, 3)))  # translations of the (pure-translation) transforms
    for n_, m_ in ((0, 1), (1, 0)):
        e = tr[n_] - tr[m_]  # T_n(g_m) - T_m(g_m) for translations
        lev = g[m_].astype(np.float64) - g[n_] + 0.0  # T_n(g_m) - T_n(g_n)
        en = np.linalg.norm(e)
        assert en > 1e-3  # Huber active
        w = wreg2 * float(np.float32(1e-3)) / en
        Jr = np.zeros((3, 12))
        Jr[:, 6 * n_:6 * n_ + 3] = -np.array([[0, -lev[2], lev[1]], [lev[2], 0, -lev[0]], [-lev[1], lev[0], 0]])
        Jr[:, 6 * n_ + 3:6 * n_ + 6] = np.eye(3)
        Jr[:, 6 * m_ + 3:6 * m_ + 6] = -np.eye(3)
        Hd += w * Jr.T @ Jr
        gd -= w * Jr.T @ e
        cost += w * en * en
    Hd += float(np.float32(1e-4)) * np.eye(12)
    Hs = S.H.toarray()
    assert np.allclose(Hs, Hd, rtol=1e-9, atol=1e-12) and np.allclose(S.g.reshape(-1), gd, rtol=1e-9, atol=1e-15)
    assert S.cost == pytest.approx(cost, rel=1e-9)
    assert S.row_blocks.tolist() == [2, 2] and S.cols.tolist() == [0, 1, 1, 0]


def test_fewer_nodes_than_k_plus_one():
    cfg, c, intr, P, Nm, dq = _scene("T0", 2, 4)
    D, k = 3, 4
    nodes, dq3, w = c["node_pos"][:D], dq[:D], np.full(D, 0.4, np.float32)
    verts, normals = c["verts"][::16], c["normals"][::16]
    idx, wn, reg = O.graph6(nodes, w, k, verts)
    assert (idx[:, 3] == -1).all() and (reg[:, 2:] == -1).all()
    S = Statement6(nodes, dq3, w, verts, normals, P, Nm, intr, PRM, idx, reg, wn=wn, pattern="weights")
    dump, (_, st) = O.solve6_dump(nodes, dq3, w, k, verts, normals, P, Nm, intr, num_iter=1, gn_iter=1, linear_iter=1, **PRM)
    assert st["valid_first"] == S.valid > 0
    _compare_with_oracle(S, dump)  # (float64 on both sides: every vertex, ambiguous or not)


def test_negated_transforms_give_the_same_system():
    cfg, c, intr, P, Nm, dq = _scene("T0", 6, 4, rough=0.01)
    idx, wn, reg = O.graph6(c["node_pos"], c["node_w"], 4, c["verts"])
    S = Statement6(c["node_pos"], dq, c["node_w"], c["verts"], c["normals"], P, Nm, intr, PRM, idx, reg, wn=wn, pattern="weights")
    S2 = Statement6(c["node_pos"], -dq, c["node_w"], c["verts"], c["normals"], P, Nm, intr, PRM, idx, reg, wn=wn, pattern="weights")
    assert S2.valid == S.valid and np.array_equal(S2.cols, S.cols)
    assert np.allclose(S2.blocks, S.blocks, rtol=1e-12, atol=1e-12 * np.abs(S.blocks).max())
    assert np.allclose(S2.g, S.g, rtol=1e-12, atol=1e-12 * np.abs(S.g).max())
    # and half of them negated: the hemisphere signs undo it
    dqh = dq.copy()
    dqh[::2] *= -1
    S3 = Statement6(c["node_pos"], dqh, c["node_w"], c["verts"], c["normals"], P, Nm, intr, PRM, idx, reg, wn=wn, pattern="weights")
    assert np.allclose(S3.blocks, S.blocks, rtol=1e-12, atol=1e-12 * np.abs(S.blocks).max())


def test_rigid_field_has_no_regulariser_residual():
    """every node carries the same rigid motion: every edge residual is 0, the regulariser adds to H only"""
    cfg, c, intr, P, Nm, dq = _scene("T0", 0, 4)
    D = len(dq)
    r = np.array([0.995, 0.05, -0.08, 0.02])
    r /= np.linalg.norm(r)
    from solve6_statement import pure, qmul
    d = 0.5 * qmul(pure(np.array([0.01, -0.004, 0.02])), r)
    R = np.tile(np.r_[r, d], (D, 1)).astype(np.float32)
    idx, wn, reg = O.graph6(c["node_pos"], c["node_w"], 4, c["verts"])
    S0 = Statement6(c["node_pos"], R, c["node_w"], c["verts"], c["normals"], P, Nm, intr, dict(PRM, lambda_=0.0), idx, reg, wn=wn, pattern="weights")
    S = Statement6(c["node_pos"], R, c["node_w"], c["verts"], c["normals"], P, Nm, intr, PRM, idx, reg, wn=wn, pattern="weights")
    assert S.valid > 0
    assert np.abs(S.r[S.N:]).max() <= 1e-15
    assert S.cost == pytest.approx(S0.cost, rel=1e-12)
    assert np.allclose(S.g, S0.g, rtol=0, atol=1e-12 * np.abs(S0.g).max())
    assert (S.blocks[S.cols == np.repeat(np.arange(D), S.row_blocks)][:, 3:, 3:].trace(axis1=1, axis2=2)
            > S0.blocks[S0.cols == np.repeat(np.arange(D), S0.row_blocks)][:, 3:, 3:].trace(axis1=1, axis2=2)).all()


def test_all_rows_rejected_without_regulariser():
    cfg, c, intr, P, Nm, dq = _scene("T0", 0, 4)
    empty = np.full_like(P, np.nan)
    idx, wn, reg = O.graph6(c["node_pos"], c["node_w"], 4, c["verts"])
    S = Statement6(c["node_pos"], dq, c["node_w"], c["verts"], c["normals"], empty, empty, intr, dict(PRM, lambda_=0.0),
                   idx, reg, wn=wn, pattern="weights")
    assert S.valid == 0 and S.cost == 0.0 and not S.g.any()
    diag = S.cols == np.repeat(np.arange(S.D), S.row_blocks)
    assert np.array_equal(S.blocks[diag], np.broadcast_to(float(np.float32(1e-4)) * np.eye(6), (S.D, 6, 6)))
    assert not S.blocks[~diag].any()
    assert not S.solve().any()
