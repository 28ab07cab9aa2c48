"""CPU tests of tests/warp_statement.py (the numpy / fp64 statement of the warp-field seam the -m gpu tests compare
csrc/knn.hip, csrc/warp.hip, csrc/dqb_device.hpp and csrc/dq_device.hpp with).  No GPU."""
import json
import os

import numpy as np
import pytest

import oracle as O
import warp_statement as W
from gpu_util_cpu import rot

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "dq_kat.json")))


def _ulp_diff(a, b):
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ------------------------------------------------------------------ the reference's own known answers
def _fix(name):
    a = KAT["fixtures"][name]
    return W.dq_from_euler(*[KAT["rad"][x] for x in a[:3]], *[float(x) for x in a[3:]])


def _ev(e):
    op = e[0]
    if op == "fix":
        return _fix(e[1])
    if op == "rodrigues":
        return W.dq_from_rodrigues(e[1], [0, 0, 0])
    if op == "scale":
        return W.dq_scale(_ev(e[1]), e[2])
    if op == "normalize":
        return W.dq_normalize(_ev(e[1]))
    a, b = _ev(e[1]), _ev(e[2])
    return {"add": lambda: a + b, "sub": lambda: a - b, "mul": lambda: W.dq_mul(a, b)}[op]()


@pytest.mark.parametrize("case", KAT["transforms"], ids=lambda c: c["name"])
def test_statement_reproduces_the_known_transforms(case):
    out = W.dq_transform(_ev(case["expr"]), np.asarray(case["v"], np.float64))
    np.testing.assert_allclose(out, case["expect"], atol=KAT["tol"], rtol=0)


@pytest.mark.parametrize("case", KAT["cases"], ids=lambda c: c["name"])
def test_statement_reproduces_the_known_algebra(case):
    dq = _ev(case["expr"])
    if case.get("expect_real") is not None:
        np.testing.assert_allclose(dq[:4], case["expect_real"], atol=KAT["tol"], rtol=0)
    if case.get("expect_real_of") is not None:
        np.testing.assert_allclose(dq[:4], _ev(case["expect_real_of"])[:4], atol=KAT["tol"], rtol=0)
    if case.get("expect_dual") is not None:
        np.testing.assert_allclose(dq[4:], case["expect_dual"], atol=KAT["tol"], rtol=0)


# ------------------------------------------------------------------ rigid motions, by 4 x 4 matrices
def _euler_matrix(yaw, pitch, roll):
    """the rotation of dq_from_euler's quaternion: about z by yaw, about y by pitch, about x by roll"""
    return rot([0, 0, 1], yaw) @ rot([0, 1, 0], pitch) @ rot([1, 0, 0], roll)


def test_a_rigid_motion_shared_by_all_nodes_moves_every_vertex_by_that_motion():
    """k = 1 and a vertex on its node (weight 1): the blend IS the node's transform, v -> R v + t.  (With more neighbours
    the reference's "blend" is the ordered PRODUCT of the weighted transforms — the next test.)"""
    rng = np.random.default_rng(0)
    D = 50
    nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
    ang, t = (0.3, -0.2, 0.5), np.array([0.05, -0.02, 0.07])
    dq = np.tile(W.dq_from_euler(*ang, *t), (D, 1))
    node_w = np.full(D, 0.1, np.float32)
    ov, on = W.warp(nodes, dq.astype(np.float32), node_w, 1, nodes, nodes)
    R = _euler_matrix(*ang)
    want = nodes.astype(np.float64) @ R.T + t
    assert np.abs(ov - want).max() < 1e-7  # (the node transforms were rounded to float32)
    assert np.abs(on - want).max() < 1e-7  # transformNormal: the same formula, translation included
    # a pure translation shared by k nodes: the dual parts add, the vertex moves by (sum of weights) t
    dq = np.tile(W.dq_from_euler(0, 0, 0, *t), (D, 1)).astype(np.float32)
    verts = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    idx = W.knn(nodes, verts, 4)
    ov, _ = W.warp(nodes, dq, node_w, 4, verts)
    wsum = W.weights64(nodes, node_w, verts, idx).sum(1)
    assert np.abs(ov - (verts + wsum[:, None] * t)).max() < 1e-7


@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_the_blend_is_the_composition_of_the_weighted_rigid_motions(k):
    """w q (dual part scaled) is the rigid motion (R, w t); the ordered product of dual quaternions is the composition of
    the motions, the LAST neighbour applied first.  Checked against products of 4 x 4 matrices built from Euler angles —
    no quaternion on that side."""
    rng = np.random.default_rng(k)
    D, n = 40, 60
    nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
    node_w = rng.uniform(0.2, 0.6, D).astype(np.float32)
    ang, t = rng.uniform(-0.4, 0.4, (D, 3)), rng.uniform(-0.1, 0.1, (D, 3))
    dq = W.dq_from_euler(ang[:, 0], ang[:, 1], ang[:, 2], t[:, 0], t[:, 1], t[:, 2])
    assert np.abs(dq.astype(np.float32) - np.stack([O.dq_from_euler(*ang[i], *t[i]) for i in range(D)])).max() < 1e-6
    verts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    idx = W.knn(nodes, verts, k)
    w = W.weights64(nodes, node_w, verts, idx)
    # (fp64 node transforms on both sides: the statement takes float32 ones, so hand it the rounded ones and build the
    # matrices from the same rounded quaternions' rotation and translation)
    dq32 = dq.astype(np.float32)
    ov, _ = W.warp_graph(nodes, dq32, node_w, idx, verts)
    for v in range(n):
        M = np.eye(4)
        for j in range(k):
            q = dq32[idx[v, j]].astype(np.float64)
            qw, qx, qy, qz = q[:4]
            R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                          [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                          [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
            tt = 2 * W.qmul(q[4:], q[:4] * [1, -1, -1, -1])[1:]  # getTranslation :94-97: (2 dual) conj(real)
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R, w[v, j] * tt
            M = M @ T
        # (the product's real part is normalised at the end; unit-norm float32 inputs leave ~1e-7 of scale in R)
        want = M[:3, :3] @ verts[v].astype(np.float64) + M[:3, 3]
        assert np.abs(ov[v] - want).max() < 5e-6, (v, ov[v], want)
    # and the Euler-angle matrix is that rotation
    assert np.abs(W.dq_transform(W.dq_from_euler(*ang[0], 0, 0, 0), np.eye(3)).T - _euler_matrix(*ang[0])).max() < 1e-12


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("D,k,n", [(2048, 4, 3000), (500, 8, 2000), (3000, 16, 1000), (5, 8, 100), (1, 4, 10), (1025, 5, 777),
                                    (40, 1, 500), (300, 3, 500), (300, 7, 500), (300, 9, 500)])
def test_knn_weights_and_flags_equal_the_oracle(D, k, n):
    rng = np.random.default_rng(D + k)
    nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
    node_w = rng.uniform(0.05, 0.5, D).astype(np.float32)
    q = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    q[:min(n, D)] = nodes[:min(n, D)]
    idx = W.knn(nodes, q, k)
    assert np.array_equal(idx, O.knn(nodes, q, k, threads=4))
    w = W.weights(nodes, node_w, q, idx)
    for v in range(0, n, max(1, n // 200)):
        ref = [O.transformation_weight(nodes[i], float(node_w[i]), q[v]) if i >= 0 else 0.0 for i in idx[v]]
        assert _ulp_diff(w[v], np.array(ref, np.float32)).max() <= 1
    assert np.array_equal(W.unsupported_flags(nodes, node_w, k, q), O.unsupported_flags(nodes, node_w, k, q, threads=4))


def test_knn_ties_and_nan():
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    q = (g[::5] + np.float32(0.5)).astype(np.float32)
    assert np.array_equal(W.knn(g, q, 8), O.knn(g, q, 8))
    # the contract for a NaN query: no neighbour (the oracle's insertion loop takes the first k nodes instead — it states
    # nanoflann's loop, not dfa_knn's contract; the kernels' keys never admit a NaN distance)
    q[3, 1] = np.nan
    idx = W.knn(g, q, 8)
    assert (idx[3] == -1).all() and (idx[[2, 4]] >= 0).all()
    assert W.unsupported_flags(g, np.ones(len(g), np.float32), 8, q)[3] == 1


def _oracle_deviation(D, k, n):
    c = W.matrix_case(D, k, n)
    nodes, dq, node_w, verts, nrm = c["nodes"], c["dq"], c["node_w"], c["verts"], c["normals"]
    sv, sn = W.warp(nodes, dq, node_w, k, verts, nrm)
    ov, on = O.warp_to_live(nodes, dq, node_w, k, verts, nrm, threads=4)
    m = 200
    sq = W.calc_dqb(nodes, dq, node_w, k, verts[:m])
    oq = np.stack([O.calc_dqb(nodes, dq, node_w, k, verts[i]) for i in range(m)])
    return max(W.deviation(ov, sv), W.deviation(on, sn), W.deviation(oq, sq))


def test_the_recorded_oracle_deviation_holds_over_the_gpu_tests_inputs():
    """KERNEL_BOUND is twice ORACLE_DEVIATION, and ORACLE_DEVIATION is a record of this measurement: the largest absolute
    deviation of the float32 oracle from the fp64 statement over every shape of the GPU tests' matrix.  Above 1e-5 the
    statement or the oracle would be wrong."""
    worst = {}
    for D, k, n in W.MATRIX:
        worst[(D, k, n)] = _oracle_deviation(D, k, n)
    top = max(worst.values())
    print("oracle deviation from the fp64 statement: %.3e (at %r)" % (top, max(worst, key=worst.get)))
    assert top <= W.ORACLE_DEVIATION < 1e-5
    assert top > W.ORACLE_DEVIATION / 2  # the record is a measurement, not a generous round number
