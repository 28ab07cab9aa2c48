"""CPU statement of the warp-field seam in numpy: the k-NN contract of dfa_knn, the RBF weights, and — in fp64 throughout —
the reference's ordered dual-quaternion "blend" (Warpfield::calcDQB, src/dynfu/warp_field.cpp:127-148), transformVertex /
transformNormal (include/dynfu/utils/dual_quaternion.hpp:204-228) and Warpfield::getUnsupportedVertices (:34-62).

knn and unsupported_flags are exact statements (integer results of float32 / fp64 decisions the contract spells out).
calc_dqb and warp are the MATHEMATICAL statement, not an operation-order copy of csrc/dq_device.hpp or oracle/dq_oracle.c:
float32 code is compared with them within KERNEL_BOUND, which is twice the largest deviation of the float32 oracle measured
over the GPU tests' own inputs (matrix_case below; tests/test_warp_statement_cpu.py measures it again on every run).

Dual quaternions are 8 numbers: real w, x, y, z; dual w, x, y, z.
"""
import numpy as np

f32 = np.float32

# The largest |oracle - statement| over every shape of MATRIX (vertices, normals and blended dual quaternions), measured on
# the CPU: see DESIGN_NOTES.md.  The kernels share the oracle's operation order and differ from it by exp's last bit only;
# they are allowed twice the oracle's own deviation, and nothing else.
ORACLE_DEVIATION = 9.0e-7  # measured 8.783e-07, at (D, k, n) = (1024, 16, 2000)
KERNEL_BOUND = 2 * ORACLE_DEVIATION

K_LIST = (1, 3, 4, 5, 8, 9, 16)
D_LIST = (2, 63, 64, 300, 1024, 2048)


def want_grid(D, n):
    """csrc/capi_internal.hpp: the uniform-grid search is taken for D >= 64 and (D * n >= 2^22 or D >= 1024)"""
    return D >= 64 and (D * n >= (1 << 22) or D >= 1024)


def matrix_sizes(D):
    """vertex counts of a shape: either side of want_grid where D allows both searches"""
    if 64 <= D < 1024:
        return [2000, (1 << 22) // D + 500]
    return [2000]


MATRIX = [(D, k, n) for D in D_LIST for k in K_LIST for n in matrix_sizes(D)]


def matrix_case(D, k, n):
    """the inputs of one shape: nodes, radii, general rigid node transforms (rotation + translation, as the existing warp
    test draws them), vertices (the first ones exactly on nodes) and unit normals — all float32"""
    rng = np.random.default_rng(1000 * D + 10 * k + (n > 2000))
    nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
    node_w = rng.uniform(0.05, 0.5, D).astype(np.float32)
    dq = dq_from_euler(*rng.uniform(-0.2, 0.2, (3, D)), *rng.uniform(-0.05, 0.05, (3, D))).astype(np.float32)
    verts = rng.uniform(-1.1, 1.1, (n, 3)).astype(np.float32)
    verts[:min(n, D)] = nodes[:min(n, D)]
    nrm = rng.standard_normal((n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return dict(nodes=nodes, node_w=node_w, dq=dq, verts=verts, normals=nrm)


# ------------------------------------------------------------------------------------------ k-NN, weights
def knn(nodes, query, k, chunk=2048):
    """dfa_knn's contract: per query the k nodes with the smallest (squared distance, index), ascending; the float32
    distance is ((d0*d0 + d1*d1) + d2*d2) with d = query - node (nanoflann L2_Simple_Adaptor); -1 padded when D < k;
    a NaN distance is never a neighbour (a NaN query gets all -1).  int32 (n, k)."""
    nodes = np.asarray(nodes, np.float32).reshape(-1, 3)
    query = np.asarray(query, np.float32).reshape(-1, 3)
    D, n = len(nodes), len(query)
    out = np.full((n, k), -1, np.int32)
    m = min(k, D)
    for s in range(0, n, chunk):
        q = query[s:s + chunk]
        with np.errstate(all="ignore"):
            d = q[:, None, :] - nodes[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        key = np.where(np.isnan(d2), np.float32(np.inf), d2)
        order = np.argsort(key, axis=1, kind="stable")[:, :m]  # stable: equal distances keep the lower index first
        got = np.take_along_axis(d2, order, 1)
        out[s:s + chunk, :m] = np.where(np.isnan(got), -1, order)
    return out


def weights64(nodes, node_w, query, idx):
    """Node::getTransformationWeight (src/dynfu/utils/node.cpp:29-36) of the neighbours idx (n, k): exp(-|g - v|^2 / (2 w^2))
    in fp64 from the float32 differences g - v; 0 for an absent neighbour.  fp64 (n, k)."""
    nodes = np.asarray(nodes, np.float32).reshape(-1, 3)
    query = np.asarray(query, np.float32).reshape(-1, 3)
    j = np.maximum(idx, 0)
    with np.errstate(all="ignore"):
        d = (nodes[j] - query[:, None, :]).astype(np.float64)  # the float32 difference, then double (pow(float, int))
        w = np.asarray(node_w, np.float32)[j].astype(np.float64)
        out = np.exp(-(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) / (2 * (w * w)))
    return np.where(idx >= 0, out, 0.0)


def weights(nodes, node_w, query, idx):
    """... rounded to float32, as the reference stores it.  The kernels may differ by 1 float ulp (two libms)."""
    return weights64(nodes, node_w, query, idx).astype(np.float32)


# ------------------------------------------------------------------------------------------ dual quaternions, fp64
def qmul(a, b):
    """Hamilton product, arrays (..., 4)"""
    aw, ax, ay, az = np.moveaxis(np.asarray(a, np.float64), -1, 0)
    bw, bx, by, bz = np.moveaxis(np.asarray(b, np.float64), -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def dq_mul(a, b):
    """dual_quaternion.hpp:127-129: (ra rb, ra db + da rb)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.concatenate([qmul(a[..., :4], b[..., :4]), qmul(a[..., :4], b[..., 4:]) + qmul(a[..., 4:], b[..., :4])], -1)


def dq_scale(a, s):
    """:120: a scalar scales the dual part only"""
    a = np.asarray(a, np.float64)
    return np.concatenate([a[..., :4], a[..., 4:] * np.asarray(s, np.float64)[..., None]], -1)


def dq_normalize(a):
    """:139-144: the real part divided by its norm, the dual part as it is"""
    a = np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        return np.concatenate([a[..., :4] / np.linalg.norm(a[..., :4], axis=-1, keepdims=True), a[..., 4:]], -1)


def dq_from_rotation_translation(rot, t):
    """:42-45: real = rot / |rot|, dual = ((0, t) real) / 2"""
    rot, t = np.asarray(rot, np.float64), np.asarray(t, np.float64)
    real = rot / np.linalg.norm(rot, axis=-1, keepdims=True)
    return np.concatenate([real, 0.5 * qmul(np.concatenate([np.zeros(t.shape[:-1] + (1,)), t], -1), real)], -1)


def dq_from_euler(yaw, pitch, roll, x, y, z):
    """:48-67"""
    yaw, pitch, roll = (np.asarray(v, np.float64) for v in (yaw, pitch, roll))
    cy, sy, cr, sr, cp, sp = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2)
    rot = np.stack([cy * cr * cp + sy * sr * sp, cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp,
                    sy * cr * cp - cy * sr * sp], -1)
    return dq_from_rotation_translation(rot, np.stack(np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (x, y, z))), -1))


def dq_from_rodrigues(rod, t):
    """:70-86: angle 2 atan |rod| about rod / |rod|"""
    rod = np.asarray(rod, np.float64)
    nrm = np.linalg.norm(rod)
    theta = 2 * np.arctan(nrm)
    rot = np.concatenate([[np.cos(theta / 2)], np.sin(theta / 2) * rod / nrm])
    return dq_from_rotation_translation(rot, t)


def dq_transform(a, v):
    """transformVertex :204-215 (transformNormal :217-228 is the same formula, translation included):
    v + 2 r x (r x v + w v) + 2 (w d - d0 r + r x d)"""
    a, v = np.asarray(a, np.float64), np.asarray(v, np.float64)
    w, r, d0, d = a[..., 0:1], a[..., 1:4], a[..., 4:5], a[..., 5:8]
    with np.errstate(all="ignore"):
        return v + 2 * np.cross(r, np.cross(r, v) + w * v) + 2 * (w * d - d0 * r + np.cross(r, d))


IDENTITY = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])


def calc_dqb_graph(nodes, node_dq, node_w, idx, pts):
    """Warpfield::calcDQB with the neighbours given: normalize(identity . (w1 q1) . (w2 q2) ...) over the present
    neighbours in list order.  fp64 (n, 8)."""
    node_dq = np.asarray(node_dq, np.float32).reshape(-1, 8).astype(np.float64)
    w = weights64(nodes, node_w, pts, idx)
    acc = np.tile(IDENTITY, (len(idx), 1))
    for j in range(idx.shape[1]):
        on = idx[:, j] >= 0
        with np.errstate(all="ignore"):
            prod = dq_mul(acc, dq_scale(node_dq[np.maximum(idx[:, j], 0)], w[:, j]))
        acc = np.where(on[:, None], prod, acc)
    return dq_normalize(acc)


def calc_dqb(nodes, node_dq, node_w, k, pts):
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    return calc_dqb_graph(nodes, node_dq, node_w, knn(nodes, pts, k), pts)


def warp_graph(nodes, node_dq, node_w, idx, verts, normals=None):
    """Warpfield::warpToLive (:150-171) with the neighbours given: (vertices, normals or None), fp64"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    dq = calc_dqb_graph(nodes, node_dq, node_w, idx, verts)
    ov = dq_transform(dq, verts.astype(np.float64))
    on = None if normals is None else dq_transform(dq, np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64))
    return ov, on


def warp(nodes, node_dq, node_w, k, verts, normals=None):
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    return warp_graph(nodes, node_dq, node_w, knn(nodes, verts, k), verts, normals)


def unsupported_flags(nodes, node_w, k, verts):
    """Warpfield::getUnsupportedVertices (:34-62): 1 where min over the k nearest nodes of |v - g| / w is >= 1.  The root is
    the fp64 root of the fp64 squares of the float32 differences, rounded to float32 (:45-46); the divide is a float32
    divide; the minimum starts at HUGE_VALF and takes a quotient with `<=` (a NaN never enters).  uint8 (n,)."""
    nodes = np.asarray(nodes, np.float32).reshape(-1, 3)
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    if len(nodes) == 0:
        return np.ones(len(verts), np.uint8)
    idx = knn(nodes, verts, k)
    j = np.maximum(idx, 0)
    with np.errstate(all="ignore"):
        d = (verts[:, None, :] - nodes[j]).astype(np.float64)
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(np.float32)
        q = dist / np.asarray(node_w, np.float32)[j]
    q = np.where((idx >= 0) & ~np.isnan(q), q, np.float32(np.inf))
    return (q.min(axis=1) >= np.float32(1)).astype(np.uint8)


def deviation(got, want):
    """largest absolute deviation where `want` is finite; NaN positions must agree"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    ok = np.isfinite(want)
    return float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
