"""CPU statement of dfa_tsdf_integrate_warped6 in numpy: one depth frame integrated into a volume through the north-star
(6-DoF) warp field, whose nodes live in a frame of their own.

Built on warp_statement (knn, weights64) and tsdf_warped_statement (voxel_positions, support_quotients, probe, update,
tsdf_tolerance).  Per voxel, in the numbering of include/dynfu_amd.h:
  1. v = (x, y, z) * voxel_size, float32 products (exact by contract);
  2. c = R_n v + t_n.  The search and the support rule are exact statements over float32 inputs, so they are made at the
     float32 c the header's expression gives (c32: the fused dot of the rigid integrate, then + t) — the blend below takes
     the fp64 product c64;
  3. the k nearest nodes of c32 (warp_statement.knn) and the support quotient there (support_quotients);
  4. unsupported: left alone (SKIP) or p = c (RIGID);
  5. supported, in fp64: the weights of warp_statement.weights64 at c32 divided by their sum, the zero pattern of their float32
     rounding (as solve6_statement.rbf); the sign of every active transform against the first active one; a = sum w~ s r,
     b = sum w~ s d; p = (vec(a c64 a*) + 2 vec(b a*)) / |a|^2 when |a|^2 > 0, else c64;
  6. vc64 = R_c p + t_c.
Step 7 is tsdf_warped_statement's (probe, update) at vc64 rounded to float32 once.

DECIDED voxels follow tsdf_warped_statement's rule — every decision the same at the 27 points vc64 + rho s, support quotient
not within 1e-6 of 1 — with one addition: a supported voxel with a hemisphere dot product within 1e-4 of 0 is undecided
(solve6_statement's ambiguity rule: float32 may take the other sign).

rho is measured, not chosen: camera_points(with32=True) evaluates steps 1-6 in numpy float32 as well (apply32, blend32: operation
by operation in the order of csrc/blend6_device.hpp), and WARPED6_DEVIATION is the largest |vc32 - vc64| / L over all the cases of
tests/tsdf_warped6_cases.py, L = max(1, largest |coordinate| in the volume, node or camera frame).  rho = 2 WARPED6_DEVIATION L:
the factor 2 is the project's margin for a second libm and another instruction order (warp_statement.KERNEL_BOUND = 2
ORACLE_DEVIATION).  tests/test_tsdf_warped6_statement_cpu.py measures it again on every run.
"""
import numpy as np

import tsdf_statement as TS
import tsdf_warped_statement as WST
import warp_statement as WS

f32 = np.float32
SKIP, RIGID = WST.SKIP, WST.RIGID
HEMI_MARGIN = 1e-4

# largest |vc32 - vc64| / L over every case of tsdf_warped6_cases.CASES, measured on the CPU
WARPED6_DEVIATION = 3.5e-7  # measured 3.481e-07, at the case odd_scan_moved (the blend alone, "volume" frames: 2.5e-07)


def _rt64(aff12):
    a = np.asarray(aff12, np.float32).reshape(-1).astype(np.float64)
    return a[:9].reshape(3, 3), a[9:12]


def apply32(aff12, pts):
    """mulR(A, p) + t as the kernels write it (tsdf_statement.mat: the fused dot), float32 (n, 3); pts itself for None"""
    pts = np.asarray(pts, np.float32)
    if aff12 is None:
        return pts
    R, t = TS._rt(aff12)
    r = TS.mat(R, [pts[:, 0], pts[:, 1], pts[:, 2]])
    return np.stack([r[i] + t[i] for i in range(3)], 1).astype(np.float32)


def apply64(aff12, pts):
    pts = np.asarray(pts, np.float64)
    if aff12 is None:
        return pts
    R, t = _rt64(aff12)
    return pts @ R.T + t


def compose(b, a):
    """b after a (12 floats each), fp64 product rounded to float32"""
    Ra, ta = _rt64(a)
    Rb, tb = _rt64(b)
    return np.concatenate([(Rb @ Ra).reshape(-1), Rb @ ta + tb]).astype(np.float32)


def invert(a):
    """the inverse of a rigid transform (12 floats), fp64, rounded to float32"""
    R, t = _rt64(a)
    return np.concatenate([R.T.reshape(-1), -R.T @ t]).astype(np.float32)


# ------------------------------------------------------------------------------------------ the blend, fp64
def _qmul(a, b):
    return WS.qmul(a, b)


def _conj(a):
    return a * np.array([1.0, -1.0, -1.0, -1.0])


def _pure(v):
    return np.concatenate([np.zeros(v.shape[:-1] + (1,)), v], -1)


def blend64(node_dq, idx, w64, c64):
    """step 5 for points with neighbour lists idx (n, k) and raw fp64 weights w64: (p (n, 3) fp64, hemisphere-ambiguous (n,))"""
    dq = np.asarray(node_dq, np.float32).reshape(-1, 8).astype(np.float64)
    n = len(idx)
    nz = (idx >= 0) & (w64.astype(np.float32) > 0)
    wsum = w64.sum(1)
    wn = np.where(nz, w64 / np.where(wsum > 0, wsum, 1.0)[:, None], 0.0)
    q = dq[np.maximum(idx, 0)]  # (n, k, 8)
    first = np.where(nz.any(1), nz.argmax(1), 0)
    r0 = q[np.arange(n), first, :4]
    dots = (q[..., :4] * r0[:, None, :]).sum(-1)
    s = np.where(dots < 0, -1.0, 1.0)
    amb = (nz & (np.abs(dots) < HEMI_MARGIN)).any(1)
    f = wn * s
    a = (f[..., None] * q[..., :4]).sum(1)
    b = (f[..., None] * q[..., 4:]).sum(1)
    m = (a * a).sum(1)
    ok = nz.any(1) & (m > 0)
    ms = np.where(ok, m, 1.0)
    p = (_qmul(_qmul(a, _pure(c64)), _conj(a))[:, 1:] + 2.0 * _qmul(b, _conj(a))[:, 1:]) / ms[:, None]
    return np.where(ok[:, None], p, c64), amb


# ------------------------------------------------------------------------------------------ the blend, float32 op by op
def _qmul32(a, b):
    """dq_device.hpp qmul: every product and every sum rounded, left to right"""
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _qdot32(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2] + a[..., 3] * b[..., 3]


def blend32(node_dq, idx, w32, c32, k):
    """the row normalisation, blend and blend_point of csrc/blend6_device.hpp in numpy float32: p (n, 3) float32"""
    dq = np.asarray(node_dq, np.float32).reshape(-1, 8)
    n, kk = idx.shape
    w32 = np.asarray(w32, np.float32)
    total = np.zeros(n, np.float32)
    for j in range(min(k, kk)):
        total = total + w32[:, j]
    with np.errstate(all="ignore"):
        wn = np.where((total > 0)[:, None], w32 / np.where(total > 0, total, f32(1))[:, None], f32(0)).astype(np.float32)
    a = np.zeros((n, 4), np.float32)
    b = np.zeros((n, 4), np.float32)
    r0 = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    have = np.zeros(n, bool)
    for j in range(min(k, kk)):
        on = (idx[:, j] >= 0) & (wn[:, j] != 0)
        q = dq[np.maximum(idx[:, j], 0)]
        take = on & ~have
        r0 = np.where(take[:, None], q[:, :4], r0)
        have |= on
        sg = np.where(_qdot32(q[:, :4], r0) < 0, f32(-1), f32(1)).astype(np.float32)
        w = (wn[:, j] * sg).astype(np.float32)
        a = np.where(on[:, None], a + q[:, :4] * w[:, None], a)
        b = np.where(on[:, None], b + q[:, 4:] * w[:, None], b)
    m = _qdot32(a, a)
    ac = a * np.array([1, -1, -1, -1], np.float32)
    cq = np.concatenate([np.zeros((n, 1), np.float32), c32], 1)
    u = _qmul32(_qmul32(a, cq), ac)[:, 1:]
    t = _qmul32(b, ac)[:, 1:]
    with np.errstate(all="ignore"):
        im = f32(1) / m
        p = ((u + f32(2) * t) * im[:, None]).astype(np.float32)
    return np.where((m > 0)[:, None], p, c32)


# ------------------------------------------------------------------------------------------ steps 1-6
def camera_points(shape, voxel_size, vol2node, node2cam, nodes, node_dq, node_w, k, mode, with32=False):
    """steps 1-6.  dict: v, c32 (n, 3) float32; supported, active, hemi (n,) bool; qmin (n,) float32; vc64 (n, 3) fp64; with32:
    vc32 (n, 3), the float32 evaluation"""
    v = WST.voxel_positions(shape, voxel_size)
    n = len(v)
    nodes = np.zeros((0, 3), np.float32) if nodes is None else np.asarray(nodes, np.float32).reshape(-1, 3)
    c32 = apply32(vol2node, v)
    c64 = apply64(vol2node, v.astype(np.float64))
    supported = np.zeros(n, bool)
    hemi = np.zeros(n, bool)
    qmin = np.full(n, np.inf, np.float32)
    p = c64.copy()
    p32 = c32.copy()
    if len(nodes):
        idx = WS.knn(nodes, c32, k)
        qmin = WST.support_quotients(nodes, node_w, idx, c32)
        supported = qmin < f32(1)
        if supported.any():
            s = np.flatnonzero(supported)
            w64 = WS.weights64(nodes, node_w, c32[s], idx[s])
            p[s], hemi[s] = blend64(node_dq, idx[s], w64, c64[s])
            if with32:
                p32[s] = blend32(node_dq, idx[s], w64.astype(np.float32), c32[s], k)
    active = supported | (mode == RIGID)
    out = dict(v=v, c32=c32, supported=supported, active=active, hemi=hemi, qmin=qmin, vc64=apply64(node2cam, p))
    if with32:
        out["vc32"] = apply32(node2cam, p32)
    return out


def frame_scale(c):
    """L: max(1, largest |coordinate| of a voxel in the volume frame, in the node frame, of an active voxel in the camera frame)"""
    act = c["active"]
    return max(1.0, float(np.abs(c["v"]).max()), float(np.abs(c["c32"]).max()), float(np.abs(c["vc64"][act]).max()) if act.any() else 0.0)


def deviation(shape, voxel_size, vol2node, node2cam, nodes, node_dq, node_w, k, mode):
    """largest |vc32 - vc64| / L over the active voxels of one call"""
    c = camera_points(shape, voxel_size, vol2node, node2cam, nodes, node_dq, node_w, k, mode, with32=True)
    act = c["active"]
    if not act.any():
        return 0.0
    return float(np.abs(c["vc32"][act].astype(np.float64) - c["vc64"][act]).max()) / frame_scale(c)


def integrate(vol, dists, voxel_size, trunc, max_weight, vol2node, node2cam, fx, fy, cx, cy, nodes, node_dq, node_w, k, mode):
    """The call on vol (uint32 (Z, Y, X)).  dict: vol, updated, decided, supported (bool (Z, Y, X)), tsdf (float32 (Z, Y, X)),
    qmin (float32 (Z, Y, X)), rho, L."""
    vol = np.array(vol, np.uint32)
    shape = vol.shape
    c = camera_points(shape, voxel_size, vol2node, node2cam, nodes, node_dq, node_w, k, mode)
    act, vc64 = c["active"], c["vc64"]
    L = frame_scale(c)
    rho = 2 * WARPED6_DEVIATION * L
    n = len(act)
    upd, px, py, tsdf = np.zeros(n, bool), np.full(n, -1), np.full(n, -1), np.full(n, np.nan, np.float32)
    decided = (np.abs(c["qmin"].astype(np.float64) - 1.0) > WST.Q_MARGIN) & ~c["hemi"]
    if act.any():
        a = np.flatnonzero(act)
        u0, x0, y0, t0 = WST.probe(vc64[a].astype(np.float32), dists, trunc, fx, fy, cx, cy)
        upd[a], px[a], py[a], tsdf[a] = u0, x0, y0, t0
        same = np.ones(len(a), bool)
        for s in np.ndindex(3, 3, 3):
            if s == (1, 1, 1):
                continue
            u, x, y, t = WST.probe((vc64[a] + rho * (np.array(s, np.float64) - 1)).astype(np.float32), dists, trunc, fx, fy, cx, cy)
            same &= (u == u0) & (x == x0) & (y == y0) & ((t == 1) == (t0 == 1))
        decided[a] &= same
    flat = vol.reshape(-1)
    if upd.any():
        flat[upd] = WST.update(flat[upd], tsdf[upd], max_weight)
    r = lambda m: m.reshape(shape)
    return dict(vol=vol, updated=r(upd), decided=r(decided), supported=r(c["supported"]), tsdf=r(tsdf), qmin=r(c["qmin"]), rho=rho, L=L)
