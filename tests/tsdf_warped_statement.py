"""CPU statement of dfa_tsdf_integrate_warped in numpy: one depth frame integrated into a volume through the warp field.

Steps 1-6 (voxel position, neighbours, support, blend, camera frame) are stated in fp64 on top of warp_statement — knn and
unsupported_flags are exact statements, warp_graph is the mathematical blend — and the camera-frame point is rounded to
float32 once.  Step 7 is the reference's integrate (src/kfusion/cuda/tsdf_volume.cu:65-91) per voxel in float32, after
tsdf_statement.integrate.

A float32 kernel cannot reproduce an fp64 warp bit for bit, and the update of a voxel is a chain of decisions (inside the
image? which texel? zero? behind the surface? clamped to 1?) that an ulp can flip.  So the statement also says which
voxels are DECIDED: those whose every decision is the same at all 27 points vc64 + rho * s, s in {-1, 0, 1}^3, and whose
support quotient is not within 1e-6 of 1.  rho = 2 * warp_statement.KERNEL_BOUND * L with L = max(1, largest |coordinate|
of a voxel or of a supported vc): KERNEL_BOUND is the project's bound of the float32 warp against fp64 at coordinates of
order 1, L scales it, and the factor 2 covers the vol2cam product (at most 4 ulp of L, about 5e-7 L).  On decided voxels a
kernel must agree with the statement exactly in the update set and the weights, and within tsdf_tolerance() in the
distance; an undecided voxel holds its input or a valid update.
"""
import numpy as np

import warp_statement as WS
from extract_statement import fma32, pack, unpack
from tsdf_statement import dot

f32 = np.float32
SKIP, RIGID = 0, 1  # DFA_WARPED_SKIP, DFA_WARPED_RIGID
Q_MARGIN = 1e-6


def voxel_positions(shape, voxel_size):
    """step 1: v = (x vsx, y vsy, z vsz), float32 products, for a (Z, Y, X) volume in memory order — (n, 3) float32"""
    Z, Y, X = shape
    vs = np.asarray(voxel_size, np.float32)
    z, y, x = np.meshgrid(np.arange(Z, dtype=np.float32), np.arange(Y, dtype=np.float32), np.arange(X, dtype=np.float32),
                          indexing="ij")
    return np.stack([(x * vs[0]).ravel(), (y * vs[1]).ravel(), (z * vs[2]).ravel()], 1).astype(np.float32)


def support_quotients(nodes, node_w, idx, pts):
    """min over the neighbours idx of |v - g| / w, the arithmetic of warp_statement.unsupported_flags; inf without one"""
    nodes = np.asarray(nodes, np.float32).reshape(-1, 3)
    j = np.maximum(idx, 0)
    with np.errstate(all="ignore"):
        d = (pts[:, None, :] - nodes[j]).astype(np.float64)
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(np.float32)
        q = dist / np.asarray(node_w, np.float32)[j]
    return np.where((idx >= 0) & ~np.isnan(q), q, f32(np.inf)).min(axis=1)


def camera_points(shape, voxel_size, vol2cam, nodes, node_dq, node_w, k, mode):
    """steps 1-6 in fp64.  dict: v (n, 3) float32; supported, active (n,) bool; qmin (n,) float32; vc64 (n, 3)"""
    v = voxel_positions(shape, voxel_size)
    n = len(v)
    nodes = np.zeros((0, 3), np.float32) if nodes is None else np.asarray(nodes, np.float32).reshape(-1, 3)
    supported = np.zeros(n, bool)
    qmin = np.full(n, np.inf, np.float32)
    p = v.astype(np.float64)
    if len(nodes):
        idx = WS.knn(nodes, v, k)  # step 2
        # step 3: warp_statement.unsupported_flags' rule with the quotient kept (the decided set needs it) and the search
        # shared — tests/test_tsdf_warped_statement_cpu.py holds the two against each other on every case
        qmin = support_quotients(nodes, node_w, idx, v)
        supported = qmin < f32(1)
        if supported.any():  # step 5
            p[supported] = WS.warp_graph(nodes, node_dq, node_w, idx[supported], v[supported])[0]
    active = supported | (mode == RIGID)  # step 4
    a = np.asarray(vol2cam, np.float32).reshape(-1).astype(np.float64)
    vc64 = p @ a[:9].reshape(3, 3).T + a[9:12]  # step 6
    return dict(v=v, supported=supported, active=active, qmin=qmin, vc64=vc64)


def probe(vc, dists, trunc, fx, fy, cx, cy):
    """step 7, first half (tsdf_volume.cu:65-80, tsdf_statement.integrate :99-111) at camera-frame points vc (n, 3) float32:
    (updated (n,) bool, px, py (n,) int64 — -1 where nothing is fetched —, tsdf (n,) float32, NaN where not updated)"""
    vc = [np.asarray(vc, np.float32)[:, c] for c in range(3)]
    dists = np.asarray(dists, np.uint16)
    rows, cols = dists.shape
    Dtex = dists.view(np.float16).astype(np.float32)
    trunc = f32(trunc)
    inv_trunc = f32(1) / trunc
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    with np.errstate(divide="ignore", invalid="ignore"):
        coox = fma32(fx, vc[0] / vc[2], cx)
        cooy = fma32(fy, vc[1] / vc[2], cy)
    out = (coox < 0) | (cooy < 0) | (coox >= f32(cols)) | (cooy >= f32(rows))
    fetch = ~out & np.isfinite(coox) & np.isfinite(cooy)
    px = np.where(fetch, np.floor(np.where(fetch, coox, 0)), -1).astype(np.int64)
    py = np.where(fetch, np.floor(np.where(fetch, cooy, 0)), -1).astype(np.int64)
    Dp = np.where(fetch, Dtex[np.maximum(py, 0), np.maximum(px, 0)], f32(0))
    skip = out | ~fetch | (Dp == 0) | (vc[2] <= 0)
    with np.errstate(invalid="ignore"):
        sdf = Dp - np.sqrt(dot(vc, vc))
        upd = ~skip & (sdf >= -trunc)
        tsdf = np.where(upd, np.fmin(f32(1), sdf * inv_trunc), f32(np.nan)).astype(np.float32)
    return upd, px, py, tsdf


def update(old, tsdf, max_weight):
    """step 7, second half (:82-90, tsdf_statement.integrate :112-116): the packed voxels after the running average"""
    F, W = unpack(old)
    Wf = W.astype(np.float32)
    new = fma32(F, Wf, tsdf) / (Wf + f32(1))
    return pack(new, np.minimum(W.astype(np.int64) + 1, int(max_weight)))


def integrate(vol, dists, voxel_size, trunc, max_weight, vol2cam, fx, fy, cx, cy, nodes, node_dq, node_w, k, mode):
    """The call on vol (uint32 (Z, Y, X)).  dict: vol (the new volume), updated, decided, supported (bool (Z, Y, X)),
    tsdf (float32 (Z, Y, X): this frame's distance of the updated voxels), rho, L."""
    vol = np.array(vol, np.uint32)
    shape = vol.shape
    c = camera_points(shape, voxel_size, vol2cam, nodes, node_dq, node_w, k, mode)
    act = c["active"]
    vc64 = c["vc64"]
    L = max(1.0, float(np.abs(c["v"]).max()), float(np.abs(vc64[c["supported"]]).max()) if c["supported"].any() else 0.0)
    rho = 2 * WS.KERNEL_BOUND * L
    upd, px, py, tsdf = (np.zeros(len(act), bool), np.full(len(act), -1), np.full(len(act), -1),
                         np.full(len(act), np.nan, np.float32))
    decided = np.abs(c["qmin"].astype(np.float64) - 1.0) > Q_MARGIN
    if act.any():
        a = np.flatnonzero(act)
        u0, x0, y0, t0 = probe(vc64[a].astype(np.float32), dists, trunc, fx, fy, cx, cy)
        upd[a], px[a], py[a], tsdf[a] = u0, x0, y0, t0
        same = np.ones(len(a), bool)
        for s in np.ndindex(3, 3, 3):
            if s == (1, 1, 1):
                continue
            u, x, y, t = probe((vc64[a] + rho * (np.array(s, np.float64) - 1)).astype(np.float32), dists, trunc, fx, fy, cx, cy)
            same &= (u == u0) & (x == x0) & (y == y0) & ((t == 1) == (t0 == 1))
        decided[a] &= same
    flat = vol.reshape(-1)
    if upd.any():
        flat[upd] = update(flat[upd], tsdf[upd], max_weight)
    r = lambda m: m.reshape(shape)
    return dict(vol=vol, updated=r(upd), decided=r(decided), supported=r(c["supported"]), tsdf=r(tsdf), rho=rho, L=L)


def tsdf_tolerance(rho, trunc):
    """of the unpacked distance on a decided voxel: rho sqrt(3) / trunc is the shift of sdf / trunc under a displacement
    of rho per axis, 2^-11 one fp16 step at |tsdf| <= 1"""
    return rho * np.sqrt(3.0) / float(trunc) + 2.0 ** -11
