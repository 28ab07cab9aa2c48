"""CPU statement of dfa_rigid_sums_cloud (one linearisation of the rigid pre-alignment of north-star mode)
and of Warpfield::composeRigid, in numpy.  Written from include/dynfu_amd.h, not from dynfu_amd/csrc/icp.hip.

Per vertex c with normal n0, float32 (dot() is csrc/device_math.hpp's: the two trailing products fused):
    s = R c + t                                       no row if c.x is NaN or s.z > 0 fails
    u = rint(fx * (s.x / s.z) + cx), w likewise       unfused, ties to even; no row outside [0, cols) x [0, rows)
    L, Ln = the float4 pixels of the two maps         no row if L.x or Ln.x is NaN
    sqrt(dot(s - L, s - L)) <= dist_thresh            and, with normals, dot(R n0, Ln) >= cos_thresh (signed)
    row = (s x Ln, Ln | dot(Ln, L - s))               the cross product unfused
The 27 products row_i row_j (img_statement.SUM_PAIRS) are formed in float32 and added in float64.  rigid_sums64() adds the
same sums with s, the row and the products in float64 over the vertices matched in float32 (that set and its pixels are the
contract), their rounding scale abs64 and the number of knife-edge vertices: those within KNIFE_ULPS float32 ulps of a pixel
boundary, of s.z = 0 or of a gate while still alive there.

compose_rigid() is T o dq in float64: real part r_T r, dual part r_T d + d_T r (quaternions (w, x, y, z))."""
import numpy as np

from img_statement import KNIFE_ULPS, SUM_PAIRS, _ulp, icp_update, per_sum_units  # noqa: F401  (re-exported)
from solve6_statement import pure, qmul
from tsdf_statement import dot

f32 = np.float32


def _terms(vertices, normals, aff12, vmap, nmap, intr, dist_thresh, cos_thresh):
    v = np.asarray(vertices, np.float32)
    N = v.shape[0]
    c = [v[:, k] for k in range(3)]
    a = np.asarray(aff12, np.float32).reshape(-1)
    R, t = a[:9].reshape(3, 3), a[9:12]
    fx, fy, cx, cy = (f32(x) for x in intr)
    vmap, nmap = np.asarray(vmap, np.float32), np.asarray(nmap, np.float32)
    H, W = vmap.shape[:2]
    dth, cth = f32(dist_thresh), f32(cos_thresh)
    with np.errstate(all="ignore"):
        s = [(dot(R[k], c) + t[k]).astype(np.float32) for k in range(3)]
        ok = ~np.isnan(c[0]) & (s[2] > 0)
        knife = ~np.isnan(c[0]) & (np.abs(s[2]) <= KNIFE_ULPS * _ulp(R[2, 0] * c[0], R[2, 1] * c[1], R[2, 2] * c[2], t[2]))
        qx, qy = (s[0] / s[2]).astype(np.float32), (s[1] / s[2]).astype(np.float32)
        uf = ((fx * qx).astype(np.float32) + cx).astype(np.float32)
        wf = ((fy * qy).astype(np.float32) + cy).astype(np.float32)
        u, w = np.rint(uf), np.rint(wf)
        # a pixel boundary: the unrounded coordinate at a half-integer (the image's edges are two of them)
        for coord, prod, cc in ((uf, fx * qx, cx), (wf, fy * qy, cy)):
            knife |= ok & np.isfinite(coord) & (np.abs(np.abs(coord - np.floor(coord)) - f32(0.5)) <= KNIFE_ULPS * _ulp(prod, cc))
        ok &= (u >= 0) & (w >= 0) & (u < f32(W)) & (w < f32(H))  # a NaN or an infinity is outside
        iu = np.where(ok, u, 0).astype(np.int64)
        iw = np.where(ok, w, 0).astype(np.int64)
        L4, Ln4 = vmap[iw, iu], nmap[iw, iu]
        ok &= ~np.isnan(L4[:, 0]) & ~np.isnan(Ln4[:, 0])
        L = [L4[:, k] for k in range(3)]
        Ln = [Ln4[:, k] for k in range(3)]
        sl = [s[k] - L[k] for k in range(3)]
        dist = np.sqrt(dot(sl, sl))
        knife |= ok & (np.abs(dist - dth) <= KNIFE_ULPS * _ulp(dist, dth))
        ok &= dist <= dth
        if normals is not None:
            n = np.asarray(normals, np.float32)
            n0 = [n[:, k] for k in range(3)]
            ns = [dot(R[k], n0) for k in range(3)]
            cosv = dot(ns, Ln)
            knife |= ok & (np.abs(cosv - cth) <= KNIFE_ULPS * _ulp(ns[0] * Ln[0], ns[1] * Ln[1], ns[2] * Ln[2], cth))
            ok &= cosv >= cth
        cross = [s[1] * Ln[2] - s[2] * Ln[1], s[2] * Ln[0] - s[0] * Ln[2], s[0] * Ln[1] - s[1] * Ln[0]]
        row = cross + Ln + [dot(Ln, [L[k] - s[k] for k in range(3)])]
    rows = np.zeros((N, 7), np.float32)
    for k in range(7):
        rows[:, k] = np.where(ok, row[k], f32(0))
    return dict(ok=ok, rows=rows, knife=knife, iu=iu, iw=iw, R=R, t=t, c=c, L=L, Ln=Ln)


def sums_of_rows(rows):
    """the 27 sums of float32 rows (N, 7): float32 products added in float64"""
    return np.array([np.sum((rows[:, i] * rows[:, j]).astype(np.float64)) for i, j in SUM_PAIRS], np.float64)


def rigid_sums(vertices, normals, aff12, vmap, nmap, intr, dist_thresh, cos_thresh):
    """-> (27 float64 sums of the float32 products, matched mask (N,), float32 rows (N, 7), zero where unmatched)"""
    T = _terms(vertices, normals, aff12, vmap, nmap, intr, dist_thresh, cos_thresh)
    return sums_of_rows(T["rows"]), T["ok"], T["rows"]


def rigid_sums64(vertices, normals, aff12, vmap, nmap, intr, dist_thresh, cos_thresh):
    """rigid_sums() plus the exact statement -> (sums, ok, rows, sum64, abs64, knife); see the module docstring"""
    T = _terms(vertices, normals, aff12, vmap, nmap, intr, dist_thresh, cos_thresh)
    ok = T["ok"]
    f8 = np.float64
    R, t = T["R"].astype(f8), T["t"].astype(f8)
    with np.errstate(all="ignore"):
        c = [x.astype(f8) for x in T["c"]]
        s = [R[k, 0] * c[0] + R[k, 1] * c[1] + R[k, 2] * c[2] + t[k] for k in range(3)]
        L = [x.astype(f8) for x in T["L"]]
        n = [x.astype(f8) for x in T["Ln"]]
        row = [s[1] * n[2] - s[2] * n[1], s[2] * n[0] - s[0] * n[2], s[0] * n[1] - s[1] * n[0], n[0], n[1], n[2],
               n[0] * (L[0] - s[0]) + n[1] * (L[1] - s[1]) + n[2] * (L[2] - s[2])]
        row = [r[ok] for r in row]
        sum64 = np.array([np.sum(row[i] * row[j]) for i, j in SUM_PAIRS], f8)
        abs64 = np.array([np.sum(np.abs(row[i] * row[j])) for i, j in SUM_PAIRS], f8)
    return sums_of_rows(T["rows"]), ok, T["rows"], sum64, abs64, int(T["knife"].sum())


# ------------------------------------------------------------------------------------------------ composeRigid ----
def quat_of(R):
    """unit quaternion (w, x, y, z) of a rotation matrix, float64 (the branch with the largest pivot)"""
    R = np.asarray(R, np.float64)
    cand = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                     1 - R[0, 0] - R[1, 1] + R[2, 2]])
    i = int(cand.argmax())
    h = 0.5 * np.sqrt(cand[i])
    if i == 0:
        q = [h, (R[2, 1] - R[1, 2]) / (4 * h), (R[0, 2] - R[2, 0]) / (4 * h), (R[1, 0] - R[0, 1]) / (4 * h)]
    elif i == 1:
        q = [(R[2, 1] - R[1, 2]) / (4 * h), h, (R[0, 1] + R[1, 0]) / (4 * h), (R[0, 2] + R[2, 0]) / (4 * h)]
    elif i == 2:
        q = [(R[0, 2] - R[2, 0]) / (4 * h), (R[0, 1] + R[1, 0]) / (4 * h), h, (R[1, 2] + R[2, 1]) / (4 * h)]
    else:
        q = [(R[1, 0] - R[0, 1]) / (4 * h), (R[0, 2] + R[2, 0]) / (4 * h), (R[1, 2] + R[2, 1]) / (4 * h), h]
    q = np.array(q)
    return q / np.linalg.norm(q)


def dq_of(aff12):
    """(r_T, d_T) of 12 numbers (R row-major, then t): d_T = 1/2 t^ r_T"""
    a = np.asarray(aff12, np.float64).reshape(-1)
    r = quat_of(a[:9].reshape(3, 3))
    return r, 0.5 * qmul(pure(a[9:12]), r)


def compose_rigid(dq, aff12):
    """T o dq_i for every row of dq (D, 8), float64: real part r_T r, dual part r_T d + d_T r"""
    dq = np.asarray(dq, np.float64)
    rT, dT = dq_of(aff12)
    r, d = dq[:, :4], dq[:, 4:]
    return np.concatenate([qmul(rT, r), qmul(rT, d) + qmul(dT, r)], 1)


def blend_points(dq, idx, wn, c, dtype=np.float64):
    """the north-star blend (csrc/blend6_device.hpp) of points c (N, 3): a = sum w~ s r, b = sum w~ s d over the k nodes
    idx (N, k) with normalised weights wn, s the sign of r . r_0 against the first; p = (vec(a c a*) + 2 vec(b a*)) / |a|^2.
    dtype: the arithmetic (float32: every operation rounded to float32, in numpy's order)"""
    sgn = np.array([1, -1, -1, -1], dtype)
    q = np.asarray(dq, dtype)[idx]
    s = np.where((q[..., :4] * q[:, :1, :4]).sum(-1) < 0, dtype(-1), dtype(1))
    f = np.asarray(wn, dtype) * s
    a, b = (f[..., None] * q[..., :4]).sum(1), (f[..., None] * q[..., 4:]).sum(1)
    m = (a * a).sum(1)
    c = np.asarray(c, dtype)
    cq = np.concatenate([np.zeros((len(c), 1), dtype), c], 1)
    p = (qmul(qmul(a, cq), a * sgn)[:, 1:] + dtype(2) * qmul(b, a * sgn)[:, 1:]) / m[:, None]
    assert p.dtype == dtype
    return p


def apply_rigid(aff12, p):
    """R p + t of 12 numbers at points (N, 3), float64"""
    a = np.asarray(aff12, np.float64).reshape(-1)
    return np.asarray(p, np.float64) @ a[:9].reshape(3, 3).T + a[9:12]
