"""CPU statement of the TSDF half of the hot path in numpy float32: compute_dists, clear, integrate, both raycasts and
the raycaster's normals.

It is a second reading of the reference's sources, written from them and not from oracle/tsdf_oracle.c:
src/kfusion/cuda/imgproc.cu:233-254 (compute_dists), src/kfusion/cuda/tsdf_volume.cu:11-121 (clear, integrate) and
:128-386 (raycast), with the helpers of include/kfusion/cuda/device.hpp (Projector :40-45, Reprojector :50-54, pack /
unpack :59-67, Mat3f * v and Aff3f * v :74-78) and temp_utils.hpp (normalized :91, quiet NaN = 0x7fffffff :21).
tests/test_tsdf_statement_cpu.py checks it on hand-made inputs and against the oracle; the -m gpu tests compare the
HIP kernels with it directly.

Arithmetic convention (the one oracle/oracle.h documents):
  - every operation is a float32 operation in the source's order, round-to-nearest-even, subnormals kept;
  - a multiply-add is fused (fma32, one rounding) only where the source writes __fmaf_rn (the Projector, integrate's
    running average) and where the project contracts nvcc's a*b + c: dot() = fma(z, z', fma(y, y', x * x')),
    compute_dists' xl*xl + yl*yl and interpolate's `tsdf += u * wa * wb * wc`.  Every other product and sum is rounded
    on its own (nvcc is free to contract more of them; the project does not);
  - the approximate intrinsics are the correctly rounded operation they stand for: __fdividef -> `/`, __fsqrt_rn and
    sqrtf -> sqrt, rsqrt(v) -> 1 / sqrt(v) (two roundings);
  - __float2half_rn is round-to-nearest-even (numpy's float32 -> float16), __float2int_rn round-half-even, the
    point-sampled texture fetch the texel floor(coordinate), static_cast<ushort>(float) truncates and saturates.

Raycast bounds: fetch_tsdf (tsdf_volume.cu:187-193) reads the nearest voxel with no bounds check; the source relies on
the ray staying inside [0, size - voxel] (:210-213).  Here a fetch outside the volume raises RayLeftVolume instead of
reading anything, so that every test of the statement also tests that claim.
"""
import numpy as np

from extract_statement import fma32, pack, unpack

f32 = np.float32
QNAN = np.array(0x7FFFFFFF, np.uint32).view(np.float32)[()]  # numeric_limits<float>::quiet_NaN()


class RayLeftVolume(AssertionError):
    """fetch_tsdf was asked for a voxel outside the volume"""


def dot(a, b):
    """temp_utils dot(): a.x*b.x + a.y*b.y + a.z*b.z with the two trailing products fused"""
    return fma32(a[2], b[2], fma32(a[1], b[1], f32(a[0]) * f32(b[0])))


def mat(R, v):
    """device.hpp:74-76: the rows of R (3x3) dotted with v (3 arrays)"""
    return [dot(R[i], v) for i in range(3)]


def _rt(aff12):
    a = np.asarray(aff12, np.float32).reshape(-1)
    return a[:9].reshape(3, 3), a[9:12]


def normalized(v):
    """temp_utils.hpp:91 v * rsqrt(dot(v, v)), rsqrt as 1 / sqrt"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f32(1) / np.sqrt(dot(v, v))
        return [(v[k] * inv).astype(np.float32) for k in range(3)]


# ------------------------------------------------------------------------------------------- compute_dists, clear --
def compute_dists(depth, fx, fy, cx, cy):
    """imgproc.cu:233-254: dists = half(depth * lambda * 0.001), lambda = |(x - cx) / fx, (y - cy) / fy, 1|; the host
    passes finv = 1 / f (:252).  The kernel's guard `x < cols || y < rows` (:237) is read as the in-image test."""
    depth = np.asarray(depth, np.uint16)
    rows, cols = depth.shape
    finvx, finvy = f32(1) / f32(fx), f32(1) / f32(fy)
    xl = ((np.arange(cols, dtype=np.float32) - f32(cx)) * finvx)[None, :]
    yl = ((np.arange(rows, dtype=np.float32) - f32(cy)) * finvy)[:, None]
    lam = np.sqrt(fma32(yl, yl, xl * xl) + f32(1))
    m = (depth.astype(np.float32) * lam) * f32(0.001)
    return m.astype(np.float16).view(np.uint16)


def clear(shape):
    """tsdf_volume.cu:11-22: every voxel pack_tsdf(0.f, 0) = 0"""
    return np.zeros(shape, np.uint32)


# ------------------------------------------------------------------------------------------------------ integrate --
def integrate(vol, dists, voxel_size, trunc, max_weight, vol2cam, fx, fy, cx, cy):
    """tsdf_volume.cu:43-121 on vol (uint32, (Z, Y, X)); returns the new volume.  Vectorised over (y, x), one pass per
    slice; vc is accumulated slice by slice (:64 vc += zstep), also over skipped voxels."""
    vol = np.array(vol, np.uint32)
    Z, Y, X = vol.shape
    dists = np.asarray(dists, np.uint16)
    rows, cols = dists.shape
    vs = np.asarray(voxel_size, np.float32)
    R, t = _rt(vol2cam)
    trunc = f32(trunc)
    inv_trunc = f32(1) / trunc  # :106
    zstep = [R[k, 2] * vs[2] for k in range(3)]  # :58 third column of R times voxel_size.z
    yy, xx = np.meshgrid(np.arange(Y, dtype=np.float32), np.arange(X, dtype=np.float32), indexing="ij")
    vx = [xx * vs[0], yy * vs[1], np.zeros_like(xx)]  # :60
    vc = [(c + t[k]).astype(np.float32) for k, c in enumerate(mat(R, vx))]  # :61 vol2cam * vx = R vx + t
    Dtex = dists.view(np.float16).astype(np.float32)
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    for z in range(Z):
        with np.errstate(divide="ignore", invalid="ignore"):
            coox = fma32(fx, vc[0] / vc[2], cx)  # Projector, device.hpp:40-45
            cooy = fma32(fy, vc[1] / vc[2], cy)
        out = (coox < 0) | (cooy < 0) | (coox >= f32(cols)) | (cooy >= f32(rows))  # :70
        fetch = ~out & np.isfinite(coox) & np.isfinite(cooy)
        px = np.where(fetch, np.floor(np.where(fetch, coox, 0)), 0).astype(np.int64)  # :73 point sampling: the texel
        py = np.where(fetch, np.floor(np.where(fetch, cooy, 0)), 0).astype(np.int64)  # the coordinate lies in
        Dp = np.where(fetch, Dtex[py, px], f32(0))
        skip = out | (Dp == 0) | (vc[2] <= 0)  # :74 (a NaN coordinate comes only with vc.z == 0)
        with np.errstate(invalid="ignore"):
            sdf = Dp - np.sqrt(dot(vc, vc))  # :77
            upd = ~skip & (sdf >= -trunc)  # :79
        if upd.any():
            tsdf = np.fmin(f32(1), sdf[upd] * inv_trunc)  # :80
            F, W = unpack(vol[z][upd])  # :83-84
            Wf = W.astype(np.float32)
            new = fma32(F, Wf, tsdf) / (Wf + f32(1))  # :86
            Wn = np.minimum(W.astype(np.int64) + 1, int(max_weight))  # :87
            vol[z][upd] = pack(new, Wn)  # :90
        vc = [(vc[k] + zstep[k]).astype(np.float32) for k in range(3)]  # :64
    return vol


# -------------------------------------------------------------------------------------------------------- raycast --
def interpolate(vol, cf):
    """tsdf_volume.cu:146-171: trilinear interpolation at voxel coordinates cf (3 arrays); NaN where floor(cf) leaves
    [0, dim - 2] on any axis"""
    Z, Y, X = vol.shape
    dims = (X, Y, Z)
    with np.errstate(invalid="ignore"):
        g = [np.floor(cf[k]) for k in range(3)]  # __float2int_rd
        inside = np.ones(np.shape(cf[0]), bool)
        for k in range(3):
            inside &= (g[k] >= 0) & (g[k] < dims[k] - 1)  # :153-155
    gi = [np.where(inside, g[k], 0).astype(np.int64) for k in range(3)]
    a, b, c = ((cf[k] - gi[k].astype(np.float32)).astype(np.float32) for k in range(3))
    one = f32(1)

    def u(dx, dy, dz):
        return unpack(vol[gi[2] + dz, gi[1] + dy, gi[0] + dx])[0]

    with np.errstate(invalid="ignore", over="ignore"):
        t = np.zeros(np.shape(a), np.float32)
        t = fma32((u(0, 0, 0) * (one - a)) * (one - b), one - c, t)  # :162-169
        t = fma32((u(0, 0, 1) * (one - a)) * (one - b), c, t)
        t = fma32((u(0, 1, 0) * (one - a)) * b, one - c, t)
        t = fma32((u(0, 1, 1) * (one - a)) * b, c, t)
        t = fma32((u(1, 0, 0) * a) * (one - b), one - c, t)
        t = fma32((u(1, 0, 1) * a) * (one - b), c, t)
        t = fma32((u(1, 1, 0) * a) * b, one - c, t)
        t = fma32((u(1, 1, 1) * a) * b, c, t)
    return np.where(inside, t, QNAN).astype(np.float32)


def compute_normal(vol, voxel_size, delta_factor, p):
    """tsdf_volume.cu:320-336 at points p (3 arrays, volume metric frame); gradient_delta = voxel * factor (:361)"""
    vs = np.asarray(voxel_size, np.float32)
    vinv = f32(1) / vs  # :362
    gd = vs * f32(delta_factor)
    n = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(3):
            hi = [(p[j] + gd[k] if j == k else p[j]) for j in range(3)]
            lo = [(p[j] - gd[k] if j == k else p[j]) for j in range(3)]
            F1 = interpolate(vol, [(hi[j] * vinv[j]).astype(np.float32) for j in range(3)])
            F2 = interpolate(vol, [(lo[j] * vinv[j]).astype(np.float32) for j in range(3)])
            n.append(((F1 - F2) / gd[k]).astype(np.float32))
    return normalized(n)


def vertex_normals(vol, voxel_size, delta_factor, points):
    """compute_normal of (n, 4) points -> (n, 4) {nx, ny, nz, 0}"""
    pts = np.asarray(points, np.float32).reshape(-1, 4)
    n = compute_normal(np.asarray(vol, np.uint32), voxel_size, delta_factor, [pts[:, k] for k in range(3)])
    out = np.zeros_like(pts)
    for k in range(3):
        out[:, k] = n[k]
    return out


def intersect(org, d, box_max):
    """tsdf_volume.cu:128-144 (box_min = 0; tmin.x / tmax.x enter both outer max / min)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = [f32(1) / d[k] for k in range(3)]
        tbot = [inv[k] * (f32(0) - org[k]) for k in range(3)]
        ttop = [inv[k] * (box_max[k] - org[k]) for k in range(3)]
    tmin = [np.fmin(ttop[k], tbot[k]) for k in range(3)]
    tmax = [np.fmax(ttop[k], tbot[k]) for k in range(3)]
    tnear = np.fmax(np.fmax(tmin[0], tmin[1]), np.fmax(tmin[0], tmin[2]))
    tfar = np.fmin(np.fmin(tmax[0], tmax[1]), np.fmin(tmax[0], tmax[2]))
    return tnear.astype(np.float32), tfar.astype(np.float32)


def _fetch(vol, vinv, p, live):
    """fetch_tsdf (:187-193) for the rays in `live`; raises RayLeftVolume if one of them leaves the volume"""
    Z, Y, X = vol.shape
    idx = []
    for k, dim in enumerate((X, Y, Z)):
        i = np.rint(np.where(live, p[k] * vinv[k], f32(0)))  # __float2int_rn, round half to even
        bad = live & ~((i >= 0) & (i <= dim - 1))
        if bad.any():
            j = int(np.flatnonzero(bad)[0])
            raise RayLeftVolume("ray %d fetches index %r on axis %d of a volume of %d" % (j, float(i[j]), k, dim))
        idx.append(i.astype(np.int64))
    return unpack(vol[idx[2], idx[1], idx[0]])[0]


def raycast(vol, voxel_size, trunc, cam2vol, Rinv, fx, fy, cx, cy, step_factor, delta_factor, cols, rows):
    """The shared body of the two raycast operators (tsdf_volume.cu:195-318) over the rows x cols rays.  Returns
    (hit mask, vertex (3 arrays, camera frame), normal (3 arrays, camera frame)) of shape (rows, cols)."""
    vol = np.asarray(vol, np.uint32)
    Z, Y, X = vol.shape
    vs = np.asarray(voxel_size, np.float32)
    R, t = _rt(cam2vol)
    Ri = np.asarray(Rinv, np.float32).reshape(3, 3)
    size = vs * np.array([X, Y, Z], np.float32)  # :359
    time_step = f32(trunc) * f32(step_factor)  # :360
    vinv = f32(1) / vs  # :362
    finvx, finvy = f32(1) / f32(fx), f32(1) / f32(fy)  # Reprojector: finv = 1 / f
    n = rows * cols
    u = np.tile(np.arange(cols, dtype=np.float32), rows)
    v = np.repeat(np.arange(rows, dtype=np.float32), cols)
    pix = [(f32(1) * (u - f32(cx))) * finvx, (f32(1) * (v - f32(cy))) * finvy, np.ones(n, np.float32)]  # reproj(x, y, 1)
    d = normalized(mat(R, pix))  # :208
    org = [np.full(n, t[k], np.float32) for k in range(3)]  # :207
    box_max = size - vs  # :213
    tmin, tmax = intersect(org, d, box_max)  # :216
    tmin = np.fmax(f32(0), tmin)  # :218-219
    live = ~(tmin >= tmax)  # :220
    tmax = (tmax - time_step).astype(np.float32)  # :223
    vstep = [d[k] * time_step for k in range(3)]  # :224
    with np.errstate(invalid="ignore"):  # rays that miss may have an infinite tmin
        nxt = [(org[k] + d[k] * tmin).astype(np.float32) for k in range(3)]  # :225
    hit = np.zeros(n, bool)
    vert = [np.full(n, QNAN, np.float32) for _ in range(3)]
    nrm = [np.full(n, QNAN, np.float32) for _ in range(3)]
    Fnext = np.where(live, _fetch(vol, vinv, nxt, live), f32(0))  # :227, before the loop's first test
    tcurr = tmin.copy()
    live &= tcurr < tmax  # :228
    while live.any():
        Fcurr, curr = Fnext, nxt
        nxt = [np.where(live, nxt[k] + vstep[k], nxt[k]).astype(np.float32) for k in range(3)]  # :231
        Fnext = np.where(live, _fetch(vol, vinv, nxt, live), Fnext)  # :233
        back = live & (Fcurr < 0) & (Fnext > 0)  # :234-235
        cross = live & (Fcurr > 0) & (Fnext < 0)  # :237
        if cross.any():
            i = np.flatnonzero(cross)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                Ft = interpolate(vol, [curr[k][i] * vinv[k] for k in range(3)])  # :238
                Ftdt = interpolate(vol, [nxt[k][i] * vinv[k] for k in range(3)])  # :239
                Ts = tcurr[i] - (time_step * Ft) / (Ftdt - Ft)  # :241
                vx = [(org[k][i] + d[k][i] * Ts).astype(np.float32) for k in range(3)]  # :243
                nn = compute_normal(vol, vs, delta_factor, vx)  # :244
                ok = ~np.isnan(nn[0] * nn[1] * nn[2])  # :246
                nc = mat(Ri, nn)  # :247
                pc = mat(Ri, [vx[k] - t[k] for k in range(3)])  # :248
            j = i[ok]
            hit[j] = True
            for k in range(3):
                vert[k][j] = pc[k][ok]
                nrm[k][j] = nc[k][ok]
        live &= ~back & ~cross
        tcurr = np.where(live, tcurr + time_step, tcurr).astype(np.float32)  # :228
        live &= tcurr < tmax
    shp = (rows, cols)
    return hit.reshape(shp), [a.reshape(shp) for a in vert], [a.reshape(shp) for a in nrm]


def raycast_points(vol, voxel_size, trunc, cam2vol, Rinv, fx, fy, cx, cy, step_factor, delta_factor, cols, rows):
    """points variant (:258-318): float4 points and normals {., ., ., 0}; misses all four quiet NaN (:267)"""
    hit, vert, nrm = raycast(vol, voxel_size, trunc, cam2vol, Rinv, fx, fy, cx, cy, step_factor, delta_factor, cols, rows)
    P = np.full((rows, cols, 4), QNAN, np.float32)
    N = np.full((rows, cols, 4), QNAN, np.float32)
    for k in range(3):
        P[..., k][hit] = vert[k][hit]
        N[..., k][hit] = nrm[k][hit]
    P[..., 3][hit] = 0
    N[..., 3][hit] = 0
    return P, N


def raycast_depth(vol, voxel_size, trunc, cam2vol, Rinv, fx, fy, cx, cy, step_factor, delta_factor, cols, rows):
    """depth variant (:195-256): ushort(vertex.z * 1000) (0 on a miss, :204) and float4 normals"""
    hit, vert, nrm = raycast(vol, voxel_size, trunc, cam2vol, Rinv, fx, fy, cx, cy, step_factor, delta_factor, cols, rows)
    N = np.full((rows, cols, 4), QNAN, np.float32)
    for k in range(3):
        N[..., k][hit] = nrm[k][hit]
    N[..., 3][hit] = 0
    mm = np.where(hit, vert[2] * f32(1000), f32(0))  # :251
    D = np.trunc(np.clip(np.nan_to_num(mm, nan=0.0), 0, 65535)).astype(np.uint16)
    return D, N
