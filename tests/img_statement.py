"""CPU statement of the depth pre-processing (src/kfusion/cuda/imgproc.cu) and of one linearisation of the rigid
projective ICP (src/kfusion/cuda/proj_icp.cu) in numpy float32.

It is a second reading of the reference's sources, written from them and not from oracle/img_oracle.c or
oracle/icp_oracle.c.  tests/test_img_statement_cpu.py checks it on hand-made inputs and against the oracle; the -m gpu
tests compare the HIP kernels with it directly.  Arithmetic convention as in tests/tsdf_statement.py (the one
oracle/oracle.h documents), plus two choices of the project that this module restates:
  - __expf in the bilateral weight has no portable definition; the project replaces it by a fixed sequence of IEEE
    operations (exp_neg below, the same sequence as oracle/img_oracle.c documents), so that the filter is bit-exact;
  - the bilateral's `(value - depth) * (value - depth)` (:29) is an int product that wraps for depth steps beyond
    46 340 mm; the project squares in float instead (the same number wherever the int product is defined).
Undefined outputs are the reference's numeric_limits<float>::quiet_NaN(), the bit pattern 0x7fffffff
(temp_utils.hpp:21).

The ICP statement forms the correspondence tests, the `float row[7]` and every product row[i] * row[j] in float32 as
proj_icp.cu:28-100 and :335-353 do, and adds the 27 products in float64: the reference's float tree reduction depends
on its tile order and is not restated.  icp64() adds the same sums with rows and products in float64 (sum64), their
rounding scale (abs64) and the number of knife-edge pixels; icp_update() is the host's 6x6 step (projective_icp.cpp:136-152)
in float64.
"""
import numpy as np

from extract_statement import fma32
from tsdf_statement import QNAN, dot, normalized

f32 = np.float32
LOG2E = f32(1.44269504088896341)
_EXP_C = [f32(c) for c in (0.00015403530393381608, 0.0013333558146428443, 0.009618129107628477, 0.05550410866482158,
                           0.2402265069591007, 0.6931471805599453, 1.0)]


def exp_neg(x):
    """the project's __expf for x <= 0: 2^n * p(f), t = x log2(e), n = rint(t), f = t - n, p the degree-6 Taylor
    polynomial of 2^f in Horner form with fused multiply-adds; 0 where t < -126"""
    x = np.asarray(x, np.float32)
    t = x * LOG2E
    ok = t >= f32(-126)
    n = np.rint(np.where(ok, t, f32(0))).astype(np.float32)
    f = (t - n).astype(np.float32)
    p = np.full(x.shape, _EXP_C[0], np.float32)
    for c in _EXP_C[1:]:
        p = fma32(p, f, c)
    s = np.ldexp(np.float32(1), n.astype(np.int32)).astype(np.float32)
    return np.where(ok, p * s, f32(0)).astype(np.float32)


def _shift(img, dy, dx, fill=0):
    """img[y + dy, x + dx] at every (y, x), `fill` outside"""
    H, W = img.shape[:2]
    m = max(abs(dy), abs(dx))
    pad = np.full((H + 2 * m, W + 2 * m) + img.shape[2:], fill, img.dtype)
    pad[m:m + H, m:m + W] = img
    return pad[m + dy:m + dy + H, m + dx:m + dx + W]


# --------------------------------------------------------------------------------------------------- bilateral ----
def bilateral(depth, ksz, sigma_spatial, sigma_depth):
    """imgproc.cu:8-53.  The window is cy in [max(y - ksz/2, 0), min(y - ksz/2 + ksz, rows - 1)) and likewise in x
    (:18-25): its upper end excludes the last row and column of the image (so a 1-pixel-wide image has an empty window,
    0 / 0, and __float2int_rn(NaN) = 0)."""
    src = np.asarray(depth, np.uint16)
    H, W = src.shape
    sd = f32(sigma_depth) * f32(1000)  # :44
    ss_inv = f32(0.5) / (f32(sigma_spatial) * f32(sigma_spatial))  # :50
    sd_inv = f32(0.5) / (sd * sd)  # :51
    value = src.astype(np.int64)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sum1 = np.zeros((H, W), np.float32)
    sum2 = np.zeros((H, W), np.float32)
    h = ksz // 2
    for oy in range(-h, ksz - h):  # cy ascending (:24)
        for ox in range(-h, ksz - h):  # cx ascending (:25)
            cy, cx = yy + oy, xx + ox
            ok = (cy >= 0) & (cy < H - 1) & (cx >= 0) & (cx < W - 1)
            d = _shift(src, oy, ox).astype(np.int64)
            space2 = f32(ox * ox + oy * oy)  # :28
            diff = (value - d).astype(np.float32)
            color2 = diff * diff  # :29
            w = exp_neg(-(space2 * ss_inv + color2 * sd_inv))  # :31
            sum1 = np.where(ok, sum1 + d.astype(np.float32) * w, sum1).astype(np.float32)  # :33
            sum2 = np.where(ok, sum2 + w, sum2).astype(np.float32)  # :34
    with np.errstate(invalid="ignore", divide="ignore"):
        q = sum1 / sum2  # :37
    r = np.where(np.isnan(q), 0, np.rint(np.nan_to_num(q, nan=0.0))).astype(np.int64)
    return (r & 0xFFFF).astype(np.uint16)


def truncate_depth(depth, max_dist):
    """imgproc.cu:60-77: 0 where depth > ushort(max_dist * 1000)"""
    d = np.array(depth, np.uint16)
    md = int(np.trunc(f32(max_dist) * f32(1000)))
    d[d > md] = 0
    return d


def depth_pyr(depth, sigma_depth):
    """imgproc.cu:84-122: (rows/2, cols/2); mean of the 5x5 window cx in [max(0, 2x - 2), min(2x + 3, cols - 1))
    (likewise in y) of the values within 3 sigma of the centre src(2y, 2x), int division; 0 if none"""
    src = np.asarray(depth, np.uint16).astype(np.int64)
    H, W = src.shape
    h, w = H // 2, W // 2
    s3 = (f32(sigma_depth) * f32(1000)) * f32(3)  # :115, :120
    yy, xx = np.meshgrid(np.arange(h) * 2, np.arange(w) * 2, indexing="ij")
    centre = src[yy, xx]  # :92
    tot = np.zeros((h, w), np.int64)
    cnt = np.zeros((h, w), np.int64)
    D = 5
    for oy in range(-(D // 2), D - D // 2):
        for ox in range(-(D // 2), D - D // 2):
            cy, cx = yy + oy, xx + ox
            ok = (cy >= 0) & (cy < H - 1) & (cx >= 0) & (cx < W - 1)  # :94-102
            val = np.where(ok, src[np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)], 0)
            take = ok & (np.abs(val - centre).astype(np.float32) < s3)  # :104
            tot += np.where(take, val, 0)
            cnt += take
    return np.where(cnt == 0, 0, tot // np.maximum(cnt, 1)).astype(np.uint16)  # :109


# ------------------------------------------------------------------------------------------------------ normals ----
def _reproj(u, v, z, finvx, finvy, cx, cy):
    """Reprojector (device.hpp:50-54): (z (u - cx) finv.x, z (v - cy) finv.y, z)"""
    return [(z * (u - cx)) * finvx, (z * (v - cy)) * finvy, z]


def _normals(depth, fx, fy, cx, cy):
    """the common part of compute_normals_kernel (:129-157) and points_normals_kernel (:187-215): (defined mask, v00,
    -normalized(cross(v01 - v00, v10 - v00)))"""
    d = np.asarray(depth, np.uint16)
    H, W = d.shape
    finvx, finvy, cx, cy = f32(1) / f32(fx), f32(1) / f32(fy), f32(cx), f32(cy)
    z = d.astype(np.float32) * f32(0.001)
    z00, z01, z10 = z, _shift(z, 0, 1), _shift(z, 1, 0)
    u = np.arange(W, dtype=np.float32)[None, :]
    v = np.arange(H, dtype=np.float32)[:, None]
    inner = np.zeros((H, W), bool)
    inner[:H - 1, :W - 1] = True  # :141 / :198
    ok = inner & ((z00 * z01) * z10 != 0)  # :147 / :206
    v00 = _reproj(u, v, z00, finvx, finvy, cx, cy)
    v01 = _reproj(u + f32(1), v, z01, finvx, finvy, cx, cy)
    v10 = _reproj(u, v + f32(1), z10, finvx, finvy, cx, cy)
    a = [v01[k] - v00[k] for k in range(3)]
    b = [v10[k] - v00[k] for k in range(3)]
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]  # cross()
    n = normalized(c)
    return ok, [np.broadcast_to(v00[k], (H, W)) for k in range(3)], [-n[k] for k in range(3)]


def normals_mask_depth(depth, fx, fy, cx, cy):
    """computeNormalsAndMaskDepth (:129-181) -> (masked depth, normals (H, W, 4)); undefined normals are
    {NaN, NaN, NaN, 0} (:139) and mask their pixel's depth to 0 (:165-166) once every normal exists (second kernel)"""
    d = np.array(depth, np.uint16)
    ok, _, n = _normals(d, fx, fy, cx, cy)
    N = np.zeros(d.shape + (4,), np.float32)
    for k in range(3):
        N[..., k] = np.where(ok, n[k], QNAN)
    d[np.isnan(N[..., 0])] = 0
    return d, N


def points_normals(depth, fx, fy, cx, cy):
    """computePointNormals (:187-226) -> (points, normals), (H, W, 4) each; undefined pixels all-NaN (:196)"""
    ok, v00, n = _normals(depth, fx, fy, cx, cy)
    H, W = np.shape(depth)
    P = np.full((H, W, 4), QNAN, np.float32)
    N = np.full((H, W, 4), QNAN, np.float32)
    for k in range(3):
        P[..., k][ok] = v00[k][ok]
        N[..., k][ok] = n[k][ok]
    P[..., 3][ok] = 0
    N[..., 3][ok] = 0
    return P, N


def _sum4(a, k):
    """(a00 + a01 + a10 + a11) of every 2x2 block, component k, left to right"""
    return ((a[0::2, 0::2, k] + a[0::2, 1::2, k]) + a[1::2, 0::2, k]) + a[1::2, 1::2, k]


def resize_depth_normals(depth, normals):
    """resize_depth_normals_kernel (:258-310): (rows/2, cols/2); a block with a zero depth gives 0 and an all-NaN
    normal, otherwise the int mean depth and the mean normal (x 0.25, w NaN as initialised, :269)"""
    d = np.asarray(depth, np.uint16).astype(np.int64)
    n = np.asarray(normals, np.float32)
    H, W = d.shape
    h, w = H // 2, W // 2
    d, n = d[:2 * h, :2 * w], n[:2 * h, :2 * w]
    d00, d01, d10, d11 = d[0::2, 0::2], d[0::2, 1::2], d[1::2, 0::2], d[1::2, 1::2]
    ok = (d00 * d01 != 0) & (d10 * d11 != 0)  # :279
    D = np.where(ok, (d00 + d01 + d10 + d11) // 4, 0).astype(np.uint16)
    N = np.full((h, w, 4), QNAN, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            N[..., k] = np.where(ok, _sum4(n, k) * f32(0.25), QNAN)  # :287-289 (x 0.25 is exact in float and double)
    return D, N


def resize_points_normals(points, normals):
    """resize_points_normals_kernel (:314-359): a block with a NaN x gives {NaN, NaN, NaN, 0}, otherwise the means"""
    p = np.asarray(points, np.float32)
    n = np.asarray(normals, np.float32)
    H, W = p.shape[:2]
    h, w = H // 2, W // 2
    p, n = p[:2 * h, :2 * w], n[:2 * h, :2 * w]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = ~np.isnan(((p[0::2, 0::2, 0] * p[0::2, 1::2, 0]) * p[1::2, 0::2, 0]) * p[1::2, 1::2, 0])  # :333
        V = np.zeros((h, w, 4), np.float32)
        N = np.zeros((h, w, 4), np.float32)
        for k in range(3):
            V[..., k] = np.where(ok, _sum4(p, k) * f32(0.25), QNAN)
            N[..., k] = np.where(ok, _sum4(n, k) * f32(0.25), QNAN)
    return V, N


# ---------------------------------------------------------------------------------------------------------- ICP ----
SUM_PAIRS = [(i, j) for i in range(6) for j in range(i, 7)]  # StreamHelper::get's order (projective_icp.cpp:39-57)
B_SUMS = [6, 12, 17, 21, 24, 26]                             # the right-hand side b among the 27
KNIFE_ULPS = 4


def _ulp(*mags):
    """float32 spacing at the largest of the given magnitudes (elementwise)"""
    m = np.zeros(np.broadcast(*mags).shape, np.float32)
    for v in mags:
        m = np.fmax(m, np.abs(np.asarray(v, np.float32)))  # fmax: a NaN magnitude never marks a pixel
    return np.spacing(m)


def _icp_terms(curr, ncurr, prev, nprev, aff12, intr, dist_thres, angle_thres, fused=False):
    """find_coresp and the row in float32 -> dict.  The matched mask `ok`, the correspondence (iw, iu) and `knife` (the
    pixels with a gate quantity within KNIFE_ULPS float32 ulps of its threshold, counted only while the pixel is still
    alive at that gate; the ulp is taken at the larger of the quantity's operands and the threshold) never depend on
    `fused`.  With fused=True every a*b + c of s (R p + t as one chain of three fmas), of the cross product and of the
    dots is evaluated with one rounding: the other legitimate float32 reading of the same source lines."""
    depth_variant = np.asarray(curr).dtype == np.uint16
    H, W = np.shape(curr)[:2]
    a = np.asarray(aff12, np.float32).reshape(-1)
    R, t = a[:9].reshape(3, 3), a[9:12]
    fx, fy, cx, cy = (f32(v) for v in intr)
    finvx, finvy = f32(1) / fx, f32(1) / fy  # setLevelIntr (projective_icp.cpp:15-20), f and c given per level
    min_cosine = f32(np.cos(np.float64(f32(angle_thres))))  # projective_icp.cpp:10-13
    dist2 = f32(dist_thres) * f32(dist_thres)
    u = np.broadcast_to(np.arange(W, dtype=np.float32)[None, :], (H, W))
    v = np.broadcast_to(np.arange(H, dtype=np.float32)[:, None], (H, W))
    nc = np.asarray(ncurr, np.float32)
    nprev = np.asarray(nprev, np.float32)
    if depth_variant:
        src_z = np.asarray(curr, np.uint16)
        ok = src_z != 0  # :44
        p = _reproj(u, v, src_z.astype(np.float32) * f32(0.001), finvx, finvy, cx, cy)  # :47
    else:
        vc = np.asarray(curr, np.float32)
        ok = ~np.isnan(vc[..., 0])  # :74
        p = [vc[..., k] for k in range(3)]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = [(dot(R[k], p) + t[k]).astype(np.float32) for k in range(3)]  # aff * p = R p + t
        qx, qy = s[0] / s[2], s[1] / s[2]
        coox = fma32(fx, qx, cx)  # proj (:28-33)
        cooy = fma32(fy, qy, cy)
        knife = ok & ((np.abs(s[2]) <= KNIFE_ULPS * _ulp(R[2, 0] * p[0], R[2, 1] * p[1], R[2, 2] * p[2], t[2]))
                      | (np.minimum(np.abs(coox), np.abs(coox - f32(W))) <= KNIFE_ULPS * _ulp(fx * qx, cx, f32(W)))
                      | (np.minimum(np.abs(cooy), np.abs(cooy - f32(H))) <= KNIFE_ULPS * _ulp(fy * qy, cy, f32(H))))
        ok &= ~((s[2] <= 0) | (coox < 0) | (cooy < 0) | (coox >= f32(W)) | (cooy >= f32(H)))  # :50 / :80
        ok &= np.isfinite(coox) & np.isfinite(cooy)
        iu = np.where(ok, np.floor(np.where(ok, coox, 0)), 0).astype(np.int64)  # point-sampled texture
        iw = np.where(ok, np.floor(np.where(ok, cooy, 0)), 0).astype(np.int64)
        if depth_variant:
            dst_z = np.asarray(prev, np.uint16)[iw, iu]
            ok &= dst_z != 0  # :54
            d = _reproj(coox, cooy, dst_z.astype(np.float32) * f32(0.001), finvx, finvy, cx, cy)  # :57
        else:
            vp = np.asarray(prev, np.float32)[iw, iu]
            ok &= ~np.isnan(vp[..., 0])  # :84
            d = [vp[..., k] for k in range(3)]
        sd = [s[k] - d[k] for k in range(3)]
        sqr = dot(sd, sd)
        knife |= ok & (np.abs(sqr - dist2) <= KNIFE_ULPS * _ulp(sqr, dist2))
        ok &= ~(sqr > dist2)  # :59-61 norm_sqr
        ns = [dot(R[k], [nc[..., j] for j in range(3)]) for k in range(3)]  # aff.R * ncurr
        npv = nprev[iw, iu]
        n = [npv[..., k] for k in range(3)]
        cosine = np.abs(dot(ns, n))
        knife |= ok & (np.abs(cosine - min_cosine) <= KNIFE_ULPS * _ulp(ns[0] * n[0], ns[1] * n[1], ns[2] * n[2], min_cosine))
        ok &= ~(cosine < min_cosine)  # :66-68
        if fused:
            s = [fma32(R[k, 2], p[2], fma32(R[k, 1], p[1], fma32(R[k, 0], p[0], t[k]))) for k in range(3)]
            cross = [fma32(s[1], n[2], -(s[2] * n[1])), fma32(s[2], n[0], -(s[0] * n[2])), fma32(s[0], n[1], -(s[1] * n[0]))]
        else:
            cross = [s[1] * n[2] - s[2] * n[1], s[2] * n[0] - s[0] * n[2], s[0] * n[1] - s[1] * n[0]]  # cross(s, n)
        row = cross + [n[0], n[1], n[2], dot(n, [d[k] - s[k] for k in range(3)])]  # :346-348
    rows = np.zeros((H, W, 7), np.float32)
    for k in range(7):
        rows[..., k] = np.where(ok, row[k], f32(0))  # :350
    return dict(ok=ok, rows=rows, knife=knife, iu=iu, iw=iw, n=n, depth_variant=depth_variant, R=R, t=t,
                intr=(fx, fy, cx, cy), finv=(finvx, finvy))


def sums_of_rows(rows):
    """the 27 sums of float32 rows (H, W, 7): float32 products added in float64"""
    return np.array([np.sum((rows[..., i] * rows[..., j]).astype(np.float64)) for i, j in SUM_PAIRS], np.float64)


def icp(curr, ncurr, prev, nprev, aff12, intr, dist_thres=0.1, angle_thres=0.3490658503988659, fused=False):
    """One linearisation of proj_icp.cu: find_coresp (:41-99; the depth variant when curr is a uint16 depth image,
    the points variant for (H, W, 4) vertex maps) and the row of icp_helper_kernel (:335-353) at every pixel.
    Returns (27 float64 sums in StreamHelper::get's order, i <= j < 7, projective_icp.cpp:39-57; matched mask (H, W);
    the float32 rows (H, W, 7), zero where unmatched).  fused: see _icp_terms; the mask is the same."""
    T = _icp_terms(curr, ncurr, prev, nprev, aff12, intr, dist_thres, angle_thres, fused)
    return sums_of_rows(T["rows"]), T["ok"], T["rows"]


def icp64(curr, ncurr, prev, nprev, aff12, intr, dist_thres=0.1, angle_thres=0.3490658503988659):
    """icp() plus the exact statement.  Returns (sums, ok, rows, sum64, abs64, knife):
    sum64[q]  the 27 sums over the pixels matched in float32 (that mask and its correspondences are the contract), with
              s = R p + t, the re-projections, the row and the products formed in float64 from the same float32 inputs
              (images, affine, intrinsics and the float32 1 / f and 0.001f the kernel holds);
    abs64[q]  sum over those pixels of |row_i row_j|: the scale of legitimate rounding of sum q;
    knife     the number of knife-edge pixels (see _icp_terms): where a contracted a*b + c may decide a gate otherwise."""
    T = _icp_terms(curr, ncurr, prev, nprev, aff12, intr, dist_thres, angle_thres)
    ok, iu, iw = T["ok"], T["iu"], T["iw"]
    f8 = np.float64
    R, t = T["R"].astype(f8), T["t"].astype(f8)
    fx, fy, cx, cy = (f8(v) for v in T["intr"])
    finvx, finvy = (f8(v) for v in T["finv"])
    H, W = ok.shape
    mm = f8(f32(0.001))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if T["depth_variant"]:
            z = np.asarray(curr, np.uint16).astype(f8) * mm
            uu, vv = np.arange(W, dtype=f8)[None, :], np.arange(H, dtype=f8)[:, None]
            p = [z * (uu - cx) * finvx, z * (vv - cy) * finvy, z]
        else:
            p = [np.asarray(curr, np.float32)[..., k].astype(f8) for k in range(3)]
        s = [R[k, 0] * p[0] + R[k, 1] * p[1] + R[k, 2] * p[2] + t[k] for k in range(3)]
        if T["depth_variant"]:
            z = np.asarray(prev, np.uint16)[iw, iu].astype(f8) * mm
            coox, cooy = fx * (s[0] / s[2]) + cx, fy * (s[1] / s[2]) + cy
            d = [z * (coox - cx) * finvx, z * (cooy - cy) * finvy, z]
        else:
            vp = np.asarray(prev, np.float32)[iw, iu]
            d = [vp[..., k].astype(f8) for k in range(3)]
        n = [c.astype(f8) for c in T["n"]]
        row = [s[1] * n[2] - s[2] * n[1], s[2] * n[0] - s[0] * n[2], s[0] * n[1] - s[1] * n[0], n[0], n[1], n[2],
               n[0] * (d[0] - s[0]) + n[1] * (d[1] - s[1]) + n[2] * (d[2] - s[2])]
        row = [r[ok] for r in row]
        sum64 = np.array([np.sum(row[i] * row[j]) for i, j in SUM_PAIRS], f8)
        abs64 = np.array([np.sum(np.abs(row[i] * row[j])) for i, j in SUM_PAIRS], f8)
    return sums_of_rows(T["rows"]), ok, T["rows"], sum64, abs64, int(T["knife"].sum())


def per_sum_units(got, sum64, abs64):
    """|got[q] - sum64[q]| in units of 2^-24 abs64[q], per sum (0 where both are exactly equal, also at abs64 = 0)"""
    got, sum64, abs64 = (np.asarray(v, np.float64) for v in (got, sum64, abs64))
    with np.errstate(invalid="ignore", divide="ignore"):
        diff = np.abs(got - sum64)
        return np.where(diff == 0, 0.0, diff / (2.0 ** -24 * abs64))


def unpack_sums(sums27):
    """StreamHelper::get (projective_icp.cpp:39-57): the 27 sums -> (A symmetric 6x6, b), float64"""
    A, b = np.zeros((6, 6)), np.zeros(6)
    for q, (i, j) in enumerate(SUM_PAIRS):
        if j == 6:
            b[i] = sums27[q]
        else:
            A[i, j] = A[j, i] = sums27[q]
    return A, b


def rodrigues(r):
    """cv::Affine3(rvec, t)'s rotation: the identity below DBL_EPSILON, else cos I + (1 - cos) k k^T + sin [k]x"""
    r = np.asarray(r, np.float64)
    th = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if not th > np.finfo(np.float64).eps:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * K


def icp_update(sums27, aff12):
    """The host step of one iteration (projective_icp.cpp:136-152) in float64: unpack A and b, refuse a system with
    |det A| < 1e-15 or a NaN determinant, otherwise solve A x = b and put the increment (Rodrigues of x[:3],
    translation x[3:]) on the left of the current affine.  -> (ok, 12 float32: R row-major then t; the input when not ok).
    The product is formed in float64 and rounded to float32 once."""
    a = np.asarray(aff12, np.float32).reshape(-1)
    A, b = unpack_sums(np.asarray(sums27, np.float64))
    with np.errstate(all="ignore"):
        det = np.linalg.det(A)
    if np.isnan(det) or abs(det) < 1e-15:
        return False, a.copy()
    x = np.linalg.solve(A, b)
    Ri = rodrigues(x[:3])
    R, t = a[:9].reshape(3, 3).astype(np.float64), a[9:].astype(np.float64)
    return True, np.concatenate([(Ri @ R).reshape(-1), Ri @ t + x[3:]]).astype(np.float32)
