"""The cases of dfa_rigid_sums_cloud, shared by tests/test_rigid_align_statement_cpu.py (which checks the hand-made answers
in both statements, measures the constants recorded here and checks that no shape case has a knife-edge vertex) and
tests/test_gpu_rigid_align.py (which runs the kernel on them).

The scene is tests/icp_cases.render's (two spheres before a tilted wall: roll is observable) at 80 x 60 pixels, f = 64 (at
525 / 8 two vertices of the NEAR cases lie on a knife edge).
The CLOUD is the valid pixels of img_statement.points_normals of the first camera, which stands at icp_cases.motion(); the
LIVE maps are those of the second camera, at the origin.  So the transform that takes the cloud into the live camera's
frame is motion() itself, and an estimate `pose` of a case means pose o motion(): what is left to recover is `pose`
(icp_cases.NEAR, MID: mid-iteration; CONVERGED: residuals of a tenth of a millimetre)."""
import functools

import numpy as np

import icp_cases as K
from gpu_util_cpu import rot
import img_statement as St
import rigid_align_statement as RS

f32 = np.float32
NAN = f32(np.nan)
GATES = dict(dist_thresh=0.1, cos_thresh=0.5)  # NorthStarParameters' defaults

# The constant c of the per-sum bar |got[q] - sum64[q]| <= c 2^-24 abs64[q], measured by
# tests/test_rigid_align_statement_cpu.py as 4 x the largest deviation of the float32 statement from the fp64 one, rounded up
# to a power of two: MEASURED_UNITS over the cases that are not nearly converged, MEASURED_UNITS_CONVERGED over those (d - s
# cancels four digits there that abs64 of a b sum does not see, as in icp_cases).
MEASURED_UNITS, C_BAR = 157.6, 1024                       # worst at N = 1: one vertex, nothing averages
MEASURED_UNITS_CONVERGED, C_BAR_CONVERGED = 1597.8, 8192  # 80x60 CONVERGED
# The trajectory's pose gap between the float32-driven and the fp64-driven run (largest pose entry difference over the 10
# iterations), and the bar of the GPU-driven one: icp_cases.pose_bar(gap) = 4 x, rounded up to two digits.
MEASURED_POSE_GAP, POSE_BAR = 6.15e-8, 2.5e-7
# Left-invariance in float32: the largest difference between the blend of compose_rigid(dq, T) and T applied to the blend of
# dq, both evaluated in float32 arithmetic, over the two transforms of the CPU test (metres); the GPU check's bar is 4 x.
MEASURED_INVARIANCE_GAP, INVARIANCE_BAR = 8.57e-7, 4 * 8.57e-7

W, H, F = 80, 60, 64.0
INTR = (F, F, W / 2 - 0.5, H / 2 - 0.5)
CROP = (53, 37, 14, 12)  # cols, rows, x0, y0
CUT_AT = 1500            # the cloud cut to N vertices starts here: the middle of the image, not its border rows
CUTS = (0, 1, 63, 64, 65, 255, 256, 257, 1031)


def affine_of(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(-1), np.asarray(t, np.float64)]).astype(np.float32)


def estimate(pose):
    """pose o motion() as 12 float32"""
    P = K.affine(pose).astype(np.float64)
    R, t = K.motion()
    Rp, tp = P[:9].reshape(3, 3), P[9:]
    return affine_of(Rp @ R, Rp @ t + tp)


@functools.lru_cache(maxsize=None)
def _scene():
    """((cloud maps V, N of the first camera), (live maps of the second)) at W x H"""
    R, t = K.motion()
    first = St.points_normals(K.render(W, H, F, R, t), *INTR)
    second = St.points_normals(K.render(W, H, F, np.eye(3), np.zeros(3)), *INTR)
    return first, second


def _cloud(V, Nm):
    ok = ~np.isnan(V[..., 0]) & ~np.isnan(Nm[..., 0])
    return np.ascontiguousarray(V[ok][:, :3]), np.ascontiguousarray(Nm[ok][:, :3])


# name: (crop?, cut N or None, stride, with normals, map padding in pixels, pose)
CASES = {}
for _pose_name in ("NEAR", "MID", "CONVERGED"):
    CASES["80x60 " + _pose_name] = (False, None, 3, True, 0, _pose_name)
    CASES["53x37 " + _pose_name] = (True, None, 3, True, 0, _pose_name)
for _n in CUTS:
    CASES["80x60 N=%d" % _n] = (False, _n, 3, True, 0, "NEAR")
CASES["80x60 stride 4"] = (False, None, 4, True, 0, "NEAR")
CASES["80x60 N=257 stride 4"] = (False, 257, 4, True, 0, "MID")
CASES["80x60 no normals"] = (False, None, 3, False, 0, "NEAR")
CASES["53x37 no normals stride 4"] = (True, None, 4, False, 0, "MID")
CASES["53x37 padded"] = (True, None, 3, True, 3, "NEAR")
CASES["80x60 N=1031 stride 4 padded"] = (False, 1031, 4, True, 5, "CONVERGED")
CONVERGED_CASES = tuple(n for n, c in CASES.items() if c[5] == "CONVERGED")


def c_of(name):
    return C_BAR_CONVERGED if name in CONVERGED_CASES else C_BAR


def with_stride(a, stride):
    """(N, 3) -> (N, stride): the 4th float is NaN, never to be looked at"""
    if stride == 3:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(np.concatenate([a, np.full((len(a), 1), NAN, np.float32)], 1))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict(vertices (N, stride), normals (N, stride) or None, aff (12,), vmap, nmap (rows, cols, 4) contiguous, intr,
    pad): the padding is for the caller to apply (pitched())"""
    crop, cut, stride, with_n, pad, pose = CASES[name]
    (V, Nm), (LV, LN) = _scene()
    fx, fy, cx, cy = INTR
    if crop:
        cols, rows, x0, y0 = CROP
        V, Nm, LV, LN = (np.ascontiguousarray(m[y0:y0 + rows, x0:x0 + cols]) for m in (V, Nm, LV, LN))
        cx, cy = cx - x0, cy - y0
    v, n = _cloud(V, Nm)
    if cut is not None:
        v, n = v[CUT_AT:CUT_AT + cut], n[CUT_AT:CUT_AT + cut]
        assert len(v) == cut
    return dict(vertices=with_stride(v, stride), normals=with_stride(n, stride) if with_n else None,
                aff=estimate(getattr(K, pose)), vmap=LV, nmap=LN, intr=(fx, fy, cx, cy), pad=pad)


def pitched(a, extra, fill):
    """(rows, cols, 4) -> (storage (rows, cols + extra, 4), view of its first cols columns); the padding holds `fill`"""
    Hh, Ww = a.shape[:2]
    wide = np.empty((Hh, Ww + extra, 4), np.float32)
    wide[...] = fill
    wide[:, :Ww] = a
    return wide, wide[:, :Ww]


def stated(name):
    """the fp64 statement of a case -> (sums, ok, rows, sum64, abs64, knife)"""
    c = inputs(name)
    return RS.rigid_sums64(c["vertices"], c["normals"], c["aff"], c["vmap"], c["nmap"], c["intr"], **GATES)


def within_bar(got, sum64, abs64, c):
    return K.within_bar(got, sum64, abs64, c)


# ---------------------------------------------------------------------------------------------------- trajectory ----
ITERS = K.SCHEDULE[0]  # 10: KinFu's count at full resolution


def trajectory(sums_at):
    """ITERS iterations from the identity over the whole 80 x 60 cloud: sums_at(case, aff12) -> 27 sums, St.icp_update after
    each (a refused update fails).  -> [aff12 after each iteration]"""
    c = inputs("80x60 NEAR")
    aff = affine_of(np.eye(3), np.zeros(3))
    out = []
    for it in range(ITERS):
        ok, aff = St.icp_update(sums_at(c, aff), aff)
        assert ok, it
        out.append(aff)
    return out


def sums32(c, aff):
    return RS.rigid_sums(c["vertices"], c["normals"], aff, c["vmap"], c["nmap"], c["intr"], **GATES)[0].astype(np.float32)


def sums64(c, aff):
    return RS.rigid_sums64(c["vertices"], c["normals"], aff, c["vmap"], c["nmap"], c["intr"], **GATES)[3]


def pose_gap(a, b):
    return max(float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ left-invariance ----
def _rigid64(axis, angle, t):
    """12 float64: an orthonormal R to float64 precision (a float32 rounding of a rotation is a rotation only to 1e-7)"""
    return np.concatenate([rot(axis, angle).astype(np.float64).reshape(-1), np.asarray(t, np.float64)])


T_SMALL = _rigid64(*K.NEAR)                                   # 0.6 degrees, 8 mm
T_40 = _rigid64([0.3, 1.0, -0.2], np.deg2rad(40.0), [0.12, -0.07, 0.2])
INV_D, INV_N, INV_K = 37, 1031, 8


@functools.lru_cache(maxsize=None)
def invariance_problem():
    """a plan of D = 37 nodes, N = 1031 vertices, k = 8 on the cloud of the 80 x 60 scene: nodes at every 100th vertex with
    random rigid transforms of up to 0.2 rad and 5 cm -> dict(node_pos, node_w, node_dq (float32), canon, canon_n, idx
    (N, k) nearest first, wn (N, k) normalised radial basis weights in float64)"""
    c = inputs("80x60 NEAR")
    canon, canon_n = c["vertices"][:INV_N * 3:3], c["normals"][:INV_N * 3:3]
    assert len(canon) == INV_N
    node_pos = np.ascontiguousarray(canon[::28][:INV_D])
    assert len(node_pos) == INV_D
    rng = np.random.default_rng(20)
    node_w = np.full(INV_D, 0.25, np.float32)
    om = rng.normal(size=(INV_D, 3))
    om *= (rng.uniform(0.02, 0.2, INV_D) / np.linalg.norm(om, axis=1))[:, None]
    th = np.linalg.norm(om, axis=1)
    r = np.concatenate([np.cos(th / 2)[:, None], np.sin(th / 2)[:, None] * om / th[:, None]], 1)
    t = rng.uniform(-0.05, 0.05, (INV_D, 3))
    dq = np.concatenate([r, 0.5 * RS.qmul(RS.pure(t), r)], 1).astype(np.float32)
    d2 = ((canon[:, None, :].astype(np.float64) - node_pos[None].astype(np.float64)) ** 2).sum(-1)
    idx = np.argsort(d2, 1, kind="stable")[:, :INV_K]
    w = np.exp(-np.take_along_axis(d2, idx, 1) / (2 * 0.25 ** 2))
    return dict(node_pos=node_pos, node_w=node_w, node_dq=dq, canon=np.ascontiguousarray(canon),
                canon_n=np.ascontiguousarray(canon_n), idx=idx, wn=w / w.sum(1, keepdims=True))


# --------------------------------------------------------------------------------------------------- edge values ----
EV = dict(cols=8, rows=6, pad=3, intr=(4.0, 4.0, 3.0, 2.0), dist_thresh=0.25, cos_thresh=0.5)
IDENT = affine_of(np.eye(3), np.zeros(3))


def _up(x):
    return np.nextafter(f32(x), f32(np.inf))


def _down(x):
    return np.nextafter(f32(x), f32(-np.inf))


def edge_values_maps():
    """-> (vertex map storage, normal map storage), (rows, cols + pad, 4) float32 each: the first `cols` columns are the
    maps (NaN where nothing is seen), the padding is poison — a point and a normal every vertex below would match, had
    they been read"""
    vs = np.zeros((EV["rows"], EV["cols"] + EV["pad"], 4), np.float32)
    ns = np.zeros_like(vs)
    vs[...] = (0.0, 0.0, 1.0, 0.0)
    ns[...] = (0.0, 0.0, -1.0, 0.0)
    vs[:, :EV["cols"]] = NAN
    ns[:, :EV["cols"]] = NAN
    for (col, row), L in {(2, 2): (-0.25, 0, 1), (4, 2): (0.25, 0, 1), (0, 2): (-0.75, 0, 1), (7, 2): (1.0, 0, 1),
                          (5, 2): (0.5, 0, 1), (3, 3): (0, 0.25, 1.25), (3, 4): (0, 0.5, _up(1.25)),
                          (2, 0): (-0.25, -0.5, 1)}.items():
        vs[row, col] = L + (0.0,)
        ns[row, col] = (0.0, 0.0, -1.0, 0.0)
    ns[2, 5, 0] = NAN  # L finite, Ln.x NaN
    return vs, ns


def edge_values_vertices():
    """-> (vertices (N, 3), normals (N, 3), expected matched (N,), expected without normals (N,)) at the identity estimate;
    u = 4 x / z + 3, w = 4 y / z + 2, dist_thresh = 0.25, cos_thresh = 0.5"""
    back = (0, 0, -1)  # a normal facing the camera, as the live normals do
    rows = [
        ((-0.125, 0, 1), back, 1, 1),           # u = 2.5 -> 2 (even; half-up would say 3, a miss): 0.125 from (-0.25, 0, 1)
        ((0.125, 0, 1), back, 1, 1),            # u = 3.5 -> 4 (even; half-down would say 3, a miss)
        ((-0.875, 0, 1), back, 1, 1),           # u = -0.5 -> -0: column 0
        ((_down(-0.875), 0, 1), back, 0, 0),    # one ulp below -0.5 -> -1: outside
        ((1.125, 0, 1), back, 0, 0),            # u = 7.5 = cols - 0.5 -> 8 (even): outside
        ((_down(1.125), 0, 1), back, 1, 1),     # just below 7.5 -> 7
        ((0, 0, 0), back, 0, 0),                # z == 0
        ((0, 0, -1), back, 0, 0),               # z < 0
        ((NAN, 0, 1), back, 0, 0),              # c.x NaN
        ((0, 0, 1), back, 0, 0),                # pixel (3, 2): L.x NaN
        ((0.5, 0, 1), back, 0, 0),              # pixel (5, 2): L finite, Ln.x NaN
        ((0, 0.25, 1), back, 1, 1),             # pixel (3, 3): |s - L| = 0.25 = dist_thresh exactly
        ((0, 0.5, 1), back, 0, 0),              # pixel (3, 4): L.z one ulp farther
        ((-0.25, 0, 1), (0, 0, -0.5), 1, 1),    # cosine = 0.5 = cos_thresh exactly
        ((-0.25, 0, 1), (0, 0, -_down(0.5)), 0, 1),  # one ulp below
        ((-0.25, 0, 1), (0, 0, 1), 0, 1),       # facing away: cosine -1 (|cosine| would pass)
        ((3e38, 0, 1e-30), back, 0, 0),         # x / z overflows: u = inf is outside
        ((-0.25, -0.625, 1), back, 1, 1),       # w = -0.5 -> -0: row 0
        ((0, 0.875, 1), back, 0, 0),            # w = 5.5 = rows - 0.5 -> 6 (even): outside
    ]
    return (np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.float32),
            np.array([r[2] for r in rows], np.int64), np.array([r[3] for r in rows], np.int64))
