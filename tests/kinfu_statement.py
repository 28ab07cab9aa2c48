"""CPU statement of the rigid frame loop: kfusion::KinFu::operator() (dynfu_amd/host/src/kinfu.cpp), the level loop of
ProjectiveICP::estimateTransform (projective_icp.cpp) and the pose algebra of TsdfVolume (tsdf_volume.cpp), composed
from the kernels' statements.

Composition only: every kernel is the function of tests/img_statement.py or tests/tsdf_statement.py that the -m gpu
tests already compare with the HIP kernel.  New here is the host arithmetic of dfa_host/types.hpp, restated in float32 in
the written order, one rounding per operation (the host build has no FMA target):
  - Affine3f::operator*: R_ij = (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j, t_i = ((a_i0 t_0 + a_i1 t_1) + a_i2 t_2) + t_i;
  - inverse_rotation: cofactors of float products and differences, the determinant and 1 / det in double, every entry
    (float)(cofactor * (1 / det));
  - inv(): t = -(Ri t), the three products added left to right;
  - Intr::operator()(level): every component divided by (float)(1 << level);
  - TsdfVolume's voxel size (size / dims) and its truncation distance, never below 2.1f voxel edges, in the order the
    KinFu constructor sets them.

Affines are 12 float32: R row-major, then t (Affine3f::to12).  Every stage function takes its inputs explicitly, so that
a test can feed it the bits a device run produced.  A planted defect is chosen with `defect=`; each is a one-line
deviation from the host code (DEFECTS).
"""
import numpy as np

import img_statement as I
import tsdf_statement as T

f32 = np.float32
MAX_PYRAMID_LEVELS = 4
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
CTOR_ANGLE = f32(20.0) * f32(0.017453293)  # ProjectiveICP::ProjectiveICP (projective_icp.cpp:12)

DEFECTS = {
    "levels_fine_to_coarse": "estimateTransform runs the levels 0 ... used-1",
    "icp_intr_not_divided": "runLevel passes the level-0 intrinsics at every level",
    "maps_intr_not_divided": "computePointNormals gets intr instead of intr(level)",
    "ctor_gates": "the tracker keeps ProjectiveICP's constructor gates (20 degrees) instead of KinFuParams'",
    "affine_times_prev": "the pose chain is affine * prev_pose",
    "vol2cam_no_inverse": "integrate forms camera_pose * volume_pose",
    "cam2vol_no_inverse": "raycast forms volume_pose * camera_pose",
    "raycast_prev_pose": "the model is raycast from the previous pose",
    "no_clear": "integrate accumulates into the previous frame's volume",
    "model_pyr_stale": "the model pyramid's levels above 0 are not rebuilt",
    "no_truncation": "depthTruncation is skipped",
    "iter_minus_l0": "one iteration fewer at level 0",
    "iter_minus_l1": "one iteration fewer at level 1",
    "iter_minus_l2": "one iteration fewer at level 2",
}


def _check(defect):
    assert defect is None or defect in DEFECTS, defect


# ---------------------------------------------------------------------------------------------- types.hpp ----
def _a12(a):
    a = np.asarray(a, np.float32).reshape(-1)
    assert a.size == 12
    return a


def aff_mul(a, b):
    """Affine3f::operator* (types.hpp:48-56): a * b, b applied first"""
    a, b = _a12(a), _a12(b)
    r = np.zeros(12, np.float32)
    for i in range(3):
        for j in range(3):
            r[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j]
        r[9 + i] = ((a[3 * i] * b[9] + a[3 * i + 1] * b[10]) + a[3 * i + 2] * b[11]) + a[9 + i]
    return r


def inverse_rotation(a):
    """Affine3f::inverse_rotation (types.hpp:59-70) -> 9 float32"""
    m = np.asarray(a, np.float32).reshape(-1)[:9]
    f8 = np.float64
    c = lambda p, q, r, s: m[p] * m[q] - m[r] * m[s]  # float products, float difference
    det = (f8(m[0]) * f8(c(4, 8, 5, 7)) - f8(m[1]) * f8(c(3, 8, 5, 6))) + f8(m[2]) * f8(c(3, 7, 4, 6))
    if det == 0.0:
        raise ZeroDivisionError("Affine3f: singular rotation")
    inv = f8(1.0) / det
    cof = [c(4, 8, 5, 7), c(2, 7, 1, 8), c(1, 5, 2, 4), c(5, 6, 3, 8), c(0, 8, 2, 6), c(2, 3, 0, 5), c(3, 7, 4, 6),
           c(1, 6, 0, 7), c(0, 4, 1, 3)]
    return np.array([f32(f8(v) * inv) for v in cof], np.float32)


def aff_inv(a):
    """Affine3f::inv (types.hpp:71-76)"""
    a = _a12(a)
    r = np.zeros(12, np.float32)
    r[:9] = inverse_rotation(a)
    for i in range(3):
        r[9 + i] = -((r[3 * i] * a[9] + r[3 * i + 1] * a[10]) + r[3 * i + 2] * a[11])
    return r


def intr_level(intr, level):
    """Intr::operator()(level) (types.hpp:90-93)"""
    div = f32(1 << level)
    return tuple(f32(v) / div for v in intr)


# ----------------------------------------------------------------------------------------------- parameters ----
class Params:
    """KinFuParams (kfusion/kinfu.hpp) with default_params()'s values; keyword arguments override"""

    def __init__(self, **kw):
        self.cols, self.rows = 640, 480
        self.intr = None
        self.volume_dims = (512, 512, 512)
        self.volume_size = (3.0, 3.0, 3.0)
        self.volume_pose = None
        self.bilateral_sigma_depth, self.bilateral_sigma_spatial, self.bilateral_kernel_size = 0.04, 4.5, 7
        self.icp_truncate_depth_dist = 0.0
        self.icp_dist_thres, self.icp_angle_thres = f32(0.1), f32(30.0) * f32(0.017453293)
        self.icp_iter_num = (10, 5, 4, 0)
        self.tsdf_trunc_dist, self.tsdf_max_weight = 0.04, 64
        self.raycast_step_factor, self.gradient_delta_factor = 0.75, 0.5
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)
        if self.intr is None:
            self.intr = (525.0, 525.0, self.cols // 2 - 0.5, self.rows // 2 - 0.5)
        self.intr = tuple(f32(v) for v in self.intr)
        if self.volume_pose is None:  # Affine3f().translate(-size.x / 2, -size.y / 2, 0.5f)
            s = np.asarray(self.volume_size, np.float32)
            self.volume_pose = np.concatenate([IDENTITY[:9], [-s[0] / f32(2), -s[1] / f32(2), f32(0.5)]])
        self.volume_pose = _a12(self.volume_pose).copy()
        assert self.volume_dims[0] % 32 == 0  # KinFu::KinFu (kinfu.cpp:11)

    @property
    def schedule(self):
        """ProjectiveICP::setIterationsNum (projective_icp.cpp:18-21)"""
        s = [0] * MAX_PYRAMID_LEVELS
        for i, n in enumerate(self.icp_iter_num[:MAX_PYRAMID_LEVELS]):
            s[i] = int(n)
        return s

    @property
    def levels(self):
        """getUsedLevelsNum (:23-28)"""
        s = self.schedule
        i = MAX_PYRAMID_LEVELS - 1
        while i >= 0 and not s[i]:
            i -= 1
        return i + 1

    def _voxel(self, size):
        return np.asarray(size, np.float32) / np.asarray(self.volume_dims, np.float32)  # getVoxelSize

    @property
    def voxel_size(self):
        return self._voxel(self.volume_size)

    @property
    def trunc(self):
        """setTruncDist as the KinFu constructor reaches it (kinfu.cpp:12-15): with the volume's default 3 m size when
        tsdf_trunc_dist is set, then once more when setSize re-applies it"""
        t = max(f32(self.tsdf_trunc_dist), f32(2.1) * self._voxel((3.0, 3.0, 3.0)).max())
        return max(t, f32(2.1) * self.voxel_size.max())


# ---------------------------------------------------------------------------------------------------- stages ----
def curr_maps(depth, params, defect=None):
    """kinfu.cpp:45-50 -> dict(dists, depth_pyr, points_pyr, normals_pyr), `levels` entries each"""
    _check(defect)
    p = params
    depth = np.asarray(depth, np.uint16)
    dists = T.compute_dists(depth, *p.intr)
    d = I.bilateral(depth, p.bilateral_kernel_size, p.bilateral_sigma_spatial, p.bilateral_sigma_depth)
    if p.icp_truncate_depth_dist > 0 and defect != "no_truncation":
        d = I.truncate_depth(d, p.icp_truncate_depth_dist)
    pyr = [d]
    for _ in range(1, p.levels):
        pyr.append(I.depth_pyr(pyr[-1], p.bilateral_sigma_depth))
    P, N = [], []
    for i in range(p.levels):
        pi, ni = I.points_normals(pyr[i], *(p.intr if defect == "maps_intr_not_divided" else intr_level(p.intr, i)))
        P.append(pi)
        N.append(ni)
    return dict(dists=dists, depth_pyr=pyr, points_pyr=P, normals_pyr=N)


def _sums32(rows):
    """the 27 sums with the products and the additions in float32, in a defined order: down every column, then along the
    column sums (accumulate is sequential by definition; np.sum's pairwise blocks depend on the build)"""
    acc = lambda a, axis: np.add.accumulate(a, axis=axis, dtype=np.float32)
    return np.array([acc(acc(rows[..., i] * rows[..., j], 0)[-1], 0)[-1] for i, j in I.SUM_PAIRS], np.float64)


MODES = ("64", "32", "fused", "f32sums")


def estimate_transform(curr_points, curr_normals, prev_points, prev_normals, params, mode="64", defect=None):
    """ProjectiveICP::estimateTransform, points variant (projective_icp.cpp:61-72) with runLevel (:30-46).
    mode: which reading of one linearisation feeds icp_update: "64" the float64 sums of icp64, "32" the plain float32
    rows, "fused" the rows with contracted multiply-adds, "f32sums" the plain rows added in float32.
    -> dict(ok, affine (12 float32), knife, matched, levels): knife and matched per iteration in the order run.  ok False
    is a refused update: the track is lost."""
    _check(defect)
    assert mode in MODES
    p = params
    sched = list(p.schedule)
    for lv in range(3):
        if defect == "iter_minus_l%d" % lv:
            assert sched[lv] > 0
            sched[lv] -= 1
    dist = p.icp_dist_thres
    angle = CTOR_ANGLE if defect == "ctor_gates" else p.icp_angle_thres
    order = list(range(p.levels - 1, -1, -1))
    if defect == "levels_fine_to_coarse":
        order.reverse()
    aff = IDENTITY.copy()
    out = dict(ok=True, knife=[], matched=[], levels=[])
    for level in order:
        intr = p.intr if defect == "icp_intr_not_divided" else intr_level(p.intr, level)
        args = (curr_points[level], curr_normals[level], prev_points[level], prev_normals[level])
        for _ in range(sched[level]):
            if mode == "64":
                _, ok, _, sums, _, knife = I.icp64(*args, aff, intr, dist, angle)
            else:
                t = I._icp_terms(*args, aff, intr, dist, angle, fused=(mode == "fused"))
                ok, knife = t["ok"], int(t["knife"].sum())
                sums = _sums32(t["rows"]) if mode == "f32sums" else I.sums_of_rows(t["rows"])
            out["knife"].append(knife)
            out["matched"].append(int(ok.sum()))
            out["levels"].append(level)
            good, aff = I.icp_update(sums, aff)
            if not good:
                out["ok"] = False
                out["affine"] = aff
                return out
    out["affine"] = aff
    return out


def next_pose(prev_pose, affine, defect=None):
    """kinfu.cpp:63: poses_.back() * affine"""
    _check(defect)
    return aff_mul(affine, prev_pose) if defect == "affine_times_prev" else aff_mul(prev_pose, affine)


def integrate(dists, pose, params, into=None, defect=None):
    """TsdfVolume::integrate / clearAndIntegrate (tsdf_volume.cpp:38-54, :155-167) into a cleared volume, or `into`"""
    _check(defect)
    p = params
    X, Y, Z = p.volume_dims
    vol2cam = aff_mul(pose if defect == "vol2cam_no_inverse" else aff_inv(pose), p.volume_pose)
    vol = T.clear((Z, Y, X)) if into is None else into
    return T.integrate(vol, dists, p.voxel_size, p.trunc, p.tsdf_max_weight, vol2cam, *p.intr)


def raycast_model(vol, pose, params, defect=None):
    """TsdfVolume::raycast, points variant (tsdf_volume.cpp:182-194) -> (points, normals) of level 0"""
    _check(defect)
    p = params
    cam2vol = aff_mul(p.volume_pose if defect == "cam2vol_no_inverse" else aff_inv(p.volume_pose), pose)
    return T.raycast_points(vol, p.voxel_size, p.trunc, cam2vol, inverse_rotation(cam2vol), *p.intr,
                            p.raycast_step_factor, p.gradient_delta_factor, p.cols, p.rows)


def model_pyramid(points0, normals0, levels):
    """kinfu.cpp:70-71: level l from level l - 1"""
    P, N = [points0], [normals0]
    for _ in range(1, levels):
        pi, ni = I.resize_points_normals(P[-1], N[-1])
        P.append(pi)
        N.append(ni)
    return P, N


# ------------------------------------------------------------------------------------------------ the loop ----
def new_state(params):
    """KinFu::reset (kinfu.cpp:29-34)"""
    X, Y, Z = params.volume_dims
    return dict(counter=0, poses=[IDENTITY.copy()], volume=T.clear((Z, Y, X)), prev_points=None, prev_normals=None)


def frame(state, depth, params, mode="64", defect=None):
    """KinFu::operator() (kinfu.cpp:42-76) on `state` (changed in place).  -> dict(result, counter, pose, maps, icp):
    maps is curr_maps' dict, icp estimate_transform's (None for a first frame)."""
    _check(defect)
    p = params
    maps = curr_maps(depth, p, defect)
    out = dict(maps=maps, icp=None)
    if state["counter"] == 0:
        state["volume"] = integrate(maps["dists"], state["poses"][-1], p, into=state["volume"], defect=defect)
        state["prev_points"], state["prev_normals"] = maps["points_pyr"], maps["normals_pyr"]
        state["counter"] += 1
        out.update(result=False)
    else:
        icp = estimate_transform(maps["points_pyr"], maps["normals_pyr"], state["prev_points"], state["prev_normals"], p,
                                 mode, defect)
        out["icp"] = icp
        if not icp["ok"]:
            keep = state["prev_points"], state["prev_normals"]  # reset() leaves the images alone
            state.update(new_state(p))
            state["prev_points"], state["prev_normals"] = keep
            out.update(result=False)
        else:
            before = state["poses"][-1]
            state["poses"].append(next_pose(before, icp["affine"], defect))
            state["volume"] = integrate(maps["dists"], state["poses"][-1], p,
                                        into=state["volume"] if defect == "no_clear" else None, defect=defect)
            P0, N0 = raycast_model(state["volume"], before if defect == "raycast_prev_pose" else state["poses"][-1], p, defect)
            P, N = model_pyramid(P0, N0, p.levels)
            if defect == "model_pyr_stale":
                P[1:], N[1:] = state["prev_points"][1:], state["prev_normals"][1:]
            state["prev_points"], state["prev_normals"] = P, N
            state["counter"] += 1
            out.update(result=state["counter"] > 2)
    out.update(counter=state["counter"], pose=state["poses"][-1].copy())
    return out
