"""The cases of the rigid frame loop's statement tests (tests/test_kinfu_statement_cpu.py, tests/test_gpu_kinfu_frames.py):
the scene of tests/cpp/test_host_kinfu.cpp in numpy, the cases, the per-frame record both tests speak, and the stage
comparisons.

A record is what `test_host_kinfu dump` writes for one frame, or the same quantities from the statement chain
(chain_records): result, counter, pose, dists, depth_pyr / points_pyr / normals_pyr (the measured side), volume,
model_points / model_normals (the maps the next frame is aligned against).  Each expect_* function states one stage from
the record's OWN inputs, so that one ulp in a pose does not cascade into the next stage; `defect=` plants one of
kinfu_statement.DEFECTS into the stated side.

E32 holds, per case, the recorded e32 (the largest entry-wise difference, over the frames, between the affine of the
float64 ICP chain and each of the three float32 readings; measured by the CPU test, which also holds the record to within
a factor 2 plus 2^-23 of what it measures).  The pose tolerance of a case is tol = 16 max(e32, 2^-23 (1 + |t|)): the
device's sums differ from the statement's in reduction order only, the class of rounding the three readings span, and 16
covers the accumulation over up to 19 iterations.
"""
import numpy as np

import kinfu_statement as K
from img_statement import resize_points_normals, rodrigues

SPHERES = [((0.25, -0.1, 1.6), 0.45), ((-0.55, 0.3, 2.0), 0.3)]
WALL_N, WALL_D = np.array([0.3, 0.2, -0.933]), -2.6 * 0.933  # wall: n . X = d


def pose_at(i, motion=1.0):
    """camera pose of frame i: 0.6 degrees about y and (6, -3, 4) mm per frame, times `motion` -> (R 3x3, t), float64"""
    a = 0.0105 * motion * i
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return R, motion * i * np.array([0.006, -0.003, 0.004])


def render(W, H, fx, fy, R, t, spheres=None, wall=True):
    """depth (uint16 mm) of two spheres in front of a tilted wall from camera pose X_world = R X_cam + t; a border of 3
    pixels stays empty.  spheres: another list of (centre, radius) instead of SPHERES; wall=False: nothing behind them"""
    cx, cy = W // 2 - 0.5, H // 2 - 0.5
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dw = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ np.asarray(R, np.float64).T
    best = np.full((H, W), 1e9)
    for c, rad in (SPHERES if spheres is None else spheres):
        oc = np.asarray(t, np.float64) - np.array(c)
        a, b, cc = (dw * dw).sum(-1), 2 * (dw @ oc), oc @ oc - rad * rad
        disc = b * b - 4 * a * cc
        with np.errstate(invalid="ignore"):
            s = (-b - np.sqrt(disc)) / (2 * a)
        best = np.where((disc > 0) & (s > 0) & (s < best), s, best)
    den = dw @ WALL_N
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (WALL_D - WALL_N @ np.asarray(t, np.float64)) / den
    if wall:
        best = np.where((np.abs(den) > 1e-6) & (s > 0) & (s < best), s, best)
    d = np.where(best < 60.0, np.rint(best * 1000.0), 0).astype(np.uint16)
    out = np.zeros((H, W), np.uint16)
    out[3:H - 3, 3:W - 3] = d[3:H - 3, 3:W - 3]
    return out


def _small(W, H, **kw):
    return dict(cols=W, rows=H, intr=(525.0 * W / 640.0, 525.0 * H / 480.0, W // 2 - 0.5, H // 2 - 0.5), **kw)


def _tilted_volume_pose():
    """a volume frame turned by about 6 degrees about an oblique axis: with the default pure translation a swapped
    product or a missing inverse partly cancels"""
    return np.concatenate([rodrigues([0.05, -0.08, 0.06]).reshape(-1), [-1.55, -1.15, 0.45]]).astype(np.float32)


# frames: the number of frames; motion: multiple of pose_at's step; empty: frames replaced by an all-zero image
CASES = {
    "default": dict(params=_small(96, 72, volume_dims=(96, 96, 96)), frames=4, motion=1.0),
    "short": dict(params=_small(96, 72, volume_dims=(96, 96, 96), icp_iter_num=(2, 2, 2)), frames=3, motion=8.0),
    "tilted_noncubic": dict(params=_small(96, 72, volume_dims=(96, 64, 128), volume_size=(3.0, 2.5, 3.4),
                                          volume_pose=_tilted_volume_pose(), icp_iter_num=(0, 2, 0)), frames=3, motion=4.0),
    "odd_truncated": dict(params=_small(90, 70, volume_dims=(64, 64, 64), icp_truncate_depth_dist=2.55,
                                        icp_iter_num=(0, 0, 3)), frames=3, motion=4.0),
    "lost": dict(params=_small(96, 72, volume_dims=(64, 64, 64)), frames=3, motion=1.0, empty=(1,)),
}
# the recorded e32 per case (see the module docstring; profiles/kinfu_frame_statement.md)
E32 = {"default": 8.7e-8, "short": 7.9e-8, "tilted_noncubic": 5.5e-8, "odd_truncated": 2.0e-7, "lost": 0.0}  # lost: no ICP runs


def params_of(name):
    return K.Params(**CASES[name]["params"])


def depths_of(name):
    c, p = CASES[name], params_of(name)
    out = []
    for i in range(c["frames"]):
        if i in c.get("empty", ()):
            out.append(np.zeros((p.rows, p.cols), np.uint16))
        else:
            out.append(render(p.cols, p.rows, float(p.intr[0]), float(p.intr[1]), *pose_at(i, c["motion"])))
    return out


def pose_tolerance(name, pose):
    return 16.0 * max(E32[name], 2.0 ** -23 * (1.0 + float(np.abs(np.asarray(pose, np.float64)[9:]).max())))


def truth_error(name, i, pose):
    """(max |dR|, max |dt|) of a 12-float pose against the true camera path"""
    R, t = pose_at(i, CASES[name]["motion"])
    pose = np.asarray(pose, np.float64)
    return float(np.abs(pose[:9].reshape(3, 3) - R).max()), float(np.abs(pose[9:] - t).max())


# ---------------------------------------------------------------------------------------------------- records ----
def chain_records(name, mode="32", defect=None):
    """the statement chain over the case's frames -> (records, icps): a record per frame, estimate_transform's dict per
    frame (None for a first frame)"""
    p = params_of(name)
    state = K.new_state(p)
    recs, icps = [], []
    for depth in depths_of(name):
        o = K.frame(state, depth, p, mode, defect)
        m = o["maps"]
        recs.append(dict(result=o["result"], counter=o["counter"], pose=o["pose"], dists=m["dists"], depth_pyr=m["depth_pyr"],
                         points_pyr=m["points_pyr"], normals_pyr=m["normals_pyr"], volume=state["volume"],
                         model_points=state["prev_points"], model_normals=state["prev_normals"]))
        icps.append(o["icp"])
    return recs, icps


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b))


def is_first(prev):
    """the frame after `prev` (None: the first of all) meets frame_counter_ == 0"""
    return prev is None or prev["counter"] == 0


# ----------------------------------------------------------------------------------------------------- stages ----
def expect_measured(depth, params, defect=None):
    """stage a: dists and the measured pyramids from the depth frame -> dict name -> array"""
    m = K.curr_maps(depth, params, defect)
    out = dict(dists=m["dists"])
    for lv in range(params.levels):
        out["depth%d" % lv] = m["depth_pyr"][lv]
        out["points%d" % lv] = m["points_pyr"][lv]
        out["normals%d" % lv] = m["normals_pyr"][lv]
    return out


def got_measured(rec, params):
    out = dict(dists=rec["dists"])
    for lv in range(params.levels):
        out["depth%d" % lv] = rec["depth_pyr"][lv]
        out["points%d" % lv] = rec["points_pyr"][lv]
        out["normals%d" % lv] = rec["normals_pyr"][lv]
    return out


def expect_pose(prev, rec, params, mode="64", defect=None):
    """stage b: the pose after this frame from the record's measured maps and the previous record's model maps and pose
    -> (pose or None when the track is lost, estimate_transform's dict or None for a first frame)"""
    if is_first(prev):
        return K.IDENTITY.copy(), None
    icp = K.estimate_transform(rec["points_pyr"], rec["normals_pyr"], prev["model_points"], prev["model_normals"], params,
                               mode, defect)
    if not icp["ok"]:
        return None, icp
    return K.next_pose(prev["pose"], icp["affine"], defect), icp


def expect_volume(prev, rec, params, defect=None):
    """stage c: the volume from the record's dists and pose bits"""
    into = prev["volume"] if (defect == "no_clear" and not is_first(prev)) else None
    return K.integrate(rec["dists"], rec["pose"], params, into=into, defect=defect)


def expect_model(prev, rec, params, defect=None):
    """stage d: the model maps -> (points_pyr, normals_pyr).  A first frame's are its measured maps; later level 0 is the
    raycast of the record's volume from the record's pose, level l the resize of the RECORD's level l - 1."""
    if is_first(prev):
        return rec["points_pyr"], rec["normals_pyr"]
    pose = prev["pose"] if defect == "raycast_prev_pose" else rec["pose"]
    P0, N0 = K.raycast_model(rec["volume"], pose, params, defect)
    P, N = [P0], [N0]
    for lv in range(1, params.levels):
        if defect == "model_pyr_stale":
            pi, ni = prev["model_points"][lv], prev["model_normals"][lv]
        else:
            pi, ni = resize_points_normals(rec["model_points"][lv - 1], rec["model_normals"][lv - 1])
        P.append(pi)
        N.append(ni)
    return P, N


# ------------------------------------------------------------------------------------------------ comparison ----
STAGE_OF = dict(no_truncation="a", maps_intr_not_divided="a", levels_fine_to_coarse="b", icp_intr_not_divided="b",
                ctor_gates="b", affine_times_prev="b", iter_minus_l0="b", iter_minus_l1="b", iter_minus_l2="b",
                vol2cam_no_inverse="c", no_clear="c", cam2vol_no_inverse="d", raycast_prev_pose="d", model_pyr_stale="d")
assert set(STAGE_OF) == set(K.DEFECTS)


def compare(name, recs, depths, defect=None, stages="abcd"):
    """The records of a run of case `name` against the stages stated from the records' own inputs.
    -> (bad, poses): bad lists (frame, quantity) for every quantity that must be equal bit for bit and is not (stages a,
    c, d; with stage b the results, the counters and a first frame's identity pose; stage e, the lost track, whenever the
    stated ICP refuses a frame); poses holds per frame None or dict(diff, tol, ratio, knife, matched), diff =
    max |pose_rec - pose_ref| (stage b)."""
    p = params_of(name)
    bad, poses = [], []
    prev = None
    for i, (rec, depth) in enumerate(zip(recs, depths)):
        if "a" in stages:
            want, got = expect_measured(depth, p, defect), got_measured(rec, p)
            bad += [(i, k) for k in want if not same(want[k], got[k])]
        first = is_first(prev)
        pose, icp = expect_pose(prev, rec, p, "64", defect)
        lost = pose is None
        if "b" in stages or lost:
            counter = 1 if first else 0 if lost else prev["counter"] + 1
            if bool(rec["result"]) != (counter > 2):
                bad.append((i, "result"))
            if int(rec["counter"]) != counter:
                bad.append((i, "counter"))
            if first or lost:
                if not same(rec["pose"], K.IDENTITY):
                    bad.append((i, "pose"))
                poses.append(None)
            else:
                diff = float(np.abs(np.asarray(rec["pose"], np.float64) - pose).max())
                tol = pose_tolerance(name, pose)
                poses.append(dict(diff=diff, tol=tol, ratio=diff / tol, knife=list(icp["knife"]), matched=list(icp["matched"])))
        if lost:  # stage e: KinFu::reset cleared the volume and left the model maps alone
            want_volume = np.zeros_like(rec["volume"])
            wantP, wantN = prev["model_points"], prev["model_normals"]
        else:
            want_volume = expect_volume(prev, rec, p, defect) if "c" in stages else None
            wantP, wantN = expect_model(prev, rec, p, defect) if "d" in stages else (None, None)
        if want_volume is not None and not same(want_volume, rec["volume"]):
            bad.append((i, "volume"))
        if wantP is not None:
            for lv in range(p.levels):
                if not same(wantP[lv], rec["model_points"][lv]):
                    bad.append((i, "model_points%d" % lv))
                if not same(wantN[lv], rec["model_normals"][lv]):
                    bad.append((i, "model_normals%d" % lv))
        prev = rec
    return bad, poses
