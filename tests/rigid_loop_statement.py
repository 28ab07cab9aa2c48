"""CPU statement of dfa_rigid_align_cloud (the device-resident rigid Gauss-Newton of north-star mode) in
numpy, on top of rigid_align_statement.rigid_sums / rigid_sums64 (one linearisation) and img_statement.icp_update (one pose
update).  Written from include/dynfu_amd.h, not from dynfu_amd/csrc.

Levels run in the order given.  Level l linearises over vertices[::level_step[l]] at the pose reached, at most level_iters[l]
times.  A refused update ends the call: status 1, the reported pose is aff0.  An accepted update whose twist x = (rvec, tvec)
has |rvec| < stop_rot and |tvec| < stop_trans ends its level; the next level starts from the pose reached.  Thresholds of 0
never stop.  Iterations are numbered over the whole schedule, those that do not run included (their trace rows stay NaN)."""
import numpy as np

import img_statement as St
import rigid_align_statement as RS

DET_GATE = 1e-15


def twist(sums27):
    """-> (det A, x) of the 27 sums in float64; x is None where icp_update refuses"""
    A, b = St.unpack_sums(np.asarray(sums27, np.float64))
    with np.errstate(all="ignore"):
        det = np.linalg.det(A)
    if np.isnan(det) or abs(det) < DET_GATE:
        return det, None
    return det, np.linalg.solve(A, b)


def run(vertices, normals, aff0, vmap, nmap, intr, gates, level_step, level_iters, stop_rot=0.0, stop_trans=0.0, fp64=False):
    """-> dict(aff (12,) float32, status, iters_run [per level], rows: per scheduled iteration None (did not run) or
    dict(level, pose (12,) float32 linearised at, sums (27,) the float32 statement's as float32 — or sum64 with fp64 —,
    matched, det, rot, trans (None when refused)), poses: the pose after every iteration that ran)"""
    aff0 = np.asarray(aff0, np.float32).reshape(-1)
    aff, status = aff0.copy(), 0
    rows, poses, iters_run = [], [], [0] * len(level_step)
    for l, (step, iters) in enumerate(zip(level_step, level_iters)):
        v = np.ascontiguousarray(vertices[::step])
        n = None if normals is None else np.ascontiguousarray(normals[::step])
        finished = False
        for _ in range(iters):
            if status or finished:
                rows.append(None)
                continue
            s32, ok, _, sum64, _, _ = RS.rigid_sums64(v, n, aff, vmap, nmap, intr, **gates)
            sums = sum64 if fp64 else s32.astype(np.float32)
            det, x = twist(sums)
            row = dict(level=l, pose=aff.copy(), sums=sums, matched=int(ok.sum()), det=float(det), rot=None, trans=None)
            rows.append(row)
            iters_run[l] += 1
            if x is None:
                status = 1
                continue
            okay, aff = St.icp_update(sums, aff)
            assert okay
            poses.append(aff.copy())
            row["rot"], row["trans"] = float(np.linalg.norm(x[:3])), float(np.linalg.norm(x[3:]))
            finished = row["rot"] < stop_rot and row["trans"] < stop_trans
    ran = [r for r in rows if r is not None]
    return dict(aff=aff0.copy() if status else aff, status=status, iters_run=iters_run, rows=rows, poses=poses,
                matched_first=ran[0]["matched"] if ran else 0, matched_last=ran[-1]["matched"] if ran else 0)
