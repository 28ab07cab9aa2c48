"""The schedules of dfa_rigid_align_cloud, shared by tests/test_rigid_loop_statement_cpu.py (which runs the statement,
measures the constants recorded here and checks that no decision of a schedule sits on a knife edge) and
tests/test_gpu_rigid_loop.py (which runs the kernels on them).  The clouds and maps are rigid_align_cases': the 80 x 60
scene, its whole cloud (N = 3 869) or a cut of it, every loop starting from the identity (what is to be recovered is
icp_cases.motion())."""
import functools

import numpy as np

import icp_cases as K
import rigid_align_cases as C
import rigid_loop_statement as LS

GATES = C.GATES
IDENT = C.IDENT

# name: (case of rigid_align_cases, level_step, level_iters, stop_rot, stop_trans)
SCHEDULES = {
    "full 1x10": ("80x60 NEAR", (1,), (10,), 0.0, 0.0),                          # rigid_align_cases.trajectory
    "4-2-1": ("80x60 NEAR", (4, 2, 1), (4, 5, 10), 0.0, 0.0),
    "16-4-1 stop 2e-5": ("80x60 NEAR", (16, 4, 1), (4, 5, 10), 2e-5, 2e-5),   # KinFu's {10, 5, 4}, coarsest first
    "N=257 4-1": ("80x60 N=257", (4, 1), (3, 4), 0.0, 0.0),                      # 65 vertices: one workgroup; 257: two
    "N=1031 4-1": ("80x60 N=1031", (4, 1), (3, 4), 0.0, 0.0),                    # 258 vertices: two workgroups; 1031: five
    "stride 4": ("80x60 stride 4", (4, 1), (2, 3), 0.0, 0.0),
    "padded maps": ("53x37 padded", (4, 1), (2, 3), 0.0, 0.0),
    "no normals": ("80x60 no normals", (4, 1), (2, 3), 0.0, 0.0),
}
# Degenerate clouds: ONE vertex in the level gives a matrix of rank one, which icp_update refuses (its determinant is zero up
# to rounding, 25 decades under the gate) — status 1, the pose aff0, one iteration counted and every later launch idle.
SINGULAR = {
    "N=1 4-1": ("80x60 N=1", (4, 1), (3, 4), 0.0, 0.0),
    "step larger than N": ("80x60 NEAR", (5000,), (3,), 0.0, 0.0),  # ceil(3869 / 5000) = 1: vertex 0 alone
}
STOP = "16-4-1 stop 2e-5"

# Per schedule the largest pose-entry difference, over the iterations, between the loop driven by the float32 statement's sums
# and the loop driven by sum64 (tests/test_rigid_loop_statement_cpu.py measures it; both run the same iterations), and the bar
# of the device's final pose against the fp64-driven loop: icp_cases.pose_bar(gap) = 4 x, rounded up to two digits.
MEASURED_POSE_GAP = {
    "full 1x10": 6.15e-8, "4-2-1": 6.43e-8, "16-4-1 stop 2e-5": 6.33e-8, "N=257 4-1": 2.50e-6, "N=1031 4-1": 3.01e-7,
    "stride 4": 5.77e-8, "padded maps": 8.43e-8, "no normals": 6.52e-8,
}
POSE_BAR = {name: K.pose_bar(gap) for name, gap in MEASURED_POSE_GAP.items()}
# The statement's iterations of the schedule with a stop: levels (16, 4, 1) run 4, 2 and 4 of their (4, 5, 10).  The twist
# norms nearest to the threshold of 2e-5 are 4.4e-5 (above: level 0 goes on) and 6.3e-6 (below: level 1 stops); the CPU test
# asserts that none lies within a factor 2 of it, so the device's decisions are the statement's.
STOP_ITERS_RUN = [4, 2, 4]


def inputs(name):
    case, steps, iters, stop_rot, stop_trans = {**SCHEDULES, **SINGULAR}[name]
    return C.inputs(case), steps, iters, stop_rot, stop_trans


@functools.lru_cache(maxsize=None)
def stated(name, fp64=False):
    """the statement's run of a schedule (rigid_loop_statement.run)"""
    c, steps, iters, stop_rot, stop_trans = inputs(name)
    return LS.run(c["vertices"][:, :3], None if c["normals"] is None else c["normals"][:, :3], IDENT, c["vmap"], c["nmap"],
                  c["intr"], GATES, steps, iters, stop_rot, stop_trans, fp64=fp64)


def pose_gap(a, b):
    assert len(a["poses"]) == len(b["poses"])
    return max(float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) for x, y in zip(a["poses"], b["poses"]))
