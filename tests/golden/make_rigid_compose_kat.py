"""Writes tests/golden/rigid_compose_kat.json: known answers of Warpfield::composeRigid, computed by the float64 statement
tests/rigid_align_statement.py:compose_rigid (dq(T) o dq_i: real part r_T r, dual part r_T d + d_T r) and rounded to float32
once.  tests/cpp/test_host_rigid_align.cpp feeds the same float32 transform and dual quaternions to the host adaptor.
    python tests/golden/make_rigid_compose_kat.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_cases as K  # noqa: E402
import rigid_align_cases as C  # noqa: E402
import rigid_align_statement as RS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rigid_compose_kat.json")
D = 5


def cases():
    dq = C.invariance_problem()["node_dq"][:D]
    poses = {
        "identity": ([0, 0, 1], 0.0, [0, 0, 0]),
        "near": K.NEAR,
        "forty_degrees": ([0.3, 1.0, -0.2], np.deg2rad(40.0), [0.12, -0.07, 0.2]),
        "about_x_170_degrees": ([1.0, 0.02, -0.01], np.deg2rad(170.0), [-0.5, 0.25, 1.5]),   # the trace is negative: the
        "about_y_175_degrees": ([0.01, 1.0, 0.03], np.deg2rad(175.0), [0.3, -0.2, 0.1]),     # other branches of the
        "about_z_179_degrees": ([-0.02, 0.01, 1.0], np.deg2rad(179.0), [0.0, 2.0, -1.0]),    # matrix-to-quaternion rule
        "translation_only": ([0, 0, 1], 0.0, [3.0, -2.0, 0.5]),
    }
    out = []
    for name, pose in poses.items():
        T = K.affine(pose)  # float32, as the adaptor receives it
        after = RS.compose_rigid(dq, T).astype(np.float32)
        out.append(dict(name=name, T=[float(v) for v in T], dq=[float(v) for v in dq.reshape(-1)],
                        after=[float(v) for v in after.reshape(-1)]))
    return out


if __name__ == "__main__":
    made = cases()
    with open(OUT, "w") as f:
        json.dump(dict(cases=made), f, indent=1, allow_nan=False)
        f.write("\n")
    print(OUT, [c["name"] for c in made])
