"""Writes tests/golden/icp_update_kat.json: known answers of the host step of one rigid-ICP iteration, computed by the
float64 statement tests/img_statement.py:icp_update (numpy's determinant and solve, Rodrigues, the product rounded to
float32 once).  tests/cpp/test_host_icp.cpp feeds the same 27 float32 sums and the affine to kfusion::cuda::icp_update.
    python tests/golden/make_icp_update_kat.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_cases as K  # noqa: E402
import img_statement as St  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "icp_update_kat.json")


def pack(A, b):
    """(A, b) -> 27 float32 sums in StreamHelper::get's order"""
    return np.array([b[i] if j == 6 else A[i, j] for i, j in St.SUM_PAIRS], np.float32)


def cases():
    out = []

    def add(name, sums, before, check_affine=True):
        sums = np.asarray(sums, np.float32)
        ok, after = St.icp_update(sums.astype(np.float64), before)
        out.append(dict(name=name, sums=[None if np.isnan(v) else float(v) for v in sums],  # null: JSON has no NaN
                        before=[float(v) for v in np.asarray(before, np.float32)],
                        ok=bool(ok), check_affine=bool(check_affine), after=[float(v) for v in after]))

    pose = K.affine(K.NEAR)
    args, li = K.inputs("640x480", "points")
    vga = St.icp(*args, pose, li)[0].astype(np.float32)
    add("vga", vga, pose)
    zero_b = vga.copy()
    zero_b[St.B_SUMS] = 0
    add("vga_zero_b", zero_b, pose)
    add("all_zero", np.zeros(27), pose)
    rng = np.random.default_rng(11)
    rows = rng.normal(0, 1, (500, 6))
    rows[:, 5] = 0  # no row sees the sixth unknown: A has a zero row and column
    add("rank5", pack(rows.T @ rows, rows.T @ rng.normal(0, 0.01, 500)), pose)
    for name, last in (("det_just_above_gate", 1.001), ("det_just_below_gate", 0.999)):  # det = 1e-15 * last (1 +- 1e-7)
        add(name, pack(np.diag([1e-3] * 5 + [last]), np.full(6, 1e-4)), pose, check_affine=False)
    rows = rng.normal(0, 1, (500, 6)) * [1.0, 1.2, 0.8, 0.5, 0.6, 0.7]
    A = rows.T @ rows
    add("theta_1e-9", pack(A, A @ [6e-10, -7e-10, 4e-10, 2e-3, -1e-3, 3e-3]), pose)
    add("theta_0.5", pack(A, A @ [0.3, -0.35, 0.2, 0.05, -0.02, 0.1]), pose)
    nan = vga.copy()
    nan[7] = np.nan  # A[1][1]
    add("nan_in_A", nan, pose)
    return out


if __name__ == "__main__":
    made = cases()
    with open(OUT, "w") as f:
        json.dump(dict(cases=made), f, indent=1, allow_nan=False)
        f.write("\n")
    print(OUT, [(c["name"], c["ok"]) for c in made])
