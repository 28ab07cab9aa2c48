"""Where does the rigid loop's drift against the true camera path come from?  tests/cpp/test_host_kinfu.cpp attributes it
to integrate() sampling the depth image at texel floor(projection), half a pixel off the ray convention of the measured
maps and of the raycaster.  Decided at the level of the statement (tests/kinfu_statement.py, CPU only): the statement
chain runs over the scene of the test twice, as written and with integrate() alone given cx + 0.5, cy + 0.5 (the texel
NEAREST the projection), and prints the error of the pose chain against the true path per frame.

usage: python tools/kinfu_drift_experiment.py 320 240 256 5 >> profiles/kinfu_frame_statement.md   (cols rows volume frames)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import kinfu_cases as C  # noqa: E402
import tsdf_statement as T  # noqa: E402

W, H, dim, frames = (int(v) for v in sys.argv[1:5])
C.CASES["drift"] = dict(params=C._small(W, H, volume_dims=(dim, dim, dim)), frames=frames, motion=1.0)
stated = T.integrate
rows = []
for shift in (0.0, 0.5):
    def integrate(vol, dists, voxel, trunc, max_weight, vol2cam, fx, fy, cx, cy, _s=np.float32(shift)):
        return stated(vol, dists, voxel, trunc, max_weight, vol2cam, fx, fy, np.float32(cx) + _s, np.float32(cy) + _s)
    T.integrate = integrate
    recs, _ = C.chain_records("drift", "64")
    rows.append([C.truth_error("drift", i, r["pose"]) for i, r in enumerate(recs)])
T.integrate = stated
print("\n%d x %d, %d^3, default schedule, the C++ test's motion; max |dR|, max |dt| (m) against the true path\n" % (W, H, dim))
print("| frame | as written | integrate samples the nearest texel |\n|---|---|---|")
for i, (a, b) in enumerate(zip(*rows)):
    print("| %d | %.5f, %.5f | %.5f, %.5f |" % (i, a[0], a[1], b[0], b[1]))
