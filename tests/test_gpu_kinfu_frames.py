"""kfusion::KinFu::operator() on the device against the composed statement (tests/kinfu_statement.py), frame by frame
and stage by stage.

Per case (tests/kinfu_cases.py) the frames are written to a directory, `test_host_kinfu dump` runs KinFu over them once
as a child process and writes what every frame left behind, and each stage is then stated from the DEVICE'S OWN inputs,
so that one ulp in a pose does not cascade:
  a. dists and every level of the measured depth, point and normal maps from the depth frame: bit for bit;
  b. the pose: the float32 product of the device's previous pose with the affine of the float64 ICP chain on the device's
     measured maps and previous model maps, within tol = 16 max(e32, 2^-23 (1 + |t|)) (kinfu_cases.pose_tolerance; e32
     recorded per case and held by tests/test_kinfu_statement_cpu.py); the return values and the frame counters;
  c. the volume: the statement's integrate into a cleared volume from the device's dists and pose bits through the
     restated inv(pose) * volume_pose: bit for bit;
  d. the model maps: level 0 the statement's raycast of the device's volume from the device's pose through the restated
     inv(volume_pose) * pose and its inverse_rotation, level l the resize of the device's level l - 1: bit for bit;
  e. the lost track: after an empty frame the result is false, the counter 0, the pose the identity, the volume zero and
     the model maps untouched; the next frame is handled as a first frame.
The same comparison with a defect planted into the stated side fails for every defect of kinfu_statement.DEFECTS
(tests/test_kinfu_statement_cpu.py).  Figures: profiles/kinfu_frame_statement.md."""
import os
import subprocess

import numpy as np
import pytest

import kinfu_cases as C
import kinfu_statement as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    from dynfu_amd import build as B
    return B.build_cpp_tests()["test_host_kinfu"]


def _g(v):
    return "%.9g" % float(np.float32(v))  # nine digits carry a float32 exactly


def write_case(name, directory):
    p, depths = C.params_of(name), C.depths_of(name)
    lines = ["cols %d" % p.cols, "rows %d" % p.rows, "intr " + " ".join(_g(v) for v in p.intr),
             "volume_dims %d %d %d" % tuple(p.volume_dims), "volume_size " + " ".join(_g(v) for v in p.volume_size),
             "volume_pose " + " ".join(_g(v) for v in p.volume_pose),
             "bilateral %s %s %d" % (_g(p.bilateral_sigma_depth), _g(p.bilateral_sigma_spatial), p.bilateral_kernel_size),
             "icp_truncate_depth_dist " + _g(p.icp_truncate_depth_dist), "icp_dist_thres " + _g(p.icp_dist_thres),
             "icp_angle_thres " + _g(p.icp_angle_thres),
             "icp_iter_num %d %s" % (len(p.icp_iter_num), " ".join("%d" % n for n in p.icp_iter_num)),
             "tsdf_trunc_dist " + _g(p.tsdf_trunc_dist), "tsdf_max_weight %d" % p.tsdf_max_weight,
             "raycast_step_factor " + _g(p.raycast_step_factor), "gradient_delta_factor " + _g(p.gradient_delta_factor),
             "frames %d" % len(depths)]
    with open(os.path.join(directory, "params.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    for i, d in enumerate(depths):
        assert d.dtype == np.uint16 and d.shape == (p.rows, p.cols)
        d.tofile(os.path.join(directory, "depth_%d.bin" % i))
    return p, depths


def read_records(directory, p, frames):
    X, Y, Z = p.volume_dims
    recs = []
    for i in range(frames):
        f = lambda name: os.path.join(directory, "f%d_%s" % (i, name))
        result, counter = (int(v) for v in open(f("status.txt")).read().split())
        img = lambda name, lv, dtype, ch: np.fromfile(f("%s%d.bin" % (name, lv)), dtype).reshape(
            (p.rows >> lv, p.cols >> lv) + ((4,) if ch else ()))
        L = range(p.levels)
        recs.append(dict(result=bool(result), counter=counter, pose=np.fromfile(f("pose.bin"), np.float32),
                         dists=np.fromfile(f("dists.bin"), np.uint16).reshape(p.rows, p.cols),
                         depth_pyr=[img("depth", lv, np.uint16, False) for lv in L],
                         points_pyr=[img("points", lv, np.float32, True) for lv in L],
                         normals_pyr=[img("normals", lv, np.float32, True) for lv in L],
                         volume=np.fromfile(f("volume.bin"), np.uint32).reshape(Z, Y, X),
                         model_points=[img("model_points", lv, np.float32, True) for lv in L],
                         model_normals=[img("model_normals", lv, np.float32, True) for lv in L]))
        assert recs[-1]["pose"].shape == (12,)
    return recs


@pytest.mark.parametrize("name", list(C.CASES))
def test_kinfu_frames_stage_by_stage(exe, tmp_path, name):
    p, depths = write_case(name, str(tmp_path))
    r = subprocess.run(["timeout", "-k", "10", "120", exe, "dump", str(tmp_path)], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recs = read_records(str(tmp_path), p, len(depths))
    # what the constructor derived from the parameters
    d = open(os.path.join(str(tmp_path), "derived.txt")).read().split()
    assert int(d[0]) == p.levels and int(d[7]) == p.tsdf_max_weight
    got = np.array([float(v) for v in d[1:7]], np.float32)
    want = np.array([p.trunc, *p.voxel_size, p.icp_dist_thres, p.icp_angle_thres], np.float32)
    assert C.same(got, want), (got, want)

    bad, poses = C.compare(name, recs, depths)
    chain, _ = C.chain_records(name, "64")  # the statement alone, for the errors against the true camera path
    for i, (rec, q) in enumerate(zip(recs, poses)):
        line = "%s frame %d: result %d counter %d" % (name, i, rec["result"], rec["counter"])
        if rec["counter"]:
            line += "; against the true path max |dR| %.3e |dt| %.3e (device), %.3e %.3e (statement chain)" % (
                C.truth_error(name, i, rec["pose"]) + C.truth_error(name, i, chain[i]["pose"]))
        if q is not None:
            line += "; |pose_dev - pose_ref| %.3e tol %.3e ratio %.3f knife %d matched %d..%d" % (
                q["diff"], q["tol"], q["ratio"], sum(q["knife"]), min(q["matched"]), max(q["matched"]))
        print(line)
    assert bad == []
    empty = C.CASES[name].get("empty", ())
    for i, q in enumerate(poses):
        if i == 0 or i in empty or (i - 1) in empty:
            assert q is None
        else:
            assert sum(q["knife"]) == 0 and q["ratio"] <= 1, (i, q)
    for i in empty:  # stage e, spelled out
        assert not recs[i]["result"] and recs[i]["counter"] == 0 and C.same(recs[i]["pose"], K.IDENTITY)
        assert not recs[i]["volume"].any()
        assert not recs[i + 1]["result"] and recs[i + 1]["counter"] == 1 and C.same(recs[i + 1]["pose"], K.IDENTITY)
        assert all(C.same(a, b) for a, b in zip(recs[i + 1]["model_points"], recs[i + 1]["points_pyr"]))
