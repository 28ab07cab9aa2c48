"""The cases of the north-star frame loop's statement tests (tests/test_northstar_statement_cpu.py,
tests/test_gpu_northstar_frames.py): the scene, the three configurations, the parameter file `test_host_northstar_frames dump`
reads and the per-frame record it writes.

The scene: kinfu_cases.render with two spheres of its own and without the wall — a small sphere A in front of a larger sphere
B that it half covers — seen by a camera that moves sideways by MOTION per step (X_world = R X_cam + t).  The wall of
kinfu_cases' scene is nine tenths of that model's surface and nothing ever hides more than a hundredth of it, so the hidden
share the masked cases need cannot be had from it: here A's shadow on B moves with the camera and hides a strip of B the model
holds.  96 x 72 pixels, a 64^3 volume of 1.8 m around the two spheres (28 mm voxels).  How regrow_colour's scene, steps and
weight floor were chosen: profiles/northstar_frame_statement.md.

A record is a dict per frame: the arrays and numbers DynFusion's accessors give after the frame (see read_records)."""
import os

import numpy as np

import kinfu_cases as KC
import kinfu_statement as K

f32 = np.float32
W, H = 96, 72
SPHERES = [((0.12, 0.02, 1.25), 0.25), ((-0.16, -0.03, 2.15), 0.42)]  # A, B
# regrow_colour: mirrored, so that what frame 0 does not see (the columns from PARTIAL_FIRST on) is the flank of the large sphere
# — a surface flat enough for two rigid sightings 6 cm apart to agree on within the truncation distance
SCENES = {"regrow_colour": [((-0.20, 0.02, 1.25), 0.22), ((0.12, -0.03, 2.15), 0.42)]}
MOTION = dict(angle=0.012, t=(0.06, -0.01, 0.008))  # per frame: radians about y, metres


def pose_at(i):
    """camera pose of frame i -> (R 3x3, t), float64"""
    a = MOTION["angle"] * i
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return R, i * np.array(MOTION["t"])


def planted(i):
    """the rigid motion of the scene in the camera frame between frame 0 and frame i: X_cam_i = T X_cam_0, 12 float64"""
    R, t = pose_at(i)
    return np.concatenate([R.T.reshape(-1), -R.T @ t])


def render(fx, fy, R, t, x_max=None, spheres=None):
    """kinfu_cases.render without its wall: depth (uint16 mm) of `spheres` (SPHERES) from camera pose (R, t); x_max: no depth from
    that column on"""
    out = KC.render(W, H, fx, fy, R, t, spheres=SPHERES if spheres is None else spheres, wall=False)
    if x_max is not None:
        out[:, x_max:] = 0
    return out


KINFU = dict(cols=W, rows=H, intr=(525.0 * W / 640.0, 525.0 * H / 480.0, W // 2 - 0.5, H // 2 - 0.5), volume_dims=(64, 64, 64),
             volume_size=(1.8, 1.8, 1.8), volume_pose=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, -0.9, -0.9, 0.8], np.float32))
# DynFuParams::defaultParams() with the switches off; a case overrides
DEFAULTS = dict(tukeyOffset=4.652, psi_data=0.01, psi_reg=1e-4, L=4, beta=4, epsilon=0.08, mesh_normals=1, north_star=1,
                model_view=0, north_star_fuse_canonical=0, north_star_fuse_color=0, canonical_max_color_weight=255, fuse_knn_field=0,
                north_star_visible_only=0, fuse_unsupported_rigid=0, north_star_regrow_canonical=0, canonical_min_weight=2,
                north_star_rigid_prealign=0, rigid_prealign_iters=10, rigid_prealign_device=0, rigid_prealign_steps=(16, 4, 1),
                rigid_prealign_level_iters=(4, 5, 10), rigid_prealign_stop=(1e-5, 1e-5), north_star_reg_hierarchy=0,
                reg_level_slots=(4, 2, 2), numIter=2, gnIter=3, linearIter=64, distThresh=0.1, cosThresh=0.5, damping=1e-4, gnTol=1e-3,
                nodeStep=128, warp_knn=8)
DEFAULTS["lambda"] = 200.0
FRAMES = 4
CASES = {
    "plain": dict(nodeStep=150, warp_knn=4),
    "aligned_visible_fused": dict(nodeStep=150, north_star_rigid_prealign=1, rigid_prealign_device=1, model_view=1,
                                  north_star_visible_only=1, north_star_fuse_canonical=1, fuse_knn_field=1, north_star_reg_hierarchy=1),
    "regrow_colour": dict(nodeStep=14, epsilon=0.05, canonical_min_weight=1, north_star_rigid_prealign=1, rigid_prealign_iters=4, model_view=1, north_star_visible_only=1,
                          north_star_fuse_canonical=1, fuse_unsupported_rigid=1, north_star_regrow_canonical=1, north_star_fuse_color=1,
                          canonical_max_color_weight=3),
}
PARTIAL_FIRST = {"regrow_colour": 50}  # frame 0 has no depth from this column on
EMPTY = {"regrow_colour": (2,)}  # all-zero depth frames
# the camera's step count at every frame (default 0, 1, 2, 3).  regrow_colour: 1.75 steps to frame 1, so that A's shadow hides a
# twentieth of the cloud that frame leaves behind; an empty frame shows nothing, so the camera waits through frame 2; 1.25 steps
# more to frame 3 (1.75 more, 10.5 cm from a cloud of two frames, and the four-iteration host loop loses the model)
STEPS = {"regrow_colour": (0, 1.75, 1.75, 3.0)}


class Case:
    """one configuration: .kinfu (kinfu_statement.Params), every key of DEFAULTS as an attribute (float32 where the host's is)"""

    def __init__(self, name):
        self.name = name
        self.kinfu = K.Params(**dict(KINFU, **CASES[name].get("kinfu", {})))
        self.values = dict(DEFAULTS, **{k: v for k, v in CASES[name].items() if k != "kinfu"})
        for k, v in self.values.items():
            setattr(self, k if k != "lambda" else "lambda_", v)
        self.frames = FRAMES
        self.k = min(self.warp_knn, 8)  # northStarKnn
        self.reg_levels = min(self.L + 1, len(self.reg_level_slots))  # DynFuParams::regLevels

    @property
    def solve_params(self):
        """the parameters solve6_statement.Statement6 reads"""
        return dict(dist_thresh=self.distThresh, cos_thresh=self.cosThresh, tukey_offset=self.tukeyOffset, psi_data=self.psi_data,
                    psi_reg=self.psi_reg, lambda_=self.lambda_, damping=self.damping)


def steps_of(name):
    return STEPS.get(name, tuple(range(FRAMES)))


def depths_of(name):
    p = K.Params(**KINFU)
    out = []
    for i in range(FRAMES):
        if i in EMPTY.get(name, ()):
            out.append(np.zeros((H, W), np.uint16))
        else:
            out.append(render(float(p.intr[0]), float(p.intr[1]), *pose_at(steps_of(name)[i]),
                              x_max=PARTIAL_FIRST.get(name) if i == 0 else None, spheres=SCENES.get(name)))
    return out


def colors_of(name):
    """a seeded random b, g, r, x image per frame, (rows, cols, 4) uint8"""
    rng = np.random.default_rng(20 + len(name))
    return [rng.integers(0, 256, (H, W, 4)).astype(np.uint8) for _ in range(FRAMES)]


def _g(v):
    return "%.9g" % float(np.float32(v))  # nine digits carry a float32 exactly


def _fmt(v):
    if isinstance(v, (tuple, list)):
        return " ".join(_fmt(x) for x in v)
    return "%d" % v if isinstance(v, (int, np.integer)) else _g(v)


def write_case(name, directory):
    c = Case(name)
    p = c.kinfu
    lines = ["cols %d" % p.cols, "rows %d" % p.rows, "intr " + _fmt(p.intr), "volume_dims %d %d %d" % tuple(p.volume_dims),
             "volume_size " + _fmt(p.volume_size), "volume_pose " + _fmt(list(p.volume_pose)),
             "bilateral %s %s %d" % (_g(p.bilateral_sigma_depth), _g(p.bilateral_sigma_spatial), p.bilateral_kernel_size),
             "icp_truncate_depth_dist " + _g(p.icp_truncate_depth_dist), "tsdf_trunc_dist " + _g(p.tsdf_trunc_dist),
             "tsdf_max_weight %d" % p.tsdf_max_weight, "gradient_delta_factor " + _g(p.gradient_delta_factor), "frames %d" % c.frames]
    for k, v in c.values.items():
        if k in ("rigid_prealign_steps", "rigid_prealign_level_iters", "reg_level_slots"):
            lines.append("%s %d %s" % (k, len(v), _fmt(v)))
        else:
            lines.append("%s %s" % (k, _fmt(v)))
    with open(os.path.join(directory, "params.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    for i, d in enumerate(depths_of(name)):
        assert d.dtype == np.uint16 and d.shape == (p.rows, p.cols)
        d.tofile(os.path.join(directory, "depth_%d.bin" % i))
    if c.north_star_fuse_color:
        for i, img in enumerate(colors_of(name)):
            img.tofile(os.path.join(directory, "color_%d.bin" % i))
    return c


def read_records(directory, case):
    """what `dump` wrote -> a list of dicts, one per frame.  An array the frame's configuration does not produce is empty."""
    p = case.kinfu
    X, Y, Z = p.volume_dims
    recs = []
    for i in range(case.frames):
        f = lambda name: os.path.join(directory, "f%d_%s" % (i, name))
        st = {}
        for line in open(f("status.txt")).read().splitlines():
            key, *vals = line.split()
            st[key] = vals
        r = dict(result=bool(int(st["result"][0])), counter=int(st["counter"][0]), D=int(st["nodes"][0]), knn=int(st["knn"][0]),
                 rigid_matched=(int(st["rigid_matched_first"][0]), int(st["rigid_matched_last"][0])),
                 rigid_skipped=int(st["rigid_skipped"][0]), visible_count=int(st["visible_count"][0]),
                 initial_cost=float(st["initial_cost"][0]), final_cost=float(st["final_cost"][0]), valid_rows=int(st["valid_rows"][0]),
                 pcg_iters=int(st["pcg_iters"][0]), gn_solves=int(st["gn_solves"][0]), knn_field_nodes=int(st["knn_field_nodes"][0]),
                 regrow_skipped=int(st["regrow_skipped"][0]), canonical_vertices=int(st["canonical_vertices"][0]),
                 level_counts=[int(v) for v in st["level_counts"][1:]])
        raw = lambda name, dtype: np.fromfile(f(name + ".bin"), dtype)
        img = lambda name, dtype, ch: (lambda a: a.reshape((p.rows, p.cols) + ((ch,) if ch else ())) if a.size else a)(raw(name, dtype))
        vol = lambda name: (lambda a: a.reshape(Z, Y, X) if a.size else a)(raw(name, np.uint32))
        r.update(dists=img("dists", np.uint16, 0), depth0=img("depth0", np.uint16, 0), live_points=img("live_points", np.float32, 4),
                 live_normals=img("live_normals", np.float32, 4), live_volume=vol("live_volume"),
                 node_pos=raw("node_pos", np.float32).reshape(-1, 3), node_w=raw("node_w", np.float32),
                 node_dq=raw("node_dq", np.float32).reshape(-1, 8), node_levels=raw("node_levels", np.int32),
                 rigid_pose=raw("rigid_pose", np.float32), rigid_iters=raw("rigid_iters", np.int32).tolist(),
                 visible_flags=raw("visible_flags", np.uint8), model_points=img("model_points", np.float32, 4),
                 model_normals=img("model_normals", np.float32, 4), warped_v=raw("warped_v", np.float32).reshape(-1, 3),
                 warped_n=raw("warped_n", np.float32).reshape(-1, 3), canonical_v=raw("canonical_v", np.float32).reshape(-1, 3),
                 canonical_n=raw("canonical_n", np.float32).reshape(-1, 3), mesh_v=raw("mesh_v", np.float32).reshape(-1, 4),
                 mesh_i=raw("mesh_i", np.int32), canonical_volume=vol("canonical_volume"), color_volume=vol("color_volume"),
                 canonical_colors=raw("canonical_colors", np.uint32), mesh_colors=raw("mesh_colors", np.uint32))
        assert r["D"] == len(r["node_pos"]) == len(r["node_w"]) == len(r["node_dq"]) and r["rigid_pose"].shape == (12,)
        assert r["canonical_vertices"] == len(r["canonical_v"]) == len(r["canonical_n"])
        recs.append(r)
    return recs


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b))
