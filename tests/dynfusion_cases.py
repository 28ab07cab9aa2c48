"""The cases of the reference-mode frame loop's statement tests (tests/test_dynfusion_statement_cpu.py,
tests/test_gpu_dynfusion_frames.py): the three configurations, the parameter file `test_host_dynfusion_frames dump` reads and
the per-frame record it writes.

The scene, the camera's motion, the image and the volume are northstar_cases': two spheres, 96 x 72 pixels, a 64^3 volume of
1.8 m, four frames.  In reference mode the camera stays at the origin and the clouds, the nodes and the canonical volume are in
the VOLUME's frame; the scene moves in the depth frames.  How nodeStep, epsilon and the solver's budget were chosen:
profiles/dynfusion_frame_statement.md.

A record is a dict per frame: the arrays and numbers DynFusion's accessors give after the frame (see read_records)."""
import os

import numpy as np

import kinfu_statement as K
import northstar_cases as NC

f32 = np.float32
W, H = NC.W, NC.H
KINFU = NC.KINFU
FRAMES = 4
# DynFuParams::defaultParams() with the switches off and a small solver budget (DynFusion's own is 24 x 16 x 256); a case overrides
DEFAULTS = dict(tukeyOffset=4.652, psi_data=0.01, psi_reg=1e-4, L=4, beta=4, epsilon=0.05, mesh_normals=0, north_star=0,
                fuse_canonical=0, fuse_knn_field=0, fuse_unsupported_rigid=0, nodeStep=150, warp_knn=8,
                solver_numIter=1, solver_nonLinearIter=3, solver_linearIter=64)
DEFAULTS["lambda"] = 200.0
CASES = {
    "plain": dict(),
    "fused_field_rigid": dict(fuse_canonical=1, fuse_knn_field=1, fuse_unsupported_rigid=1, mesh_normals=1, warp_knn=4),
    "fused_search_skip": dict(fuse_canonical=1, nodeStep=120, solver_numIter=2),  # (earlyOut: still one outer pass)
}


class Case:
    """one configuration: .kinfu (kinfu_statement.Params), every key of DEFAULTS as an attribute"""

    def __init__(self, name):
        self.name = name
        self.kinfu = K.Params(**KINFU)
        self.values = dict(DEFAULTS, **CASES[name])
        for k, v in self.values.items():
            setattr(self, k if k != "lambda" else "lambda_", v)
        self.frames = FRAMES
        self.k = self.warp_knn  # Warpfield::setKnn: the warp, the solve's graphs, the fusion and the growth all read it

    @property
    def one_pass(self):
        """CombinedSolver::solveAll with earlyOut (DynFusion's constructor sets it): a single outer pass"""
        return min(1, self.solver_numIter)


def depths_of(name):
    p = K.Params(**KINFU)
    return [NC.render(float(p.intr[0]), float(p.intr[1]), *NC.pose_at(i)) for i in range(FRAMES)]


def _g(v):
    return "%.9g" % float(np.float32(v))  # nine digits carry a float32 exactly


def _fmt(v):
    if isinstance(v, (tuple, list)):
        return " ".join(_fmt(x) for x in v)
    return "%d" % v if isinstance(v, (int, np.integer)) else _g(v)


def params_text(c):
    p = c.kinfu
    lines = ["cols %d" % p.cols, "rows %d" % p.rows, "intr " + _fmt(p.intr), "volume_dims %d %d %d" % tuple(p.volume_dims),
             "volume_size " + _fmt(p.volume_size), "volume_pose " + _fmt(list(p.volume_pose)),
             "bilateral %s %s %d" % (_g(p.bilateral_sigma_depth), _g(p.bilateral_sigma_spatial), p.bilateral_kernel_size),
             "icp_truncate_depth_dist " + _g(p.icp_truncate_depth_dist), "tsdf_trunc_dist " + _g(p.tsdf_trunc_dist),
             "tsdf_max_weight %d" % p.tsdf_max_weight, "gradient_delta_factor " + _g(p.gradient_delta_factor), "frames %d" % c.frames]
    lines += ["%s %s" % (k, _fmt(v)) for k, v in c.values.items()]
    return "\n".join(lines) + "\n"


def write_case(name, directory):
    c = Case(name)
    with open(os.path.join(directory, "params.txt"), "w") as f:
        f.write(params_text(c))
    for i, d in enumerate(depths_of(name)):
        assert d.dtype == np.uint16 and d.shape == (c.kinfu.rows, c.kinfu.cols)
        d.tofile(os.path.join(directory, "depth_%d.bin" % i))
    return c


def read_derived(directory):
    """what the constructor derived from the parameters -> (trunc, voxel size (3,), max_weight)"""
    d = open(os.path.join(directory, "derived.txt")).read().split()
    return np.float32(d[0]), np.array(d[1:4], np.float32), int(d[4])


def link_records(recs):
    """what frame i + 1's statement needs of frame i - 1, carried in frame i's record: the node count and the transforms the
    frame started from (none before frame 0)"""
    for i, r in enumerate(recs):
        prev = recs[i - 1] if i else None
        r["prev_D"] = prev["D"] if prev else 0
        r["prev_node_dq"] = prev["node_dq"] if prev else np.zeros((0, 8), np.float32)
    return recs


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
                 initial_cost=float(st["initial_cost"][0]), final_cost=float(st["final_cost"][0]),
                 knn_field_nodes=int(st["knn_field_nodes"][0]), knn_field_k=int(st["knn_field_k"][0]), warp_graph_searches=int(st["warp_graph_searches"][0]))
        raw = lambda name, dtype: np.fromfile(f(name + ".bin"), dtype)
        img = lambda name, dtype: (lambda a: a.reshape(p.rows, p.cols) if a.size else a)(raw(name, dtype))
        vol = lambda name: (lambda a: a.reshape(Z, Y, X) if a.size else a)(raw(name, np.uint32))
        r.update(dists=img("dists", np.uint16), depth0=img("depth0", np.uint16), live_volume=vol("live_volume"),
                 node_pos=raw("node_pos", np.float32).reshape(-1, 3), node_w=raw("node_w", np.float32),
                 node_dq=raw("node_dq", np.float32).reshape(-1, 8), canonical_volume=vol("canonical_volume"))
        for cloud in ("live", "warped", "corresponding", "canonical"):
            r[cloud + "_v"] = raw(cloud + "_v", np.float32).reshape(-1, 3)
            r[cloud + "_n"] = raw(cloud + "_n", np.float32).reshape(-1, 3)
            assert len(r[cloud + "_v"]) == len(r[cloud + "_n"])
        assert r["D"] == len(r["node_pos"]) == len(r["node_w"]) == len(r["node_dq"])
        recs.append(r)
    return link_records(recs)


bits, same = NC.bits, NC.same
