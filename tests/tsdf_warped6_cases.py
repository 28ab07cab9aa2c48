"""The cases of the north-star warped-integrate tests (dfa_tsdf_integrate_warped6), shared by the CPU statement tests and the
-m gpu tests.  Scene, nodes and starting volumes are tsdf_warped_cases' (scene, node_set, start_volume); what is new is the
frame set-up — the nodes of the north-star warp field live in a frame of their own:

  "volume"  both transforms absent (NULL): the volume frame is the node frame and the camera frame.  The volume sits in the
            positive octant, so the camera is at its corner looking along +z, with intrinsics that put the volume in view and a
            depth frame of its own (the same sphere in front of a wall);
  "posed"   vol2node is a rotation of 0.3 rad about a skew axis plus a translation of the order of a volume edge; nodes and node
            transforms are given in that frame; node2cam = vol2cam . vol2node^-1 with the scene's vol2cam: the camera has not moved;
  "moved"   as "posed", with node2cam another rigid motion (a further 0.05 rad and 0.03 edges): the camera has moved since
            frame 0.

The matrix holds tsdf_warped_cases' four volumes ((32, 32, 32), (50, 38, 44), (9, 7, 14), (1, 2, 12): see there why), the
(D, k) pairs (300, 8), (63, 4), (2, 8), (1024, 8), (0, 8), (64, 3) — k <= 8 here; the last is k <= 4 with the node grid, which
starts at D = 64 —, identity and general node transforms, both modes, an
empty and a junk starting volume.  "antipodal" is "main_posed_rigid_junk" with every second node's dual quaternion negated:
q and -q are the same motion, and the statement's volume must be the same, exactly.
"""
import functools

import numpy as np

import tsdf_statement as TS
import tsdf_warped6_statement as W6
import tsdf_warped_cases as CS

MAX_WEIGHT = CS.MAX_WEIGHT
INTR_VOLUME = (40.0, 40.0, 0.19, -9.57)  # "volume": the volume's centre (x / z = y / z = 1) lands at (40.19, 30.43) of 80 x 60

#        name                      (X, Y, Z)     D    k  transforms  mode      start    frame
CASES = {
    "main_volume_skip":       ((32, 32, 32),  300, 8, "general",  W6.SKIP,  "empty", "volume"),
    "main_posed_rigid_junk":  ((32, 32, 32),  300, 8, "general",  W6.RIGID, "junk",  "posed"),
    "odd_scan_moved":         ((50, 38, 44),   63, 4, "general",  W6.SKIP,  "junk",  "moved"),
    "odd_grid_rigid_posed":   ((50, 38, 44),  300, 8, "identity", W6.RIGID, "empty", "posed"),
    "big_moved":              ((32, 32, 32), 1024, 8, "general",  W6.SKIP,  "junk",  "moved"),
    "padded":                 ((9, 7, 14),      2, 8, "general",  W6.RIGID, "junk",  "posed"),
    "thin":                   ((1, 2, 12),     63, 4, "identity", W6.SKIP,  "junk",  "volume"),
    "thin_padded":            ((1, 2, 12),      2, 8, "general",  W6.RIGID, "empty", "moved"),
    "no_nodes_skip":          ((9, 7, 14),      0, 8, "identity", W6.SKIP,  "junk",  "posed"),
    "no_nodes_rigid":         ((32, 32, 32),    0, 8, "identity", W6.RIGID, "junk",  "posed"),
    "antipodal":              ((32, 32, 32),  300, 8, "general",  W6.RIGID, "junk",  "posed"),
    "tiny_k3_grid_moved":     ((9, 7, 14),     64, 3, "general",  W6.SKIP,  "junk",  "moved"),
}
MAIN = ("main_volume_skip", "main_posed_rigid_junk", "odd_scan_moved", "odd_grid_rigid_posed", "big_moved")
ANTIPODAL_OF = {"antipodal": "main_posed_rigid_junk"}


def rigid(axis, angle, t):
    """12 floats (R row-major, t) of the rotation by `angle` about `axis` followed by the translation t, float32"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return np.concatenate([R.reshape(-1), np.asarray(t, np.float64)]).astype(np.float32)


def volume_dists(sc):
    """the depth frame of the "volume" set-up: camera at the volume's corner, axes the volume's; the scene's sphere, else a wall
    at 0.9 edges; ~5 % of the texels zero"""
    rng = np.random.default_rng(int(sc["edge"] * 1e6) % 9973)
    fx, fy, cx, cy = INTR_VOLUME
    u, v = np.meshgrid(np.arange(CS.COLS), np.arange(CS.ROWS))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, float)], -1)
    s = sc["centre"]
    A, B, C = (d * d).sum(-1), -2 * (d @ s), s @ s - sc["radius"] ** 2
    disc = B * B - 4 * A * C
    with np.errstate(invalid="ignore"):
        zs = (-B - np.sqrt(disc)) / (2 * A)
    depth = np.where(disc > 0, zs, 0.9 * sc["edge"])
    depth_mm = np.round(depth * 1000).astype(np.uint16)
    depth_mm[rng.random(depth_mm.shape) < 0.05] = 0
    return TS.compute_dists(depth_mm, *INTR_VOLUME)


def frames(sc, frame):
    """(vol2node, node2cam, dists, intrinsics) of a set-up; the transforms 12 float32 each or None"""
    if frame == "volume":
        return None, None, volume_dists(sc), INTR_VOLUME
    e = sc["edge"]
    vol2node = rigid([0.3, -0.5, 0.81], 0.3, [0.9 * e, -0.6 * e, 1.1 * e])
    node2cam = W6.compose(sc["vol2cam"], W6.invert(vol2node))
    if frame == "moved":
        node2cam = W6.compose(rigid([-0.7, 0.2, 0.4], 0.05, [0.03 * e, -0.02 * e, 0.025 * e]), node2cam)
    return vol2node, node2cam, sc["dists"], CS.INTR


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs and the statement's answer of one case (computed once per process; treat as read-only)"""
    dims, D, k, transforms, mode, start, frame = CASES[name]
    seed = sorted(CASES).index(ANTIPODAL_OF.get(name, name))
    sc = CS.scene(dims, 400 + seed)
    vol2node, node2cam, dists, intr = frames(sc, frame)
    pos, dq, w = CS.node_set(sc, D, transforms, 500 + seed)  # positions in the volume's frame ...
    if vol2node is not None and D:
        pos = W6.apply64(vol2node, pos.astype(np.float64)).astype(np.float32)  # ... taken to the node frame; the transforms act there
    if name in ANTIPODAL_OF:
        dq = dq.copy()
        dq[1::2] = -dq[1::2]
    vol = CS.start_volume(dims, start, 600 + seed)
    ref = W6.integrate(vol, dists, sc["voxel_size"], sc["trunc"], MAX_WEIGHT, vol2node, node2cam, *intr, pos, dq, w, k, mode)
    for a in (vol, pos, dq, w, dists, vol2node, node2cam, *ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    sc = dict(sc, dists=dists)
    return dict(name=name, dims=dims, D=D, k=k, mode=mode, frame=frame, vol=vol, nodes=pos, node_dq=dq, node_w=w, ref=ref,
                vol2node=vol2node, node2cam=node2cam, intr=intr, **sc)


def measured_deviation(name):
    """tsdf_warped6_statement.deviation on the inputs of one case"""
    c = case(name)
    return W6.deviation(c["vol"].shape, c["voxel_size"], c["vol2node"], c["node2cam"], c["nodes"], c["node_dq"], c["node_w"], c["k"],
                        c["mode"])
