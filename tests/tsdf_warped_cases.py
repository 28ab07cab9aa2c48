"""The cases of the warped-integrate tests, shared by the CPU statement tests and the -m gpu tests: a sphere in front of a
back wall seen by a camera tilted about y, deformation nodes on the sphere, and the statement's answer computed once per case.

Between them the cases hold four volumes, seven (D, k) pairs, identity and general node transforms, both
modes, an empty and a junk starting volume.  The shapes are small on purpose: the odd volumes exercise partial bricks in
x and y ((50, 38, 44): no multiple of the 64 x 4 x 1 brick; (9, 7, 14) and (1, 2, 12): less than one brick wide), (32, 32, 32)
and (50, 38, 44) have several bricks in y and z, D = 63 takes the scan of all nodes and D >= 64 the node grid, D = 2 < k gives
padded lists.  The two "tiny" cases close the list of kernel instantiations: k <= 4 with the node grid (D = 64, the first
size that takes it) and k = 16 with the scan.  case() seeds a case by its place in sorted(CASES): a new name has to sort
after the last one, or every case behind it silently gets other inputs.
"""
import functools

import numpy as np

import tsdf_statement as TS
import tsdf_warped_statement as WST
import warp_statement as WS

MAX_WEIGHT = 64
COLS, ROWS, F = 80, 60, 70.0
INTR = (F, F, COLS / 2.0 - 0.31, ROWS / 2.0 + 0.43)  # fx, fy, cx, cy
TILT = 0.15  # rad about y

#        name                 (X, Y, Z)     D     k  transforms  mode       start
CASES = {
    "main_skip":        ((32, 32, 32),  300,  8, "general",  WST.SKIP,  "empty"),
    "main_rigid_junk":  ((32, 32, 32),  300,  8, "general",  WST.RIGID, "junk"),
    "odd_scan":         ((50, 38, 44),   63,  4, "general",  WST.SKIP,  "junk"),
    "odd_grid_rigid":   ((50, 38, 44),  300,  8, "identity", WST.RIGID, "empty"),
    "k16":              ((32, 32, 32), 1024, 16, "general",  WST.SKIP,  "junk"),
    "padded":           ((9, 7, 14),      2,  8, "general",  WST.RIGID, "junk"),
    "thin":             ((1, 2, 12),     63,  4, "identity", WST.SKIP,  "junk"),
    "thin_padded":      ((1, 2, 12),      2,  8, "general",  WST.SKIP,  "empty"),
    "no_nodes_skip":    ((9, 7, 14),      0,  8, "identity", WST.SKIP,  "junk"),
    "no_nodes_rigid":   ((32, 32, 32),    0,  8, "identity", WST.RIGID, "junk"),
    "tiny_k4_grid":     ((9, 7, 14),     64,  4, "general",  WST.RIGID, "junk"),
    "tiny_k16_scan":    ((9, 7, 14),     63, 16, "general",  WST.SKIP,  "junk"),
}
MAIN = ("main_skip", "main_rigid_junk", "odd_scan", "odd_grid_rigid", "k16")  # the cases of the vacuity guard


def scene(dims, seed):
    """volume geometry, camera and the depth frame: dict with voxel_size, trunc, vol2cam (12 floats), dists (uint16 halves),
    centre and radius of the sphere (volume frame, metres)"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    voxel = np.float32(1.0 / max(dims) if max(dims) >= 32 else 0.07)
    vs = np.array([voxel] * 3, np.float32)
    size = vs.astype(np.float64) * np.array(dims)
    edge = float(size.max())
    centre = size / 2
    radius = 0.3 * edge
    trunc = np.float32(3 * voxel)
    # camera 1.3 edges in front of the volume centre, looking along +z, tilted about y.  Off the centre in y, and a principal
    # point off the texel corners: with either on the voxel grid a whole plane of unwarped voxels projects EXACTLY onto a texel
    # boundary (vc.y = 0, coo.y = cy), and 3 % of a RIGID case is undecided by construction
    cth, sth = np.cos(TILT), np.sin(TILT)
    R = np.array([[cth, 0, sth], [0, 1, 0], [-sth, 0, cth]])
    cam = centre + np.array([0.25 * edge, 0.0617 * edge, -1.3 * edge])
    vol2cam = np.concatenate([R.reshape(-1), -R @ cam]).astype(np.float32)
    # depth: the sphere, else a wall at constant camera depth behind it; ~5 % of the texels zero
    fx, fy, cx, cy = INTR
    u, v = np.meshgrid(np.arange(COLS), np.arange(ROWS))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, float)], -1)
    sc = R @ (centre - cam)
    A, B, C = (d * d).sum(-1), -2 * (d @ sc), sc @ sc - radius * radius
    disc = B * B - 4 * A * C
    with np.errstate(invalid="ignore"):
        zs = (-B - np.sqrt(disc)) / (2 * A)
    depth = np.where(disc > 0, zs, 1.3 * edge + 0.45 * edge)
    depth_mm = np.round(depth * 1000).astype(np.uint16)
    depth_mm[rng.random(depth_mm.shape) < 0.05] = 0
    dists = TS.compute_dists(depth_mm, *INTR)
    return dict(voxel_size=vs, trunc=trunc, vol2cam=vol2cam, dists=dists, centre=centre, radius=radius, edge=edge)


def node_set(sc, D, transforms, seed):
    """D nodes on the sphere with radii of 0.1 .. 0.25 volume edges: (pos (D, 3), dq (D, 8), w (D,)) float32"""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((D, 3))
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-9)
    pos = (sc["centre"] + sc["radius"] * n).astype(np.float32)
    w = (rng.uniform(0.1, 0.25, D) * sc["edge"]).astype(np.float32)
    if transforms == "identity":
        dq = np.tile(WS.IDENTITY, (D, 1)).astype(np.float32)
    else:
        dq = WS.dq_from_euler(*rng.uniform(-0.1, 0.1, (3, D)), *rng.uniform(-0.03, 0.03, (3, D))).astype(np.float32)
    return pos, dq.reshape(D, 8), w


def start_volume(dims, start, seed):
    X, Y, Z = dims
    if start == "empty":
        return np.zeros((Z, Y, X), np.uint32)
    rng = np.random.default_rng(seed)
    halves = rng.uniform(-1, 1, (Z, Y, X)).astype(np.float16).view(np.uint16).astype(np.uint32)
    weights = rng.choice(np.array([0, 1, 2, 17, MAX_WEIGHT - 1, MAX_WEIGHT], np.uint32), (Z, Y, X))
    return (halves | (weights << 16)).astype(np.uint32)  # (weight 0 with any distance is a valid voxel too)


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs and the statement's answer of one case (computed once per process; treat as read-only)"""
    dims, D, k, transforms, mode, start = CASES[name]
    seed = sorted(CASES).index(name)
    sc = scene(dims, 100 + seed)
    pos, dq, w = node_set(sc, D, transforms, 200 + seed)
    vol = start_volume(dims, start, 300 + seed)
    ref = WST.integrate(vol, sc["dists"], sc["voxel_size"], sc["trunc"], MAX_WEIGHT, sc["vol2cam"], *INTR, pos, dq, w, k, mode)
    for a in (vol, pos, dq, w, sc["dists"], *ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return dict(name=name, dims=dims, D=D, k=k, mode=mode, vol=vol, nodes=pos, node_dq=dq, node_w=w, ref=ref, **sc)
