"""Inputs of the regularisation-hierarchy tests (tests/reg_hierarchy_statement.py): node sets, and for the two that are
solved a whole scene — canonical vertices with normals and analytic live maps.  Everything is in the camera frame."""
import numpy as np

EPS = 0.05


# ------------------------------------------------------------------------------------------------------------- strip
STRIP_COLS = 48
STRIP_Z = 1.013
STRIP_INTR = (100.0, 100.0, 8.0, 6.0)  # fx, fy, cx, cy
STRIP_IMAGE = (16, 256)                # rows, cols: x up to 2.4 m at z = 1 lands below column 250
STRIP_SHIFT = 0.005                    # the live surface: the strip moved 5 mm along its normal (towards the camera)
STRIP_DATA_END = 0.2                   # vertices with x below this keep their data rows


def strip_nodes():
    """96 nodes in two rows of 48, spacing EPS, 0.013 / 0.02 off the lattice: node 2 i + j at column i, row j"""
    i, j = np.meshgrid(np.arange(STRIP_COLS), np.arange(2), indexing="ij")
    return np.stack([0.013 + EPS * i.ravel(), 0.02 + EPS * j.ravel(), np.full(i.size, STRIP_Z)], 1).astype(np.float32)


def strip_scene():
    """the strip as a solve: vertices on a lattice of EPS / 2 over the nodes' extent, normals towards the camera, live maps
    of the plane z = STRIP_Z - STRIP_SHIFT, and the mask of the data end"""
    nodes = strip_nodes()
    xs = np.arange(0.0, 0.013 + EPS * (STRIP_COLS - 1) + 0.0131, EPS / 2)
    ys = np.arange(0.0, 0.02 + EPS + 0.0201, EPS / 2)
    x, y = np.meshgrid(xs, ys, indexing="ij")
    verts = np.stack([x.ravel(), y.ravel(), np.full(x.size, STRIP_Z)], 1).astype(np.float32)
    normals = np.tile(np.float32([0, 0, -1]), (len(verts), 1))
    vmap, nmap = plane_maps(STRIP_Z - STRIP_SHIFT, STRIP_INTR, STRIP_IMAGE)
    D = len(nodes)
    dq = np.zeros((D, 8), np.float32)
    dq[:, 0] = 1
    return dict(nodes=nodes, dq=dq, w=np.full(D, 3 * EPS, np.float32), verts=verts, normals=normals, vmap=vmap, nmap=nmap,
                intr=STRIP_INTR, mask=(verts[:, 0] < STRIP_DATA_END).astype(np.uint8))


def plane_maps(z, intr, image):
    fx, fy, cx, cy = intr
    rows, cols = image
    u, v = np.meshgrid(np.arange(cols), np.arange(rows))
    vmap = np.zeros((rows, cols, 4), np.float32)
    vmap[..., 0], vmap[..., 1], vmap[..., 2] = (u - cx) / fx * z, (v - cy) / fy * z, z
    nmap = np.zeros_like(vmap)
    nmap[..., 2] = -1
    return vmap, nmap


def knn_numpy(node_pos, query, k):
    """exhaustive float64 k-NN, ties to the lower index, -1 padded (the statement's data graph)"""
    p, q = np.asarray(node_pos, np.float64), np.asarray(query, np.float64)
    d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(2)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    out = np.full((len(q), k), -1, np.int32)
    out[:, :order.shape[1]] = order
    return out


# ------------------------------------------------------------------------------------------------------------ sphere
SPHERE_R = 0.6
SPHERE_C = np.array([0.11, -0.07, 1.5])
SPHERE_INTR = (120.0, 120.0, 79.5, 59.5)
SPHERE_IMAGE = (120, 160)


def _fibonacci(n):
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    ang = np.pi * (3 - np.sqrt(5)) * i
    return np.stack([np.sqrt(1 - z * z) * np.cos(ang), np.sqrt(1 - z * z) * np.sin(ang), z], 1)


def sphere_nodes():
    """a sphere of 0.6 m centred off the origin — x and y of both signs —, 60 000 points voxel-filtered at EPS (the first
    point of every cell stays): a few thousand nodes, table collisions, negative floor division"""
    pts = (SPHERE_C + SPHERE_R * _fibonacci(60000)).astype(np.float32)
    cell = np.floor((pts - np.float32(0.017)) / np.float32(EPS)).astype(np.int64)
    _, first = np.unique(cell, axis=0, return_index=True)
    return pts[np.sort(first)]


def sphere_scene():
    """the sphere as a solve: 12 000 vertices with outward normals, live maps of the same sphere moved by 4 mm"""
    nodes = sphere_nodes()
    d = _fibonacci(12000)
    verts = (SPHERE_C + SPHERE_R * d).astype(np.float32)
    normals = d.astype(np.float32)
    vmap, nmap = sphere_maps(SPHERE_C + np.array([0.003, -0.002, 0.002]), SPHERE_R, SPHERE_INTR, SPHERE_IMAGE)
    D = len(nodes)
    dq = np.zeros((D, 8), np.float32)
    dq[:, 0] = 1
    return dict(nodes=nodes, dq=dq, w=np.full(D, 3 * EPS, np.float32), verts=verts, normals=normals, vmap=vmap, nmap=nmap,
                intr=SPHERE_INTR)


def sphere_maps(c, r, intr, image):
    fx, fy, cx, cy = intr
    rows, cols = image
    u, v = np.meshgrid(np.arange(cols), np.arange(rows))
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, float)], -1)
    a = (ray * ray).sum(-1)
    b = ray @ c
    disc = b * b - a * (c @ c - r * r)
    t = (b - np.sqrt(np.maximum(disc, 0))) / a
    hit = disc > 0
    p = ray * t[..., None]
    vmap = np.full((rows, cols, 4), np.nan, np.float32)
    nmap = np.full((rows, cols, 4), np.nan, np.float32)
    vmap[hit, :3], vmap[hit, 3] = p[hit], 0
    nmap[hit, :3], nmap[hit, 3] = (p[hit] - c) / r, 0
    return vmap, nmap


# --------------------------------------------------------------------------------------------------------- node sets
def node_sets():
    """name -> (D, 3) float32"""
    s = sphere_nodes()
    two = np.float32([[0.31, -0.42, 0.9], [0.31, -0.42, 0.9], [0.36, -0.42, 0.9], [-0.2, 0.1, 1.1], [0.29, -0.40, 0.92]])
    nan = strip_nodes()[:24].copy()
    nan[5] = np.nan
    return {"strip": strip_nodes(), "sphere": s, "D0": np.zeros((0, 3), np.float32), "D1": s[:1].copy(), "D2": s[:2].copy(),
            "coincident": two, "nan": nan}


# (k, slots) the rows are checked with, for BETAS x levels 1 .. 4: the first `levels` of the slots, a fourth level taking none
CONFIGS = [(4, (2, 1, 1)), (8, (4, 2, 2))]
BETAS = (2, 4)


def slots_for(slots, levels):
    return (tuple(slots) + (0,) * 8)[:levels]
