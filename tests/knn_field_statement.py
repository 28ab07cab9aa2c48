"""The statement of the k-NN field (dfa_knn_field_*, include/dynfu_amd.h) in numpy, for the reference-mode cases of
tests/tsdf_warped_cases.py (vol2node absent: the search position of a voxel is v = (x, y, z) * voxel_size), the north-star cases
of tests/tsdf_warped6_cases.py and the field's own cases of tests/knn_field_cases.py (with a vol2node the search position is
c = R_n v + t_n).

  * bricks are 64 x 4 x 1 voxels; the box of a brick spans the positions of its first and last voxel INSIDE the volume;
  * WITHOUT a frame a brick MUST be stored when the distance from its box to some node is below that node's own radius — fp64
    arithmetic on the float32 positions (must_store).  WITH a frame a brick must be stored when it holds a voxel (inside the
    volume) with |c32 - g_m| < w_m for some node m, evaluated as warp_statement.unsupported_flags evaluates the support rule: the
    fp64 root of the float32 differences, rounded to float32, compared in float32 — "the stored bricks hold every supported
    voxel", per voxel and exact.  The same voxel rule without a frame is a subset of the box rule (the CPU tests assert it);
  * a brick MAY be stored only when its box — fp64, volume frame — lies within 1.002 w_m + 2e-6 L_m of some node m taken back to
    the volume's frame by the fp64 inverse of vol2node: twice the widening csrc/warped_mark_device.hpp states (1e-3 relative plus
    1e-6 L), L_m the sum mark_radius_framed states (2 ext + max|g_node| + max|g_vol| + max|t|; without a frame max(ext, max|g|)).
    The exception is a NaN radius, which may and must store every brick (knn_field.hip, field_mark_kernel);
  * the row of every voxel of a stored brick is warp_statement.knn(nodes, c32, k): ascending by (float32 squared distance,
    index), -1 padded when D < k.  A voxel of a brick that is not stored has a row of -1.

c32 = tsdf_warped6_statement.apply32(vol2node, v) is the fused dot and then + t, as to_node_frame (csrc/knn_field_device.hpp)
writes it.  Without a frame c32 is v, which every kernel forms by one float32 product per axis: the rows are exact, ties included,
everywhere.  The same holds for a frame whose R has entries 0 and +-1 only and whose c32 equals the fp64 product c64 at every voxel
(exact_frame; "ties_lattice_posed"): each sum has one non-zero term and nothing is rounded in any order of evaluation.  For every
other frame the numpy emulation of the fused dot is not proven equal to the device's bits, so a voxel is DECIDED only when the
k + 1 smallest fp64 distances at c64 (all of them when D <= k) are pairwise more than 2 rho apart, and AMBIGUOUS otherwise:

  rho = 2 max |d32 - d64| over all (voxel, node) pairs of the case — d32 the root of the float32 dist2 at c32, d64 the fp64
  distance at c64 —, measured, not chosen; the factor 2 is the project's margin for another instruction order
  (warp_statement.KERNEL_BOUND = 2 ORACLE_DEVIATION).

At a decided voxel of a stored brick the device's row is the float32 statement's, id for id.  At an ambiguous voxel the row must
be VALID: min(k, D) distinct ids of [0, D), then -1; their fp64 distances ascend up to 2 rho; no node outside the row is nearer
than the row's last by more than 2 rho.  At most AMBIGUOUS_CAP of a case's voxels may be ambiguous (raster_cases' cap).

FIELD_DEVIATION holds max |d32 - d64| per framed case as measured on the CPU (WARPED6_DEVIATION's counterpart, per case and in
metres: the cases' coordinates differ by a factor of five); tests/test_knn_field_statement_cpu.py measures it again on every run
and fails above the constant.
"""
import functools

import numpy as np

import knn_field_cases as KC
import tsdf_warped6_cases as C6
import tsdf_warped6_statement as W6
import tsdf_warped_cases as CS
import tsdf_warped_statement as WST
import warp_statement as WS

BRICK = (64, 4, 1)  # x, y, z
AMBIGUOUS_CAP = 0.02

# largest |d32 - d64| in metres per framed case with nodes, measured on the CPU (the measured value, and the largest |coordinate|
# in play, beside each).  A prefix of a case's nodes deviates no more than the whole case.
FIELD_DEVIATION = {
    ("six", "main_posed_rigid_junk"): 2.4e-7,   # measured 2.364e-07, coordinates up to 2.28
    ("six", "odd_scan_moved"): 2.2e-7,          # measured 2.145e-07, 2.16
    ("six", "odd_grid_rigid_posed"): 2.4e-7,    # measured 2.321e-07, 2.16
    ("six", "big_moved"): 2.4e-7,               # measured 2.362e-07, 2.28
    ("six", "padded"): 1.8e-7,                  # measured 1.713e-07, 2.09
    ("six", "thin_padded"): 8.0e-8,             # measured 7.962e-08, 1.69
    ("six", "antipodal"): 2.4e-7,               # measured 2.364e-07, 2.28
    ("six", "tiny_k3_grid_moved"): 1.9e-7,      # measured 1.849e-07, 2.09
    ("field", "ties_lattice_posed"): 0.0,       # exact: a quarter turn and whole voxels of 1/64
    ("field", "radii_posed"): 9.6e-7,           # measured 9.586e-07, 11.3 (the node ten edges outside the volume)
    ("field", "radii_nan_posed"): 9.6e-7,       # the same positions
    ("field", "turned"): 3.9e-7,                # measured 3.898e-07, 6.58
}


def brick_grid(dims):
    """bricks along (x, y, z)"""
    return tuple((d + b - 1) // b for d, b in zip(dims, BRICK))


def brick_of_voxels(dims):
    """(Z, Y, X) int: the index of every voxel's brick, x fastest: (bz nby + by) nbx + bx"""
    X, Y, Z = dims
    nbx, nby, _ = brick_grid(dims)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return ((z // BRICK[2]) * nby + y // BRICK[1]) * nbx + x // BRICK[0]


def brick_boxes(dims, voxel_size):
    """per axis (lo, hi), each (bricks along the axis,) fp64: the positions of a brick's first and last voxel inside the volume"""
    nb = brick_grid(dims)
    vs = np.asarray(voxel_size, np.float32)
    out = []
    for c in range(3):
        first = np.arange(nb[c]) * BRICK[c]
        last = np.minimum(first + BRICK[c] - 1, dims[c] - 1)
        a, b = (first.astype(np.float32) * vs[c]).astype(np.float64), (last.astype(np.float32) * vs[c]).astype(np.float64)
        out.append((np.minimum(a, b), np.maximum(a, b)))
    return out


def box_distances(dims, voxel_size, g):
    """(D, bricks) fp64: the distance from every brick's box to every point of g (D, 3), volume frame; bricks flat in the order
    of brick_of_voxels"""
    box = brick_boxes(dims, voxel_size)
    d = [np.maximum(np.maximum(box[c][0][None, :] - g[:, c:c + 1], g[:, c:c + 1] - box[c][1][None, :]), 0.0) for c in range(3)]
    d2 = d[2][:, :, None, None] ** 2 + d[1][:, None, :, None] ** 2 + d[0][:, None, None, :] ** 2  # (D, nbz, nby, nbx)
    return np.sqrt(d2).reshape(len(g), -1)


def exact_frame(vol2node, c32, c64):
    """no frame, or one that no order of evaluation rounds: entries of R in {0, 1, -1} and c32 == c64 at every voxel"""
    if vol2node is None:
        return True
    R = np.asarray(vol2node, np.float32)[:9]
    return bool(np.isin(R, (0.0, 1.0, -1.0)).all() and np.array_equal(c32.astype(np.float64), c64))


def positions(dims, voxel_size, vol2node=None):
    """(v, c32 float32, c64 fp64), each (n, 3) in the volume's memory order"""
    X, Y, Z = dims
    v = WST.voxel_positions((Z, Y, X), voxel_size)
    return v, W6.apply32(vol2node, v), W6.apply64(vol2node, v.astype(np.float64))


def nodes_in_volume_frame(nodes, vol2node):
    """(D, 3) fp64: the nodes taken back by the fp64 inverse of vol2node"""
    g = np.asarray(nodes, np.float32).reshape(-1, 3).astype(np.float64)
    if vol2node is None:
        return g
    a = np.asarray(vol2node, np.float32).astype(np.float64)
    return (g - a[9:12]) @ np.linalg.inv(a[:9].reshape(3, 3)).T


def must_store(dims, voxel_size, nodes, node_w, vol2node=None):
    """bool per brick (flat, the order of brick_of_voxels).  Without a frame: some node's own radius reaches the brick's box.
    With one: the brick holds a voxel that some node supports (pairs()["must_voxel"])"""
    nodes = np.asarray(nodes, np.float32).reshape(-1, 3)
    w = np.asarray(node_w, np.float32).reshape(-1)
    nb = brick_grid(dims)
    if len(nodes) == 0:
        return np.zeros(nb[2] * nb[1] * nb[0], bool)
    if vol2node is not None:
        return pairs(dims, voxel_size, nodes, w, 1, vol2node)["must_voxel"]
    with np.errstate(invalid="ignore"):
        return (box_distances(dims, voxel_size, nodes.astype(np.float64)) < w.astype(np.float64)[:, None]).any(0)


def may_store(dims, voxel_size, nodes, node_w, vol2node=None):
    """bool per brick: the upper bound of the stored set (every brick when a radius is NaN)"""
    nodes = np.asarray(nodes, np.float32).reshape(-1, 3)
    w = np.asarray(node_w, np.float32).reshape(-1).astype(np.float64)
    nb = brick_grid(dims)
    if len(nodes) == 0:
        return np.zeros(nb[2] * nb[1] * nb[0], bool)
    if np.isnan(w).any():
        return np.ones(nb[2] * nb[1] * nb[0], bool)
    gv = nodes_in_volume_frame(nodes, vol2node)
    ext = float((np.abs(np.asarray(voxel_size, np.float32).astype(np.float64)) * np.array(dims)).max())
    if vol2node is None:
        L = np.maximum(ext, np.abs(gv).max(1))
    else:
        tmax = float(np.abs(np.asarray(vol2node, np.float32)[9:12].astype(np.float64)).max())
        L = 2 * ext + np.abs(nodes.astype(np.float64)).max(1) + np.abs(gv).max(1) + tmax
    return (box_distances(dims, voxel_size, gv) <= (1.002 * w + 2e-6 * L)[:, None]).any(0)


def rows(dims, voxel_size, nodes, k, vol2node=None):
    """(Z, Y, X, k) int32: warp_statement.knn at every voxel's search position"""
    X, Y, Z = dims
    return WS.knn(nodes, positions(dims, voxel_size, vol2node)[1], k).reshape(Z, Y, X, k)


def pairs(dims, voxel_size, nodes, node_w, k, vol2node=None, chunk=1024):
    """one pass over all (voxel, node) pairs -> dict: deviation (largest |d32 - d64|), gap ((n,) fp64: the smallest difference
    between two of the k + 1 smallest fp64 distances, inf with fewer than two), tie ((n,) bool: two of the k + 1 smallest float32
    squared distances are equal), must_voxel (bricks,) bool, scale (L_case)"""
    nodes = np.asarray(nodes, np.float32).reshape(-1, 3)
    w = np.asarray(node_w, np.float32).reshape(-1)
    _, c32, c64 = positions(dims, voxel_size, vol2node)
    n, D = len(c32), len(nodes)
    g64 = nodes.astype(np.float64)
    m = min(k + 1, D)
    gap, tie, sup, dev = np.full(n, np.inf), np.zeros(n, bool), np.zeros(n, bool), 0.0
    for s in range(0, n, chunk):
        q = c32[s:s + chunk]
        with np.errstate(all="ignore"):
            d = q[:, None, :] - nodes[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]  # warp_statement.knn's
            d32 = np.sqrt(d2.astype(np.float64))
            e = c64[s:s + chunk, None, :] - g64[None, :, :]
            d64 = np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2])
            dev = max(dev, float(np.abs(d32 - d64).max()))
            # the support rule of warp_statement.unsupported_flags, for every node
            dd = d.astype(np.float64)
            dist = np.sqrt(dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1] + dd[..., 2] * dd[..., 2]).astype(np.float32)
            sup[s:s + chunk] = (dist < w[None, :]).any(1)
        if m >= 2:
            near = np.sort(np.partition(d64, m - 1, 1)[:, :m], 1)
            gap[s:s + chunk] = np.diff(near, axis=1).min(1)
            near2 = np.sort(np.partition(d2, m - 1, 1)[:, :m], 1)
            tie[s:s + chunk] = (np.diff(near2, axis=1) == 0).any(1)
    nb = brick_grid(dims)
    must = np.zeros(nb[2] * nb[1] * nb[0], bool)
    must[np.unique(brick_of_voxels(dims).ravel()[sup])] = True
    scale = max(1.0, float(np.abs(c32).max()), float(np.abs(c64).max()), float(np.abs(nodes).max()))
    return dict(deviation=dev, gap=gap, tie=tie, must_voxel=must, scale=scale)


def inputs(name, kind="ref", k=None):
    """dict(dims, voxel_size, k, D, nodes, node_w, vol2node) of a case of tsdf_warped_cases ("ref"), tsdf_warped6_cases ("six") or
    knn_field_cases ("field", at one of its k values)"""
    if kind == "field":
        return KC.case(name, k)
    c = CS.case(name) if kind == "ref" else C6.case(name)
    return dict(name=name, dims=c["dims"], voxel_size=c["voxel_size"], k=c["k"], D=c["D"], nodes=c["nodes"], node_w=c["node_w"],
                vol2node=c.get("vol2node"))


@functools.lru_cache(maxsize=None)
def case_pairs(name, D=None, kind="ref", k=None):
    """pairs() on (the first D > 0 nodes of) a case, once per process"""
    c = inputs(name, kind, k)
    D = c["D"] if D is None else D
    return pairs(c["dims"], c["voxel_size"], c["nodes"][:D], c["node_w"][:D], c["k"], c["vol2node"])


@functools.lru_cache(maxsize=None)
def case(name, D=None, kind="ref", k=None):
    """the statement on (the first D nodes of) a case: dict(must, may (bricks,), rows (Z, Y, X, k), brick (Z, Y, X), ambiguous
    (Z, Y, X) bool, rho, deviation (max |d32 - d64|; with a frame), every_brick, framed, and the inputs nodes, node_w, c64, k, D);
    computed once per process, read-only.  The pass over all pairs is made for the cases with a frame only: without one nothing
    is ambiguous and the box rule needs no voxel"""
    c = inputs(name, kind, k)
    D = c["D"] if D is None else D
    X, Y, Z = c["dims"]
    nodes, w, k, vol2node = c["nodes"][:D], c["node_w"][:D], c["k"], c["vol2node"]
    _, c32, c64 = positions(c["dims"], c["voxel_size"], vol2node)
    ambiguous, rho, deviation = np.zeros(len(c32), bool), 0.0, 0.0
    must = must_store(c["dims"], c["voxel_size"], nodes if vol2node is None else nodes[:0], w)
    if vol2node is not None and D:
        p = case_pairs(name, D, kind, k)
        must, deviation = p["must_voxel"], p["deviation"]
        if not exact_frame(vol2node, c32, c64):
            rho = 2 * deviation
            ambiguous = p["gap"] <= 2 * rho
    out = dict(must=must, may=may_store(c["dims"], c["voxel_size"], nodes, w, vol2node), rows=WS.knn(nodes, c32, k).reshape(Z, Y, X, k),
               brick=brick_of_voxels(c["dims"]), ambiguous=ambiguous.reshape(Z, Y, X), c64=c64, nodes=np.asarray(nodes), node_w=np.asarray(w))
    for a in out.values():
        a.setflags(write=False)
    out.update(rho=rho, deviation=deviation, k=k, D=D, framed=vol2node is not None, every_brick=bool(D and np.isnan(w).any()), name=name)
    return out


def stored_bricks(got, s):
    """(bricks,) bool from looked-up rows (Z, Y, X, k): the bricks with a voxel that has a neighbour (D > 0: every voxel of a
    stored brick has one)"""
    stored = np.zeros(len(s["must"]), bool)
    stored[np.unique(s["brick"][got[..., 0] >= 0])] = True
    return stored


def check_stored(stored, s):
    """the stored set (bricks,) bool against the lower and the upper bound -> list of complaints (empty: none)"""
    bad = []
    if s["every_brick"] and not stored.all():
        bad.append("a NaN radius must store every brick: %d of %d are" % (int(stored.sum()), len(stored)))
    if (s["must"] & ~stored).any():
        bad.append("%d bricks that must be stored are not" % int((s["must"] & ~stored).sum()))
    if (stored & ~s["may"]).any():
        bad.append("%d stored bricks lie beyond the widened reach of every node" % int((stored & ~s["may"]).sum()))
    return bad


def check_rows(got, s, stored=None):
    """looked-up rows (Z, Y, X, k) against the statement s = case(...), on the voxels of the bricks `stored` (bricks,) bool
    (default: stored_bricks(got, s)) -> (list of complaints, number of ambiguous voxels whose row is valid and not the float32
    statement's)"""
    stored = stored_bricks(got, s) if stored is None else stored
    has = stored[s["brick"]]
    bad = []
    differ = (got != s["rows"]).any(-1) & has
    dec = differ & ~s["ambiguous"]
    if dec.any():
        z, y, x = (int(a[0]) for a in np.nonzero(dec))
        bad.append("%d decided voxels differ from the statement, first (x, y, z) = (%d, %d, %d): %s, statement %s" %
                   (int(dec.sum()), x, y, z, got[z, y, x].tolist(), s["rows"][z, y, x].tolist()))
    amb = np.flatnonzero((differ & s["ambiguous"]).ravel())
    if len(amb):
        k, D = s["k"], s["D"]
        r = got.reshape(-1, k)[amb]
        m = min(k, D)
        shape_ok = (r[:, :m] >= 0).all(1) & (r[:, :m] < D).all(1) & (r[:, m:] == -1).all(1)
        srt = np.sort(r[:, :m], 1)
        shape_ok &= (np.diff(srt, axis=1) > 0).all(1) if m > 1 else True
        j = np.clip(r[:, :m], 0, D - 1)
        e = s["c64"][amb][:, None, :] - s["nodes"].astype(np.float64)[None, :, :]
        d = np.sqrt((e * e).sum(-1))  # (n_amb, D)
        dr = np.take_along_axis(d, j, 1)
        ascend = (np.diff(dr, axis=1) >= -2 * s["rho"]).all(1) if m > 1 else np.ones(len(amb), bool)
        outside = np.ones_like(d, bool)
        np.put_along_axis(outside, j, False, 1)
        nearest_out = np.where(outside, d, np.inf).min(1)
        complete = nearest_out >= dr[:, -1] - 2 * s["rho"]
        ok = shape_ok & ascend & complete
        if not ok.all():
            bad.append("%d ambiguous voxels hold an invalid row, first (flat index %d): %s" %
                       (int((~ok).sum()), int(amb[~ok][0]), r[~ok][0].tolist()))
    if not (got[~has] == -1).all():
        bad.append("rows of voxels that are not stored must be -1")
    return bad, int(len(amb))
