"""The statement of the k-NN field (dfa_knn_field_*, include/dynfu_amd.h) in numpy, for the reference-mode cases of
tests/tsdf_warped_cases.py (vol2node absent: the search position of a voxel is v = (x, y, z) * voxel_size).

  * bricks are 64 x 4 x 1 voxels; the box of a brick spans the positions of its first and last voxel INSIDE the volume;
  * a brick MUST be stored when the distance from its box to some node is below that node's own radius — fp64 arithmetic on
    the float32 positions.  The library widens the radius (as the pre-pass of the warped sweeps does), so it may store more;
  * the row of every voxel of a stored brick is warp_statement.knn(nodes, v, k): ascending by (float32 squared distance,
    index), -1 padded when D < k — exact, ties included.  A voxel of a brick that is not stored has a row of -1.
"""
import functools

import numpy as np

import tsdf_warped_cases as CS
import tsdf_warped_statement as WST
import warp_statement as WS

BRICK = (64, 4, 1)  # x, y, z


def brick_grid(dims):
    """bricks along (x, y, z)"""
    return tuple((d + b - 1) // b for d, b in zip(dims, BRICK))


def brick_of_voxels(dims):
    """(Z, Y, X) int: the index of every voxel's brick, x fastest: (bz nby + by) nbx + bx"""
    X, Y, Z = dims
    nbx, nby, _ = brick_grid(dims)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return ((z // BRICK[2]) * nby + y // BRICK[1]) * nbx + x // BRICK[0]


def must_store(dims, voxel_size, nodes, node_w):
    """bool per brick (flat, the order of brick_of_voxels): some node's own radius reaches the brick's box"""
    nb = brick_grid(dims)
    vs = np.asarray(voxel_size, np.float32)
    lo, hi = [], []
    for c in range(3):
        first = np.arange(nb[c]) * BRICK[c]
        last = np.minimum(first + BRICK[c] - 1, dims[c] - 1)
        a, b = (first.astype(np.float32) * vs[c]).astype(np.float64), (last.astype(np.float32) * vs[c]).astype(np.float64)
        lo.append(np.minimum(a, b)), hi.append(np.maximum(a, b))
    out = np.zeros(nb[2] * nb[1] * nb[0], bool)
    g = np.asarray(nodes, np.float32).reshape(-1, 3).astype(np.float64)
    w = np.asarray(node_w, np.float32).reshape(-1).astype(np.float64)
    if len(g) == 0:
        return out
    d = [np.maximum(np.maximum(lo[c][None, :] - g[:, c:c + 1], g[:, c:c + 1] - hi[c][None, :]), 0.0) for c in range(3)]  # (D, nb_c)
    d2 = d[2][:, :, None, None] ** 2 + d[1][:, None, :, None] ** 2 + d[0][:, None, None, :] ** 2  # (D, nbz, nby, nbx)
    return (np.sqrt(d2) < w[:, None, None, None]).any(0).ravel()


def rows(dims, voxel_size, nodes, k):
    """(Z, Y, X, k) int32: warp_statement.knn at every voxel position"""
    X, Y, Z = dims
    v = WST.voxel_positions((Z, Y, X), voxel_size)
    return WS.knn(nodes, v, k).reshape(Z, Y, X, k)


@functools.lru_cache(maxsize=None)
def case(name, D=None):
    """the statement on (the first D nodes of) a case of tsdf_warped_cases: dict(must (bricks,), rows (Z, Y, X, k),
    brick (Z, Y, X)); computed once per process, read-only"""
    c = CS.case(name)
    D = c["D"] if D is None else D
    nodes, w = c["nodes"][:D], c["node_w"][:D]
    out = dict(must=must_store(c["dims"], c["voxel_size"], nodes, w), rows=rows(c["dims"], c["voxel_size"], nodes, c["k"]),
               brick=brick_of_voxels(c["dims"]))
    for a in out.values():
        a.setflags(write=False)
    return out
