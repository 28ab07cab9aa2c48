"""CPU statement of dfa_marching_cubes_indexed_min_weight (include/dynfu_amd.h) in numpy, twice.

1. By the contract's equivalence: mc_indexed_statement.indexed on a copy of the volume in which every voxel of weight
   < min_weight has its weight field zeroed, distance bits kept (`zeroed`, `indexed_min_weight`).  This is what the -m gpu
   tests compare the device call with.
2. By the floor rule itself, no copy (`indexed_by_rule`): a voxel is observed when weight >= min_weight; a cube is valid when
   its eight corners are observed; a lattice edge is a vertex when its two voxels differ in `distance < 0` and one of the up
   to four cubes around it is valid; a valid cube emits its case's table row.  Positions and order as mc_indexed_statement.

tests/test_mc_min_weight_statement_cpu.py asserts that the two agree.
"""
import numpy as np

import mc_indexed_statement as IS
import mc_statement as MS

f32 = np.float32

WEIGHTS = np.array([0, 1, 2, 3, 65535], np.uint32)  # what the tests draw weights from ...
# ... with these odds: a cube is valid at floor 1 / 2 / 3 / 65535 with probability 0.96^8 = 0.72 / 0.90^8 = 0.43 /
# 0.82^8 = 0.20 / 0.72^8 = 0.07, so every floor keeps cubes and every step of the floor removes some
WEIGHT_ODDS = np.array([0.04, 0.06, 0.08, 0.10, 0.72])


def zeroed(vol, min_weight):
    """the volume with the weight field of every voxel of weight < min_weight set to 0; distance bits kept"""
    vol = np.asarray(vol).view(np.uint32)
    return np.where((vol >> 16) >= np.uint32(min_weight), vol, vol & np.uint32(0xFFFF)).astype(np.uint32)


def indexed_min_weight(vol, cell, tri, nv, min_weight):
    """(vertices (n, 4) float32, indices (m,) int32, keys (n,) int64): statement 1"""
    assert 1 <= min_weight <= 65535
    return IS.indexed(zeroed(vol, min_weight), cell, tri, nv)


def with_weights(vol, seed):
    """the volume's distances with weights drawn from WEIGHTS"""
    vol = np.asarray(vol).view(np.uint32)
    rng = np.random.default_rng(seed)
    w = WEIGHTS[rng.choice(len(WEIGHTS), size=vol.shape, p=WEIGHT_ODDS)]
    return ((vol & np.uint32(0xFFFF)) | (w << 16)).astype(np.uint32)


# ------------------------------------------------------------------------------------------- statement 2
def observed(vol, min_weight):
    return (np.asarray(vol).view(np.uint32) >> 16) >= np.uint32(min_weight)


def valid_cubes(vol, min_weight):
    """(Z - 1, Y - 1, X - 1) bool: all eight corners observed"""
    ok = observed(vol, min_weight)
    Z, Y, X = ok.shape
    return (ok[:-1, :-1, :-1] & ok[:-1, :-1, 1:] & ok[:-1, 1:, :-1] & ok[:-1, 1:, 1:] &
            ok[1:, :-1, :-1] & ok[1:, :-1, 1:] & ok[1:, 1:, :-1] & ok[1:, 1:, 1:])


def vertex_edges(vol, min_weight):
    """(Z, Y, X, 3) bool: edge (lower voxel, axis) is a vertex.  Cube by cube: a valid cube marks its twelve edges, an edge
    is a vertex where it is marked and its two voxels differ in sign class."""
    vol = np.asarray(vol).view(np.uint32)
    Z, Y, X = vol.shape
    neg = MS.half_to_float(vol) < f32(0)
    v = valid_cubes(vol, min_weight)
    marked = np.zeros((Z, Y, X, 3), bool)
    for a in range(3):          # the four edges of a cube along axis a start at the cube's corner displaced by (0|1, 0|1)
        o1, o2 = [k for k in range(3) if k != a]  # in the two other axes (x = 0, y = 1, z = 2)
        for d1 in (0, 1):
            for d2 in (0, 1):
                off = [0, 0, 0]
                off[o1], off[o2] = d1, d2
                dx, dy, dz = off
                marked[dz:dz + Z - 1, dy:dy + Y - 1, dx:dx + X - 1, a] |= v
    cross = np.zeros((Z, Y, X, 3), bool)
    cross[:, :, :X - 1, 0] = neg[:, :, :-1] != neg[:, :, 1:]
    cross[:, :Y - 1, :, 1] = neg[:, :-1, :] != neg[:, 1:, :]
    cross[:Z - 1, :, :, 2] = neg[:-1] != neg[1:]
    return marked & cross


def soup_edge_keys(vol, tri, nv, min_weight):
    """per soup vertex, in ascending cube and table order: the key of its lattice edge"""
    vol = np.asarray(vol).view(np.uint32)
    Z, Y, X = vol.shape
    tri = np.asarray(tri, np.int64).reshape(256, 16)
    per_case = MS.vertices_per_case(nv)
    neg = MS.half_to_float(vol) < f32(0)
    case = np.zeros((Z - 1, Y - 1, X - 1), np.int64)
    for k, (dx, dy, dz) in enumerate(MS.CORNER):
        case |= neg[dz:dz + Z - 1, dy:dy + Y - 1, dx:dx + X - 1].astype(np.int64) << k
    case[~valid_cubes(vol, min_weight)] = 0
    out = []
    for cz, cy, cx in zip(*np.nonzero(per_case[case])):
        cs = case[cz, cy, cx]
        for e in tri[cs, :per_case[cs]]:
            c0, c1 = MS.CORNER[MS.EDGE[e, 0]], MS.CORNER[MS.EDGE[e, 1]]
            low = np.minimum(c0, c1)
            axis = int(np.argmax(c0 != c1))
            out.append(3 * (((cz + low[2]) * Y + cy + low[1]) * X + cx + low[0]) + axis)
    return np.asarray(out, np.int64)


def indexed_by_rule(vol, cell, tri, nv, min_weight):
    """(vertices, indices, keys): statement 2"""
    act = vertex_edges(vol, min_weight)
    keys = np.flatnonzero(act.reshape(-1))
    ident = np.full(act.size, -1, np.int32)
    ident[keys] = np.arange(len(keys), dtype=np.int32)
    ekeys = soup_edge_keys(vol, tri, nv, min_weight)
    idx = ident[ekeys] if len(ekeys) else np.zeros(0, np.int32)
    return IS.positions(vol, cell, keys), idx, keys
