"""CPU statement of the indexed mesh of include/dynfu_amd.h (dfa_marching_cubes_indexed) in numpy float32, written from the
contract and tests/mc_statement.py's helpers.

Vertices: a lattice edge — lower voxel (x, y, z), axis 0 / 1 / 2 towards +x / +y / +z — is a vertex when its two voxels differ
in `distance < 0` and one of the up to four cubes around it has eight non-zero weights.  Order: ascending key
3 * (z*X*Y + y*X + x) + axis.  Position: float4 {x, y, z, 1}, vertex_interp from the LOW voxel to the HIGH one,
t = (0 - f_lo) / (f_hi - f_lo + 1e-15), p = p_lo + t * (p_hi - p_lo) on all three axes, corners at (i + 0.5) * cell; every
operation a float32 operation, nothing fused.

Indices: one per soup vertex of mc_statement.marching_cubes, in its order (ascending cube, table order): the id of the vertex
of the lattice edge that the cube's edge is.  A table row that names an edge which is no vertex gets -1 here (the contract
leaves it open); tests/test_mc_indexed_statement_cpu.py asserts that neither table does that.
"""
import numpy as np

import mc_statement as MS

f32 = np.float32


def valid_cubes(vol):
    """(Z - 1, Y - 1, X - 1) bool: all eight weights of the cube are non-zero"""
    ok = (np.asarray(vol).view(np.uint32) >> 16) != 0
    Z, Y, X = ok.shape
    v = np.ones((Z - 1, Y - 1, X - 1), bool)
    for dx, dy, dz in MS.CORNER:
        v &= ok[dz:dz + Z - 1, dy:dy + Y - 1, dx:dx + X - 1]
    return v


def vertex_edges(vol):
    """(Z, Y, X, 3) bool: edge (voxel, axis) is a vertex — the sign and weight rule, no table.  Flattened in C order its
    index is the key."""
    vol = np.asarray(vol).view(np.uint32)
    Z, Y, X = vol.shape
    neg = MS.half_to_float(vol) < f32(0)
    vp = np.zeros((Z + 1, Y + 1, X + 1), bool)  # vp[k + 1] = cube k; cubes -1 and dim - 1 do not exist
    vp[1:Z, 1:Y, 1:X] = valid_cubes(vol)
    act = np.zeros((Z, Y, X, 3), bool)
    # +x: cubes (x, y - 1 .. y, z - 1 .. z)
    around = vp[:-1, :-1, 1:X] | vp[1:, :-1, 1:X] | vp[:-1, 1:, 1:X] | vp[1:, 1:, 1:X]
    act[:, :, :X - 1, 0] = (neg[:, :, :-1] != neg[:, :, 1:]) & around
    # +y: cubes (x - 1 .. x, y, z - 1 .. z)
    around = vp[:-1, 1:Y, :-1] | vp[1:, 1:Y, :-1] | vp[:-1, 1:Y, 1:] | vp[1:, 1:Y, 1:]
    act[:, :Y - 1, :, 1] = (neg[:, :-1, :] != neg[:, 1:, :]) & around
    # +z: cubes (x - 1 .. x, y - 1 .. y, z)
    around = vp[1:Z, :-1, :-1] | vp[1:Z, 1:, :-1] | vp[1:Z, :-1, 1:] | vp[1:Z, 1:, 1:]
    act[:Z - 1, :, :, 2] = (neg[:-1] != neg[1:]) & around
    return act


def positions(vol, cell, keys):
    """float4 {x, y, z, 1} of the edges `keys`, from the low voxel to the high one"""
    vol = np.asarray(vol).view(np.uint32)
    Z, Y, X = vol.shape
    cell = np.asarray(cell, np.float32)
    keys = np.asarray(keys, np.int64)
    axis, lin = keys % 3, keys // 3
    lo = [lin % X, (lin // X) % Y, lin // (X * Y)]
    hi = [lo[k] + (axis == k) for k in range(3)]
    F = MS.half_to_float(vol)
    f_lo, f_hi = F[lo[2], lo[1], lo[0]], F[hi[2], hi[1], hi[0]]
    out = np.zeros((len(keys), 4), np.float32)
    out[:, 3] = 1
    with np.errstate(all="ignore"):
        t = (f32(0) - f_lo) / ((f_hi - f_lo) + f32(1e-15))
        for k in range(3):
            p_lo = (lo[k].astype(np.float32) + f32(0.5)) * cell[k]
            p_hi = (hi[k].astype(np.float32) + f32(0.5)) * cell[k]
            out[:, k] = p_lo + t * (p_hi - p_lo)
    return out


def soup_edges(vol, tri, nv):
    """per soup vertex of mc_statement.marching_cubes, in its order: (key of its lattice edge, True where the cube's edge runs
    from the low voxel to the high one — MS.EDGE's direction)"""
    vol = np.asarray(vol).view(np.uint32)
    Z, Y, X = vol.shape
    tri = np.asarray(tri, np.int64).reshape(256, 16)
    per_case = MS.vertices_per_case(nv)
    cases = MS._cases(MS.half_to_float(vol) < f32(0), (vol >> 16) != 0)
    n_cube = per_case[cases]
    cz, cy, cx = np.nonzero(n_cube)
    n = n_cube[cz, cy, cx]
    total = int(n.sum())
    if total == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    owner = np.repeat(np.arange(len(n)), n)
    j = np.arange(total) - np.repeat(np.cumsum(n) - n, n)
    e = tri[cases[cz, cy, cx][owner], j]
    assert ((e >= 0) & (e < 12)).all()
    c0, c1 = MS.CORNER[MS.EDGE[e, 0]], MS.CORNER[MS.EDGE[e, 1]]
    low = np.minimum(c0, c1)
    axis = np.argmax(c0 != c1, axis=1)
    x, y, z = cx[owner] + low[:, 0], cy[owner] + low[:, 1], cz[owner] + low[:, 2]
    return 3 * ((z * Y + y) * X + x) + axis, (c0 == low).all(axis=1)


def indexed(vol, cell, tri, nv):
    """(vertices (n, 4) float32, indices (m,) int32, keys (n,) int64) of the whole volume"""
    act = vertex_edges(vol)
    keys = np.flatnonzero(act.reshape(-1))
    ident = np.full(act.size, -1, np.int32)
    ident[keys] = np.arange(len(keys), dtype=np.int32)
    ekeys, _ = soup_edges(vol, tri, nv)
    return positions(vol, cell, keys), ident[ekeys], keys
