"""CPU statement of marching cubes over the packed TSDF volume in numpy float32, and an fp64 checker of a mesh.

What it states is the reference's src/kfusion/cuda/marching_cubes.cu — computeCubeIndex (:35-73), getNodeCoo (:181-190),
vertex_interp (:192-199), the edge list of TrianglesGenerator (:232-243) — with the output contract of
include/dynfu_amd.h (dfa_marching_cubes): vertices in ascending linear voxel index z*X*Y + y*X + x of their cube, inside
a cube in the order of the case table's row, float4 {x, y, z, 1}.  Every operation is a float32 operation in the
reference's order and nothing is fused (the library is built with -ffp-contract=off).  The table clamps are the ones
csrc/mc.hip documents: cases 0 and 255 emit nothing, a case emits 3 * (min(max(nv, 0), 15) / 3) vertices.

It works slab-wise: vertices(vol, cell, tri, nv, z0, z1) gives the vertices whose CUBE has z in [z0, z1), with absolute
coordinates; slabs taken in ascending z concatenate to the whole output.  `vol` may be the whole volume or only the
slices [z_base, z_base + len(vol)) of it — that is what makes 512^3 and 1024^3 affordable on the host.

check_mesh_fp64 is independent of all of the above but the voxel packing: it knows no table and no vertex order.

The parity tests compare the kernels' bits against this module; tests/test_mc_statement_cpu.py checks the module itself.
"""
import numpy as np

f32 = np.float32

# corner k of cube (x, y, z) sits at (x + dx, y + dy, z + dz): marching_cubes.cu:37-60 / :218-225
CORNER = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)
# edge e runs from corner EDGE[e, 0] (p0, f0) to corner EDGE[e, 1] (p1, f1): :232-243
EDGE = np.array([(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)], np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def half_to_float(packed):
    """the fp16 distance of packed voxels as float32 (exact: denormals, infinities and NaN included)"""
    return (np.asarray(packed, np.uint32) & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)


def negative_int(packed):
    """`float(fp16 distance) < 0` by integer work only: sign set, not a zero, not a NaN (-inf is negative)"""
    h = np.asarray(packed, np.uint32)
    mag = h & 0x7FFF
    return ((h & 0x8000) != 0) & (mag != 0) & (mag <= 0x7C00)


def vertices_per_case(nv):
    """vertices a case emits: 0 for cases 0 and 255, else 3 * (min(max(nv, 0), 15) / 3)"""
    n = 3 * (np.clip(np.asarray(nv, np.int64), 0, 15) // 3)
    n[0] = n[255] = 0
    return n


def _slices(vol, z0, z1, z_base, Z):
    """the slices [z0, z1] of the volume (cubes of z0 .. z1 - 1 need slice z1 too); z1 is clamped to Z - 1"""
    vol = np.asarray(vol)
    if vol.dtype != np.uint32:
        vol = vol.view(np.uint32)
    Z = z_base + vol.shape[0] if Z is None else Z
    z1 = Z - 1 if z1 is None else min(z1, Z - 1)
    if z1 <= z0:
        return None, z1
    assert z0 >= z_base and z1 < z_base + vol.shape[0], "the slab needs slices %d..%d" % (z0, z1)
    return vol[z0 - z_base:z1 - z_base + 1], z1


def _cases(neg, ok):
    """cube cases from the per-voxel `distance < 0` and `weight != 0` of n + 1 slices: (n, Y - 1, X - 1) uint8"""
    n, Y, X = neg.shape[0] - 1, neg.shape[1], neg.shape[2]
    ci = np.zeros((n, Y - 1, X - 1), np.uint8)
    valid = np.ones((n, Y - 1, X - 1), bool)
    for k, (dx, dy, dz) in enumerate(CORNER):
        sl = (slice(dz, dz + n), slice(dy, dy + Y - 1), slice(dx, dx + X - 1))
        ci |= neg[sl].astype(np.uint8) << np.uint8(k)  # :63-71
        valid &= ok[sl]                                # :38-60: any weight 0 -> case 0
    return np.where(valid, ci, np.uint8(0))


def cube_cases(vol, z0=0, z1=None, z_base=0, Z=None, integer=False):
    """computeCubeIndex of the cubes with z in [z0, z1): uint8 (z1 - z0, Y - 1, X - 1).  Bit k is set where corner k's
    fp16 distance, converted to float32, is < 0 (integer=True: the same decision on the bits); 0 where a weight is 0."""
    s, z1 = _slices(vol, z0, z1, z_base, Z)
    if s is None:
        return np.zeros((0, max(np.asarray(vol).shape[1] - 1, 0), max(np.asarray(vol).shape[2] - 1, 0)), np.uint8)
    neg = negative_int(s) if integer else half_to_float(s) < f32(0)
    return _cases(neg, (s >> 16) != 0)


def cube_counts(vol, nv, z0=0, z1=None, z_base=0, Z=None):
    """vertices per cube with z in [z0, z1), integer work only: int64 (z1 - z0, Y - 1, X - 1)"""
    return vertices_per_case(nv)[cube_cases(vol, z0, z1, z_base, Z, integer=True)]


def count(vol, nv, z0=0, z1=None, z_base=0, Z=None):
    """the count-only form: how many vertices the cubes with z in [z0, z1) emit.  Integer work only, and only over the
    bounding box (in y and x) of the voxels with a negative distance and a weight: a cube without one emits nothing."""
    s, z1 = _slices(vol, z0, z1, z_base, Z)
    if s is None:
        return 0
    if not (s & np.uint32(0x8000)).any():  # (no sign bit in the slab: most of a large volume ends here)
        return 0
    live = (negative_int(s) & ((s >> 16) != 0)).any(axis=0)
    if not live.any():
        return 0
    ys, xs = np.flatnonzero(live.any(axis=1)), np.flatnonzero(live.any(axis=0))
    y0, y1 = max(ys[0] - 1, 0), min(ys[-1] + 2, s.shape[1])
    x0, x1 = max(xs[0] - 1, 0), min(xs[-1] + 2, s.shape[2])
    if y1 - y0 < 2 or x1 - x0 < 2:
        return 0
    c = s[:, y0:y1, x0:x1]
    cases = _cases(negative_int(c), (c >> 16) != 0)
    return int(np.bincount(cases.reshape(-1), minlength=256) @ vertices_per_case(nv))


def vertices(vol, cell, tri, nv, z0=0, z1=None, z_base=0, Z=None):
    """The vertices of the cubes with z in [z0, z1) as (n, 4) float32 {x, y, z, 1} in the output order, with absolute
    coordinates.  vol: uint32 (len, Y, X) holding the slices z_base .. z_base + len - 1 of a volume of Z slices."""
    s, z1 = _slices(vol, z0, z1, z_base, Z)
    if s is None:
        return np.zeros((0, 4), np.float32)
    cell = np.asarray(cell, np.float32)
    tri = np.asarray(tri, np.int64).reshape(256, 16)
    per_case = vertices_per_case(nv)
    F = half_to_float(s)
    cases = _cases(F < f32(0), (s >> 16) != 0)
    n_cube = per_case[cases]
    cz, cy, cx = np.nonzero(n_cube)  # C order = ascending linear voxel index
    n = n_cube[cz, cy, cx]
    total = int(n.sum())
    out = np.zeros((total, 4), np.float32)
    out[:, 3] = 1
    if total == 0:
        return out
    owner = np.repeat(np.arange(len(n)), n)                 # the cube of every vertex
    j = np.arange(total) - np.repeat(np.cumsum(n) - n, n)    # its position in the table row
    e = tri[cases[cz, cy, cx][owner], j]                     # :251-253
    assert ((e >= 0) & (e < 12)).all(), "the case table holds no edge where num_verts says there is a vertex"
    c0, c1 = CORNER[EDGE[e, 0]], CORNER[EDGE[e, 1]]
    base = (cx[owner], cy[owner], cz[owner])
    f0 = F[base[2] + c0[:, 2], base[1] + c0[:, 1], base[0] + c0[:, 0]]
    f1 = F[base[2] + c1[:, 2], base[1] + c1[:, 1], base[0] + c1[:, 0]]
    with np.errstate(all="ignore"):
        t = (f32(0) - f0) / ((f1 - f0) + f32(1e-15))         # :193
        for k in range(3):
            i = base[k] + (z0 if k == 2 else 0)
            p0 = ((i + c0[:, k]).astype(np.float32) + f32(0.5)) * cell[k]  # getNodeCoo :181-190
            p1 = ((i + c1[:, k]).astype(np.float32) + f32(0.5)) * cell[k]
            out[:, k] = p0 + t * (p1 - p0)                    # :194-196, all three axes as the reference has them
    return out


def marching_cubes(vol, cell, tri, nv, slab=16):
    """the whole output, slab by slab: (points (n, 4) float32, n)"""
    Z = np.asarray(vol).shape[0]
    parts = [vertices(vol, cell, tri, nv, z, z + slab) for z in range(0, max(Z - 1, 1), slab)]
    pts = np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)
    return pts, len(pts)


class MeshError(AssertionError):
    pass


def check_mesh_fp64(points, vol, cell, ulps=4.0, allow_nonfinite=False):
    """Every vertex of `points` ((n, >= 3) float32) lies on a lattice edge of `vol` between two voxel centres of opposite
    sign class (distance < 0 against not) and non-zero weight, at the fp64 linear zero crossing of the two fp16 values.
    No table, no vertex order.  Raises MeshError; returns (axis, x, y, z, end) of every vertex's edge: its lower voxel, and
    end = 1 / 2 where the vertex sits exactly on the edge's lower / upper voxel centre (0 elsewhere).

    The two coordinates across the edge must be lattice coordinates EXACTLY: float32((i + 0.5) * cell), since
    p0 + t * 0 is p0 for every finite t.  The coordinate along the edge is held to a derived bound.  With u = 2^-24 and
    X0 < X1 the exact lattice coordinates (i + 0.5) c and (i + 1.5) c of the two voxels, M = X1, the float32 evaluation of
    vertex_interp makes these errors against x* = X0 + t* (X1 - X0), t* = f0 / (f0 - f1) in [0, 1]:
      * p0, p1 = X (1 + d): u M each (one product; i + 0.5 is exact);
      * f1 - f0: one rounding (two fp16 values are multiples of 2^-24, their difference may need more than 24 bits);
        adding 1e-15 changes nothing (|f1 - f0| >= 2^-24, whose half ulp is above 1e-15); the quotient rounds once more:
        t = t* (1 + e), |e| <= 2 u;
      * w = fl(p1 - p0): |w - (X1 - X0)| <= 2 u M + u c;
      * fl(t w): |.. - t* (X1 - X0)| <= (2 u M + u c) + 2 u c + u c = 2 u M + 4 u c;
      * fl(p0 + ..): u M from p0, u M from the last rounding.
    Sum: 4 u M + 4 u c, and c <= M / 1.5, so |p - x*| < 6.7 u M; u M <= ulp(M) / 2 ... ulp(M).  The bound used is
    `ulps` = 4 float32 ulps of M taken as 2^-23 M each (= 8 u M): the derivation with a little room, not a fitted number.
    Edges with an infinite or NaN distance have no fp64 crossing; a vertex there is accepted where float32 arithmetic gives
    a finite point (f1 = +-inf: t = 0) and otherwise only with allow_nonfinite (NaN coordinates cannot name an edge)."""
    vol = np.asarray(vol)
    if vol.dtype != np.uint32:
        vol = vol.view(np.uint32)
    Z, Y, X = vol.shape
    dims = (X, Y, Z)
    p32 = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    cell32 = np.asarray(cell, np.float32)
    finite = np.isfinite(p32).all(axis=1)
    if not allow_nonfinite and not finite.all():
        raise MeshError("%d vertices with non-finite coordinates, first at %d" % ((~finite).sum(), np.flatnonzero(~finite)[0]))
    n = len(p32)
    p = p32.astype(np.float64)
    c = cell32.astype(np.float64)
    near = [np.rint(np.where(finite, p[:, k], 0.0) / c[k] - 0.5).astype(np.int64) for k in range(3)]  # nearest lattice index
    on = [((near[k].astype(np.float32) + f32(0.5)) * cell32[k]) == p32[:, k] for k in range(3)]        # exactly a lattice coordinate
    passed = np.zeros(n, bool)
    edge = np.full((n, 5), -1, np.int64)
    worst = 0.0
    for a in range(3):
        b, d = [k for k in range(3) if k != a]
        for lo_off in (-1, 0):  # the vertex is within half a cell of lattice index near[a]: its edge starts there or one below
            lo = near[a] + lo_off
            idx = [None] * 3
            idx[a], idx[b], idx[d] = lo, near[b], near[d]
            ok = finite & on[b] & on[d] & (lo >= 0) & (lo + 1 < dims[a])
            for k in (b, d):
                ok &= (idx[k] >= 0) & (idx[k] < dims[k])
            sel = np.flatnonzero(ok & ~passed)
            if len(sel) == 0:
                continue
            i0 = [idx[k][sel] for k in range(3)]
            i1 = list(i0)
            i1[a] = i0[a] + 1
            vA, vB = vol[i0[2], i0[1], i0[0]], vol[i1[2], i1[1], i1[0]]
            fA, fB = half_to_float(vA).astype(np.float64), half_to_float(vB).astype(np.float64)
            good = ((vA >> 16) != 0) & ((vB >> 16) != 0) & ((fA < 0) != (fB < 0))
            xA, xB = (i0[a] + 0.5) * c[a], (i0[a] + 1.5) * c[a]
            with np.errstate(all="ignore"):
                xs = xA + (fA / (fA - fB)) * (xB - xA)
                err = np.abs(p[sel, a] - xs)
            bound = ulps * 2.0 ** -23 * xB
            hit = good & (err <= bound)  # (NaN: False)
            if hit.any():
                worst = max(worst, float((err[hit] / (2.0 ** -23 * xB[hit])).max()))
            passed[sel[hit]] = True
            at = np.where(on[a][sel[hit]], 1 + (near[a][sel[hit]] - i0[a][hit]), 0)
            e = np.stack([np.full(hit.sum(), a), i0[0][hit], i0[1][hit], i0[2][hit], at], 1)
            edge[sel[hit]] = e
    bad = finite & ~passed
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise MeshError("%d of %d vertices are on no sign-changing lattice edge at its fp64 zero crossing within %g ulps; "
                        "first: vertex %d = %r" % (bad.sum(), n, ulps, i, p32[i].tolist()))
    check_mesh_fp64.worst_ulps = worst
    return edge


def check_voxel_order(edge, dims):
    """The output contract's order, as far as an edge list can show it: vertex i belongs to one of the (up to four)
    cubes that contain its edge (up to eight around a voxel centre, where the edge is not unique), and the cubes' linear
    indices must be able to ascend along the output.  Necessary
    condition: the running maximum of the LOWEST candidate cube never exceeds a vertex's HIGHEST candidate cube.
    edge: what check_mesh_fp64 returns."""
    X, Y, Z = dims
    e = edge[edge[:, 0] >= 0]
    a = e[:, 0]
    lo = [None] * 3
    hi = [None] * 3
    for k, dim in enumerate((X, Y, Z)):
        v = e[:, 1 + k] + ((a == k) & (e[:, 4] == 2))          # (the voxel itself for a vertex on a voxel centre)
        along = (a == k) & (e[:, 4] == 0)                       # along the edge the cube starts at the edge's lower voxel
        lo[k] = np.where(along, v, np.maximum(v - 1, 0))
        hi[k] = np.where(along, v, np.minimum(v, dim - 2))
    lin = lambda q: (q[2] * Y + q[1]) * X + q[0]
    lowest, highest = lin(lo), lin(hi)
    if len(e) and (np.maximum.accumulate(lowest) > highest).any():
        i = int(np.flatnonzero(np.maximum.accumulate(lowest) > highest)[0])
        raise MeshError("vertex %d comes after a vertex of a later cube" % i)
