"""The meshes and cameras of the rasteriser tests, shared by tests/test_raster_statement_cpu.py (no GPU) and
tests/test_gpu_raster.py.  case(name) -> dict(vertices (N, 4) float32, normals (N, 4) float32 or None, indices int32 (3 T),
world2cam (12 floats or None), intr (fx, fy, cx, cy), z_near, cols, rows); reference(name) is rasterize32 of it, computed
once and read-only.

  a         one triangle in 16 x 16 with its vertices ON pixel centres: the top-left rule decides the boundary (COVERAGE_A)
  b_cw/ccw  a quad as two triangles, its diagonal through pixel centres, in both windings
  c         two coplanar copies (the lower number wins) and two parallel triangles, the farther one first
  d         two triangles that cross, so the winner changes inside a box
  e         every skip rule next to one drawn triangle
  f         no triangle
  g         70 triangles: numbers 3 and 40 cover most of a 64 x 48 image, the others about a pixel each
  h         one triangle over all of 640 x 480 (the GPU test gives it pitched maps)
  i         the welded marching-cubes mesh of the synthetic sphere fused into 64^3, 160 x 120 camera, vertex normals
  j         i from a camera turned about the volume's centre
"""
import functools

import numpy as np

import raster_statement as RS
from gpu_util_cpu import aff12, rot

NAMES = ("a", "b_cw", "b_ccw", "c", "d", "e", "f", "g", "h", "i", "j")

# case a, row j from the top, '#' = covered: the triangle (2, 2), (10, 2), (2, 10).  Its top edge (row 2) and its left edge
# (column 2) own their centres, corner (2, 2) included; the third edge, i + j = 12, owns none — so neither do the corners
# (10, 2) and (2, 10) that lie on it
COVERAGE_A = ("................",
              "................",
              "..########......",
              "..#######.......",
              "..######........",
              "..#####.........",
              "..####..........",
              "..###...........",
              "..##............",
              "..#.............",
              "................",
              "................",
              "................",
              "................",
              "................",
              "................")

PIXEL_GRID = (1.0, 1.0, 0.0, 0.0)  # fx, fy, cx, cy: a vertex (x, y, 1) lands on u = x, v = y exactly


def _v4(xyz):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.ones((len(xyz), 1), np.float32)], 1)


def _case(xyz, tris, intr, cols, rows, normals=None, world2cam=None, z_near=0.1):
    return dict(vertices=_v4(xyz), normals=None if normals is None else np.ascontiguousarray(normals, np.float32),
                indices=np.asarray(tris, np.int32).reshape(-1), world2cam=world2cam, intr=tuple(float(v) for v in intr),
                z_near=float(z_near), cols=cols, rows=rows)


def _small_triangles(rng, n, cols, rows, intr, z_lo, z_hi):
    """n triangles of about a pixel, anywhere in the image (camera frame)"""
    fx, fy, cx, cy = intr
    uv = rng.uniform([2, 2], [cols - 3, rows - 3], (n, 1, 2)) + rng.uniform(-0.9, 0.9, (n, 3, 2))
    z = rng.uniform(z_lo, z_hi, (n, 1)) + rng.uniform(-0.01, 0.01, (n, 3))
    return np.stack([(uv[..., 0] - cx) / fx * z, (uv[..., 1] - cy) / fy * z, z], -1).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    """(vertices, normals, indices, volume, voxel, trunc, intr, cols, rows) of the synthetic sphere in front of its wall, fused
    into 64^3 by the numpy statement (render_scenes.statement_volume) and extracted by the indexed marching-cubes statement"""
    import mc_indexed_statement as IS
    import render_scenes
    import tsdf_statement as S
    from mc_util import default_tables
    vol, voxel, trunc, intr, cols, rows = render_scenes.statement_volume("T0", "turned")
    tri, nv = default_tables()
    verts, idx, _ = IS.indexed(vol, voxel, tri, nv)
    normals = S.vertex_normals(vol, voxel, render_scenes.DELTA, verts)
    for a in (verts, normals, idx, vol):
        a.setflags(write=False)
    return verts, normals, idx.astype(np.int32), vol, voxel, trunc, intr, cols, rows


def sphere_camera(name):
    """world2cam (the mesh is in the volume's frame) of case i / j.  i: the sequence's camera moved 0.45 m to the right and
    0.2 m down, so that a quarter of the view looks past the edge of the wall the sequence saw.  j: turned by 0.3 rad about
    the volume's centre on top of that."""
    from dynfu_amd import synth
    t = np.array(synth.VOLUME_POSE_T, np.float64) - np.array([0.45, 0.2, 0.0])
    if name == "i":
        return aff12(np.eye(3), t)
    R = rot([0.2, 1, 0.1], 0.3)
    c = np.full(3, synth.VOLUME_SIZE / 2)
    return aff12(R, (c - R @ c) + t)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "a":
        return _case([[2, 2, 1], [10, 2, 1], [2, 10, 1]], [0, 1, 2], PIXEL_GRID, 16, 16)
    if name in ("b_cw", "b_ccw"):
        quad = [[3, 3, 1], [11, 3, 1], [11, 9, 1], [3, 9, 1]]  # the diagonal (3, 3) - (11, 9) passes through centre (7, 6)
        return _case(quad, [0, 1, 2, 0, 2, 3] if name == "b_cw" else [0, 2, 1, 0, 3, 2], PIXEL_GRID, 16, 16)
    intr32 = (20.0, 20.0, 15.5, 15.5)
    if name == "c":
        dup = [[-0.9, -0.8, 1.5], [0.1, -0.7, 1.3], [-0.6, 0.2, 1.6]]
        far = [[-0.2, 0.0, 3.0], [1.8, 0.3, 3.0], [0.3, 2.0, 3.0]]
        near = [[0.0, 0.1, 2.0], [0.9, 0.2, 2.0], [0.2, 1.1, 2.0]]
        # (64 x 64: at 32 x 32 these four small triangles have 4 of 180 centres within 1/128 pixel of an edge, over the 2 % cap)
        return _case(dup + dup + far + near, np.arange(12), (40.0, 40.0, 31.5, 31.5), 64, 64)
    if name == "d":
        one = [[-1.2, -1.0, 1.0], [1.4, -0.2, 3.0], [-0.9, 1.3, 1.2]]
        two = [[-1.3, -0.6, 3.0], [1.2, -1.1, 1.0], [1.0, 1.4, 1.4]]
        return _case(one + two, np.arange(6), intr32, 32, 32)
    if name == "e":
        nan = np.nan
        xyz = [[-0.5, -0.5, 2.0], [0.4, -0.4, 2.0], [-0.3, 0.5, 2.2],  # 0-2: drawn
               [0.0, 0.0, 0.05],                                       # 3: nearer than z_near
               [nan, 0.0, 2.0],                                        # 4: not finite
               [1.0e6, 0.0, 1.0],                                      # 5: 2e7 pixels to the right: outside the guard band
               [30.0, 30.0, 2.0], [31.0, 30.0, 2.0], [30.0, 31.0, 2.0],  # 6-8: wholly off the image
               [0.9, 0.9, 1.5], [2.5, 1.0, 1.5], [1.0, 2.5, 1.5],      # 9-11: across the right and bottom borders
               [-0.6, -0.6, 1.0], [-3.0, -0.5, 1.0], [-0.7, -3.0, 1.0]]  # 12-14: across the left and top borders
        tris = [0, 1, 2,
                0, 1, 3,    # a vertex behind z_near
                0, 4, 2,    # a NaN vertex
                0, 1, 1,    # no area
                0, 1, 5,    # guard band
                -1, 1, 2,   # index -1
                0, 15, 2,   # index N
                6, 7, 8,    # off-screen
                9, 10, 11,  # straddles
                12, 13, 14]
        return _case(xyz, tris, intr32, 32, 32)
    if name == "f":
        return _case([[0, 0, 1], [1, 0, 1], [0, 1, 1]], [], intr32, 32, 32)
    if name == "g":
        cols, rows, intr = 64, 48, (60.0, 60.0, 31.5, 23.5)
        rng = np.random.default_rng(7)
        xyz = _small_triangles(rng, 70, cols, rows, intr, 1.0, 3.0).reshape(70, 3, 3)
        xyz[3] = [[-1.3, -0.9, 2.0], [1.4, -0.8, 1.6], [-1.0, 1.1, 2.4]]   # most of the image, tilted
        xyz[40] = [[1.3, 1.0, 1.5], [-1.2, 0.9, 2.6], [1.1, -1.0, 2.2]]    # the other half, crossing number 3
        return _case(xyz.reshape(-1, 3), np.arange(210), intr, cols, rows)
    if name == "h":
        return _case([[-3.0, -2.5, 2.0], [9.0, -2.0, 3.5], [-2.5, 8.0, 2.5]], [0, 1, 2], (525.0, 525.0, 319.5, 239.5), 640, 480)
    if name in ("i", "j"):
        verts, normals, idx, _, _, _, intr, cols, rows = sphere_mesh()
        return dict(vertices=verts, normals=normals, indices=idx, world2cam=sphere_camera(name), intr=tuple(map(float, intr)),
                    z_near=0.1, cols=cols, rows=rows)
    raise KeyError(name)


def args(c):
    """the arguments of rasterize32 / check64 after the mesh"""
    return (c["world2cam"],) + c["intr"] + (c["z_near"], c["cols"], c["rows"])


@functools.lru_cache(maxsize=None)
def reference(name, face_normals=False):
    """rasterize32 of the case: (z-buffer, points, normals), read-only"""
    c = case(name)
    out = RS.rasterize32(c["vertices"], None if face_normals else c["normals"], c["indices"], *args(c))
    for a in out:
        a.setflags(write=False)
    return out


def permuted(name, seed=1):
    """the case with its triangles in another order -> (case, permutation: new number -> old number)"""
    c = dict(case(name))
    perm = np.random.default_rng(seed).permutation(len(c["indices"]) // 3)
    c["indices"] = np.ascontiguousarray(c["indices"].reshape(-1, 3)[perm]).reshape(-1)
    return c, perm
