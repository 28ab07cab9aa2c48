"""CPU checks of the TSDF half of the hot path against a second, independent reading of the reference
(tests/tsdf_statement.py, a numpy statement of tsdf_volume.cu and imgproc.cu:233-254):

- hand-computed answers on hand-made inputs, independent of both the statement and oracle/tsdf_oracle.c;
- the statement equals the C oracle bit for bit (tsdf and weights, dists, points, normals, depth; misses are the
  reference's 0x7fffffff NaN) on seeded small scenes;
- no ray of the raycast, from the seeded scenes and from adversarial poses, asks fetch_tsdf for a voxel outside the
  volume (the statement raises where the oracle and the kernel would read).
The HIP kernels are compared with the statement by the -m gpu tests of tests/test_gpu_tsdf.py."""
import itertools

import numpy as np
import pytest

import oracle as O
import tsdf_statement as S
from gpu_util_cpu import aff12, rot

f32 = np.float32
ID9 = np.eye(3, dtype=np.float32).reshape(-1)
STEP, DELTA = 0.75, 0.5  # the raycaster's step and gradient factors of the project's configurations


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def half(x):
    return np.float16(x).view(np.uint16)


# ------------------------------------------------------------------------------------------------ hand-made ----
def _column(Z, tz, vs=0.125):
    """a 1 x 1 x Z column straight down the optical axis of a 1 x 1 image (cx = cy = 0, so lambda = 1 and every voxel
    projects onto texel 0): the camera distance of slice z is tz + z * vs"""
    voxel = np.array([vs, vs, vs], np.float32)
    return voxel, aff12(np.eye(3), [0, 0, tz]), (1.0, 1.0, 0.0, 0.0)


def _both_integrate(vol, dists, voxel, trunc, maxw, v2c, intr):
    got = S.integrate(vol, dists, voxel, trunc, maxw, v2c, *intr)
    ref = np.array(vol, np.uint32)
    O.tsdf_integrate(ref, dists, voxel, trunc, maxw, v2c, *intr)
    assert np.array_equal(got, ref)
    return got


def test_fronto_parallel_plane_gives_the_known_tsdf_per_slice_and_truncation_band():
    # surface at 1.5 m, camera 0.5 m in front of slice 0, voxel 0.125 m, trunc 0.25 m: every number below is exact
    voxel, v2c, intr = _column(16, 0.5)
    dists = S.compute_dists(np.full((1, 1), 1500, np.uint16), *intr)
    assert dists[0, 0] == half(1.5)
    vol = _both_integrate(S.clear((16, 1, 1)), dists, voxel, 0.25, 64, v2c, intr)
    F, W = S.unpack(vol[:, 0, 0])
    want = [1, 1, 1, 1, 1, 1, 1, 0.5, 0, -0.5, -1]  # min(1, (1.5 - 0.5 - z / 8) / 0.25); z = 10: sdf == -trunc, kept
    assert F[:11].tolist() == want and W[:11].tolist() == [1] * 11
    assert not vol[11:].any()  # sdf < -trunc: untouched


def test_texel_is_the_floor_of_the_projection_and_cols_is_outside():
    # two texels (1 m and 2 m), a row of 5 voxels at depth 1 projecting to x = 0, 0.5, 1, 1.5, 2 (fx = 1, cx = 0)
    voxel = np.array([0.5, 1, 1], np.float32)
    dists = np.array([[half(1.0), half(2.0)]], np.uint16)
    v2c = aff12(np.eye(3), [0, 0, 1])
    vol = _both_integrate(S.clear((1, 1, 5)), dists, voxel, 100.0, 64, v2c, (1.0, 1.0, 0.0, 0.0))
    F, W = S.unpack(vol[0, 0])
    dist = np.sqrt(np.arange(5) ** 2 * 0.25 + 1)
    Dp = np.array([1, 1, 2, 2])  # coordinate 0.5 -> texel 0, exactly 1 -> texel 1, 1.5 -> texel 1
    assert np.allclose(F[:4], (Dp - dist[:4]) / 100, atol=2e-4)
    assert W.tolist() == [1, 1, 1, 1, 0] and vol[0, 0, 4] == 0  # coordinate == cols: outside
    # coordinate 0.75: texel 0 (a rounding fetch would take texel 1)
    vol = _both_integrate(S.clear((1, 1, 2)), dists, np.array([0.75, 1, 1], np.float32), 100.0, 64, v2c,
                          (1.0, 1.0, 0.0, 0.0))
    assert abs(S.unpack(vol[0, 0, 1])[0] - (1 - np.sqrt(1.5625)) / 100) < 2e-5


def test_zero_distance_and_camera_plane_leave_the_voxel_untouched():
    # column from 0.25 m behind the camera to 1.625 m in front: vc.z < 0 for z < 2, == 0 at z = 2
    voxel, v2c, intr = _column(16, -0.25)
    junk = S.pack(np.full((16, 1, 1), 0.5, np.float32), np.full((16, 1, 1), 5, np.uint32))
    vol = _both_integrate(junk, np.array([[half(1.0)]], np.uint16), voxel, 10.0, 64, v2c, intr)
    assert np.array_equal(vol[:3], junk[:3])  # vc.z <= 0: skipped, though the texel holds a distance
    assert (S.unpack(vol[3:])[1] == 6).all()  # in front: updated
    for zero in (0x0000, 0x8000):  # Dp == +0 and -0
        vol = _both_integrate(junk, np.array([[zero]], np.uint16), voxel, 10.0, 64, v2c, intr)
        assert np.array_equal(vol, junk)


def test_weight_saturates_at_max_weight_and_the_average_uses_the_unclamped_weight():
    voxel, v2c, intr = _column(1, 1.0)
    dists = np.array([[half(3.0)]], np.uint16)  # sdf = 2 >= trunc: tsdf = 1
    vol = S.pack(np.full((1, 1, 1), 0.5, np.float32), np.full((1, 1, 1), 3, np.uint32))
    vol = _both_integrate(vol, dists, voxel, 1.0, 4, v2c, intr)
    assert S.unpack(vol)[0][0, 0, 0] == f32(0.625) and S.unpack(vol)[1][0, 0, 0] == 4  # (0.5 * 3 + 1) / 4
    vol = _both_integrate(vol, dists, voxel, 1.0, 4, v2c, intr)
    assert S.unpack(vol)[0][0, 0, 0] == np.float16(0.7) and S.unpack(vol)[1][0, 0, 0] == 4  # (0.625 * 4 + 1) / 5


def _plane_volume(dims, vs, axis, at, trunc):
    """tsdf of the plane {p[axis] = at}, positive on the low side, weight 1"""
    X, Y, Z = dims
    g = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")[::-1][axis]  # voxel index along axis
    F = np.clip((at - g * vs[axis]) / trunc, -1, 1).astype(np.float32)
    return S.pack(F, np.ones(F.shape, np.uint32))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ray_along_an_axis_hits_a_plane_at_the_analytic_depth(axis):
    dims, vs, trunc = (12, 10, 14), np.array([0.05, 0.06, 0.04], np.float32), 0.1
    at = 0.31
    vol = _plane_volume(dims, vs, axis, at, trunc)
    R = np.eye(3)[:, [(axis + 1) % 3, (axis + 2) % 3, axis]]  # camera z along the volume's axis
    org = 0.5 * vs * (np.array(dims) - 1)
    org[axis] = 0.02
    c2v = aff12(R, org)
    ri = R.T.astype(np.float32).reshape(-1)
    P, N = S.raycast_points(vol, vs, trunc, c2v, ri, 1.0, 1.0, 0.0, 0.0, STEP, DELTA, 1, 1)  # one ray, exactly on axis
    assert abs(P[0, 0, 2] - (at - 0.02)) < 0.02 * vs[axis]
    assert abs(P[0, 0, 0]) < 1e-6 and abs(P[0, 0, 1]) < 1e-6
    assert np.allclose(N[0, 0, :3], [0, 0, -1], atol=1e-5)
    Po, No = O.tsdf_raycast_points(vol, vs, trunc, c2v, ri, 1.0, 1.0, 0.0, 0.0, STEP, DELTA, 1, 1)
    assert np.array_equal(bits(P), bits(Po)) and np.array_equal(bits(N), bits(No))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ray_from_beyond_the_far_face_enters_at_size_minus_voxel(axis):
    """box_max = size - voxel (tsdf_volume.cu:213): a camera beyond the far face along an axis starts marching at
    t = cam - (size - voxel) on that axis, and the statement and the oracle agree on every bit of the hits"""
    dims, vs, trunc = (12, 10, 14), np.array([0.05, 0.06, 0.04], np.float32), 0.1
    size = vs * np.array(dims, np.float32)
    at = 0.31
    g = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")[::-1][axis]
    F = np.clip((g * vs[axis] - at) / trunc, -1, 1).astype(np.float32)  # positive toward the far face
    vol = S.pack(F, np.ones(F.shape, np.uint32))
    R = -np.eye(3)[:, [(axis + 1) % 3, (axis + 2) % 3, axis]]  # camera z along -axis
    R[:, 0] *= -1
    org = 0.5 * vs * (np.array(dims) - 1)
    org[axis] = size[axis] + 0.013
    tmin, _ = S.intersect([np.array([f32(org[k])]) for k in range(3)],
                          [np.array([f32(R[k, 2])]) for k in range(3)], size - vs)
    assert tmin[0] == f32(f32(org[axis]) - (size[axis] - vs[axis]))
    c2v = aff12(rot([1, 1, 0], 0.05) @ R, org)
    ri = np.linalg.inv(rot([1, 1, 0], 0.05) @ R).astype(np.float32).reshape(-1)
    P, N = S.raycast_points(vol, vs, trunc, c2v, ri, 20.0, 20.0, 4.0, 3.0, STEP, DELTA, 9, 7)
    Po, No = O.tsdf_raycast_points(vol, vs, trunc, c2v, ri, 20.0, 20.0, 4.0, 3.0, STEP, DELTA, 9, 7)
    assert (~np.isnan(P[..., 0])).all()
    assert np.array_equal(bits(P), bits(Po)) and np.array_equal(bits(N), bits(No))
    D, _ = S.raycast_depth(vol, vs, trunc, c2v, ri, 20.0, 20.0, 4.0, 3.0, STEP, DELTA, 9, 7)
    assert abs(int(D[3, 4]) - 1000 * (org[axis] - at)) <= 2  # the centre ray: the plane's depth, in mm


# ------------------------------------------------------------------------------------ statement == oracle ----
def _scene(seed):
    """a seeded small scene: volume dims 1 .. 70 per axis, anisotropic voxels, a rotated camera (zstep with three
    non-zero components) in front of or inside the volume, depth of a tilted plane + a bump, with holes"""
    rng = np.random.default_rng(seed)
    dims = [int(v) for v in rng.integers(1, 71, 3)]
    if seed == 0:
        dims = [70, 1, 33]
    rows, cols = [(1, 1), (37, 53), (8, 130)][seed % 3]
    vs = rng.uniform(0.02, 0.06, 3).astype(np.float32)
    size = vs * np.array(dims, np.float32)
    focal = float(rng.choice([1.0, 30.0, 120.0]))
    intr = (focal, focal * float(rng.uniform(0.9, 1.1)), (cols - 1) / 2 + float(rng.uniform(-1, 1)), (rows - 1) / 2)
    R = rot(rng.normal(size=3), float(rng.uniform(0.1, 0.5)))
    inside = seed % 4 == 3
    centre = 0.5 * size
    cam = centre + (np.array([0, 0, 0.1]) if inside else np.array([0.05, -0.03, -0.9]))
    vol2cam = aff12(R.T, -(R.T @ cam))  # camera looks along R's third column
    assert all(abs(vol2cam[k]) > 1e-3 for k in (2, 5, 8))
    yy, xx = np.mgrid[:rows, :cols]
    depth = (800 + 300 * xx / max(cols, 1) + 150 * np.sin(yy / 3.0) + rng.normal(0, 3, (rows, cols))).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.1] = 0
    trunc = float(rng.uniform(0.05, 0.2))
    cam2vol = aff12(R, cam)
    return dims, vs, intr, depth, vol2cam, cam2vol, R.T.astype(np.float32).reshape(-1), trunc, rows, cols


@pytest.mark.parametrize("seed", range(8))
def test_statement_equals_oracle_on_seeded_scenes(seed):
    dims, vs, intr, depth, v2c, c2v, ri, trunc, rows, cols = _scene(seed)
    dists = S.compute_dists(depth, *intr)
    assert np.array_equal(dists, O.compute_dists(depth, *intr))
    X, Y, Z = dims
    vol = S.clear((Z, Y, X))
    ref = np.zeros((Z, Y, X), np.uint32)
    for frame in range(2):  # the second frame reads the first one's values
        d = dists if frame == 0 else S.compute_dists(np.roll(depth, 1, axis=1), *intr)
        vol = S.integrate(vol, d, vs, trunc, 64, v2c, *intr)
        O.tsdf_integrate(ref, d, vs, trunc, 64, v2c, *intr)
        assert np.array_equal(vol, ref), (seed, frame, int((vol != ref).sum()))
    for c2, r2 in ((c2v, ri), (aff12(np.eye(3), 0.5 * vs * np.array(dims)), ID9)):
        P, N = S.raycast_points(vol, vs, trunc, c2, r2, *intr, STEP, DELTA, cols, rows)
        Po, No = O.tsdf_raycast_points(vol, vs, trunc, c2, r2, *intr, STEP, DELTA, cols, rows)
        assert np.array_equal(bits(P), bits(Po)) and np.array_equal(bits(N), bits(No))
        D, N2 = S.raycast_depth(vol, vs, trunc, c2, r2, *intr, STEP, DELTA, cols, rows)
        Do, N2o = O.tsdf_raycast_depth(vol, vs, trunc, c2, r2, *intr, STEP, DELTA, cols, rows)
        assert np.array_equal(D, Do) and np.array_equal(bits(N2), bits(N2o))


def test_statement_equals_oracle_with_hits_on_a_fused_sphere():
    """a raycast that actually hits: a sphere fused from a synthetic frame, camera moved and turned"""
    from dynfu_amd import synth
    cfg = synth.CONFIGS["T0"]
    intr = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, cam2vol, _ = synth.volume_params(cfg)
    v2c = aff12(rot([1, 0.2, 0.3], 0.2), vol2cam[9:])
    dists = S.compute_dists(synth.depth_frame(cfg, 0), *intr)
    dim = cfg["dim"]
    vol, ref = S.clear((dim, dim, dim)), np.zeros((dim, dim, dim), np.uint32)
    for _ in range(2):
        vol = S.integrate(vol, dists, voxel, trunc, 64, v2c, *intr)
        O.tsdf_integrate(ref, dists, voxel, trunc, 64, v2c, *intr)
    assert np.array_equal(vol, ref)
    R = rot([0, 1, 0.2], 0.07)
    c2v = aff12(R, cam2vol[9:] + np.array([0.02, -0.01, 0.03], np.float32))
    ri = R.T.astype(np.float32).reshape(-1)
    W, H = cfg["width"], cfg["height"]
    P, N = S.raycast_points(vol, voxel, trunc, c2v, ri, *intr, STEP, DELTA, W, H)
    Po, No = O.tsdf_raycast_points(vol, voxel, trunc, c2v, ri, *intr, STEP, DELTA, W, H)
    assert (~np.isnan(P[..., 0])).mean() > 0.5
    assert np.array_equal(bits(P), bits(Po)) and np.array_equal(bits(N), bits(No))
    D, N2 = S.raycast_depth(vol, voxel, trunc, c2v, ri, *intr, STEP, DELTA, W, H)
    Do, N2o = O.tsdf_raycast_depth(vol, voxel, trunc, c2v, ri, *intr, STEP, DELTA, W, H)
    assert np.array_equal(D, Do) and np.array_equal(bits(N2), bits(N2o))
    hit = ~np.isnan(P[..., 0])
    pts = np.zeros((int(hit.sum()), 4), np.float32)
    for k in range(3):  # the hits back in the volume frame, then the raycaster's normals there
        pts[:, k] = (c2v[9 + k] + P[..., 0][hit] * R[k, 0] + P[..., 1][hit] * R[k, 1] + P[..., 2][hit] * R[k, 2])
    assert np.array_equal(bits(S.vertex_normals(vol, voxel, DELTA, pts)), bits(O.tsdf_vertex_normals(vol, voxel, DELTA, pts)))


@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (8, 130)])
def test_compute_dists_equals_oracle(shape):
    rng = np.random.default_rng(shape[1])
    depth = rng.integers(0, 65536, shape).astype(np.uint16)  # up to 65.5 m: the half's overflow to inf included
    intr = (3.0, 2.5, shape[1] / 2 - 0.5, shape[0] / 2 - 0.5)
    assert np.array_equal(S.compute_dists(depth, *intr), O.compute_dists(depth, *intr))


# ------------------------------------------------------------------------------------------- raycast bounds ----
def _look(cam, target):
    z = np.asarray(target, float) - cam
    z /= np.linalg.norm(z)
    x = np.cross([0.1, 1, 0.3], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1)


def test_rays_never_leave_the_volume_from_adversarial_poses():
    """Camera inside, on a face, an edge or a corner of the box [0, size - voxel], or outside beyond a corner; looking
    at the centre, along each axis, through a corner; wide and narrow fields of view.  The volume is a constant positive
    tsdf, so that every ray marches from tmin to tmax.  S.raycast raises if a fetch leaves the volume."""
    count = 0
    for dims, vs in (((9, 7, 5), (0.1, 0.13, 0.07)), ((1, 4, 3), (0.1, 0.1, 0.1)), ((2, 2, 2), (0.2, 0.3, 0.25))):
        X, Y, Z = dims
        vs = np.array(vs, np.float32)
        vol = S.pack(np.full((Z, Y, X), 0.5, np.float32), np.ones((Z, Y, X), np.uint32))
        bm = vs * np.array(dims, np.float32) - vs
        cams = [bm * f32(a) for a in itertools.product([0, 0.5, 1], repeat=3)]
        cams += [bm * f32(a) for a in itertools.product([-0.5, 1.5], repeat=3)]
        for cam in cams:
            targets = [0.5 * bm, np.zeros(3), bm] + [cam + e for e in np.vstack([np.eye(3), -np.eye(3)])]
            for target in targets:
                if np.linalg.norm(np.asarray(target) - cam) < 1e-6:
                    continue
                R = _look(cam, target).astype(np.float32)
                for W, H, f in ((9, 7, 2.0), (1, 1, 1.0)):
                    S.raycast(vol, vs, 0.1, aff12(R, cam), R.T.reshape(-1), f, f, (W - 1) / 2, (H - 1) / 2, STEP,
                              DELTA, W, H)
                    count += 1
            for perm in itertools.permutations(range(3)):  # rays exactly parallel to the axes, both directions
                for sign in (1, -1):
                    R = np.eye(3)[:, perm] * sign
                    S.raycast(vol, vs, 0.1, aff12(R, cam), R.T.astype(np.float32).reshape(-1), 1.0, 1.0, 0.0, 0.0,
                              STEP, DELTA, 1, 1)
                    count += 1
    assert count > 1000


def test_fetch_outside_the_volume_raises():
    vol = S.clear((2, 2, 2))
    with pytest.raises(S.RayLeftVolume):
        S._fetch(vol, np.ones(3, np.float32), [np.array([2.0], np.float32)] * 3, np.array([True]))
