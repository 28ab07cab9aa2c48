"""The scenes of the render tests (tests/test_gpu_render.py, checked without a GPU by tests/test_render_statement_cpu.py):
the synthetic sphere of dynfu_amd/synth.py fused into a volume, and cameras whose view has BOTH surface and background —
the render kernels branch on hit / miss, and a comparison of images without one side of the branch would be empty.

Poses are in metres and do not depend on the configuration's resolution: the same cameras see the same geometry at
64^3 / 160 x 120 (where the numpy statement can raycast) and at 512^3 / VGA."""
import numpy as np

from dynfu_amd import synth
from gpu_util_cpu import aff12, rot

STEP, DELTA = synth.RAYCAST_STEP_FACTOR, synth.GRADIENT_DELTA_FACTOR
LIGHTS = ([0.0, 0.0, 0.0], [0.4, -0.3, 0.2])  # KinFuParams' default (the camera itself) and one off the optical axis
CAMERAS = ("turned", "behind")


def integration_poses(camera):
    """vol2cam (12 floats) of the frames fused into the volume: the synthetic sequence's own pose and, for the camera
    behind the sphere, a second pose turned by pi about the vertical axis through the sphere's centre — without it the
    far side of the sphere was never seen and every ray from behind leaves through a back face (a miss)"""
    t0 = np.array(synth.VOLUME_POSE_T, np.float64)
    poses = [aff12(np.eye(3), t0)]
    if camera == "behind":
        R2 = rot([0, 1, 0], np.pi)
        poses.append(aff12(R2, (synth.SPHERE_C - R2 @ synth.SPHERE_C) + R2 @ t0))
    return poses


def camera(name):
    """(cam2vol 12 floats, Rinv 9 floats) of the rendering camera"""
    t0 = np.array(synth.VOLUME_POSE_T, np.float64)
    if name == "turned":  # moved and turned by 20 degrees: a third of the view looks past what the sequence's camera saw
        R = rot([0.1, 1, 0.05], 0.35)
        pos = -t0 + np.array([0.03, -0.02, 0.01])
    else:  # behind the sphere, looking back at it, slightly off the second integration pose
        v2c = integration_poses("behind")[1]
        R2, t2 = v2c[:9].reshape(3, 3).astype(np.float64), v2c[9:].astype(np.float64)
        R = R2.T @ rot([0.1, 1, 0.05], 0.07)
        pos = -R2.T @ t2 + np.array([0.03, -0.02, 0.01])
    return aff12(R, pos), np.linalg.inv(R).astype(np.float32).reshape(-1)


def check_conditions(points, normals, light, need_specular=True):
    """a tenth of the pixels on each side of the hit / miss branch; pixels whose specular base max(0, R.V) lies strictly
    between 0 and 1 (so that the power and the reflection are exercised, not only its end points)"""
    import render_statement as R
    P, N = np.asarray(points, np.float32), np.asarray(normals, np.float32)
    hit = ~np.isnan(P[..., 0])
    assert 0.1 <= hit.mean() <= 0.9, hit.mean()
    rv, _ = R.specular([P[..., k] for k in range(3)], [N[..., k] for k in range(3)], light)
    inside = hit & (rv > 0) & (rv < 1)
    if need_specular:
        assert inside.sum() >= 0.01 * hit.sum(), (int(inside.sum()), int(hit.sum()))
    return hit, inside


def statement_volume(name, cam):
    """the scene fused by the numpy statement (small configurations only)"""
    import tsdf_statement as S
    cfg = synth.CONFIGS[name]
    intr = synth.intrinsics(cfg)
    voxel, trunc, _, _, _ = synth.volume_params(cfg)
    dists = S.compute_dists(synth.depth_frame(cfg, 0), *intr)
    dim = cfg["dim"]
    vol = S.clear((dim, dim, dim))
    for v2c in integration_poses(cam):
        vol = S.integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, v2c, *intr)
    return vol, voxel, trunc, intr, cfg["width"], cfg["height"]


def small_sphere():
    """the fused sphere tests/test_tsdf_statement_cpu.py raycasts with the statement (T0: 64^3, 160 x 120, fused twice
    through a tilted vol2cam), seen from a camera turned far enough for a tenth of the image to miss"""
    import tsdf_statement as S
    cfg = synth.CONFIGS["T0"]
    intr = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, cam2vol, _ = synth.volume_params(cfg)
    v2c = aff12(rot([1, 0.2, 0.3], 0.2), vol2cam[9:])
    dists = S.compute_dists(synth.depth_frame(cfg, 0), *intr)
    dim = cfg["dim"]
    vol = S.clear((dim, dim, dim))
    for _ in range(2):
        vol = S.integrate(vol, dists, voxel, trunc, 64, v2c, *intr)
    R = rot([0, 1, 0.2], 0.3)
    c2v = aff12(R, cam2vol[9:] + np.array([0.02, -0.01, 0.03], np.float32))
    return vol, voxel, trunc, c2v, R.T.astype(np.float32).reshape(-1), intr, cfg["width"], cfg["height"]
