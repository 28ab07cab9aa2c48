"""CPU checks of the render seam:

- tests/render_statement.py (the numpy statement of imgproc.cu:363-514) on hand-made pixels whose bytes are worked out
  here by hand, independent of the statement;
- the library exports the four entry points of the seam, and each rejects a null image (and the fused one an unknown
  mode) with DFA_ERR_INVALID before any HIP call;
- the scenes the -m gpu tests of tests/test_gpu_render.py rely on meet their input conditions (both sides of the hit /
  miss branch, a specular term strictly between 0 and 1), checked with the statements alone.
The HIP kernels are compared with the statement by tests/test_gpu_render.py."""
import ctypes

import numpy as np
import pytest

import render_statement as R
import tsdf_statement as S

f32 = np.float32
NAN = np.nan
RS_CAMERAS = ("turned", "behind")  # render_scenes.CAMERAS


def _maps(pixels):
    """[(point xyz, normal xyz), ...] -> 1 x n float4 maps"""
    P = np.zeros((1, len(pixels), 4), np.float32)
    N = np.zeros((1, len(pixels), 4), np.float32)
    for i, (p, n) in enumerate(pixels):
        P[0, i, :3], N[0, i, :3] = p, n
    return P, N


# ------------------------------------------------------------------------------------------------ hand-made ----
def test_background_ramp_top_and_bottom_row():
    # every point NaN: colour = bgr1 (1 - w) + bgr2 w, w = y / rows, bgr1 = (4, 2, 2) / 255, bgr2 = (236, 120, 120) / 255
    rows = 480
    P = np.full((rows, 3, 4), NAN, np.float32)
    img = R.render_image_points(P, P, [0, 0, 0])
    # y = 0: w = 0, colour = bgr1 exactly; float(4 / 255) * 255 and float(2 / 255) * 255 round to 4.0 and 2.0
    assert img[0].tolist() == [[4, 2, 2, 0]] * 3
    # y = 479: b = 4 + 232 * 479 / 480 = 235.52 -> 235, g = r = 2 + 118 * 479 / 480 = 119.75 -> 119
    assert img[479].tolist() == [[235, 119, 119, 0]] * 3
    # y = 160: w = 1 / 3, b = 4 + 232 / 3 = 81.33 -> 81, g = r = 2 + 118 / 3 = 41.33 -> 41
    assert img[160].tolist() == [[81, 41, 41, 0]] * 3
    # the ramp depends on the row alone, and only on NaN in x
    P2 = np.zeros((rows, 3, 4), np.float32)
    P2[..., 0] = NAN
    assert np.array_equal(R.render_image_points(P2, P2, [1, 2, 3]), img)


def test_depth_zero_is_the_background_and_depth_reprojects():
    rows, cols = 3, 2
    D = np.zeros((rows, cols), np.uint16)
    N = np.zeros((rows, cols, 4), np.float32)
    N[..., 2] = -1
    img = R.render_image_depth(D, N, 10.0, 10.0, 0.5, 1.0, [0, 0, 0])
    assert img[1].tolist() == [[81, 41, 41, 0]] * 2  # w = 1 / 3, as above
    # 2 m at the principal point (cx = 0, cy = 1; pixel (0, 1)): P = (0, 0, 2), the facing surface of the next test
    D[1, 0] = 2000
    img = R.render_image_depth(D, N, 10.0, 10.0, 0.0, 1.0, [0, 0, 0])
    assert img[1, 0].tolist() == [255, 255, 255, 0] and img[1, 1].tolist() == [81, 41, 41, 0]
    # the same pixel seen from the depth form and from the point form: P = (z (u - cx) / fx, z (v - cy) / fy, z)
    D[:] = 1500
    Pm = np.zeros((rows, cols, 4), np.float32)
    for v in range(rows):
        for u in range(cols):
            Pm[v, u, :3] = [1.5 * (u - 0.25) / 10, 1.5 * (v - 1.0) / 8, 1.5]  # exact in float32 up to the products
    assert np.array_equal(R.render_image_depth(D, N, 10.0, 8.0, 0.25, 1.0, [0.3, 0, 0]),
                          R.render_image_points(Pm, N, [0.3, 0, 0]))


def test_phong_bytes_of_hand_made_surfaces():
    light = [0, 0, 0]
    P, N = _maps([
        ([0, 0, 1], [0, 0, -1]),    # facing the light and the camera: N.L = 1, R = V: 0.3 + 0.5 + 0.2 = 1 -> 255
        ([0, 0, 1], [1, 0, 0]),     # edge-on: N.L = 0, R = -L = (0, 0, 1), R.V = -1 -> 0: 0.3 * 255 = 76.5 -> 76
        ([0, 0, 1], [0, 0, 1]),     # back face: N.L = -1 -> 0; R = 2 N (-1) - L = (0, 0, -1) = V: 0.3 + 0.2 = 0.5 -> 127
        ([0, 0, 1], [NAN, NAN, NAN]),  # a NaN normal: both max(0, NaN) are 0: 0.3 -> 76
        ([0, 0, 3], [0, 0, -2]),    # |N| = 2 (not normalised by the kernel): N.L = 2, 0.3 + 1.0 saturates -> 255
    ])
    got = R.render_image_points(P, N, light)[0]
    assert got[:, 0].tolist() == [255, 76, 127, 76, 255]
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2]) and not got[:, 3].any()


def test_off_axis_light_gives_a_specular_term_between_0_and_1():
    # P = (0, 0, 2), N = (0, 0, -1), light (1.5, 0, 0): L = (1.5, 0, -2) / 2.5 = (0.6, 0, -0.8), N.L = 0.8,
    # R = 2 N 0.8 - L = (-0.6, 0, -0.8), V = (0, 0, -1), R.V = 0.8, 0.8^20 = 0.0115292,
    # Ix = 0.3 + 0.4 + 0.2 * 0.0115292 = 0.702306, * 255 = 179.09 -> 179
    P, N = _maps([([0, 0, 2], [0, 0, -1])])
    assert R.render_image_points(P, N, [1.5, 0, 0])[0, 0].tolist() == [179, 179, 179, 0]
    rv, nl = R.specular([P[..., k] for k in range(3)], [N[..., k] for k in range(3)], [1.5, 0, 0])
    assert abs(rv[0, 0] - 0.8) < 1e-6 and abs(nl[0, 0] - 0.8) < 1e-6
    # light (2, 0, 0): L = (1, 0, -1) / sqrt 2, N.L = R.V = 0.70711, ^20 = 2^-10: 0.3 + 0.35355 + 0.000195 = 0.65375 -> 166.7
    assert R.render_image_points(P, N, [2, 0, 0])[0, 0, 0] == 166


def test_pow20_is_the_five_multiplications():
    x = np.array([0.0, 0.5, 0.8, 1.0, 2.0], np.float32)
    got = R.pow20(x)
    assert got[0] == 0 and got[1] == 2.0 ** -20 and got[3] == 1 and got[4] == 2.0 ** 20  # powers of two: exact
    # float(0.8) is off by up to 2^-24 relative, amplified 20 times by the power; the roundings of x2, x4, x5, x10, x20
    # reach the result amplified 10, 5, 4, 2 and 1 times: 42 half-ulps in all
    assert abs(got[2] - 0.8 ** 20) <= 42 * 2.0 ** -24 * 0.8 ** 20
    x2 = f32(0.8) * f32(0.8)
    x5 = (x2 * x2) * f32(0.8)
    assert got[2] == (x5 * x5) * (x5 * x5)  # this order, not pow()


def test_saturating_byte_conversions():
    c = np.array([NAN, -1, 0, 0.5, 1, 7, np.inf, -np.inf], np.float32)
    assert R.unit_to_byte(c).tolist() == [0, 0, 0, 127, 255, 255, 255, 0]  # 0.5 * 255 = 127.5 -> 127
    v = np.array([NAN, -3, 0.99, 38.25, 255, 255.5, 1e9, np.inf], np.float32)
    assert R.clamp_to_byte(v).tolist() == [0, 0, 0, 38, 255, 255, 255, 255]


def test_normal_colour_bytes():
    N = np.array([[[0, 0, -1, 0],       # r = g = 5 * 25.5 = 127.5 -> 127, b = 8.5 * 25.5 = 216.75 -> 216
                   [1, 0, 0, 0],        # r = 1.5 * 25.5 = 38.25 -> 38
                   [NAN] * 4,           # a raycast miss: 0, 0, 0
                   [0.6, -0.8, 0, 0],   # r = 2.9 * 25.5 = 73.95 -> 73, g = 7 * 25.5 = 178.5 -> 178
                   [100, -100, 0, 0]]], np.float32)  # outside [0, 256): r < 0 -> 0, g = 6502.5 -> 255
    want = [[216, 127, 127, 0], [127, 127, 38, 0], [0, 0, 0, 0], [127, 178, 73, 0], [127, 255, 0, 0]]  # b, g, r, 0
    assert R.render_tangent_colors(N)[0].tolist() == want


def test_side_by_side_is_the_two_views():
    P, N = _maps([([0, 0, 1], [0, 0, -1]), ([NAN] * 3, [NAN] * 3)])
    both = R.render_maps(P, N, [0, 0, 0], R.BOTH)
    assert both.shape == (1, 4, 4)
    assert np.array_equal(both[:, :2], R.render_maps(P, N, [0, 0, 0], R.PHONG))
    assert np.array_equal(both[:, 2:], R.render_maps(P, N, [0, 0, 0], R.NORMALS))


# ------------------------------------------------------------------------------------- the GPU tests' scenes ----
def test_the_small_fused_sphere_meets_the_input_conditions():
    """the volume and camera of test_gpu_render's comparison with the pure statement (the fused sphere of
    tests/test_tsdf_statement_cpu.py): hits and misses, a tenth of the image each, and specular terms inside (0, 1)"""
    import render_scenes as RS
    vol, voxel, trunc, c2v, ri, intr, W, H = RS.small_sphere()
    P, N = S.raycast_points(vol, voxel, trunc, c2v, ri, *intr, RS.STEP, RS.DELTA, W, H)
    for light in RS.LIGHTS:
        RS.check_conditions(P, N, light)
        img = R.render_maps(P, N, light, R.BOTH)
        assert img.shape == (H, 2 * W, 4)


@pytest.mark.parametrize("cam", RS_CAMERAS)
def test_the_cameras_of_the_gpu_tests_see_surface_and_background(cam):
    """the cameras test_gpu_render casts from, on the same geometry at 64^3 / 160 x 120: the poses are metric, so the
    shares of surface and background are those of the full-size volumes"""
    import render_scenes as RS
    vol, voxel, trunc, intr, W, H = RS.statement_volume("T0", cam)
    c2v, ri = RS.camera(cam)
    P, N = S.raycast_points(vol, voxel, trunc, c2v, ri, *intr, RS.STEP, RS.DELTA, W, H)
    for light in RS.LIGHTS:
        RS.check_conditions(P, N, light)
    D, _ = S.raycast_depth(vol, voxel, trunc, c2v, ri, *intr, RS.STEP, RS.DELTA, W, H)
    assert np.array_equal(D == 0, np.isnan(P[..., 0]))  # the depth form branches on the same pixels


# ---------------------------------------------------------------------------------------------- the library ----
@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (torch's bundled HIP runtime must be the one the library binds to)
    from dynfu_amd import build as B
    L = ctypes.CDLL(B.build())
    L.dfa_last_error.restype = ctypes.c_char_p
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.dfa_render_image_points.argtypes = [vp, i, vp, i, i, i, vp, vp, i, vp]
    L.dfa_render_image_depth.argtypes = [vp, i, vp, i, i, i, f, f, f, f, vp, vp, i, vp]
    L.dfa_render_tangent_colors.argtypes = [vp, i, i, i, vp, i, vp]
    L.dfa_tsdf_raycast_render.argtypes = [vp, i, i, i, vp, f, vp, vp, f, f, f, f, f, f, i, i, vp, i, vp, i, vp]
    return L


def test_render_entry_points_reject_bad_arguments_before_any_hip_call(lib):
    # host memory stands in for the device images: validation fails before anything would read it
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    INVALID = 1
    ray = lambda image, mode=0, step=16: lib.dfa_tsdf_raycast_render(p, 8, 8, 8, p, 0.1, p, p, 1.0, 1.0, 0.0, 0.0, 0.75, 0.5, 2, 2, p,  # noqa: E731
                                                                     mode, image, step, None)
    for name, call in (("dfa_render_image_points", lambda: lib.dfa_render_image_points(p, 32, p, 32, 2, 2, p, None, 8, None)),
                       ("dfa_render_image_depth", lambda: lib.dfa_render_image_depth(p, 4, p, 32, 2, 2, 1.0, 1.0, 0.0, 0.0, p, None, 8, None)),
                       ("dfa_render_tangent_colors", lambda: lib.dfa_render_tangent_colors(p, 32, 2, 2, None, 8, None)),
                       ("dfa_tsdf_raycast_render", lambda: ray(None))):
        assert call() == INVALID, name
        assert name.encode() in lib.dfa_last_error() and b"null image" in lib.dfa_last_error()
    assert ray(p, mode=3) == INVALID and b"unknown render mode" in lib.dfa_last_error()
    assert ray(p, mode=-1) == INVALID
    assert ray(p, mode=2, step=8) == INVALID and b"row step" in lib.dfa_last_error()  # side by side needs 2 * cols pixels
    assert lib.dfa_render_image_points(p, 16, p, 32, 2, 2, p, p, 8, None) == INVALID and b"row step" in lib.dfa_last_error()
    assert lib.dfa_render_image_points(p, 32, p, 32, 2, 2, p, p, 4, None) == INVALID and b"row step" in lib.dfa_last_error()
    assert lib.dfa_render_image_points(p, 32, p, 32, 0, 2, p, p, 8, None) == INVALID
    assert lib.dfa_render_image_points(p, 32, p, 32, 2, 2, None, p, 8, None) == INVALID  # null light pose
    assert lib.dfa_render_tangent_colors(None, 32, 2, 2, p, 8, None) == INVALID


def test_python_binding_exports_the_render_entry_points():
    import dynfu_amd
    for name in ("render_image_points", "render_image_depth", "render_tangent_colors", "tsdf_raycast_render"):
        assert callable(getattr(dynfu_amd, name)) and name in dynfu_amd.__all__
    assert (dynfu_amd.RENDER_PHONG, dynfu_amd.RENDER_NORMALS, dynfu_amd.RENDER_BOTH) == (R.PHONG, R.NORMALS, R.BOTH)
